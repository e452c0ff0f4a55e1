"""GPU: ebo_bundle_adjust against tests/bundle_ref.py.  iterations, num_evals_*, termination and the trace's flags as
equal integers; every double (poses, points, initial and final cost, trace) within 10 x the scene's delta, the largest
difference (|a - b| / max(1, |b|)) between the restatement and itself with every stated sum reversed, which is what a
legitimate change of rounding order does to that solve (the margin of the two-view and absolute-pose tests, for the
same reason).  The count of bit-equal doubles is printed.  tests/test_bundle_cpu.py checks on the CPU that no step
quality of these scenes lies within 1e-6 relative of min_relative_decrease and that no integer flips between the
two orders, which is what makes the integer comparison fair.

Scenes (bundle_ref.test_scenes; Huber 0.8) and their delta as measured on the CPU:
  a     3 frames, 1 free, 4 points: one pass of everything, S is 6 x 6                              2.4e-11
  b     2 frames, both fixed, 5 points: structure only, no reduced system                           0
  c     24 frames, 22 free, 40 points seen by a seeded 2..24: S at its cap, 132 columns             1.8e-9
  d     5 frames, 300 points, 1053 observations, 0.3 px noise, 10 % moved by up to 30 px: the
        Huber branch, lanes stride over observations and points                                     8.3e-11
  e00-e63  fix_points: one-frame problems of 4..200 points on the identity camera, one call         <= 2.9e-10
  edge  a point seen once, a free frame without observations, a point seen by fixed frames only     7.5e-13
  it0, it1  scene a with max_num_iterations 0 and 1                                                 0, 6.7e-15
  nan   scene a with a NaN coordinate: termination 2, inputs returned bit for bit                   0
"""
import ctypes as C

import numpy as np
import pytest

import bundle_ref as B
from bundle_check import INTS, check, same, same_result

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def scenes():
    return B.test_scenes()


@pytest.fixture(scope="module")
def refs(scenes):
    """name -> (the restatement's result, delta); computed once."""
    out = {}
    for name, (pr, fix, o) in scenes.items():
        fwd = B.solve(pr, B.HUBER, fix, o)
        out[name] = (fwd, B.result_difference(fwd, B.solve(pr, B.HUBER, fix, o, reverse_sums=True)))
    return out


def opts_of(ebo, o):
    return ebo.default_ba_opts(**{k: v for k, v in o.items() if k in ("max_num_iterations", "use_nonmonotonic")})


def run(ebo, c, scenes, names):
    fix, o = scenes[names[0]][1], scenes[names[0]][2]
    return c.bundle_adjust([scenes[n][0] for n in names], scenes[names[0]][0]["cam"], B.HUBER, fix_points=fix, opts=opts_of(ebo, o),
                           trace=True)


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "edge", "it0", "it1"])
def test_scene_equals_the_restatement(ebo, scenes, refs, name):
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = run(ebo, c, scenes, [name])[0]
    check(name, got, refs)
    pr = scenes[name][0]
    if name == "edge":
        assert same(got["points"][0], pr["points"][0])          # seen once: takes no part
        assert not same(got["points"][1], pr["points"][1])      # seen by the fixed frames only: still structure
        assert same(got["poses"][3], pr["poses"][3])            # free, no observation: bit for bit
        assert same(got["poses"][:2], pr["poses"][:2]) and not same(got["poses"][2], pr["poses"][2])
    if name == "b":
        assert same(got["poses"], pr["poses"]) and not same(got["points"], pr["points"])
    if name == "it0":
        assert same(got["poses"], pr["poses"]) and same(got["points"], pr["points"]) and got["summary"]["termination"] == 1
    if name in ("a", "c", "d"):
        assert got["summary"]["final_cost"] < got["summary"]["initial_cost"]


def test_refinement_batch(ebo, scenes, refs):
    """(e): 64 one-frame problems with the points held constant, in one call."""
    names = ["e%02d" % i for i in range(len(B.REFINE_SIZES))]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = run(ebo, c, scenes, names)
    for n, g in zip(names, got):
        check(n, g, refs)
        assert same(g["points"], scenes[n][0]["points"])
        assert g["summary"]["termination"] == 0


def test_a_nan_problem_fails_alone(ebo, scenes, refs):
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = run(ebo, c, scenes, ["a", "nan", "edge"])
        alone = [run(ebo, c, scenes, [n])[0] for n in ("a", "edge")]
    bad = got[1]
    assert bad["summary"]["termination"] == 2 and bad["summary"]["iterations"] == 0
    assert same(bad["poses"], scenes["nan"][0]["poses"]) and same(bad["points"], scenes["nan"][0]["points"])
    check("nan", bad, refs)
    assert same_result(got[0], alone[0]) and same_result(got[2], alone[1])


def test_a_batch_equals_each_alone_and_itself(ebo, scenes):
    """(g): a problem's result depends neither on the other problems of the call nor on the run."""
    names = ["a", "c", "d", "b", "a"]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        batch = run(ebo, c, scenes, names)
        again = run(ebo, c, scenes, names)
        alone = {n: run(ebo, c, scenes, [n])[0] for n in set(names)}
    for n, g, h in zip(names, batch, again):
        assert same_result(g, alone[n]), n
        assert same_result(g, h), n


def test_host_form_equals_device_form(ebo, scenes):
    import torch
    names = ["a", "d", "edge"]
    prs = [scenes[n][0] for n in names]
    o = ebo.default_ba_opts()
    srt = [B.sort_observations(len(p["poses"]), p["of"], p["op"], p["uv"]) for p in prs]
    off = lambda sizes: np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    fo, po, oo = off([len(p["poses"]) for p in prs]), off([len(p["points"]) for p in prs]), off([len(s[0]) for s in srt])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    d_poses = dev(np.concatenate([p["poses"].reshape(-1, 12) for p in prs]))
    d_fixed = dev(np.concatenate([p["fixed"] for p in prs]).astype(np.uint8))
    d_points = dev(np.concatenate([p["points"] for p in prs]))
    d_of, d_op, d_uv = (dev(np.concatenate([s[k] for s in srt])) for k in range(3))
    d_trace = torch.full((len(prs), o.max_num_iterations + 1, 4), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        host = c.bundle_adjust(prs, B.CAM, B.HUBER, opts=o, trace=True)
        summ = c.bundle_adjust_device(fo, po, oo, d_poses.data_ptr(), d_fixed.data_ptr(), d_points.data_ptr(), d_of.data_ptr(),
                                      d_op.data_ptr(), d_uv.data_ptr(), B.CAM, B.HUBER, opts=o, d_trace=d_trace.data_ptr())
        poses, points, trace = d_poses.cpu().numpy(), d_points.cpu().numpy(), d_trace.cpu().numpy()
        for k, h in enumerate(host):
            assert same(poses[fo[k]:fo[k + 1]].reshape(-1, 3, 4), h["poses"]) and same(points[po[k]:po[k + 1]], h["points"]), k
            assert same(trace[k], h["trace"]), k
            assert all(summ[k][f] == h["summary"][f] for f in INTS) and same(summ[k]["final_cost"], h["summary"]["final_cost"]), k
        # the device form cannot look at the indices: a problem whose observations are out of order is not solved
        before = d_poses.clone(), d_points.clone()
        d_op2 = d_op.clone()
        d_op2[int(oo[1]):int(oo[1]) + 2] = d_op2[int(oo[1]):int(oo[1]) + 2].flip(0) + torch.tensor([1, 0], dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        summ = c.bundle_adjust_device(fo, po, oo, d_poses.data_ptr(), d_fixed.data_ptr(), d_points.data_ptr(), d_of.data_ptr(),
                                      d_op2.data_ptr(), d_uv.data_ptr(), B.CAM, B.HUBER, opts=o)
        assert summ[1]["termination"] == 2 and summ[1]["iterations"] == 0
        assert torch.equal(d_poses[int(fo[1]):int(fo[2])], before[0][int(fo[1]):int(fo[2])])
        assert torch.equal(d_points[int(po[1]):int(po[2])], before[1][int(po[1]):int(po[2])])


def test_argument_and_state_errors(ebo, scenes, synth):
    import torch
    pr = scenes["a"][0]
    o = ebo.default_ba_opts()
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        def code(problem=pr, huber=B.HUBER, opts=o):
            try:
                c.bundle_adjust([problem] if isinstance(problem, dict) else problem, B.CAM, huber, opts=opts)
                return 0
            except ebo.EboError as e:
                return e.code

        assert code() == 0
        assert code([]) == 0
        with_ = lambda **kw: dict(pr, **kw)
        assert code(with_(of=np.where(np.arange(len(pr["of"])) == 3, 3, pr["of"]))) == ebo.ERR_ARG       # frame index out of range
        assert code(with_(of=np.where(np.arange(len(pr["of"])) == 3, -1, pr["of"]))) == ebo.ERR_ARG
        assert code(with_(op=np.where(np.arange(len(pr["op"])) == 5, 4, pr["op"]))) == ebo.ERR_ARG       # point index out of range
        dup = with_(of=np.append(pr["of"], pr["of"][0]), op=np.append(pr["op"], pr["op"][0]), uv=np.vstack([pr["uv"], pr["uv"][:1]]))
        assert code(dup) == ebo.ERR_ARG                                                                  # a pair twice
        for h in (0.0, -1.0, float("nan")):
            assert code(huber=h) == ebo.ERR_ARG
        assert code(opts=ebo.default_ba_opts(max_num_iterations=-1)) == ebo.ERR_ARG
        big = lambda F, P, N: dict(poses=np.tile(np.eye(3, 4), (F, 1, 1)), fixed=np.ones(F, np.uint8), points=np.ones((P, 3)),
                                   of=np.zeros(N, np.int32), op=np.zeros(N, np.int32), uv=np.zeros((N, 2)))
        assert code(big(25, 1, 0)) == ebo.ERR_ARG
        assert code(big(1, 4097, 0)) == ebo.ERR_ARG
        assert code(big(1, 1, 65536)) == ebo.ERR_ARG
        # the raw entry: problem count, offsets, null pointers
        lib = ebo.lib()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        of, op, uv = B.sort_observations(3, pr["of"], pr["op"], pr["uv"])
        poses, fixed, points = pr["poses"].copy(), pr["fixed"].astype(np.uint8), pr["points"].copy()
        fo, po, oo = (np.array([0, n], dtype=np.int32) for n in (3, 4, len(of)))
        cam = ebo.camera(B.CAM)
        summ = (ebo.Summary * 1)()
        good = [vp(fo), vp(po), vp(oo), vp(poses), vp(fixed), vp(points), vp(of), vp(op), vp(uv), C.addressof(cam), C.c_double(B.HUBER), 0,
                C.addressof(o), C.addressof(summ), None]
        assert lib.ebo_bundle_adjust(c._h, 1, *good) == 0
        for i in (0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 12, 13):
            args = list(good)
            args[i] = None
            assert lib.ebo_bundle_adjust(c._h, 1, *args) == ebo.ERR_ARG, i
        assert lib.ebo_bundle_adjust(c._h, -1, *good) == ebo.ERR_ARG
        assert lib.ebo_bundle_adjust(c._h, 65536, *good) == ebo.ERR_ARG
        for bad in (np.array([1, 3], dtype=np.int32), np.array([0, -1], dtype=np.int32)):
            args = list(good)
            args[0] = vp(bad)
            assert lib.ebo_bundle_adjust(c._h, 1, *args) == ebo.ERR_ARG
        two = np.array([0, 3, 2], dtype=np.int32)                                                        # decreasing offsets
        args = list(good)
        args[0] = vp(two)
        args[1], args[2] = vp(np.array([0, 4, 4], dtype=np.int32)), vp(np.array([0, len(of), len(of)], dtype=np.int32))
        assert lib.ebo_bundle_adjust(c._h, 2, *args) == ebo.ERR_ARG
        # while a graph records: refused, and the recording survives
        ev, _ = synth.make_window(0, n_events=3000)
        c.set_window(ev)
        d_flows = torch.zeros((c.P, 2), dtype=torch.float64, device="cuda")
        d_out = torch.zeros(3 * c.P, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())
        c.synchronize()
        codes = []

        def body():
            codes.append(code())
            try:
                c.bundle_adjust_device(fo, po, oo, 1, 1, 1, 1, 1, 1, B.CAM, B.HUBER)
                codes.append(0)
            except ebo.EboError as e:
                codes.append(e.code)
            c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())

        g = c.record(body)
        assert codes == [ebo.ERR_STATE] * 2
        g.launch()
        c.synchronize()
        g.close()
        assert code() == 0
