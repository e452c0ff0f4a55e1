"""GPU: ebo_relative_pose_refine against tests/relpose_ref.py, by the rule of tests/test_gpu_bundle.py: iterations,
num_evals_*, termination and the trace's flags as equal integers; every double (model, initial and final cost, trace)
within 10 x the scene's delta, the largest difference (|a - b| / max(1, |b|)) between the restatement and itself with
every stated sum reversed, which is what a legitimate change of rounding order does to that solve.  The count of
bit-equal doubles is printed.  tests/test_relpose_refine_cpu.py checks on the CPU that no decision of these scenes is
a coin toss and that no integer flips between the two orders, which is what makes the integer comparison fair.

Scenes (relpose_ref.test_scenes; ebo_default_ba_opts unless said) and their delta as measured on the CPU:
  m0, m4     lists of 0 and 4 inliers: not refined (iterations 0, termination 1, model untouched)            0, 0
  m5         the smallest list that is refined: 59 empty partials in the tree                               7.1e-14
  m63, m64, m65, m129, m300   the lane stride's edges: one short of a row, one row, one over, two rows
             and one, five rows                                                  4.2e-9, 1.1e-9, 2.7e-8, 4.2e-11, 4.5e-9
  m4096      64 inliers per partial                                                                         1.6e-12
  shuffled   90 of 140 in no order, the last one the pair's last index; 30 iterations, 11 rejected          5.9e-7
  it0, it1   max_num_iterations 0 and 1 (it0 returns the start with its t normalised)                       0, 0
  long_t     |t| = 0.3 on entry                                                                              9.0e-9
  nan        a NaN bearing: termination 2, the model returned bit for bit                                   0
  rotation   baseline 1e-9: the direction is not observable; 50 iterations, termination 1                   9.7e-5
  rej        a start 0.25 rad and 0.8 off with initial_radius 1e16: the first step and runs of steps rejected  1.6e-7
  invalid    initial_radius 1e-310, min_radius 0, min_lm_diagonal 0: every damped pivot is infinite, five
             invalid steps, termination 2 without one cost evaluation                                      0
  batch      70 pairs of 0..199 inliers, 3 to 50 iterations, every third list in no order                    <= 2.7e-4
"""
import ctypes as C

import numpy as np
import pytest

import relpose_ref as R

pytestmark = pytest.mark.gpu

INTS = ("iterations", "num_evals_cost", "num_evals_jac", "termination")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def same_result(x, y):
    return (same(x["model"], y["model"]) and same(x["trace"], y["trace"]) and all(x["summary"][k] == y["summary"][k] for k in INTS) and
            same(x["summary"]["initial_cost"], y["summary"]["initial_cost"]) and same(x["summary"]["final_cost"], y["summary"]["final_cost"]))


def check(name, got, want, delta):
    for k in INTS:
        assert got["summary"][k] == want["summary"][k], (name, k, got["summary"], want["summary"])
    assert np.array_equal(got["trace"][:, 3], want["trace"][:, 3]), name
    pairs = [(got[k], want[k]) for k in ("model", "trace")] + [(got["summary"][k], want["summary"][k]) for k in ("initial_cost", "final_cost")]
    equal = sum(int(((bits(a) == bits(b)) | (np.isnan(np.asarray(a, float)) & np.isnan(np.asarray(b, float)))).sum()) for a, b in pairs)
    total = sum(np.asarray(a).size for a, _ in pairs)
    worst = max(R.difference(a, b) for a, b in pairs)
    print("%s: %d of %d doubles bit-equal, largest difference %.3g, delta %.3g" % (name, equal, total, worst, delta))
    assert worst <= 10 * delta, (name, worst, delta)
    return equal, total


@pytest.fixture(scope="module")
def scenes():
    return R.test_scenes()


@pytest.fixture(scope="module")
def refs(scenes):
    """name -> (the restatement's result, delta); computed once, read only."""
    out = {}
    for name, (pair, o) in scenes.items():
        fwd = R.solve(pair, o)
        out[name] = (fwd, R.result_difference(fwd, R.solve(pair, o, reverse_sums=True)))
    return out


@pytest.fixture(scope="module")
def batch():
    """The 70 pairs, the restatement's result and delta of each; computed once, read only."""
    pairs = R.batch_scenes()
    o = R.default_opts()
    fwd = [R.solve(p, o) for p in pairs]
    delta = [R.result_difference(f, R.solve(p, o, reverse_sums=True)) for p, f in zip(pairs, fwd)]
    return pairs, fwd, delta


def refine(ebo, c, pairs, o):
    return c.relative_pose_refine(pairs, opts=ebo.default_ba_opts(**o), trace=True)


@pytest.mark.parametrize("name", ["m0", "m4", "m5", "m63", "m64", "m65", "m129", "m300", "m4096", "shuffled", "it0", "it1", "long_t",
                                  "rotation", "rej", "invalid"])
def test_scene_equals_the_restatement(ebo, scenes, refs, name):
    pair, o = scenes[name]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = refine(ebo, c, [pair], o)[0]
    check(name, got, *refs[name])
    if name in ("m0", "m4"):
        assert same(got["model"], pair["model"]) and not got["trace"].any()
    else:
        assert abs(np.linalg.norm(got["model"][:, 3]) - 1) <= 1e-14


def test_a_nan_bearing_leaves_its_neighbours_alone(ebo, scenes, refs):
    """The pair with a NaN bearing comes back bit for bit with termination 2; its two healthy neighbours in the call equal
    their results alone."""
    o = R.default_opts()
    trio = [scenes["m65"][0], scenes["nan"][0], scenes["m129"][0]]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = refine(ebo, c, trio, o)
        alone = [refine(ebo, c, [p], o)[0] for p in trio]
    check("nan", got[1], *refs["nan"])
    assert got[1]["summary"]["termination"] == 2 and same(got[1]["model"], trio[1]["model"]) and not got[1]["trace"].any()
    for k, name in ((0, "m65"), (2, "m129")):
        assert same_result(got[k], alone[k]), name
        check(name, got[k], *refs[name])


def test_a_batch_equals_each_pair_alone_and_a_second_run(ebo, batch):
    pairs, want, delta = batch
    o = R.default_opts()
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = refine(ebo, c, pairs, o)
        again = refine(ebo, c, pairs, o)
        alone = [refine(ebo, c, [p], o)[0] for p in pairs]
    equal = total = 0
    for k in range(len(pairs)):
        e, t = check("batch%d" % k, got[k], want[k], delta[k])
        equal, total = equal + e, total + t
        assert same_result(got[k], again[k]), k
        assert same_result(got[k], alone[k]), k
    print("batch: %d of %d doubles bit-equal" % (equal, total))


def test_host_form_equals_device_form_which_refuses_a_bad_index(ebo, scenes):
    import torch
    names = ["m65", "shuffled", "m4", "m129"]
    pairs = [scenes[n][0] for n in names]
    o = ebo.default_ba_opts()
    sizes = [len(p["f1"]) for p in pairs]
    off = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    cnt = np.array([len(p["idx"]) for p in pairs], np.int32)
    idx = np.zeros(off[-1], np.int32)
    for k, p in enumerate(pairs):
        idx[off[k]:off[k] + cnt[k]] = p["idx"]
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    d_f1, d_f2 = dev(np.concatenate([p["f1"] for p in pairs])), dev(np.concatenate([p["f2"] for p in pairs]))
    models = np.stack([p["model"] for p in pairs])
    rows = o.max_num_iterations + 1
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        host = c.relative_pose_refine(pairs, opts=o, trace=True)
        d_models, d_idx = dev(models), dev(idx)
        d_trace = torch.full((len(pairs), rows, 4), -7.0, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        summ = c.relative_pose_refine_device(off, d_f1.data_ptr(), d_f2.data_ptr(), d_models.data_ptr(), cnt, d_idx.data_ptr(), opts=o,
                                             d_trace=d_trace.data_ptr())
        got_models, got_trace = d_models.cpu().numpy(), d_trace.cpu().numpy()
        for k in range(len(pairs)):
            got = dict(model=got_models[k], trace=got_trace[k], summary=summ[k])
            assert same_result(got, host[k]), names[k]
        # the device form cannot look at the indices: the pair with one out of range is not solved, the others are
        bad = idx.copy()
        bad[off[1] + 3] = sizes[1]
        d_models, d_bad = dev(models), dev(bad)
        torch.cuda.synchronize()
        summ = c.relative_pose_refine_device(off, d_f1.data_ptr(), d_f2.data_ptr(), d_models.data_ptr(), cnt, d_bad.data_ptr(), opts=o)
        after = d_models.cpu().numpy()
        assert summ[1]["termination"] == 2 and summ[1]["iterations"] == 0 and same(after[1], models[1])
        for k in (0, 2, 3):
            assert summ[k] == host[k]["summary"] and same(after[k], host[k]["model"]), names[k]
        # and the host form, which can look, refuses the call
        broken = dict(pairs[1], idx=bad[off[1]:off[1] + cnt[1]])
        with pytest.raises(ebo.EboError) as err:
            c.relative_pose_refine([pairs[0], broken], opts=o)
        assert err.value.code == ebo.ERR_ARG


def test_argument_errors_and_the_recording_state(ebo, scenes, synth):
    pair = scenes["m65"][0]
    n = len(pair["f1"])
    off = np.array([0, n], np.int32)
    f1, f2 = np.ascontiguousarray(pair["f1"]), np.ascontiguousarray(pair["f2"])
    idx = np.zeros(n, np.int32)
    idx[:len(pair["idx"])] = pair["idx"]
    model = np.ascontiguousarray(pair["model"]).copy()
    summ = (ebo.Summary * 1)()
    o = ebo.default_ba_opts()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = ebo.lib()
    import torch

    def call(c, off=off, cnt=len(pair["idx"]), f1=f1, model=model, opts=o, summ=summ):
        cnt = np.array([cnt], np.int32)
        return lib.ebo_relative_pose_refine(c._h, 1, vp(off), vp(f1) if f1 is not None else None, vp(f2), vp(model) if model is not None else None,
                                            vp(cnt), vp(idx), C.addressof(opts) if opts is not None else None,
                                            C.addressof(summ) if summ is not None else None, None)

    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        assert call(c, off=np.array([0, -1], np.int32)) == ebo.ERR_ARG        # decreasing offsets
        assert call(c, off=np.array([1, n], np.int32)) == ebo.ERR_ARG         # not from 0
        assert call(c, cnt=n + 1) == ebo.ERR_ARG and call(c, cnt=-1) == ebo.ERR_ARG
        assert call(c, f1=None) == ebo.ERR_ARG and call(c, model=None) == ebo.ERR_ARG and call(c, opts=None) == ebo.ERR_ARG
        assert call(c, summ=None) == ebo.ERR_ARG
        assert call(c, opts=ebo.default_ba_opts(max_num_iterations=-1)) == ebo.ERR_ARG
        assert lib.ebo_relative_pose_refine(c._h, 65536, vp(off), vp(f1), vp(f2), vp(model), vp(idx), vp(idx), C.addressof(o),
                                            C.addressof(summ), None) == ebo.ERR_ARG
        assert lib.ebo_relative_pose_refine(c._h, -1, vp(off), vp(f1), vp(f2), vp(model), vp(idx), vp(idx), C.addressof(o),
                                            C.addressof(summ), None) == ebo.ERR_ARG
        assert same(model, pair["model"])
        assert call(c) == 0 and summ[0].termination == 0
        assert c.relative_pose_refine([]) == []
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
            codes.append(call(c))
            try:
                c.relative_pose_refine_device(off, 1, 1, 1, [len(pair["idx"])], 1)
                codes.append(0)
            except ebo.EboError as e:
                codes.append(e.code)
            c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())

        g = c.record(body)
        assert codes == [ebo.ERR_STATE] * 2
        g.launch()
        c.synchronize()
        g.close()
        model[:] = pair["model"]
        assert call(c) == 0


def test_the_timing_brackets_the_call(ebo, scenes):
    pair, o = scenes["m300"]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        c.two_view_timing(True)
        refine(ebo, c, [pair], o)
        ms = c.two_view_timing(False)
    assert ms[0] > 0.0 and ms[4] >= ms[0] and ms[1] == ms[2] == ms[3] == 0.0
