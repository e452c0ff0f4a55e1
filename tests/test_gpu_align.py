"""GPU: ebo_align_sim3 against tests/align_ref.py.  Every double of every result (scale, R, t, rmse, mean, min, max) is
bit-equal to the restatement, count and status are equal integers.  The cases are align_ref.gpu_cases: segments of 3,
63, 64, 65, 128 and 129 points (the lane stride's tails), of 0, 1 and 2 points (status 1), a NaN inside a segment and
just outside it, an infinite model coordinate (status 2), collinear and coincident points (status 3), a planar scene, a
mirrored one, one 1e4 from the origin, and fix_scale; a batch of 70 segments mixing them, each equal to itself alone;
every prefix 6 .. 40 of one trajectory against 35 single calls; the _device form; the argument errors."""
import ctypes as C

import numpy as np
import pytest

import align_ref as A

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return A.gpu_cases()


@pytest.fixture(scope="module")
def refs(cases):
    """name -> the restatement's results; computed once, read only."""
    return {name: A.align_segments(d, m, segs, fix) for name, (d, m, segs, fix) in cases.items()}


def check(name, got, want):
    assert len(got) == len(want), name
    for k, (g, w) in enumerate(zip(got, want)):
        assert g["status"] == w["status"] and g["count"] == w["count"], (name, k, g, w)
        for f in ("scale", "R", "t", "rmse", "mean", "min", "max"):
            assert A.same_bits(g[f], w[f]), (name, k, f, g[f], w[f])


EXPECTED_STATUS = {"n3": [0], "n63": [0], "n64": [0], "n65": [0], "n128": [0], "n129": [0], "short": [1] * 5,
                   "nan": [2, 0, 0, 1], "inf_model": [2, 0], "collinear": [3, 3], "coincident": [3], "planar": [0],
                   "mirrored": [0], "offset": [0], "fix_scale": [0]}


@pytest.mark.parametrize("name", sorted(EXPECTED_STATUS))
def test_case_equals_the_restatement(ebo, cases, refs, name):
    d, m, segs, fix = cases[name]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = c.align_sim3(d, m, segs, fix_scale=fix)
    assert [w["status"] for w in refs[name]] == EXPECTED_STATUS[name]
    check(name, got, refs[name])
    for g in got:
        if g["status"] == 0:
            assert abs(np.linalg.det(g["R"]) - 1.0) <= 1e-14
        else:
            assert g["scale"] == 1.0 and np.array_equal(g["R"], np.eye(3)) and not g["t"].any() and g["rmse"] == 0.0
    if name == "fix_scale":
        assert A.same_bits(got[0]["scale"], 1.0)


def test_a_nan_just_outside_a_segment_does_not_matter(ebo, cases):
    """Segments (0, 5) and (6, 10) border the NaN at point 5: they equal the same points of the clean arrays."""
    d, m, _, _ = cases["nan"]
    clean, _, _, _ = cases["short"]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = c.align_sim3(d, m, [(0, 5), (6, 10)])
        want = c.align_sim3(clean, m, [(0, 5), (6, 10)])
    for g, w in zip(got, want):
        assert g["status"] == 0 and A.same_result(g, w)


def test_a_batch_of_70_equals_each_segment_alone_and_the_restatement(ebo):
    data, model, segs = A.batch70()
    assert len(segs) == 70
    want = A.align_segments(data, model, segs)
    assert {w["status"] for w in want} == {0, 1, 2, 3}
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = c.align_sim3(data, model, segs)
        again = c.align_sim3(data, model, segs)
        alone = [c.align_sim3(data, model, [s])[0] for s in segs]
    check("batch70", got, want)
    for k in range(70):
        assert A.same_result(got[k], again[k]) and A.same_result(got[k], alone[k]), k


def test_all_prefixes_of_a_trajectory_equal_single_calls(ebo):
    gt, est = A.trajectory(40)
    segs = [(0, k) for k in range(6, 41)]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = c.align_sim3(gt, est, segs)
        single = [c.align_sim3(gt[:k], est[:k], [(0, k)])[0] for k in range(6, 41)]
    assert len(got) == 35
    check("prefixes", got, A.align_segments(gt, est, segs))
    for g, s in zip(got, single):
        assert g["status"] == 0 and A.same_result(g, s)
    assert abs(got[-1]["scale"] - 1.7) <= 0.05 and got[-1]["rmse"] <= 0.05


def test_device_form_equals_host_form(ebo):
    import torch
    data, model, segs = A.batch70()
    d_data = torch.from_numpy(np.ascontiguousarray(data)).to("cuda")
    d_model = torch.from_numpy(np.ascontiguousarray(model)).to("cuda")
    torch.cuda.synchronize()
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        for fix in (False, True):
            host = c.align_sim3(data, model, segs, fix_scale=fix)
            dev = c.align_sim3_device(len(data), d_data.data_ptr(), d_model.data_ptr(), segs, fix_scale=fix)
            for k, (h, g) in enumerate(zip(host, dev)):
                assert A.same_result(h, g), (fix, k)
    assert np.array_equal(d_data.cpu().numpy(), data, equal_nan=True)


def test_argument_errors_and_the_recording_state(ebo, cases, synth):
    import torch
    d, m, _, _ = cases["n65"]
    d, m = np.ascontiguousarray(d), np.ascontiguousarray(m)
    n = len(d)
    res = (ebo.AlignResult * 2)()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = ebo.lib()

    def call(c, n_points=n, data=d, model=m, n_seg=1, sb=(0,), se=(n,), res=res):
        sb, se = np.array(sb, np.int32), np.array(se, np.int32)
        return lib.ebo_align_sim3(c._h, n_points, vp(data) if data is not None else None, vp(model) if model is not None else None,
                                  n_seg, vp(sb) if len(sb) else None, vp(se) if len(se) else None, 0,
                                  C.addressof(res) if res is not None else None)

    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        assert call(c, data=None) == ebo.ERR_ARG and call(c, model=None) == ebo.ERR_ARG and call(c, res=None) == ebo.ERR_ARG
        assert call(c, sb=()) == ebo.ERR_ARG and call(c, se=()) == ebo.ERR_ARG
        assert call(c, n_points=-1) == ebo.ERR_ARG and call(c, n_seg=-1) == ebo.ERR_ARG and call(c, n_seg=65536) == ebo.ERR_ARG
        assert call(c, sb=(5,), se=(4,)) == ebo.ERR_ARG                       # ends before it begins
        assert call(c, sb=(-1,), se=(4,)) == ebo.ERR_ARG and call(c, se=(n + 1,)) == ebo.ERR_ARG   # outside [0, n_points]
        with pytest.raises(ebo.EboError) as err:
            c.align_sim3(d, m, [(0, n), (3, n + 1)])
        assert err.value.code == ebo.ERR_ARG
        assert call(c) == 0 and res[0].status == 0 and res[0].count == n
        assert call(c, sb=(n,), se=(n,)) == 0 and res[0].status == 1          # empty, at the end: allowed
        assert c.align_sim3(d, m, []) == []
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
                c.align_sim3_device(n, 1, 1, [(0, n)])
                codes.append(0)
            except ebo.EboError as e:
                codes.append(e.code)
            c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())

        g = c.record(body)
        assert codes == [ebo.ERR_STATE] * 2
        g.launch()
        c.synchronize()
        g.close()
        assert call(c) == 0


def test_the_timing_brackets_the_call(ebo, cases):
    d, m, segs, _ = cases["n129"]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        c.two_view_timing(True)
        c.align_sim3(d, m, segs)
        ms = c.two_view_timing(False)
    assert ms[0] > 0.0 and ms[4] >= ms[0] and ms[1] == ms[2] == ms[3] == 0.0
