"""GPU: ebo_trajectory_rpe against tests/rpe_ref.py.  Every double of every result (the translation's and the rotation's
rmse, mean, min, max) is bit-equal to the restatement, count and status are equal integers.  The cases are
rpe_ref.gpu_cases: pair counts 1, 63, 64, 65, 128 and 129 (the lane stride's tails); one segment at deltas 1, 2, 7, n - 1
(one pair), n and n + 3 (status 1); relative rotations of exactly 0, 1e-9, pi / 2, pi - 1e-9 and exactly pi; scales other
than 1 and none; a trajectory 1e4 from the origin; a NaN in a rotation entry and an Inf in a translation entry inside a
segment (status 2) and just outside it; a non-finite scale; a batch of 70 units mixing them, each equal to itself alone
and to a second run; every prefix 6 .. 40 x deltas {1, 3, 10} of one trajectory against the single calls; the _device
form; the argument errors."""
import ctypes as C

import numpy as np
import pytest

import rpe_ref as T

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return T.gpu_cases()


@pytest.fixture(scope="module")
def refs(cases):
    """name -> the restatement's results; computed once, read only."""
    return {name: T.rpe_units(gt, est, segs, deltas, scales) for name, (gt, est, segs, deltas, scales) in cases.items()}


def check(name, got, want):
    assert len(got) == len(want), name
    for k, (g, w) in enumerate(zip(got, want)):
        assert g["status"] == w["status"] and g["count"] == w["count"], (name, k, g, w)
        assert g["segment"] == w["segment"] and g["delta"] == w["delta"], (name, k)
        for f in T.FIELDS:
            assert T.same_bits(g[f], w[f]), (name, k, f, g[f], w[f])


EXPECTED_STATUS = {"pairs": [0] * 6, "deltas": [0, 0, 0, 0, 1, 1, 0, 0, 0, 1, 1, 1], "angles": [0] * 5, "scale": [0] * 6,
                   "offset": [0, 0], "nan_rot": [2, 2, 1, 1, 0, 0, 0, 0], "inf_trans": [2, 2, 2, 2, 0, 0, 0, 0],
                   "bad_scale": [2, 2, 2, 2, 0, 0, 1, 1]}


@pytest.mark.parametrize("name", sorted(EXPECTED_STATUS))
def test_case_equals_the_restatement(ebo, cases, refs, name):
    gt, est, segs, deltas, scales = cases[name]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = c.trajectory_rpe(gt, est, segs, deltas, scales)
    assert [w["status"] for w in refs[name]] == EXPECTED_STATUS[name]
    check(name, got, refs[name])
    for g in got:
        if g["status"] != 0:
            assert all(g[f] == 0.0 for f in T.FIELDS)
    if name == "pairs":
        assert [g["count"] for g in got] == [1, 63, 64, 65, 128, 129]
    if name == "deltas":
        assert [g["count"] for g in got[:6]] == [19, 18, 13, 1, 0, 0]
    if name == "angles":
        want = [0.0, 1e-9, np.pi / 2, np.pi - 1e-9, np.pi]
        assert T.same_bits(got[0]["rot_max"], 0.0) and T.same_bits(got[4]["rot_min"], np.pi)
        assert all(abs(g["rot_mean"] - w) <= 1e-14 for g, w in zip(got, want))
    if name == "scale":
        # the third segment is the first with scale 1: a scale array of ones is the call without one
        with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
            plain = c.trajectory_rpe(gt, est, segs[:1], deltas)
        assert all(T.same_result(a, b) for a, b in zip(got[4:], plain)) and not T.same_result(got[0], plain[0])


def test_a_bad_entry_just_outside_a_segment_does_not_matter(ebo, cases):
    """The segments that border the NaN at pose 5 and the Inf at pose 6 equal the same poses of the clean arrays."""
    clean_gt, bad_est, _, _, _ = cases["nan_rot"]
    bad_gt, clean_est, _, _, _ = cases["inf_trans"]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        want = c.trajectory_rpe(clean_gt, clean_est, [(0, 5), (6, 12), (0, 6), (7, 12)], [1, 2])
        got = c.trajectory_rpe(clean_gt, bad_est, [(0, 5), (6, 12)], [1, 2]) + c.trajectory_rpe(bad_gt, clean_est, [(0, 6), (7, 12)], [1, 2])
    for g, w in zip(got, want):
        assert g["status"] == 0 and T.same_result(g, w)


def test_a_batch_of_70_equals_each_unit_alone_and_the_restatement(ebo):
    gt, est, segs, deltas, scales = T.batch70()
    want = T.rpe_units(gt, est, segs, deltas, scales)
    assert len(want) == 70 and {w["status"] for w in want} == {0, 1, 2}
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = c.trajectory_rpe(gt, est, segs, deltas, scales)
        again = c.trajectory_rpe(gt, est, segs, deltas, scales)
        alone = [c.trajectory_rpe(gt, est, [s], [d], [sc])[0] for s, sc in zip(segs, scales) for d in deltas]
    check("batch70", got, want)
    for k in range(70):
        assert T.same_result(got[k], again[k]) and T.same_result(got[k], alone[k]), k


def test_all_prefixes_of_a_trajectory_equal_single_calls(ebo):
    gt, est = T.helix(40, 5, 1e-2)
    segs = [(0, k) for k in range(6, 41)]
    deltas = [1, 3, 10]
    scales = list(np.linspace(0.5, 2.0, len(segs)))
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = c.trajectory_rpe(gt, est, segs, deltas, scales)
        single = [r for k, s in zip(range(6, 41), scales) for r in c.trajectory_rpe(gt[:k], est[:k], [(0, k)], deltas, [s])]
    assert len(got) == 105
    check("prefixes", got, T.rpe_units(gt, est, segs, deltas, scales))
    for g, s in zip(got, single):
        assert g["status"] == (1 if g["count"] == 0 else 0) and T.same_result(g, s)
    assert [g["count"] for g in got[:3]] == [5, 3, 0] and [g["count"] for g in got[-3:]] == [39, 37, 30]


def test_device_form_equals_host_form(ebo):
    import torch
    gt, est, segs, deltas, scales = T.batch70()
    d_gt = torch.from_numpy(np.ascontiguousarray(gt)).to("cuda")
    d_est = torch.from_numpy(np.ascontiguousarray(est)).to("cuda")
    torch.cuda.synchronize()
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        for sc in (scales, None):
            host = c.trajectory_rpe(gt, est, segs, deltas, sc)
            dev = c.trajectory_rpe_device(len(gt), d_gt.data_ptr(), d_est.data_ptr(), segs, deltas, sc)
            for k, (h, g) in enumerate(zip(host, dev)):
                assert T.same_result(h, g), (sc is None, k)
    assert np.array_equal(d_gt.cpu().numpy(), gt, equal_nan=True) and np.array_equal(d_est.cpu().numpy(), est, equal_nan=True)


def test_argument_errors_and_the_recording_state(ebo, cases, synth):
    import torch
    gt, est, _, _, _ = cases["offset"]
    gt, est = np.ascontiguousarray(gt), np.ascontiguousarray(est)
    n = len(gt)
    res = (ebo.RpeResult * 4)()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = ebo.lib()
    MARK = 7.25

    def stamp():
        for r in res:
            r.trans_rmse, r.rot_max, r.count, r.status = MARK, MARK, -5, -6

    def untouched():
        return all(r.trans_rmse == MARK and r.rot_max == MARK and r.count == -5 and r.status == -6 for r in res)

    def call(c, n_poses=n, gt=gt, est=est, n_seg=1, sb=(0,), se=(n,), scale=None, n_del=2, dl=(1, 2), res=res):
        sb, se, dl = np.array(sb, np.int32), np.array(se, np.int32), np.array(dl, np.int32)
        sc = np.array(scale, np.float64) if scale is not None else None
        return lib.ebo_trajectory_rpe(c._h, n_poses, vp(gt) if gt is not None else None, vp(est) if est is not None else None,
                                      n_seg, vp(sb) if len(sb) else None, vp(se) if len(se) else None,
                                      vp(sc) if sc is not None else None, n_del, vp(dl) if len(dl) else None,
                                      C.addressof(res) if res is not None else None)

    def refused(c, **kw):
        stamp()
        rc = call(c, **kw)
        return rc == ebo.ERR_ARG and untouched() and b"ebo_trajectory_rpe" in lib.ebo_last_error(c._h)

    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        assert refused(c, gt=None) and refused(c, est=None) and call(c, res=None) == ebo.ERR_ARG
        assert refused(c, sb=()) and refused(c, se=()) and refused(c, dl=())
        assert refused(c, n_poses=-1) and refused(c, n_seg=-1) and refused(c, n_seg=65536)
        assert refused(c, n_del=-1) and refused(c, n_del=17, dl=(1,) * 17)
        assert refused(c, sb=(5,), se=(4,))                                   # ends before it begins
        assert refused(c, sb=(-1,), se=(4,)) and refused(c, se=(n + 1,))      # outside [0, n_poses]
        assert refused(c, dl=(1, 0)) and refused(c, dl=(-3, 1))               # a delta below 1
        big = (1 << 24) + 1                                                   # refused before any pose is read
        assert refused(c, n_poses=big, se=(big,))                             # more than 2^24 poses in a segment
        with pytest.raises(ebo.EboError) as err:
            c.trajectory_rpe(gt, est, [(0, n), (3, n + 1)], [1])
        assert err.value.code == ebo.ERR_ARG
        with pytest.raises(ebo.EboError) as err:
            c.trajectory_rpe(gt, est, [(0, n)], [1, 0])
        assert err.value.code == ebo.ERR_ARG
        stamp()
        assert call(c) == 0 and res[0].status == 0 and res[0].count == n - 1 and res[1].count == n - 2 and res[2].count == -5
        assert call(c, sb=(n,), se=(n,)) == 0 and res[0].status == 1          # empty, at the end: allowed
        assert call(c, n_del=16, dl=(1,) * 16, res=(ebo.RpeResult * 16)()) == 0
        assert c.trajectory_rpe(gt, est, [], [1]) == [] and c.trajectory_rpe(gt, est, [(0, n)], []) == []
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
            stamp()
            codes.append(call(c))
            codes.append(0 if untouched() else -1)
            try:
                c.trajectory_rpe_device(n, 1, 1, [(0, n)], [1])
                codes.append(0)
            except ebo.EboError as e:
                codes.append(e.code)
            c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())

        g = c.record(body)
        assert codes == [ebo.ERR_STATE, 0, ebo.ERR_STATE]
        g.launch()
        c.synchronize()
        g.close()
        assert call(c) == 0


def test_the_timing_brackets_the_call(ebo, cases):
    gt, est, segs, deltas, scales = cases["pairs"]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        c.two_view_timing(True)
        c.trajectory_rpe(gt, est, segs, deltas, scales)
        ms = c.two_view_timing(False)
    assert ms[0] > 0.0 and ms[4] >= ms[0] and ms[1] == ms[2] == ms[3] == 0.0
