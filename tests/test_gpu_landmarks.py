"""GPU: ebo_triangulate_tracks and ebo_landmark_scores against tests/landmark_ref.py.  Every double of every result (the
point, the parallax, the largest score, every observation's score) is bit-equal to the restatement; status, counts,
winner and flags are equal integers.  The cases are landmark_ref.gpu_cases: observation counts 1, 2, 3, 15, 16, 17, 24,
25 (300 pairs, the last exhaustive one), 26 (sampled), 64, 65 and 512; max_hypotheses 1, 64 and 65; 1, 3, 4, 5, 63, 64,
65 and 1 000 landmarks a call; all six statuses with the expected list pinned (equal centres, two rays just below and
just above min_parallax, every observation an outlier, a point behind a camera, a zero bearing vector, a NaN in a pose
and an Inf in a bearing vector between landmarks that must not care); a scene 1e4 from the origin; a batch mixing them,
equal to each landmark alone, to a second run and to the reversed order; the audit of the triangulated points and of
the points moved by 5 % of their depth; the _device forms; the argument errors."""
import ctypes as C

import numpy as np
import pytest

import landmark_ref as L

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return L.gpu_cases()


@pytest.fixture(scope="module")
def refs(cases):
    """name -> the restatement's results; computed once, read only."""
    return {name: L.triangulate(b["poses"], b["offsets"], b["obs_pose"], b["obs_f"], prm) for name, (b, prm, _) in cases.items()}


def params(ebo, prm):
    return ebo.Context.landmark_params(**prm)


def triangulate(c, ebo, b, prm, **kw):
    return c.triangulate_tracks(b["poses"], b["offsets"], b["obs_pose"], b["obs_f"], params(ebo, prm), **kw)


def audit(c, ebo, b, points, prm, **kw):
    return c.landmark_scores(b["poses"], b["offsets"], b["obs_pose"], b["obs_f"], points, params(ebo, prm), **kw)


def test_the_defaults(ebo):
    p = ebo.Context.landmark_params()
    want = L.default_params()
    assert p.threshold == want["threshold"] and p.min_parallax == want["min_parallax"]
    assert (p.min_inliers, p.max_hypotheses, p.seed) == (2, 300, 0)
    assert C.sizeof(ebo.LandmarkResult) == 64 and C.sizeof(ebo.LandmarkParams) == 32


CASE_NAMES = ["obs_counts", "statuses", "min_inliers_3", "far"] + ["max_hypotheses_%d" % h for h in L.HYPOTHESIS_LIMITS] + \
    ["call_%d" % n for n in L.CALL_SIZES]


@pytest.mark.parametrize("name", CASE_NAMES)
def test_case_equals_the_restatement(ebo, cases, refs, name):
    b, prm, expected = cases[name]
    want = refs[name]
    if expected is not None:
        assert want["status"].tolist() == expected
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = triangulate(c, ebo, b, prm)
    assert L.mismatch(got, want) is None
    bad = got["status"] != 0
    assert not got["point"][bad].any()
    if name == "obs_counts":
        assert got["n_obs"].tolist() == list(L.OBS_COUNTS)
        # 25 observations are the last exhaustive count at the default limit, 26 the first sampled one
        assert got["hypotheses"].tolist() == [0, 1, 3, 105, 120, 136, 276, 300, 300, 300, 300, 300]
    if name.startswith("max_hypotheses_"):
        limit = prm["max_hypotheses"]
        assert got["hypotheses"].tolist() == [min(m * (m - 1) // 2, limit) for m in (5, 11, 12, 13, 24, 40)]
    if name == "statuses":
        assert set(got["status"].tolist()) == {0, 1, 2, 3, 4}
    if name == "min_inliers_3":
        assert got["status"][0] == 5 and got["n_inliers"][0] == 2 and got["parallax"][0] > 0.0 and got["winner"][0] == 0


def test_the_neighbours_of_a_nan_and_an_inf_do_not_care(ebo, cases):
    """Landmarks 8 .. 12 of the status batch are good, NaN pose, good, Inf bearing, good: the good ones equal themselves
    in a call without the bad ones."""
    b, prm, expected = cases["statuses"]
    assert expected[8:13] == [0, 2, 0, 2, 0]
    clean, _ = L.select(b, [8, 10, 12])
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = triangulate(c, ebo, b, prm)
        alone = triangulate(c, ebo, clean, prm)
    for i, l in enumerate((8, 10, 12)):
        assert got["status"][l] == 0 and L.same_bits(got["point"][l], alone["point"][i])
        assert L.same_bits(got["parallax"][l], alone["parallax"][i]) and got["n_inliers"][l] == alone["n_inliers"][i]


def test_the_mixed_batch_equals_each_landmark_alone_a_second_run_and_the_reversed_order(ebo, cases, refs):
    b, prm, _ = cases["mixed"]
    want = refs["mixed"]
    n = len(b["offsets"]) - 1
    assert set(want["status"].tolist()) == {0, 1, 2, 3, 4}
    order = list(range(n - 1, -1, -1))
    rev, flat = L.select(b, order)
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = triangulate(c, ebo, b, prm)
        again = triangulate(c, ebo, b, prm)
        back = triangulate(c, ebo, rev, prm)
        alone = [triangulate(c, ebo, L.select(b, [l])[0], prm) for l in range(0, n, 7)]
    assert L.mismatch(got, want) is None
    assert L.mismatch(again, got) is None
    for k in L.RESULT_DOUBLES + L.RESULT_INTS:
        assert L.same_bits(back[k].astype(np.float64), got[k][order].astype(np.float64)), k
    assert L.same_bits(back["scores"], got["scores"][flat]) and np.array_equal(back["flags"], got["flags"][flat])
    for a, l in zip(alone, range(0, n, 7)):
        for k in L.RESULT_DOUBLES + L.RESULT_INTS:
            assert L.same_bits(np.asarray(a[k][0], np.float64), np.asarray(got[k][l], np.float64)), (l, k)


def test_the_planted_outliers_are_the_ones_flagged(ebo):
    """Scenes of the builder the CPU suite checks 200 seeds of: the device lists exactly the planted outliers."""
    tracks = [L.make_track(7000 + s, m, n_out, off) for s, (m, n_out, off) in
              enumerate([(4, 1, 6.0), (4, 2, 6.0), (5, 2, 40.0), (8, 2, 6.0), (12, 1, 40.0), (24, 2, 6.0)])]
    b = L.concat([dict(poses=P, offsets=np.array([0, len(f)], np.int32), obs_pose=np.arange(len(f), dtype=np.int32), obs_f=f)
                  for P, f, _, _ in tracks])
    planted = np.concatenate([t[2] for t in tracks])
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = triangulate(c, ebo, b, L.default_params())
    assert np.all(got["status"] == 0) and np.array_equal(got["flags"] == 0, planted)


@pytest.mark.parametrize("name", ["call_65", "statuses", "obs_counts", "far"])
def test_the_audit_equals_the_restatement(ebo, cases, refs, name):
    b, prm, _ = cases[name]
    tri = refs[name]
    ok = tri["status"] == 0
    points = np.where(ok[:, None], tri["point"], 1.0)
    moved = L.moved_points(b, points)
    want = L.audit(b["poses"], b["offsets"], b["obs_pose"], b["obs_f"], points, prm)
    want_moved = L.audit(b["poses"], b["offsets"], b["obs_pose"], b["obs_f"], moved, prm)
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = audit(c, ebo, b, points, prm)
        got_moved = audit(c, ebo, b, moved, prm)
    assert L.mismatch(got, want) is None and L.mismatch(got_moved, want_moved) is None
    # what was triangulated is kept with the same flags; what moved by 5 % of its depth is culled
    assert np.all(got["status"][ok] == 0) and L.same_bits(got["point"][ok], tri["point"][ok])
    off = b["offsets"]
    for l in np.flatnonzero(ok):
        assert np.array_equal(got["flags"][off[l]:off[l + 1]], tri["flags"][off[l]:off[l + 1]])
    assert np.all(got_moved["status"][ok] != 0) and not got_moved["point"].any()


def test_scores_and_flags_may_be_left_out(ebo, cases, refs):
    b, prm, _ = cases["call_5"]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = triangulate(c, ebo, b, prm, scores=False, flags=False)
        only_flags = audit(c, ebo, b, refs["call_5"]["point"], prm, scores=False)
    assert "scores" not in got and "flags" not in got and L.mismatch(got, refs["call_5"], per_observation=False) is None
    assert np.array_equal(only_flags["flags"], refs["call_5"]["flags"])


def test_the_device_forms(ebo, cases, refs):
    torch = pytest.importorskip("torch")
    b, prm, _ = cases["mixed"]
    want = refs["mixed"]
    n, total = len(b["offsets"]) - 1, int(b["offsets"][-1])
    points = np.where(want["status"][:, None] == 0, want["point"], 1.0)
    want_audit = L.audit(b["poses"], b["offsets"], b["obs_pose"], b["obs_f"], points, prm)
    # a pose index out of range cannot be refused by a call that cannot look: that landmark alone gets status 2
    idx = b["obs_pose"].copy()
    victim = int(np.flatnonzero(want["status"] == 0)[3])
    idx[b["offsets"][victim] + 1] = len(b["poses"]) + 5
    dev = [torch.from_numpy(np.ascontiguousarray(a)).to("cuda") for a in (b["poses"], b["obs_pose"], b["obs_f"], points, idx)]
    d_res = torch.zeros(64 * n, dtype=torch.uint8, device="cuda")
    d_scores = torch.full((total,), 7.25, dtype=torch.float64, device="cuda")
    d_flags = torch.full((total,), 9, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        p = params(ebo, prm)
        c.triangulate_tracks_device(len(b["poses"]), dev[0].data_ptr(), b["offsets"], dev[1].data_ptr(), dev[2].data_ptr(),
                                    d_res.data_ptr(), p, d_scores.data_ptr(), d_flags.data_ptr())
        c.synchronize()
        got = ebo.Context.landmark_results(d_res.cpu().numpy())
        got.update(scores=d_scores.cpu().numpy(), flags=d_flags.cpu().numpy())
        assert L.mismatch(got, want) is None
        c.landmark_scores_device(len(b["poses"]), dev[0].data_ptr(), b["offsets"], dev[1].data_ptr(), dev[2].data_ptr(),
                                 dev[3].data_ptr(), d_res.data_ptr(), p)
        c.synchronize()
        assert L.mismatch(ebo.Context.landmark_results(d_res.cpu().numpy()), want_audit, per_observation=False) is None
        c.triangulate_tracks_device(len(b["poses"]), dev[0].data_ptr(), b["offsets"], dev[4].data_ptr(), dev[2].data_ptr(),
                                    d_res.data_ptr(), p)
        c.synchronize()
        out = ebo.Context.landmark_results(d_res.cpu().numpy())
    assert out["status"][victim] == 2 and not out["point"][victim].any()
    others = np.arange(n) != victim
    assert np.array_equal(out["status"][others], want["status"][others]) and L.same_bits(out["point"][others], want["point"][others])
    for d, a in zip(dev, (b["poses"], b["obs_pose"], b["obs_f"], points, idx)):
        assert np.array_equal(d.cpu().numpy(), a, equal_nan=True)


def test_argument_errors(ebo, synth, cases):
    torch = pytest.importorskip("torch")
    b, prm, _ = cases["call_5"]
    points = np.zeros((5, 3))

    def code(fn):
        try:
            fn()
            return 0
        except ebo.EboError as e:
            return e.code

    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        def tri(batch=b, **kw):
            return code(lambda: triangulate(c, ebo, batch, dict(prm, **kw)))

        def changed(**kw):
            return dict(b, **kw)

        assert tri() == 0
        for bad in (dict(threshold=0.0), dict(threshold=1.0), dict(threshold=float("nan")), dict(min_parallax=-1e-9),
                    dict(min_parallax=float("nan")), dict(min_inliers=1), dict(max_hypotheses=0), dict(max_hypotheses=4097)):
            assert tri(**bad) == ebo.ERR_ARG, bad
            assert code(lambda: audit(c, ebo, b, points, dict(prm, **bad))) == ebo.ERR_ARG, bad
        assert tri(max_hypotheses=4096, min_parallax=0.0) == 0
        off = b["offsets"].copy()
        off[0] = 1
        assert tri(changed(offsets=off)) == ebo.ERR_ARG
        off = b["offsets"].copy()
        off[2], off[3] = off[3], off[2] - 1
        assert tri(changed(offsets=off)) == ebo.ERR_ARG
        idx = b["obs_pose"].copy()
        idx[3] = len(b["poses"])
        assert tri(changed(obs_pose=idx)) == ebo.ERR_ARG
        idx[3] = -1
        assert tri(changed(obs_pose=idx)) == ebo.ERR_ARG
        # 513 observations in one landmark; 2^20 + 1 landmarks
        big = dict(poses=b["poses"], offsets=np.array([0, 513], np.int32), obs_pose=np.zeros(513, np.int32), obs_f=np.ones((513, 3)))
        assert tri(big) == ebo.ERR_ARG
        many = dict(poses=b["poses"], offsets=np.zeros((1 << 20) + 2, np.int32), obs_pose=np.zeros(0, np.int32), obs_f=np.zeros((0, 3)))
        assert tri(many) == ebo.ERR_ARG
        # needed pointers
        p = params(ebo, prm)
        res = (ebo.LandmarkResult * 5)()
        lib = ebo.lib()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        poses, f = np.ascontiguousarray(b["poses"]), np.ascontiguousarray(b["obs_f"])
        full = [c._h, len(poses), vp(poses), 5, vp(b["offsets"]), vp(b["obs_pose"]), vp(f), C.byref(p), C.addressof(res), None, None]
        assert lib.ebo_triangulate_tracks(*full) == 0
        for k in (2, 4, 5, 6, 7, 8):
            args = list(full)
            args[k] = None
            assert lib.ebo_triangulate_tracks(*args) == ebo.ERR_ARG, k
        assert lib.ebo_landmark_scores(*(full[:7] + [None] + full[7:])) == ebo.ERR_ARG
        assert lib.ebo_triangulate_tracks(None, *full[1:]) == ebo.ERR_ARG
        # no landmarks is no work
        empty = dict(poses=b["poses"], offsets=np.zeros(1, np.int32), obs_pose=np.zeros(0, np.int32), obs_f=np.zeros((0, 3)))
        assert tri(empty) == 0
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
            codes.append(tri())
            codes.append(code(lambda: audit(c, ebo, b, points, prm)))
            codes.append(code(lambda: c.triangulate_tracks_device(len(poses), 1, b["offsets"], 1, 1, 1, p)))
            codes.append(code(lambda: c.landmark_scores_device(len(poses), 1, b["offsets"], 1, 1, 1, 1, p)))
            c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())

        g = c.record(body)
        assert codes == [ebo.ERR_STATE] * 4
        g.launch()
        c.synchronize()
        g.close()
        assert tri() == 0


@pytest.mark.parametrize("lanes", ["16", "64"])
def test_the_bits_do_not_depend_on_the_lanes_per_landmark(ebo_ab, monkeypatch, cases, refs, lanes):
    """The A/B build takes the lanes per landmark from the environment where the call allows both (no landmark above
    128 observations): a wave per landmark and four landmarks per wave give the restatement's bits alike."""
    monkeypatch.setenv("EBO_LANDMARK_LANES", lanes)
    with ebo_ab.Context(loss=ebo_ab.LOSS_VARIANCE) as c:
        for name in ("call_65", "statuses", "max_hypotheses_65", "far"):
            b, prm, _ = cases[name]
            want = refs[name]
            assert L.mismatch(triangulate(c, ebo_ab, b, prm), want) is None, name
            points = np.where(want["status"][:, None] == 0, want["point"], 1.0)
            assert L.mismatch(audit(c, ebo_ab, b, points, prm),
                              L.audit(b["poses"], b["offsets"], b["obs_pose"], b["obs_f"], points, prm)) is None, name
