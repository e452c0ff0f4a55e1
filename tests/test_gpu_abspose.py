"""GPU: absolute pose on the device against tests/abspose_ref.py -- scores and flags bit for bit, the sampler as equal
integers, every hypothesis's pose within the restatement's own A3-vs-LAPACK difference x 10 (bit equality counted and
printed), "no model" marked where the restatement marks it, and the inlier counts, winner, iterations and inlier lists
as equal integers (test_abspose_cpu.py checks on the CPU that no restatement score of these frames lies within 1e-6
relative of the threshold, which is what makes that fair)."""
import numpy as np
import pytest

import abspose_ref as ap
import twoview_ref as tv

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """Bit equality, a NaN matching a NaN whatever its sign and payload (which are not part of any rule)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def params(ebo, **kw):
    kw.setdefault("threshold", ap.THRESHOLD)
    kw.setdefault("seed", ap.RANSAC_SEED)
    return ebo.two_view_params(**kw)


@pytest.fixture(scope="module")
def ref_runs():
    """The restatement's RANSAC on the four scenes, frame index = scene index, 1000 hypotheses."""
    out = []
    for i in range(len(ap.SCENES)):
        sc = ap.scene(i)
        out.append((sc, ap.ransac(sc["f"], sc["points"], seed=ap.RANSAC_SEED, frame=i)))
    return out


@pytest.fixture(scope="module")
def batch_runs():
    """The six frames of the batched call (one of 3 points, one of exactly 4), frame index = position."""
    out = []
    for k, n in enumerate(ap.BATCH_SIZES):
        sc = ap.make_scene(200 + k, n=n, outliers=0.2, noise_px=0.3)
        out.append((sc, ap.ransac(sc["f"], sc["points"], seed=ap.RANSAC_SEED, frame=k)))
    return out


@pytest.mark.parametrize("n", ap.SCORE_SIZES)
def test_scores_and_flags_are_bit_equal(ebo, n):
    """The truth, the restatement's winner and random poses; host and _device form."""
    import torch
    sc = ap.make_scene(100 + n, n=n, outliers=0.2, noise_px=0.3)
    f, p = sc["f"], sc["points"]
    poses = [sc["pose"]] + list(tv.random_motions(13, 4, angle=1.0, dist=3.0))
    if n >= 4:
        poses.insert(1, ap.ransac(f, p, seed=1, max_iterations=30)["model"])
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        d_f, d_p = torch.from_numpy(f).to("cuda"), torch.from_numpy(p).to("cuda")
        d_s = torch.zeros(n, dtype=torch.float64, device="cuda")
        d_fl = torch.zeros(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        for k, pose in enumerate(poses):
            want = ap.scores(pose, f, p)
            got, flags = c.absolute_pose_scores(pose, f, p, ap.THRESHOLD)
            assert same(got, want), (k, int((bits(got) != bits(want)).sum()))
            assert np.array_equal(flags, ap.inliers(want)), k
            c.absolute_pose_scores_device(pose, n, d_f.data_ptr(), d_p.data_ptr(), ap.THRESHOLD, d_s.data_ptr(), d_fl.data_ptr())
            c.synchronize()
            assert same(d_s.cpu().numpy(), want), k
            assert np.array_equal(d_fl.cpu().numpy().astype(bool), ap.inliers(want)), k
        assert ap.inliers(ap.scores(sc["pose"], f, p)).sum() >= int(0.7 * n)   # the truth has its inliers
        got, flags = c.absolute_pose_scores(sc["pose"], f[:0], p[:0], ap.THRESHOLD)
        assert len(got) == 0 and len(flags) == 0


@pytest.mark.parametrize("n", [4, 5, 64, 65, 1025, 65535])
def test_samples_are_equal_integers(ebo, n):
    sc = ap.make_scene(300 + n % 1000, n=n, outliers=0.0, noise_px=0.3)
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        _, diag = c.absolute_pose_ransac([0, 0, n], sc["f"], sc["points"], params(ebo, seed=1234), diagnostics=True)
    assert diag["samples"].shape == (2, 1000, 4)
    assert np.array_equal(diag["samples"][1], ap.samples(1234, 1, np.arange(1000), n))
    assert not diag["samples"][0].any()


def test_hypothesis_models_within_the_restatements_own_error(ebo, ref_runs):
    """Per scene the bound is 10 x the largest per-entry difference between the restatement's A3 and the independent
    LAPACK-based solve of the same samples, over the hypotheses for which both have a model."""
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        for i, (sc, run) in enumerate(ref_runs):
            n = len(sc["f"])
            # the frame index enters the sampler: put the scene at frame i behind i empty frames
            _, diag = c.absolute_pose_ransac([0] * (i + 1) + [n], sc["f"], sc["points"], params(ebo), diagnostics=True)
            got = diag["models"][i]
            assert np.array_equal(diag["samples"][i], run["samples"])
            lap, lap_ok = ap.solve_samples_lapack(sc["f"][run["samples"]], sc["points"][run["samples"]])
            both = lap_ok & run["valid"]
            bound = 10.0 * float(np.abs(lap[both] - run["models"][both]).max())
            got_valid = np.abs(np.nan_to_num(got, nan=1.0)).reshape(len(got), -1).max(axis=1) > 0
            diff = float(np.abs(got - run["models"]).max())
            equal = int((bits(got) == bits(run["models"])).reshape(len(got), -1).all(axis=1).sum())
            print("scene %d: %d of %d models bit-equal, %d with a model, max |device - restatement| = %.3g, bound %.3g" % (
                i, equal, len(got), int(run["valid"].sum()), diff, bound))
            assert np.array_equal(got_valid, run["valid"])
            assert diff <= bound


def test_no_model_is_marked_so_on_the_device(ebo):
    """Collinear and coincident landmarks, zero and NaN bearings, infinite landmarks: a hypothesis the restatement
    marks "no model" is an all-zero pose with a zero count on the device."""
    sc = ap.make_scene(60, n=60, outliers=0.2, noise_px=0.3)
    f, p = sc["f"], sc["points"]
    line = p.copy()
    line[:40] = np.outer(np.arange(40.0), [1.0, 2.0, 0.5]) + [0.0, 0.0, 3.0]
    twin = p.copy()
    twin[:45] = p[0]
    zero = f.copy()
    zero[::3] = 0.0
    bad_f, bad_p = f.copy(), p.copy()
    bad_f[3::11, 1] = np.nan
    bad_p[5::13] = np.inf
    fd, pd = ap.degenerate_samples()
    cases = {"collinear landmarks": (f, line), "coincident landmarks": (f, twin), "zero bearings": (zero, p),
             "NaN and infinity": (bad_f, bad_p), "all zero": (np.zeros((20, 3)), np.zeros((20, 3))),
             "four collinear": (fd[0], pd[0]), "four with a twin": (fd[1], pd[1])}
    seen_invalid = 0
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        for name, (a, b) in cases.items():
            _, diag = c.absolute_pose_ransac([0, len(a)], a, b, params(ebo, seed=5, max_iterations=200), diagnostics=True)
            ref = ap.ransac(a, b, seed=5, frame=0, max_iterations=200)
            assert np.isfinite(diag["models"]).all(), name
            got_valid = np.abs(diag["models"][0]).reshape(200, -1).max(axis=1) > 0
            print("%s: the restatement marks %d of 200 hypotheses 'no model', the device %d" % (
                name, int((~ref["valid"]).sum()), int((~got_valid).sum())))
            assert np.array_equal(got_valid, ref["valid"]), name
            assert not diag["counts"][0][~ref["valid"]].any()
            seen_invalid += int((~ref["valid"]).sum())
    assert seen_invalid > 0


@pytest.mark.parametrize("max_iterations", [1, 50, 1000])
def test_counts_winner_and_inliers_are_equal_integers(ebo, ref_runs, batch_runs, max_iterations):
    """Alone, as one call of six frames of different sizes, and run to run."""
    prm = params(ebo, max_iterations=max_iterations)
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        for runs in (ref_runs, batch_runs):
            f = np.concatenate([sc["f"] for sc, _ in runs])
            p = np.concatenate([sc["points"] for sc, _ in runs])
            offsets = np.concatenate([[0], np.cumsum([len(sc["f"]) for sc, _ in runs])])
            batched, bdiag = c.absolute_pose_ransac(offsets, f, p, prm, diagnostics=True)
            again, adiag = c.absolute_pose_ransac(offsets, f, p, prm, diagnostics=True)
            plain = c.absolute_pose_ransac(offsets, f, p, prm)
            for i, (sc, run) in enumerate(runs):
                n = len(sc["f"])
                alone, diag = c.absolute_pose_ransac([0] * (i + 1) + [n], sc["f"], sc["points"], prm, diagnostics=True)
                if n < 4:
                    for r in (batched[i], again[i], alone[i], plain[i]):
                        assert (r["found"], r["winner"], r["iterations"], r["n_inliers"]) == (False, -1, 0, 0)
                        assert len(r["inliers"]) == 0 and not r["model"].any()
                    assert not bdiag["counts"][i].any() and not bdiag["models"][i].any()
                    continue
                counts = run["counts"][:max_iterations]
                found, winner, iterations, best = ap.ransac_walk(counts, n, ap.PROBABILITY, max_iterations)
                want_inl = np.flatnonzero(ap.inliers(run["scores"][winner]) & run["valid"][winner])
                for name, r, d in (("batched", batched[i], bdiag), ("again", again[i], adiag), ("alone", alone[i], diag)):
                    nd = int((d["counts"][i] != counts).sum())
                    print("n=%d H=%d %s: %d counts differ; winner %d/%d iterations %d/%d inliers %d/%d" % (
                        n, max_iterations, name, nd, r["winner"], winner, r["iterations"], iterations, r["n_inliers"], best))
                    assert nd == 0
                    assert (r["found"], r["winner"], r["iterations"], r["n_inliers"]) == (found, winner, iterations, best)
                    assert np.array_equal(r["inliers"], want_inl)
                assert same(alone[i]["model"], batched[i]["model"])
                assert same(bdiag["models"][i], diag["models"][i])
                assert same(bdiag["models"][i], adiag["models"][i])
                assert same(batched[i]["model"], bdiag["models"][i][winner])
                assert np.array_equal(plain[i]["inliers"], want_inl) and plain[i]["winner"] == winner


def test_counts_where_a_frame_spans_several_tiles(ebo):
    """The counting kernel stages a frame in tiles of 1024 points, one workgroup per (tile, 8 hypotheses), all of them
    adding into the frame's counts: frames of 1023, 1024, 1025 and 2049 points (one tile less one, one exactly, a second
    tile of one, a third of one) and one of 3 (below the sample) in one call of 16 hypotheses.  The yardstick is the
    restatement's score of every point under the DEVICE's own pose of each hypothesis: the per-point scores are
    bit-equal to it (test_scores_and_flags_are_bit_equal), so the counts are equal integers with no allowance near the
    threshold and without the restatement's hypothesis solver."""
    sizes, H = (1023, 1024, 3, 1025, 2049), 16
    scenes = [ap.make_scene(400 + k, n=n, outliers=0.2, noise_px=0.3) for k, n in enumerate(sizes)]
    f = np.concatenate([sc["f"] for sc in scenes])
    p = np.concatenate([sc["points"] for sc in scenes])
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    prm = params(ebo, max_iterations=H)
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        res, diag = c.absolute_pose_ransac(offsets, f, p, prm, diagnostics=True)
        again, adiag = c.absolute_pose_ransac(offsets, f, p, prm, diagnostics=True)
    beyond_first_tile = 0
    for i, (sc, n) in enumerate(zip(scenes, sizes)):
        models, counts, r = diag["models"][i], diag["counts"][i], res[i]
        valid = np.abs(np.nan_to_num(models, nan=1.0)).reshape(H, -1).max(axis=1) > 0
        assert np.array_equal(counts, adiag["counts"][i]) and same(models, adiag["models"][i])
        assert (r["found"], r["winner"], r["iterations"], r["n_inliers"]) == (
            again[i]["found"], again[i]["winner"], again[i]["iterations"], again[i]["n_inliers"])
        assert np.array_equal(r["inliers"], again[i]["inliers"])
        if n < 4:
            assert not valid.any() and not counts.any()
            assert (r["found"], r["winner"], r["iterations"], r["n_inliers"]) == (False, -1, 0, 0) and len(r["inliers"]) == 0
            continue
        inl = ap.inliers(ap.scores(models, sc["f"], sc["points"])) & valid[:, None]
        want = inl.sum(axis=1).astype(np.int32)
        print("n=%d: %d valid hypotheses, device counts %s, restatement under the device's poses %s" % (
            n, int(valid.sum()), counts.tolist(), want.tolist()))
        assert valid.any()
        assert np.array_equal(counts, want)
        assert not counts[~valid].any()
        have = bool(np.abs(np.nan_to_num(r["model"], nan=1.0)).max() > 0)
        want_inl = np.flatnonzero(ap.inliers(ap.scores(r["model"], sc["f"], sc["points"]))) if have else np.zeros(0, dtype=np.int64)
        assert np.array_equal(r["inliers"], want_inl) and r["n_inliers"] == len(want_inl)
        assert r["n_inliers"] == counts[r["winner"]] and same(r["model"], models[r["winner"]])
        beyond_first_tile += int((inl[:, 1024:]).sum())
    assert beyond_first_tile > 0   # otherwise the later tiles added nothing and this test shows nothing


def test_device_form_matches_host_form(ebo, ref_runs):
    import torch
    sc, run = ref_runs[2]
    prm = params(ebo)
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        host = c.absolute_pose_ransac([0, 0, 0, 200], sc["f"], sc["points"], prm)[2]
        d_f, d_p = torch.from_numpy(sc["f"]).to("cuda"), torch.from_numpy(sc["points"]).to("cuda")
        torch.cuda.synchronize()
        dev = c.absolute_pose_ransac([0, 0, 0, 200], d_f.data_ptr(), d_p.data_ptr(), prm, device=True)[2]
    assert (host["found"], host["winner"], host["iterations"]) == (dev["found"], dev["winner"], dev["iterations"])
    assert np.array_equal(host["inliers"], dev["inliers"]) and same(host["model"], dev["model"])
    assert host["winner"] == run["winner"] and same(host["model"], run["model"])
    # the pose found is the scene's, to the accuracy 0.3 pixels of noise allow
    assert np.abs(host["model"] - sc["pose"]).max() < 0.05


def test_timing_reports_five_phases(ebo, ref_runs):
    sc, run = ref_runs[0]
    prm = params(ebo)
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        plain = c.absolute_pose_ransac([0, 200], sc["f"], sc["points"], prm)[0]
        assert c.two_view_timing(True) == (0.0,) * 5
        timed = c.absolute_pose_ransac([0, 200], sc["f"], sc["points"], prm)[0]
        ms = c.two_view_timing(False)
        print("phases [ms]: hypotheses %.4f, counting %.4f, host walk %.4f, inlier list %.4f, call %.4f" % ms)
        assert all(np.isfinite(v) and v >= 0.0 for v in ms)
        assert ms[0] > 0.0 and ms[1] > 0.0 and ms[4] > 0.0
        assert ms[0] + ms[1] + ms[2] + ms[3] <= ms[4] * 1.05
        again = c.absolute_pose_ransac([0, 200], sc["f"], sc["points"], prm)[0]
        assert c.two_view_timing(False) == ms
    for r in (timed, again):
        assert (r["winner"], r["iterations"]) == (plain["winner"], plain["iterations"]) and same(r["model"], plain["model"])
        assert np.array_equal(r["inliers"], plain["inliers"])


def test_edge_cases_are_statuses_never_faults(ebo, synth, ref_runs):
    import torch
    sc, _ = ref_runs[0]
    f, p = sc["f"], sc["points"]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        assert c.absolute_pose_ransac([0], np.zeros((0, 3)), np.zeros((0, 3)), params(ebo)) == []
        for n in (0, 3):
            r = c.absolute_pose_ransac([0, n], f[:n], p[:n], params(ebo))[0]
            assert (r["found"], r["winner"], r["iterations"], r["n_inliers"]) == (False, -1, 0, 0)
        # n = 4: every hypothesis draws all four
        r4, d4 = c.absolute_pose_ransac([0, 4], f[:4], p[:4], params(ebo, seed=3, max_iterations=20), diagnostics=True)
        assert np.array_equal(np.sort(d4["samples"][0], axis=1), np.tile(np.arange(4), (20, 1)))
        assert np.array_equal(d4["samples"][0], ap.samples(3, 0, np.arange(20), 4))
        for kw in (dict(max_iterations=0), dict(max_iterations=4097), dict(probability=0.0), dict(probability=1.0),
                   dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan"))):
            with pytest.raises(ebo.EboError) as ei:
                c.absolute_pose_ransac([0, 200], f, p, params(ebo, **kw))
            assert ei.value.code == ebo.ERR_ARG, kw
        big = np.ones((65536, 3))
        for offsets, a, b in (([0, 65536], big, big), ([0, 100, 50, 200], f, p), ([1, 200], f, p)):
            with pytest.raises(ebo.EboError) as ei:
                c.absolute_pose_ransac(offsets, a, b, params(ebo))
            assert ei.value.code == ebo.ERR_ARG, offsets
        with pytest.raises(ebo.EboError) as ei:
            c.absolute_pose_ransac(np.zeros(65537 + 1, dtype=np.int32), np.zeros((0, 3)), np.zeros((0, 3)), params(ebo))
        assert ei.value.code == ebo.ERR_ARG
        lib = ebo.lib()
        prm = params(ebo)
        import ctypes as C
        res = (ebo.TwoViewResult * 1)()
        off = np.array([0, 200], dtype=np.int32)
        idx = np.zeros(200, dtype=np.int32)
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        for args in ((None, vp(f), vp(p), C.byref(prm), res, vp(idx)), (vp(off), None, vp(p), C.byref(prm), res, vp(idx)),
                     (vp(off), vp(f), None, C.byref(prm), res, vp(idx)), (vp(off), vp(f), vp(p), None, res, vp(idx)),
                     (vp(off), vp(f), vp(p), C.byref(prm), None, vp(idx)), (vp(off), vp(f), vp(p), C.byref(prm), res, None)):
            assert lib.ebo_absolute_pose_ransac(c._h, 1, *args, None, None, None) == ebo.ERR_ARG
        assert lib.ebo_absolute_pose_scores(c._h, None, 200, vp(f), vp(p), C.c_double(1e-4), None, None) == ebo.ERR_ARG
        assert lib.ebo_absolute_pose_scores(c._h, vp(sc["pose"]), -1, vp(f), vp(p), C.c_double(1e-4), None, None) == ebo.ERR_ARG
        # while a graph records: refused, and the recording survives
        ev, gt = synth.make_window(0, n_events=3000)
        c.set_window(ev)
        d_flows = torch.zeros((c.P, 2), dtype=torch.float64, device="cuda")
        d_out = torch.zeros(3 * c.P, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())
        c.synchronize()
        codes = []

        def body():
            for call in (lambda: c.absolute_pose_ransac([0, 200], f, p, params(ebo)),
                         lambda: c.absolute_pose_scores(sc["pose"], f, p, 1e-4),
                         lambda: c.absolute_pose_scores_device(sc["pose"], 0, 0, 0, 1e-4)):
                try:
                    call()
                    codes.append(0)
                except ebo.EboError as e:
                    codes.append(e.code)
            c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())

        g = c.record(body)
        assert codes == [ebo.ERR_STATE] * 3
        g.launch()
        c.synchronize()
        g.close()
        assert c.absolute_pose_ransac([0, 200], f, p, params(ebo))[0]["found"]
