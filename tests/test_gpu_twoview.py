"""GPU: two-view geometry on the device against tests/twoview_ref.py -- the per-point closed forms bit for bit, the
sampler as equal integers, every hypothesis's model within the restatement's own Jacobi-vs-LAPACK error x 10, and the
inlier counts, winner, iterations and inlier lists as equal integers (test_twoview_cpu.py checks on the CPU that no
restatement score of these scenes lies within 1e-6 relative of the threshold, which is what makes that fair)."""
import numpy as np
import pytest

import twoview_ref as tv

pytestmark = pytest.mark.gpu


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """Bit equality, a NaN matching a NaN whatever its sign and payload (which are not part of any rule)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


def random_bearings(seed, n):
    rng = np.random.default_rng(seed)
    f = rng.normal(size=(n, 3))
    f[:, 2] = np.abs(f[:, 2]) + 0.5
    return f / np.linalg.norm(f, axis=1)[:, None]


@pytest.fixture(scope="module")
def ref_runs():
    """The restatement's RANSAC on the five scenes, pair index = scene index, 1000 hypotheses."""
    out = []
    for i in range(len(tv.SCENES)):
        sc = tv.scene(i)
        out.append((sc, tv.ransac(sc["f1"], sc["f2"], seed=tv.RANSAC_SEED, pair=i)))
    return out


def given_models(ref_runs):
    sc, run = ref_runs[0]
    gt = sc["model"]
    return [gt, run["model"]] + list(tv.random_motions(11, 100))


def test_per_point_forms_are_bit_equal(ebo, ref_runs):
    """check 6: scores, triangulation and the epipolar test for given models on 10^5 random correspondences, host and
    _device forms, and the small / odd sizes."""
    import torch
    n = 100_000
    f1, f2 = random_bearings(21, n), random_bearings(22, n)
    sc0 = ref_runs[0][0]
    f1[:200], f2[:200] = sc0["f1"], sc0["f2"]
    models = given_models(ref_runs)
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        d_f1, d_f2 = torch.from_numpy(f1).to("cuda"), torch.from_numpy(f2).to("cuda")
        d_s = torch.zeros(n, dtype=torch.float64, device="cuda")
        d_fl = torch.zeros(n, dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        worst = 0
        for k, m in enumerate(models):
            m_n = n
            want = tv.scores(m, f1[:m_n], f2[:m_n])
            got, flags = c.relative_pose_scores(m, f1[:m_n], f2[:m_n], tv.THRESHOLD)
            nd = int(((bits(got) != bits(want)) & ~(np.isnan(got) & np.isnan(want))).sum())
            worst = max(worst, nd)
            assert nd == 0, (k, nd)
            assert np.array_equal(flags, tv.inliers(want))
            c.relative_pose_scores_device(m, m_n, d_f1.data_ptr(), d_f2.data_ptr(), tv.THRESHOLD, d_s.data_ptr(), d_fl.data_ptr())
            c.synchronize()
            assert same(d_s.cpu().numpy()[:m_n], want)
            assert np.array_equal(d_fl.cpu().numpy()[:m_n].astype(bool), tv.inliers(want))
            thr = 1e-3
            wantE = tv.epipolar_residual(m, f1[:m_n], f2[:m_n]) < thr
            assert np.array_equal(c.epipolar_inliers(m, f1[:m_n], f2[:m_n], thr), wantE), k
        print("scores: %d models, worst differing words %d" % (len(models), worst))
        # triangulation: a pose pair per point over 102 poses
        poses = np.concatenate([np.hstack([np.eye(3), np.zeros((3, 1))])[None], models[0][None], tv.random_motions(12, 100)])
        rng = np.random.default_rng(23)
        pp = rng.integers(0, len(poses), size=(n, 2)).astype(np.int32)
        want = tv.triangulate(poses, pp, f1, f2)
        got = c.triangulate(poses, pp, f1, f2)
        print("triangulate: %d of %d points differ" % (int((bits(got) != bits(want)).any(axis=1).sum()), n))
        assert same(got, want)
        d_p = torch.from_numpy(poses).to("cuda")
        d_pp = torch.from_numpy(pp).to("cuda")
        d_out = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        c.triangulate_device(len(poses), d_p.data_ptr(), n, d_pp.data_ptr(), d_f1.data_ptr(), d_f2.data_ptr(), d_out.data_ptr())
        c.synchronize()
        assert same(d_out.cpu().numpy(), want)
        for m_n in (0, 1, 3, 257, 1000):
            got, flags = c.relative_pose_scores(models[0], f1[:m_n], f2[:m_n], tv.THRESHOLD)
            assert same(got, tv.scores(models[0], f1[:m_n], f2[:m_n]))
            assert len(flags) == m_n
            assert same(c.triangulate(poses, pp[:m_n], f1[:m_n], f2[:m_n]), want[:m_n])
            assert len(c.epipolar_inliers(models[0], f1[:m_n], f2[:m_n], 1e-3)) == m_n
        with pytest.raises(ebo.EboError) as ei:
            c.triangulate(poses, [[0, len(poses)]], f1[:1], f2[:1])
        assert ei.value.code == ebo.ERR_ARG


def test_known_answer_of_the_reference_triangulation_test(ebo):
    """check 1 on the device: identity, 90 degrees about z with t = (1, -1, 0), both bearings (1, 0, 0) -> (1, 0, 0)."""
    poses = np.zeros((2, 3, 4))
    poses[0, :, :3] = np.eye(3)
    poses[1, :, :3] = tv.rotation_about([0, 0, 1], np.pi / 2)
    poses[1, :, 3] = [1.0, -1.0, 0.0]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        p = c.triangulate(poses, [[0, 1]], [[1.0, 0, 0]], [[1.0, 0, 0]])
    assert np.all(np.abs(p[0] - [1, 0, 0]) <= 4 * np.spacing(np.float32(1.0)))


@pytest.mark.parametrize("n", [8, 9, 75, 200, 500, 65535])
def test_samples_are_equal_integers(ebo, n):
    """check 7."""
    f1, f2 = random_bearings(31, n), random_bearings(32, n)
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        _, diag = c.relative_pose_ransac([0, n], f1, f2, ebo.two_view_params(seed=1234), diagnostics=True)
    want = tv.samples(1234, 0, np.arange(1000), n)
    assert np.array_equal(diag["samples"][0], want)


def test_hypothesis_models_within_the_restatements_own_error(ebo, ref_runs):
    """check 8: per scene the bound is 10 x the largest per-entry difference between the restatement's Jacobi solve
    and a LAPACK solve of the same samples."""
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        for i, (sc, run) in enumerate(ref_runs):
            n = len(sc["f1"])
            # the pair index enters the sampler: put the scene at pair i behind i empty pairs
            offsets = [0] * (i + 1) + [n]
            _, diag = c.relative_pose_ransac(offsets, sc["f1"], sc["f2"], ebo.two_view_params(seed=tv.RANSAC_SEED), diagnostics=True)
            got = diag["models"][i]
            assert np.array_equal(diag["samples"][i], run["samples"])
            lap, lap_ok = tv.solve_samples_lapack(sc["f1"][run["samples"]], sc["f2"][run["samples"]])
            both = lap_ok & run["valid"]
            bound = 10.0 * float(np.abs(lap[both] - run["models"][both]).max())
            got_valid = np.abs(got).reshape(len(got), -1).max(axis=1) > 0
            diff = float(np.abs(got - run["models"]).max())
            equal = int((bits(got) == bits(run["models"])).reshape(len(got), -1).all(axis=1).sum())
            print("scene %d: %d of %d models bit-equal, max |device - restatement| = %.3g, bound %.3g" % (i, equal, len(got), diff, bound))
            assert np.array_equal(got_valid, run["valid"])
            assert diff <= bound


def test_no_model_is_marked_so_on_the_device(ebo, ref_runs):
    """check 8, second half: a hypothesis the restatement marks "no model" is an all-zero model on the device, on inputs
    that have such hypotheses (the five scenes, identical correspondences and a pure rotation have none): bearing
    vectors that are all zero, 150 of 200 zero, and a scene in which some bearings hold a NaN or an infinity (a
    hypothesis that samples one of them has no finite sum)."""
    sc, _ = ref_runs[0]
    f1, f2 = sc["f1"], sc["f2"]
    rot = tv.rotation_about([0.2, 1.0, -0.3], 0.1)
    zero1, zero2 = f1.copy(), f2.copy()
    zero1[:150], zero2[:150] = 0.0, 0.0
    bad1, bad2 = f1.copy(), f2.copy()
    bad1[::9, 1] = np.nan
    bad2[4::31] = np.inf
    cases = {"identical": (np.tile(f1[:1], (50, 1)), np.tile(f2[:1], (50, 1))), "pure rotation": (f1, f1 @ rot),
             "all zero": (np.zeros((20, 3)), np.zeros((20, 3))), "150 of 200 zero": (zero1, zero2),
             "NaN and infinity": (bad1, bad2)}
    seen_invalid = 0
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        for name, (a, b) in cases.items():
            _, diag = c.relative_pose_ransac([0, len(a)], a, b, ebo.two_view_params(seed=5, max_iterations=200), diagnostics=True)
            ref = tv.ransac(a, b, seed=5, pair=0, max_iterations=200)
            got_valid = np.abs(np.nan_to_num(diag["models"][0], nan=1.0)).reshape(200, -1).max(axis=1) > 0
            print("%s: the restatement marks %d of 200 hypotheses 'no model', the device %d" % (
                name, int((~ref["valid"]).sum()), int((~got_valid).sum())))
            assert np.array_equal(got_valid, ref["valid"]), name
            assert np.array_equal(diag["counts"][0][~ref["valid"]], np.zeros(int((~ref["valid"]).sum()), dtype=np.int32))
            seen_invalid += int((~ref["valid"]).sum())
    assert seen_invalid > 0   # otherwise this test shows nothing


def test_two_view_timing_reports_five_phases(ebo, ref_runs):
    """ebo_two_view_timing: zeros before a timed call, five finite non-negative numbers after one whose parts do not
    exceed the whole, and results that do not depend on it."""
    sc, run = ref_runs[0]
    prm = ebo.two_view_params(seed=tv.RANSAC_SEED)
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        plain = c.relative_pose_ransac([0, 200], sc["f1"], sc["f2"], prm)[0]
        assert c.two_view_timing(True) == (0.0,) * 5
        timed = c.relative_pose_ransac([0, 200], sc["f1"], sc["f2"], prm)[0]
        ms = c.two_view_timing(False)
        print("phases [ms]: hypotheses %.4f, counting %.4f, host walk %.4f, inlier list %.4f, call %.4f" % ms)
        assert all(np.isfinite(v) and v >= 0.0 for v in ms)
        assert ms[0] > 0.0 and ms[1] > 0.0 and ms[4] > 0.0
        assert ms[0] + ms[1] + ms[2] + ms[3] <= ms[4] * 1.05
        again = c.relative_pose_ransac([0, 200], sc["f1"], sc["f2"], prm)[0]
        assert c.two_view_timing(False) == ms   # switched off: the last timed call's figures stay
    for r in (timed, again):
        assert (r["winner"], r["iterations"]) == (plain["winner"], plain["iterations"]) and same(r["model"], plain["model"])
        assert np.array_equal(r["inliers"], plain["inliers"])


@pytest.mark.parametrize("max_iterations", [1, 50, 1000])
def test_counts_winner_and_inliers_are_equal_integers(ebo, ref_runs, max_iterations):
    """check 9: alone and as one call of five pairs, and run to run."""
    prm = ebo.two_view_params(seed=tv.RANSAC_SEED, max_iterations=max_iterations)
    f1 = np.concatenate([sc["f1"] for sc, _ in ref_runs])
    f2 = np.concatenate([sc["f2"] for sc, _ in ref_runs])
    offsets = np.concatenate([[0], np.cumsum([len(sc["f1"]) for sc, _ in ref_runs])])
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        batched, bdiag = c.relative_pose_ransac(offsets, f1, f2, prm, diagnostics=True)
        again, adiag = c.relative_pose_ransac(offsets, f1, f2, prm, diagnostics=True)
        plain = c.relative_pose_ransac(offsets, f1, f2, prm)
        for i, (sc, run) in enumerate(ref_runs):
            n = len(sc["f1"])
            counts = run["counts"][:max_iterations]
            found, winner, iterations, best = tv.ransac_walk(counts, n, tv.PROBABILITY, max_iterations)
            want_inl = np.flatnonzero(tv.inliers(run["scores"][winner]) & run["valid"][winner])
            alone, diag = c.relative_pose_ransac([0] * (i + 1) + [n], sc["f1"], sc["f2"], prm, diagnostics=True)
            for name, r, d, k in (("batched", batched[i], bdiag, i), ("again", again[i], adiag, i), ("alone", alone[i], diag, i)):
                nd = int((d["counts"][k] != counts).sum())
                print("scene %d H=%d %s: %d counts differ; winner %d/%d iterations %d/%d inliers %d/%d" % (
                    i, max_iterations, name, nd, r["winner"], winner, r["iterations"], iterations, r["n_inliers"], best))
                assert nd == 0
                assert (r["found"], r["winner"], r["iterations"], r["n_inliers"]) == (found, winner, iterations, best)
                assert np.array_equal(r["inliers"], want_inl)
            assert same(alone[i]["model"], batched[i]["model"])
            assert same(bdiag["models"][i], diag["models"][i])
            assert same(bdiag["models"][i], adiag["models"][i])
            assert same(batched[i]["model"], bdiag["models"][i][winner])
            assert np.array_equal(plain[i]["inliers"], want_inl) and plain[i]["winner"] == winner


def test_counts_where_a_pair_spans_several_tiles(ebo):
    """The counting kernel stages a pair in tiles of 1024 correspondences, one workgroup per (tile, 8 hypotheses), all of
    them adding into the pair's counts: pairs of 1023, 1024, 1025 and 2049 correspondences (one tile less one, one
    exactly, a second tile of one, a third of one) and one of 7 (below the sample) in one call of 16 hypotheses.  The
    yardstick is the restatement's score of every correspondence under the DEVICE's own model of each hypothesis: the
    per-point scores are bit-equal to it (test_per_point_forms_are_bit_equal), so the counts are equal integers with no
    allowance near the threshold and without the restatement's hypothesis solver."""
    sizes, H = (1023, 1024, 7, 1025, 2049), 16
    scenes = [tv.make_scene(400 + k, n, 0.1, 0.3) for k, n in enumerate(sizes)]
    f1 = np.concatenate([sc["f1"] for sc in scenes])
    f2 = np.concatenate([sc["f2"] for sc in scenes])
    offsets = np.concatenate([[0], np.cumsum(sizes)])
    prm = ebo.two_view_params(seed=tv.RANSAC_SEED, max_iterations=H)
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        res, diag = c.relative_pose_ransac(offsets, f1, f2, prm, diagnostics=True)
        again, adiag = c.relative_pose_ransac(offsets, f1, f2, prm, diagnostics=True)
    beyond_first_tile = 0
    for i, (sc, n) in enumerate(zip(scenes, sizes)):
        models, counts, r = diag["models"][i], diag["counts"][i], res[i]
        valid = np.abs(np.nan_to_num(models, nan=1.0)).reshape(H, -1).max(axis=1) > 0
        assert np.array_equal(counts, adiag["counts"][i]) and same(models, adiag["models"][i])
        assert (r["found"], r["winner"], r["iterations"], r["n_inliers"]) == (
            again[i]["found"], again[i]["winner"], again[i]["iterations"], again[i]["n_inliers"])
        assert np.array_equal(r["inliers"], again[i]["inliers"])
        if n < 8:
            assert not valid.any() and not counts.any()
            assert (r["found"], r["winner"], r["iterations"], r["n_inliers"]) == (False, -1, 0, 0) and len(r["inliers"]) == 0
            continue
        inl = tv.inliers(tv.scores(models, sc["f1"], sc["f2"])) & valid[:, None]
        want = inl.sum(axis=1).astype(np.int32)
        print("n=%d: %d valid hypotheses, device counts %s, restatement under the device's models %s" % (
            n, int(valid.sum()), counts.tolist(), want.tolist()))
        assert valid.any()
        assert np.array_equal(counts, want)
        assert not counts[~valid].any()
        have = bool(np.abs(np.nan_to_num(r["model"], nan=1.0)).max() > 0)
        want_inl = np.flatnonzero(tv.inliers(tv.scores(r["model"], sc["f1"], sc["f2"]))) if have else np.zeros(0, dtype=np.int64)
        assert np.array_equal(r["inliers"], want_inl) and r["n_inliers"] == len(want_inl)
        assert r["n_inliers"] == counts[r["winner"]] and same(r["model"], models[r["winner"]])
        beyond_first_tile += int((inl[:, 1024:]).sum())
    assert beyond_first_tile > 0   # otherwise the later tiles added nothing and this test shows nothing


def test_device_form_matches_host_form(ebo, ref_runs):
    import torch
    sc, run = ref_runs[0]
    prm = ebo.two_view_params(seed=tv.RANSAC_SEED)
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        host = c.relative_pose_ransac([0, 200], sc["f1"], sc["f2"], prm)[0]
        d_f1, d_f2 = torch.from_numpy(sc["f1"]).to("cuda"), torch.from_numpy(sc["f2"]).to("cuda")
        torch.cuda.synchronize()
        dev = c.relative_pose_ransac([0, 200], d_f1.data_ptr(), d_f2.data_ptr(), prm, device=True)[0]
    assert (host["found"], host["winner"], host["iterations"]) == (dev["found"], dev["winner"], dev["iterations"])
    assert np.array_equal(host["inliers"], dev["inliers"]) and same(host["model"], dev["model"])
    assert host["winner"] == run["winner"]


def test_edge_cases_are_statuses_never_faults(ebo, synth, ref_runs):
    """check 10."""
    import torch
    sc, _ = ref_runs[0]
    f1, f2 = sc["f1"], sc["f2"]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        assert c.relative_pose_ransac([0], np.zeros((0, 3)), np.zeros((0, 3))) == []
        for n in (0, 7):
            r = c.relative_pose_ransac([0, n], f1[:n], f2[:n])[0]
            assert (r["found"], r["winner"], r["iterations"], r["n_inliers"]) == (False, -1, 0, 0)
        # n = 8: every hypothesis draws all eight
        r8, d8 = c.relative_pose_ransac([0, 8], f1[:8], f2[:8], ebo.two_view_params(seed=3, max_iterations=20), diagnostics=True)
        ref8 = tv.ransac(f1[:8], f2[:8], seed=3, pair=0, max_iterations=20)
        assert np.array_equal(np.sort(d8["samples"][0], axis=1), np.tile(np.arange(8), (20, 1)))
        assert np.array_equal(d8["samples"][0], ref8["samples"])
        fin = np.isfinite(ref8["scores"]).all(axis=1)
        assert np.array_equal(d8["counts"][0][fin], ref8["counts"][fin])
        # a mix of short and full pairs in one call
        mixed = c.relative_pose_ransac([0, 3, 3, 203], np.concatenate([f1[:3], f1]), np.concatenate([f2[:3], f2]),
                                       ebo.two_view_params(seed=tv.RANSAC_SEED, max_iterations=50))
        assert [m["found"] for m in mixed] == [False, False, True]
        # all correspondences identical: no model can be told apart; not found or found, but no fault
        same1, same2 = np.tile(f1[:1], (50, 1)), np.tile(f2[:1], (50, 1))
        rs, ds = c.relative_pose_ransac([0, 50], same1, same2, ebo.two_view_params(max_iterations=30), diagnostics=True)
        refs = tv.ransac(same1, same2, seed=0, pair=0, max_iterations=30)
        fin = np.isfinite(refs["scores"]).all(axis=1)
        assert np.array_equal(ds["counts"][0][fin], refs["counts"][fin])
        # a pure rotation: t = 0, every hypothesis is degenerate
        rot = tv.rotation_about([0.2, 1.0, -0.3], 0.1)
        g2 = f1 @ rot
        rp, dp = c.relative_pose_ransac([0, 200], f1, g2, ebo.two_view_params(max_iterations=100), diagnostics=True)
        refp = tv.ransac(f1, g2, seed=0, pair=0, max_iterations=100)
        fin = np.isfinite(refp["scores"]).all(axis=1)
        print("pure rotation: %d of 100 hypotheses have finite restatement scores; device found=%s" % (int(fin.sum()), rp[0]["found"]))
        assert np.array_equal(dp["counts"][0][fin], refp["counts"][fin])
        # argument errors
        for kw in (dict(max_iterations=0), dict(max_iterations=4097), dict(probability=0.0), dict(probability=1.0),
                   dict(threshold=0.0), dict(threshold=-1.0), dict(threshold=float("nan"))):
            with pytest.raises(ebo.EboError) as ei:
                c.relative_pose_ransac([0, 200], f1, f2, ebo.two_view_params(**kw))
            assert ei.value.code == ebo.ERR_ARG, kw
        big = random_bearings(5, 65536)
        with pytest.raises(ebo.EboError) as ei:
            c.relative_pose_ransac([0, 65536], big, big)
        assert ei.value.code == ebo.ERR_ARG
        # while a graph records: refused, and the recording survives
        ev, gt = synth.make_window(0, n_events=3000)
        c.set_window(ev)
        d_flows = torch.zeros((c.P, 2), dtype=torch.float64, device="cuda")
        d_out = torch.zeros(3 * c.P, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())
        c.synchronize()
        codes = []
        ident = np.hstack([np.eye(3), np.ones((3, 1))])

        def body():
            for call in (lambda: c.relative_pose_ransac([0, 200], f1, f2), lambda: c.relative_pose_scores(ident, f1, f2),
                         lambda: c.triangulate([ident, ident], [[0, 1]], f1[:1], f2[:1]),
                         lambda: c.epipolar_inliers(ident, f1, f2, 1e-3),
                         lambda: c.relative_pose_scores_device(ident, 0, 0, 0, 1e-3)):
                try:
                    call()
                    codes.append(0)
                except ebo.EboError as e:
                    codes.append(e.code)
            c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())

        g = c.record(body)
        assert codes == [ebo.ERR_STATE] * 5
        g.launch()
        c.synchronize()
        g.close()
        assert c.relative_pose_ransac([0, 200], f1, f2, ebo.two_view_params(seed=tv.RANSAC_SEED))[0]["found"]
