"""CPU: the track-evaluation rules of include/ebo.h (V1-V9) as tests/trackerr_ref.py restates them -- against worked
answers chosen to be exact, against an independent statement of the interpolation and the error (numpy.interp +
numpy.hypot), the device's own text (csrc/ebo_trackerr.inc compiled for the host by tools/track_errors_serial.cpp)
against the restatement bit for bit, and the two host entries ebo_track_seeds and ebo_track_error_summary against their
restatements and worked answers."""
import ctypes as C
import os
import subprocess

import numpy as np
import pytest

import trackerr_ref as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# 10 x the worst case measured with numpy 2 on x86-64 over trackerr_ref.independent_scenes (24 tracks: 2 .. 200
# ground-truth samples, noise 0 / 0.3 / 30 px, at the origin and 1e4 px from it, times from 1 s and from 2^50 us).  The
# error is relative to max(1, |position|): numpy.interp forms slope * (t - t_j) + p_j where V3 forms
# p_j + w * (p_{j+1} - p_j), and numpy.hypot rounds once where V4 rounds three times, so both sides carry a few ulps
# of the coordinates.
BOUND_INDEPENDENT = 4.1e-15   # measured 4.1e-16: max |e - e_independent| / max(1, |x|, |y|)


def independent_scenes():
    out = []
    for k, n_gt in enumerate((2, 3, 17, 200)):
        for noise in (0.0, 0.3, 30.0):
            for offset, t0 in ((0.0, 1_000_000), (1e4, (1 << 50) + 977)):
                gt = V.gt_track(n_gt, 300 + k, t0=t0, offset=offset)
                out.append((gt, V.est_track(gt, 150, 400 + k, noise=noise)))
    return out


def track(t, xy):
    return np.array(t, np.int64), np.array(xy, np.float64).reshape(-1, 2)


def test_a_stationary_ground_truth_and_an_offset_of_3_4():
    gt = track([1000, 2000, 9000], [[10.0, 20.0]] * 3)
    est = track([500, 1000, 1500, 2000, 4000, 9000, 9001], [[13.0, 24.0]] * 7)
    r, per = V.track_error(est, gt, 5.0)
    assert r["status"] == 0 and r["first"] == 1 and r["n_comparable"] == 5 and r["n_inliers"] == 5 and r["cut"] == -1
    assert all(V.same_bits(r[f], 5.0) for f in V.DOUBLES)
    assert r["age_us"] == 8000 and r["t_first_us"] == 1000
    assert np.array_equal(per, [-1.0, 5.0, 5.0, 5.0, 5.0, 5.0, -1.0])
    # the comparison is strict: tau = 5 does not cut, the next double below 5 cuts at the first comparable sample
    r, per2 = V.track_error(est, gt, np.nextafter(5.0, 0.0))
    assert r["status"] == 0 and r["n_inliers"] == 0 and r["cut"] == 1 and r["first"] == 1 and r["n_comparable"] == 5
    assert r["age_us"] == 0 and r["t_first_us"] == 1000 and all(V.same_bits(r[f], 0.0) for f in V.DOUBLES)
    assert np.array_equal(per, per2)                                     # V8 does not depend on tau


def test_a_linear_ground_truth_with_dyadic_numbers_is_interpolated_exactly():
    # 1 / 4 px per 1024 us: every weight and every product is exact in binary
    gt = track([0, 4096, 8192, 16384], [[0.0, 64.0], [1.0, 62.0], [2.0, 60.0], [4.0, 56.0]])
    ts = [0, 1024, 2048, 4096, 5120, 8192, 12288, 16384]
    for T in ts:
        g = V.interp(gt[0], gt[1], T)
        assert V.same_bits(g[0], T / 4096.0) and V.same_bits(g[1], 64.0 - T / 2048.0), T
    # the estimate runs 0.75 px to the right of it, and leaves by 6 px more from sample 5 on
    xy = [[T / 4096.0 + 0.75 + (6.0 if k >= 5 else 0.0), 64.0 - T / 2048.0] for k, T in enumerate(ts)]
    est = track(ts, xy)
    r, per = V.track_error(est, gt, 1.0)
    assert np.array_equal(per, [0.75] * 5 + [6.75] * 3)
    assert r["status"] == 0 and r["n_inliers"] == 5 and r["cut"] == 5 and r["n_comparable"] == 8
    assert r["age_us"] == 5120 and r["t_first_us"] == 0                 # t(sample 4) - t(sample 0), by hand
    assert V.same_bits(r["err_mean"], 0.75) and V.same_bits(r["err_rmse"], 0.75) and V.same_bits(r["err_max"], 0.75)
    r, _ = V.track_error(est, gt, 6.75)
    assert r["n_inliers"] == 8 and r["cut"] == -1 and r["age_us"] == 16384
    assert V.same_bits(r["err_mean"], (5 * 0.75 + 3 * 6.75) / 8.0) and V.same_bits(r["err_max"], 6.75)
    assert V.same_bits(r["err_rmse"], np.sqrt((5 * 0.5625 + 3 * 45.5625) / 8.0))


def test_the_statuses_and_their_order():
    gt = V.gt_track(6, 1)
    est = V.est_track(gt, 10, 2)
    nothing = track([], [])
    assert V.track_error(nothing, gt, 1.0)[0]["status"] == 1
    assert V.track_error(est, (gt[0][:1], gt[1][:1]), 1.0)[0]["status"] == 1
    assert V.track_error(est, nothing, 1.0)[0]["status"] == 1
    late = (est[0] + (gt[0][-1] - gt[0][0]) + 1, est[1])
    r, per = V.track_error(late, gt, 1.0)
    assert r["status"] == 1 and all(r[f] == 0 for f in V.DOUBLES + V.INTS if f != "status") and (per == -1.0).all()
    for bad in (np.nan, np.inf, -np.inf):
        for side in (0, 1):
            e, g = (est[0], est[1].copy()), (gt[0], gt[1].copy())
            (e, g)[side][1][3, side] = bad
            r, per = V.track_error(e, g, 1.0)
            assert r["status"] == 2 and all(r[f] == 0 for f in V.DOUBLES + V.INTS if f != "status") and (per == -1.0).all()
    # a non-finite coordinate outside the span still counts, and comes before "nothing within the span"
    bad_late = (late[0], late[1].copy())
    bad_late[1][0, 0] = np.nan
    assert V.track_error(bad_late, gt, 1.0)[0]["status"] == 2
    # too few samples comes first
    bad_gt = (gt[0][:1], np.array([[np.nan, 0.0]]))
    assert V.track_error(est, bad_gt, 1.0)[0]["status"] == 1


def test_the_restatement_against_interp_and_hypot():
    worst = 0.0
    scenes = independent_scenes()
    assert len(scenes) == 24
    for gt, est in scenes:
        i0, i1, q, e = V.sample_errors(est[0], est[1], gt[0], gt[1])
        j0, j1, ei = V.independent_errors(est, gt)
        assert (i0, i1) == (j0, j1) and i1 - i0 == 150
        scale = np.maximum(1.0, np.abs(est[1][i0:i1]).max(axis=1))
        worst = max(worst, float((np.abs(e - ei) / scale).max()))
        r, _ = V.track_error(est, gt, np.inf)
        assert r["status"] == 0 and r["n_inliers"] == 150
        assert abs(r["err_mean"] - ei.mean()) <= BOUND_INDEPENDENT * scale.max()
        assert abs(r["err_rmse"] - np.sqrt((ei * ei).mean())) <= BOUND_INDEPENDENT * scale.max()
        assert abs(r["err_max"] - ei.max()) <= BOUND_INDEPENDENT * scale.max()
    print("restatement against numpy.interp + numpy.hypot, worst |de| / max(1, |x|, |y|): %.2g" % worst)
    assert worst <= BOUND_INDEPENDENT


@pytest.fixture(scope="module")
def serial(tmp_path_factory):
    """csrc/ebo_trackerr.inc compiled for the host (tools/track_errors_serial.cpp, g++ -O2 -ffp-contract=off)."""
    exe = tmp_path_factory.mktemp("trackerr") / "track_errors_serial"
    src = os.path.join(ROOT, "event-based-odomety_amd", "tools", "track_errors_serial.cpp")
    subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-o", str(exe), src])
    return exe


def test_the_device_text_on_the_host_equals_the_restatement_bit_for_bit(serial, tmp_path):
    """Every case of the GPU test and its batch of 70 units: integers equal, doubles bit-equal, per-sample errors too."""
    statuses = set()
    for name, (ests, gts, taus) in list(V.gpu_cases().items()) + [("batch70", V.batch70())]:
        V.write_problem(tmp_path / "p.bin", ests, gts, taus)
        out = subprocess.run([str(serial), str(tmp_path / "p.bin"), str(tmp_path / "r.bin"), "1"], capture_output=True, text=True)
        assert out.returncode == 0, out.stderr
        want, per = V.track_errors(ests, gts, taus)
        got, got_per = V.read_result(tmp_path / "r.bin", len(want), len(per))
        for k, (g, w) in enumerate(zip(got, want)):
            assert V.same_result(g, w), (name, k, g, w)
        assert np.array_equal(per.view(np.int64), got_per.view(np.int64)), name
        statuses |= {w["status"] for w in want}
    assert statuses == {0, 1, 2}


def test_the_cases_hold_what_they_are_named_for():
    c = V.gpu_cases()
    res = {name: V.track_errors(*v)[0] for name, v in c.items()}
    assert [r["n_inliers"] for r in res["inliers"]] == [1, 63, 64, 65, 128, 129] and all(r["cut"] == -1 for r in res["inliers"])
    assert [r["cut"] for r in res["cuts"]] == [0, 1, 63, 64, 65, 129, -1]
    assert [r["n_inliers"] for r in res["cuts"]] == [0, 1, 63, 64, 65, 129, 130]
    assert [(r["n_inliers"], r["cut"]) for r in res["tie"]] == [(5, -1), (0, 0), (5, -1)]
    assert all(V.same_bits(res["tie"][0][f], 5.0) for f in V.DOUBLES)
    assert [r["status"] for r in res["span"]] == [0, 1, 1, 1, 0]
    assert (res["span"][0]["first"], res["span"][0]["n_comparable"]) == (2, 4)      # on the first time .. on the last time
    assert [r["status"] for r in res["gt_lengths"]][::2] == [1, 0, 0, 0, 0, 0]
    assert [r["status"] for r in res["nonfinite"]] == [0, 0] + [2] * 10 + [0, 0]
    assert V.same_result(res["nonfinite"][0], res["nonfinite"][12])                 # the neighbour is unaffected
    assert [r["status"] for r in res["empty"]] == [1, 1, 1, 1, 0, 0, 1, 1]
    assert res["taus8"][0]["n_inliers"] == 0 and res["taus8"][7]["n_inliers"] == 100 and res["taus8"][7]["cut"] == -1
    assert res["far"][1]["n_inliers"] == 66 and res["far"][1]["t_first_us"] > 1 << 50
    assert res["repeats"][1]["n_inliers"] == 20


# ---- ebo_track_seeds ---------------------------------------------------------------------------------------------------
def test_seeds(ebo):
    frames = [1000, 2000, 3000, 4000]
    tracks = [
        track([1500, 2000, 2600], [[1.0, 2.0], [3.0, 5.0], [9.0, 9.0]]),            # a sample exactly on a frame time
        track([1200, 2800, 3500], [[0.0, 8.0], [4.0, 0.0], [7.0, 7.0]]),            # frame 1 between two samples
        track([2100, 2500, 2900], [[1.0, 1.0]] * 3),                                # shorter than a frame interval
        track([3000], [[6.5, 7.25]]),                                               # one sample, on a frame
        track([3200], [[1.0, 1.0]]),                                                # one sample, off every frame
        track([3500, 3900, 4000, 4000], [[0.0, 0.0], [1.0, 1.0], [2.0, 2.0], [5.0, 6.0]]),   # equal times at its end
        track([], []),                                                              # empty
        track([4500, 5000], [[1.0, 1.0]] * 2),                                      # after the last frame
        track([0, 5000], [[0.0, 0.0], [5.0, 10.0]]),                                # longer than the recording
        track([100, 1000, 1000, 1700], [[0.0, 0.0], [1.0, 1.0], [2.0, 3.0], [4.0, 4.0]]),   # equal times on a frame
    ]
    sf, sx = ebo.track_seeds(tracks, frames)
    assert sf.dtype == np.int32 and sx.dtype == np.float32
    assert list(sf) == [1, 1, -1, 2, -1, 3, -1, -1, 0, 0]
    want = [(3.0, 5.0), (2.0, 4.0), (0.0, 0.0), (6.5, 7.25), (0.0, 0.0), (5.0, 6.0), (0.0, 0.0), (0.0, 0.0), (1.0, 2.0), (2.0, 3.0)]
    assert np.array_equal(sx, np.array(want, np.float32))
    rf, rx = V.seeds(tracks, frames)
    assert np.array_equal(sf, rf) and np.array_equal(sx.view(np.int32), rx.view(np.int32))
    # seeded random tracks against the restatement, float32 bit for bit
    gts = [V.gt_track(n, 50 + n) for n in (2, 5, 9, 30)]
    tracks = [V.est_track(g, n, 60 + n, lo=g[0][0] - 30_000, hi=g[0][-1] + 30_000) for g, n in zip(gts, (3, 40, 7, 100))]
    frames = np.unique(np.concatenate([g[0] for g in gts]))
    sf, sx = ebo.track_seeds(tracks, frames)
    rf, rx = V.seeds(tracks, frames)
    assert (sf >= 0).any() and np.array_equal(sf, rf) and np.array_equal(sx.view(np.int32), rx.view(np.int32))
    assert ebo.track_seeds([], frames)[0].shape == (0,)
    assert list(ebo.track_seeds(tracks, [])[0]) == [-1] * 4
    for bad_tracks, bad_frames in (([track([5, 4], [[0.0, 0.0]] * 2)], frames), (tracks, [3, 3]), (tracks, [4, 3])):
        with pytest.raises(ebo.EboError) as err:
            ebo.track_seeds(bad_tracks, bad_frames)
        assert err.value.code == ebo.ERR_ARG


# ---- ebo_track_error_summary -------------------------------------------------------------------------------------------
def result(status=0, n_inliers=3, err_mean=1.0, age_us=1000, cut=-1):
    r, _ = V.track_error(track([], []), track([], []), 1.0)
    r.update(status=status, n_inliers=n_inliers, err_mean=np.float64(err_mean), age_us=age_us, cut=cut)
    return r


def test_the_summary(ebo):
    rs = [result(err_mean=0.5, age_us=2_000_000), result(status=1, n_inliers=0), result(err_mean=1.25, age_us=500_000, cut=7),
          result(status=2, n_inliers=0), result(n_inliers=0, cut=0, err_mean=0.0, age_us=0), result(err_mean=3.0, age_us=1)]
    s = ebo.track_error_summary(rs)
    assert s["counted"] == 3 and s["discarded"] == 3 and s["outlived"] == 2
    assert V.same_bits(s["mean_error"], ((0.5 + 1.25) + 3.0) / 3.0)
    assert V.same_bits(s["mean_age_s"], (((2_000_000.0 + 500_000.0) + 1.0) / 3.0) * 1e-6)
    w = V.summary(rs)
    assert all(s[k] == w[k] for k in ("counted", "discarded", "outlived")) and V.same_bits(s["mean_error"], w["mean_error"])
    assert V.same_bits(s["mean_age_s"], w["mean_age_s"])
    # sequential sums in track order: 1e16 + 1 + 1 is not 1 + 1 + 1e16
    a = ebo.track_error_summary([result(err_mean=1e16), result(err_mean=1.0), result(err_mean=1.0)])
    b = ebo.track_error_summary([result(err_mean=1.0), result(err_mean=1.0), result(err_mean=1e16)])
    assert V.same_bits(a["mean_error"], 1e16 / 3.0) and V.same_bits(b["mean_error"], (1e16 + 2.0) / 3.0)
    for none in ([], [result(status=1, n_inliers=0)], [result(n_inliers=0, cut=0), result(status=2, n_inliers=0)]):
        s = ebo.track_error_summary(none)
        assert s == dict(mean_error=0.0, mean_age_s=0.0, counted=0, discarded=0, outlived=0) and s == V.summary(none)
    # a results array of several taus is read with a stride
    res = (ebo.TrackErrorResult * 6)()
    for k in range(3):
        res[2 * k].n_inliers, res[2 * k].err_mean, res[2 * k].cut = 1, 100.0, -1
        res[2 * k + 1].n_inliers, res[2 * k + 1].err_mean, res[2 * k + 1].age_us, res[2 * k + 1].cut = 2, float(k), 1_000_000 * k, k
    out = ebo.TrackErrorSummary()
    assert ebo.lib().ebo_track_error_summary(3, C.addressof(res) + C.sizeof(ebo.TrackErrorResult), 2, C.addressof(out)) == 0
    assert (out.mean_error, out.mean_age_s, out.counted, out.discarded, out.outlived) == (1.0, 1.0, 3, 0, 0)
    assert ebo.lib().ebo_track_error_summary(3, C.addressof(res), 0, C.addressof(out)) == ebo.ERR_ARG
    assert ebo.lib().ebo_track_error_summary(-1, C.addressof(res), 1, C.addressof(out)) == ebo.ERR_ARG
    assert ebo.lib().ebo_track_error_summary(3, None, 1, C.addressof(out)) == ebo.ERR_ARG


def test_the_result_layout(ebo):
    """ebo_track_error_result is 64 bytes: three doubles, two int64, six int32."""
    T = ebo.TrackErrorResult
    assert C.sizeof(T) == 64
    offs = {n: getattr(T, n).offset for n, _ in T._fields_}
    assert offs == dict(err_mean=0, err_rmse=8, err_max=16, age_us=24, t_first_us=32, n_inliers=40, n_comparable=44, first=48,
                        cut=52, status=56, pad=60)
    assert C.sizeof(ebo.TrackErrorSummary) == 32 and C.sizeof(ebo.LkParams) == 32
