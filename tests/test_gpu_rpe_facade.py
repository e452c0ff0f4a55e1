"""GPU: the facade's relative-pose-error side end to end (tests/cpp/rpe_facade_test.cpp): relativePoseErrors and
relativePoseErrorsPrefixes against tests/rpe_ref.py, bit for bit; and VisualOdometryFrontEnd on the six-keyframe scene of
tests/test_gpu_odometry_facade.py with ground truth -- with useDeviceRelativeErrors() lastRelativeErrors() after the sixth
keyframe is the restatement's answer on the same paired poses, with the alignment's scale when there is one and with 1
and the flag down when there is none; without the call (and with it) every pose, match and landmark is bit-equal."""
import os
import subprocess

import numpy as np
import pytest

import abspose_ref as ap
import camera_ref
import rpe_ref as T
from test_gpu_align_facade import ACTIVE, ground_truth, loads, same_json

pytestmark = pytest.mark.gpu

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
SHARED = ("active", "stored_frames", "landmarks", "alignment_status", "alignment_scale", "aligned_gt")
CANDIDATE = ("timestamp", "pose", "Tw2c", "inliers", "localize", "alignment_status")
DELTAS = (1, 2, 5)


def as_units(js):
    """The driver's list of RelativeErrors -> the restatement's dicts; both metrics carry the count."""
    out = []
    for e in js:
        assert e["translation"]["count"] == e["rotation"]["count"]
        d = {"trans_" + k: np.float64(e["translation"][k]) for k in ("rmse", "mean", "min", "max")}
        d.update({"rot_" + k: np.float64(e["rotation"][k]) for k in ("rmse", "mean", "min", "max")})
        d.update(count=int(e["translation"]["count"]), status=e["status"], delta=e["delta"])
        out.append(d)
    return out


@pytest.fixture(scope="module")
def driver(ebo, tmp_path_factory):
    ebo.lib()
    out = tmp_path_factory.mktemp("rpe_facade")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "rpe.mk", "OUT=" + str(out), str(out / "rpe_facade_test")])
    fs = ap.make_facade_scene()
    fs["x"].tofile(str(out / "x.f64"))
    fs["visible"].astype(np.float64).tofile(str(out / "visible.f64"))
    scene_args = [repr(float(v)) for v in camera_ref.DAVIS] + [str(out / "x.f64"), str(out / "visible.f64"), str(len(fs["x"])), "55",
                                                                str(ACTIVE), str(ap.FACADE_SEED)]

    def run(cmd):
        r = subprocess.run(["timeout", "-k", "10", "300", str(out / "rpe_facade_test")] + cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return loads(r.stdout)

    def front_end(samples, mode):
        np.array([[t, *np.asarray(p, np.float64).reshape(12)] for t, p in samples], np.float64).tofile(str(out / "samples.f64"))
        return run(["frontend"] + scene_args + [str(out / "samples.f64"), str(mode)])

    def poses(gt, est, scale, first, scales, deltas):
        np.ascontiguousarray(gt, np.float64).tofile(str(out / "gt.f64"))
        np.ascontiguousarray(est, np.float64).tofile(str(out / "est.f64"))
        np.ascontiguousarray(scales, np.float64).tofile(str(out / "scales.f64"))
        return run(["poses", str(out / "gt.f64"), str(out / "est.f64"), repr(float(scale)), str(first), str(out / "scales.f64")]
                   + [str(d) for d in deltas])

    return fs, front_end, poses


def test_relative_pose_errors_and_their_prefixes(driver):
    _, _, poses = driver
    gt, est = T.helix(40, 5, 1e-2)
    deltas = [1, 3, 10, 39, 40]
    scales = np.linspace(0.5, 2.0, 35)
    got = poses(gt, est, 1.3, 6, scales, deltas)
    for key, scale in (("whole", 1.3), ("unscaled", 1.0)):
        units = as_units(got[key])
        assert [u["delta"] for u in units] == deltas and [u["status"] for u in units] == [0, 0, 0, 0, 1]
        for u, d in zip(units, deltas):
            assert T.same_result(u, T.rpe(gt, est, d, scale)), (key, d)
    assert len(got["prefixes"]) == 35
    for k, s, js in zip(range(6, 41), scales, got["prefixes"]):
        for u, d in zip(as_units(js), deltas):
            assert T.same_result(u, T.rpe(gt[:k], est[:k], d, s)), (k, d)
    assert all(T.same_result(u, w) for u, w in zip(as_units(got["prefixes_unscaled_last"]), as_units(got["unscaled"])))


def test_the_front_end_reports_the_restatements_errors_and_changes_nothing_else(driver):
    """Modes: 1 ground truth alone, 3 with the alignment, 5 with the relative errors, 7 with both."""
    fs, front_end, _ = driver
    stamps = fs["timestamps"]
    samples = ground_truth(fs, stamps)
    runs = {mode: front_end(samples, mode) for mode in (1, 3, 5, 7)}
    # the opt-in changes nothing the front end computes
    for base, with_rpe in ((1, 5), (3, 7)):
        for key in SHARED:
            assert same_json(runs[with_rpe][key], runs[base][key]), (with_rpe, key)
        assert len(runs[with_rpe]["candidates"]) == len(runs[base]["candidates"]) == 6
        for c, e in zip(runs[with_rpe]["candidates"], runs[base]["candidates"]):
            assert same_json({k: c[k] for k in CANDIDATE}, {k: e[k] for k in CANDIDATE}), (with_rpe, c["timestamp"])
        assert runs[base]["rpe"] == [] and [c["rpe_entries"] for c in runs[base]["candidates"]] == [0] * 6
        assert runs[base]["rpe_aligned"] is False and runs[base]["rpe_scale"] == 1.0
    # the paired poses: the synced ground truth relative to the first (before any alignment) and the keyframes' poses
    gt = np.array(runs[1]["aligned_gt"]).reshape(-1, 3, 4)
    assert len(gt) == 6
    for mode in (5, 7):
        got = runs[mode]
        poses = {t: np.array(p).reshape(3, 4) for t, p in got["stored_frames"] + got["active"]}
        assert sorted(poses) == stamps
        cams = np.array([poses[t] for t in stamps])
        assert [c["rpe_entries"] for c in got["candidates"]] == [3] * 6
        assert [c["rpe_pairs"] for c in got["candidates"]] == [0.0, 1.0, 2.0, 3.0, 4.0, 5.0]     # of delta 1, keyframe by keyframe
        if mode == 7:
            assert got["alignment_status"] == 0 and got["rpe_aligned"] is True and T.same_bits(got["rpe_scale"], got["alignment_scale"])
            # the estimate's unit of length is its first baseline, so the scale is about the ground truth's first step
            first_step = np.linalg.norm(gt[1, :, 3] - gt[0, :, 3])
            assert abs(got["rpe_scale"] / first_step - 1.0) <= 0.1
        else:
            assert got["alignment_status"] == 1 and got["rpe_aligned"] is False and T.same_bits(got["rpe_scale"], 1.0)
        units = as_units(got["rpe"])
        assert [u["delta"] for u in units] == list(DELTAS) and [u["count"] for u in units] == [5, 4, 1]
        for u, d in zip(units, DELTAS):
            assert u["status"] == 0 and T.same_result(u, T.rpe(gt, cams, d, got["rpe_scale"])), (mode, d)
    # with the alignment's scale the steps agree far better than without it, where they are off by the factor 1 / scale
    step = np.linalg.norm(gt[1:, :, 3] - gt[:-1, :, 3], axis=1).mean()
    scaled, plain = as_units(runs[7]["rpe"])[0], as_units(runs[5]["rpe"])[0]
    print("delta 1: mean step %.3g, translation rmse %.3g with the scale, %.3g without; rotation rmse %.3g rad"
          % (step, scaled["trans_rmse"], plain["trans_rmse"], scaled["rot_rmse"]))
    factor = abs(1.0 / runs[7]["rpe_scale"] - 1.0)
    assert scaled["trans_rmse"] <= 0.5 * plain["trans_rmse"] and plain["trans_rmse"] >= 0.5 * factor * step
    assert T.same_bits(scaled["rot_rmse"], plain["rot_rmse"])         # the rotation does not see the scale
