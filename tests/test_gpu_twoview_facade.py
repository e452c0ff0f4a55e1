"""GPU: the two-view facade end to end through the camera layer (tests/cpp/two_view_lines_test.cpp `init`): 3-D points
projected with CameraModel::project under the DAVIS240C distortion, two Keyframes built from patches at those
corners, visual_odometry::TwoViewInitializer run as the body of a keyframe hook -- against tests/twoview_ref.py on
the same bearing vectors (tests/test_twoview_cpu.py checks that this scene keeps clear of the threshold)."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import camera_ref
import twoview_ref as tv

pytestmark = pytest.mark.gpu

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def driver(ebo, tmp_path_factory):
    ebo.lib()
    out = tmp_path_factory.mktemp("twoview")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "twoview.mk", "OUT=" + str(out), str(out / "two_view_lines_test")])
    fs = tv.make_facade_scene()
    fs["x1"].tofile(str(out / "x1.f64"))
    fs["x2"].tofile(str(out / "x2.f64"))

    def run(num_of_inliers=55, refine=None):
        cmd = ["timeout", "-k", "10", "300", str(out / "two_view_lines_test"), "init"] + [repr(float(v)) for v in camera_ref.DAVIS]
        cmd += [str(out / "x1.f64"), str(out / "x2.f64"), str(num_of_inliers), str(tv.RANSAC_SEED)]
        if refine is not None:
            cmd += [repr(float(v)) for v in np.asarray(refine).reshape(12)]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    return fs, run


def rotation_angle(Ra, Rb):
    return math.acos(max(-1.0, min(1.0, (np.trace(Ra.T @ Rb) - 1.0) / 2.0)))


def unit_translation(model):
    """match.Tw2c: the model with its translation divided by sqrt((tx * tx + ty * ty) + tz * tz)."""
    out = np.array(model, dtype=np.float64).reshape(3, 4).copy()
    t = out[:, 3]
    s = t[0] * t[0] + t[1] * t[1]
    s = s + t[2] * t[2]
    out[:, 3] = t / np.sqrt(s)
    return out


def check_common(fs, got):
    n = len(fs["x1"])
    tracks = np.array(got["tracks"])
    # sorted by track id; the track only one keyframe holds is not shared; ids are 3 i + 5
    assert np.array_equal(tracks, 3 * np.arange(n) + 5)
    assert got["first_answer"] is False
    # the keyframes hold CameraModel::project of the points (host arithmetic of the facade = camera_ref.project)
    assert np.array_equal(bits(got["corners1"]), bits(fs["corners1"]))
    assert np.array_equal(bits(got["corners2"]), bits(fs["corners2"]))
    return tracks


def test_two_view_initializer_against_the_restatement(ebo, driver):
    fs, run = driver
    got = run()
    tracks = check_common(fs, got)
    f1, f2 = tv.facade_bearings(fs)
    ref = tv.ransac(f1, f2, seed=tv.RANSAC_SEED, pair=0)
    print("device: winner %d after %d, %d RANSAC inliers, %d re-selected; restatement: winner %d after %d, %d inliers" % (
        got["winner"], got["iterations"], got["ransac_inliers"], len(got["inliers"]), ref["winner"], ref["iterations"], ref["n_inliers"]))
    assert got["initialised"] is True and got["found"] == 1
    assert (got["winner"], got["iterations"], got["ransac_inliers"]) == (ref["winner"], ref["iterations"], ref["n_inliers"])
    # no refinement: the re-selection under the RANSAC model gives the RANSAC inliers back, as track ids
    assert np.array_equal(got["inliers"], tracks[ref["inliers"]])
    # the rotation: within the restatement's own error against the ground truth + the model bound of check 8
    lap, lap_ok = tv.solve_samples_lapack(f1[ref["samples"]], f2[ref["samples"]])
    both = lap_ok & ref["valid"]
    bound = 10.0 * float(np.abs(lap[both] - ref["models"][both]).max())
    Tw2c = np.array(got["Tw2c"]).reshape(3, 4)
    R_gt = fs["model"][:, :3]
    ang_dev, ang_ref = rotation_angle(Tw2c[:, :3], R_gt), rotation_angle(ref["model"][:, :3], R_gt)
    print("rotation against the ground truth: device %.4f deg, restatement %.4f deg, model bound %.3g" % (
        math.degrees(ang_dev), math.degrees(ang_ref), bound))
    assert ang_dev <= ang_ref + bound
    assert np.abs(np.array(got["ransac_model"]).reshape(3, 4) - ref["model"]).max() <= bound
    # match.Tw2c = the model with a unit translation; keyframe.pose = start.pose (identity) * Tw2c
    assert np.array_equal(bits(Tw2c), bits(unit_translation(got["ransac_model"])))
    assert abs(np.linalg.norm(Tw2c[:, 3]) - 1.0) < 1e-15
    start, pose = np.array(got["start_pose"]).reshape(3, 4), np.array(got["pose"]).reshape(3, 4)
    assert np.array_equal(start, np.hstack([np.eye(3), np.zeros((3, 1))]))
    assert np.array_equal(pose, tv.pose_mul(start, Tw2c))
    # landmarks of the inliers = twoview_ref.triangulate on the returned poses, bit for bit
    lm = np.array(got["landmarks"])
    assert np.array_equal(lm[:, 0].astype(np.int64), got["inliers"]) and got["n_landmarks"] == len(got["inliers"])
    want = tv.triangulate([start, pose], [[0, 1]] * len(ref["inliers"]), f1[ref["inliers"]], f2[ref["inliers"]])
    print("landmarks: %d of %d differ" % (int((bits(lm[:, 1:]) != bits(want)).any(axis=1).sum()), len(want)))
    assert np.array_equal(bits(lm[:, 1:]), bits(want))
    # and they are the scene's points up to the scale of the unit baseline, for the true inliers
    scale = np.linalg.norm(fs["model"][:, 3])
    good = ~fs["is_outlier"][ref["inliers"]]
    err = np.linalg.norm(lm[good, 1:] * scale - fs["x1"][ref["inliers"]][good], axis=1) / fs["x1"][ref["inliers"]][good][:, 2]
    print("landmark error relative to depth: median %.3f" % float(np.median(err)))


def test_refinement_callback_and_reselection(ebo, driver):
    """With a refinement that returns the ground-truth motion the re-selected inliers are those of
    ebo_relative_pose_scores at that motion, and Tw2c is that motion with a unit translation."""
    fs, run = driver
    got = run(refine=fs["model"])
    tracks = check_common(fs, got)
    f1, f2 = tv.facade_bearings(fs)
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        sc, flags = c.relative_pose_scores(fs["model"], f1, f2, tv.THRESHOLD)
    assert np.array_equal(flags, tv.inliers(tv.scores(fs["model"], f1, f2)))
    assert got["initialised"] is True
    assert np.array_equal(got["inliers"], tracks[flags])
    assert np.array_equal(bits(np.array(got["Tw2c"]).reshape(3, 4)), bits(unit_translation(fs["model"])))
    lm = np.array(got["landmarks"])
    want = tv.triangulate([got["start_pose"], got["pose"]], [[0, 1]] * int(flags.sum()), f1[flags], f2[flags])
    assert np.array_equal(bits(lm[:, 1:]), bits(want))


def test_too_few_inliers_do_not_initialise(driver):
    fs, run = driver
    got = run(num_of_inliers=150)
    check_common(fs, got)
    assert got["initialised"] is False and got["found"] == 1 and got["inliers"] == [] and got["n_landmarks"] == 0
