"""GPU: the facade's ground-truth side end to end (tests/cpp/aligner_test.cpp): align_cameras_sim3 over a
std::list<Keyframe> and alignPrefixes against tests/align_ref.py, bit for bit; and VisualOdometryFrontEnd on the
six-keyframe scene of tests/test_gpu_odometry_facade.py with ground truth -- with useDeviceAlignment() lastAlignment()
is the restatement's answer on the same centres and alignedGroundTruth() is sim.inverse() * gt; without it (and with
setGroundTruthSamples alone) every output is bit-equal to the existing driver's, which never heard of ground truth."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import abspose_ref as ap
import align_ref as A
import camera_ref

pytestmark = pytest.mark.gpu

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
ACTIVE = 3
SHARED = ("candidates", "active", "stored_frames", "landmarks")
CANDIDATE = ("timestamp", "added", "pose", "Tw2c", "inliers", "localize")


def loads(stdout):
    line = re.sub(r"(?<![\w.])(-?)nan\b", "NaN", stdout.strip().splitlines()[-1])
    return json.loads(re.sub(r"(?<![\w.])(-?)inf\b", r"\1Infinity", line))


def same_json(a, b):
    """Equal structure, integers and strings; doubles bit-equal (they were printed with %.17g), a NaN matching a NaN."""
    if isinstance(a, list):
        return isinstance(b, list) and len(a) == len(b) and all(same_json(x, y) for x, y in zip(a, b))
    if isinstance(a, dict):
        return isinstance(b, dict) and a.keys() == b.keys() and all(same_json(a[k], b[k]) for k in a)
    if isinstance(a, float) and isinstance(b, float):
        return A.same_bits(a, b) or (np.isnan(a) and np.isnan(b))
    return type(a) is type(b) and a == b


def as_alignment(js):
    return dict(scale=np.float64(js["scale"]), R=np.array(js["R"]).reshape(3, 3), t=np.array(js["t"]), rmse=np.float64(js["rmse"]),
                mean=np.float64(js["mean"]), min=np.float64(js["min"]), max=np.float64(js["max"]), count=int(js["count"]),
                status=js["status"])


@pytest.fixture(scope="module")
def driver(ebo, tmp_path_factory):
    ebo.lib()
    out = tmp_path_factory.mktemp("aligner")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "aligner.mk", "OUT=" + str(out), str(out / "aligner_test")])
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "abspose.mk", "OUT=" + str(out), str(out / "localize_lines_test")])
    fs = ap.make_facade_scene()
    fs["x"].tofile(str(out / "x.f64"))
    fs["visible"].astype(np.float64).tofile(str(out / "visible.f64"))
    scene_args = [repr(float(v)) for v in camera_ref.DAVIS] + [str(out / "x.f64"), str(out / "visible.f64"), str(len(fs["x"])), "55",
                                                                str(ACTIVE), str(ap.FACADE_SEED)]

    def run(cmd):
        r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return loads(r.stdout)

    def front_end(samples, mode):
        np.array([[t, *np.asarray(p, np.float64).reshape(12)] for t, p in samples], np.float64).tofile(str(out / "samples.f64"))
        return run([str(out / "aligner_test"), "frontend"] + scene_args + [str(out / "samples.f64"), str(mode)])

    def cameras(gt, est):
        np.ascontiguousarray(gt, np.float64).tofile(str(out / "gt.f64"))
        np.ascontiguousarray(est, np.float64).tofile(str(out / "est.f64"))
        return run([str(out / "aligner_test"), "cameras", str(out / "gt.f64"), str(out / "est.f64")])

    existing = run([str(out / "localize_lines_test"), "run"] + scene_args)
    return fs, front_end, cameras, existing


def ground_truth(fs, times):
    """The scene's true trajectory as a motion-capture system would report it: in another frame, at 2.5 x the scale."""
    rng = np.random.default_rng(8)
    W = A.pose_of(rng, [4.0, -1.0, 2.0])
    t0, step = fs["timestamps"][0], fs["timestamps"][1] - fs["timestamps"][0]
    out = []
    for t in times:
        k = (t - t0) / step                     # the trajectory of abspose_ref.make_facade_scene at a fractional keyframe
        pose = np.zeros((3, 4))
        pose[:, :3] = ap.tv.rotation_about([0.1, 1.0, 0.05], -0.012 * k)
        pose[:, 3] = 2.5 * np.array([0.25 * k, 0.02 * k * k, 0.04 * k])
        out.append((int(t), A._mul(W, pose)))
    return out


def test_align_cameras_over_a_list_of_keyframes(driver):
    _, _, cameras, _ = driver
    gt, est = A.trajectory(40)
    got = cameras(gt, est)
    want = A.align(gt, est)
    assert A.same_result(as_alignment(dict(got["cameras"], status=0)), want)
    assert len(got["prefixes"]) == 35
    for k, js in zip(range(6, 41), got["prefixes"]):
        assert A.same_result(as_alignment(js), A.align(gt[:k], est[:k])), k
    # sim.inverse() * reference pose: the centre goes back onto the estimate's, the rotation is turned by R^T
    first = np.array(got["aligned_first"]).reshape(3, 4)
    assert np.abs(first[:, 3] - (want["R"].T @ (gt[0] - want["t"])) / want["scale"]).max() <= 1e-13
    assert np.abs(first[:, 3] - est[0]).max() <= 5 * want["max"] / want["scale"] + 1e-12


def test_without_the_calls_nothing_changes(driver):
    """Mode 0 (nothing set) and mode 1 (setGroundTruthSamples alone) against the existing driver, and mode 2 against them:
    poses, matches, landmarks bit for bit."""
    fs, front_end, _, existing = driver
    samples = ground_truth(fs, fs["timestamps"])
    runs = [front_end(samples, mode) for mode in (0, 1, 2)]
    for mode, got in enumerate(runs):
        for key in SHARED[1:]:
            assert same_json(got[key], existing[key]), (mode, key)
        assert len(got["candidates"]) == len(existing["candidates"]) == 6
        for c, e in zip(got["candidates"], existing["candidates"]):
            assert same_json({k: c[k] for k in CANDIDATE}, {k: e[k] for k in CANDIDATE}), (mode, c["timestamp"])
    assert runs[0]["alignment"]["status"] == 1 and runs[0]["aligned_gt"] == []
    assert runs[1]["alignment"]["status"] == 1 and [c["aligned"] for c in runs[1]["candidates"]] == [1, 2, 3, 4, 5, 6]
    assert [c["alignment_status"] for c in runs[2]["candidates"]] == [1, 1, 1, 1, 1, 0]      # more than 5 poses


@pytest.mark.parametrize("case", ["exact", "late_and_between"])
def test_with_device_alignment_the_answer_is_the_restatements(driver, case):
    """exact: a sample at every keyframe's timestamp.  late_and_between: the samples start after the first keyframe, which
    therefore has no ground truth and is left out of the pairing (the reference would read gt_ out of range), and the
    other keyframes fall between samples."""
    fs, front_end, _, _ = driver
    stamps = fs["timestamps"]
    times = stamps if case == "exact" else [stamps[0] + 20000 + 30000 * j for j in range(10)]
    samples = ground_truth(fs, times)
    raw = front_end(samples, 1)
    got = front_end(samples, 2)
    with_gt = [t for t in stamps if times[0] <= t <= times[-1]]
    assert len(with_gt) == (6 if case == "exact" else 5)
    gt = np.array(raw["aligned_gt"]).reshape(-1, 3, 4)                # before an alignment: the synced poses, zeroed
    assert len(gt) == len(with_gt)
    assert np.array_equal(gt[0], np.eye(3, 4)) or np.abs(gt[0] - np.eye(3, 4)).max() <= 1e-15
    if case == "exact":
        zero = samples[0][1]
        for k, (_, pose) in enumerate(samples):
            assert np.abs(gt[k] - A._mul(A._inv(zero), pose)).max() <= 1e-14
    poses = {t: np.array(p).reshape(3, 4) for t, p in got["stored_frames"] + got["active"]}
    assert sorted(poses) == stamps
    cams = np.array([poses[t][:, 3] for t in with_gt])
    want = A.align(gt[:, :, 3], cams)
    assert want["status"] == 0 and want["count"] == len(with_gt)
    assert A.same_result(as_alignment(got["alignment"]), want)
    # alignedGroundTruth() = sim.inverse() * gt: back in the estimate's frame and scale
    aligned = np.array(got["aligned_gt"]).reshape(-1, 3, 4)
    assert len(aligned) == len(gt)
    for a, g in zip(aligned, gt):
        assert np.abs(a[:, 3] - (want["R"].T @ (g[:, 3] - want["t"])) / want["scale"]).max() <= 1e-13
        assert np.abs(a[:, :3] - want["R"].T @ g[:, :3]).max() <= 1e-14
    # and the odometry follows the truth: the ground truth is 2.5 x the unit-baseline estimate, the error a few percent
    length = np.linalg.norm(gt[-1, :, 3] - gt[0, :, 3])
    print("%s: scale %.4f, rmse %.3g of a %.3g long trajectory" % (case, want["scale"], want["rmse"], length))
    assert want["rmse"] <= 0.1 * length
