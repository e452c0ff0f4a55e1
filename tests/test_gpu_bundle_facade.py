"""GPU: the bundle-adjustment members of the odometry façade (visual_odometry/bundle_adjustment.h, the two use...
members of VisualOdometryFrontEnd, pinned by signature in tests/cpp/bundle_lines_test.cpp) against tests/bundle_ref.py.
The driver builds the active keyframes and the map from a window in a file, calls bundleAdjust / refinePose, and every
pose and landmark that comes back is compared with the restatement run on the problem the façade states -- frames in
map order with the first two constant, landmarks in ascending track id, a keyframe's corner what Patch::toCorner makes
of it, the bearing vectors' f_x / f_z, f_y / f_z on the identity camera -- under test_gpu_bundle.py's bound: integers
equal, doubles within 10 x the window's delta (the restatement against itself with every stated sum reversed).  On the
noisy window the summed squared reprojection error is lower after the optimiser than before: asserted as a sign, the
two numbers printed (what LM's accepted steps guarantee, not a measurement of accuracy)."""
import os
import subprocess

import numpy as np
import pytest

import bundle_ref as B

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CPP = os.path.join(ROOT, "tests", "cpp")


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = tmp_path_factory.mktemp("bundle_lines")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "bundle.mk", "OUT=" + str(out), str(out / "bundle_lines_test")])
    return out


def run(driver, mode, pr, fix, max_it=50):
    B.write_problem(driver / "p.f64", pr, B.HUBER, fix, B.default_opts(max_num_iterations=max_it))
    r = subprocess.run([str(driver / "bundle_lines_test"), mode, str(driver / "p.f64"), str(driver / "o.f64")], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout + r.stderr
    return np.fromfile(str(driver / "o.f64"))


def squared_error(pr, poses, points):
    q = np.einsum("nji,nj->ni", poses[pr["of"], :, :3], points[pr["op"]] - poses[pr["of"], :, 3])
    return float(((B.project_np(pr["cam"], q) - pr["uv"]) ** 2).sum())


@pytest.mark.parametrize("noise", [0.0, 0.5])
def test_bundle_adjust_equals_the_restatement(driver, noise):
    """Six keyframes, 30 landmarks seen by 2..6 of them; the file marks NO frame constant: the façade fixes the first two."""
    pr = B.scene(21, 6, 30, views=(2, 6), noise=noise, baseline=0.5)
    asked = dict(pr, fixed=np.zeros(6, np.uint8))
    got = run(driver, "adjust", asked, False)
    stated = dict(pr, fixed=np.array([1, 1, 0, 0, 0, 0], np.uint8), uv=(pr["uv"] - 4.0) + 4.0)   # Patch::toCorner
    want = B.solve(stated, B.HUBER, False)
    delta = B.result_difference(want, B.solve(stated, B.HUBER, False, reverse_sums=True))
    s = want["summary"]
    assert [int(got[0]), int(got[1])] == [s["iterations"], s["termination"]]
    poses, points = got[4:4 + 72].reshape(6, 3, 4), got[76:].reshape(30, 3)
    worst = max(B.difference(poses, want["poses"]), B.difference(points, want["points"]), B.difference(got[2:4], [s["initial_cost"], s["final_cost"]]))
    equal = int((poses == want["poses"]).sum() + (points == want["points"]).sum())
    print("noise %.1f: %d of 162 doubles bit-equal, largest difference %.3g, delta %.3g" % (noise, equal, worst, delta))
    assert worst <= 10 * delta
    assert np.array_equal(poses[:2], pr["poses"][:2])
    before, after = squared_error(stated, pr["poses"], pr["points"]), squared_error(stated, poses, points)
    print("noise %.1f: summed squared reprojection error %.6g before, %.6g after" % (noise, before, after))
    assert after < before


def test_refine_pose_equals_the_restatement(driver):
    pr = B.refine_scene(31, 40)
    got = run(driver, "refine", pr, True)
    of, op, uv = B.sort_observations(1, pr["of"], pr["op"], pr["uv"])
    n = np.sqrt((uv[:, 0] * uv[:, 0] + uv[:, 1] * uv[:, 1]) + 1.0)
    f = np.stack([uv[:, 0] / n, uv[:, 1] / n, 1.0 / n], axis=1)
    stated = dict(pr, of=of, op=op, uv=np.stack([f[:, 0] / f[:, 2], f[:, 1] / f[:, 2]], axis=1), cam=B.IDENTITY_CAM)
    assert np.array_equal(got[16:].reshape(-1, 2), stated["uv"])
    want = B.solve(stated, B.HUBER, True)
    delta = B.result_difference(want, B.solve(stated, B.HUBER, True, reverse_sums=True))
    s = want["summary"]
    assert [int(got[0]), int(got[1])] == [s["iterations"], s["termination"]]
    worst = max(B.difference(got[4:16].reshape(1, 3, 4), want["poses"]), B.difference(got[2:4], [s["initial_cost"], s["final_cost"]]))
    print("refinement: largest difference %.3g, delta %.3g, cost %.3g -> %.3g" % (worst, delta, got[2], got[3]))
    assert worst <= 10 * delta
    assert got[3] < got[2]
