"""CPU: tests/twoview_ref.py against known answers -- the yardstick of the two-view GPU tests checked on its own --
and the condition on the GPU tests' inputs that makes their exact comparisons fair."""
import json
import math
import os
import subprocess

import numpy as np
import pytest

import twoview_ref as tv


def test_known_answer_of_the_reference_triangulation_test():
    """triangulation_test.cpp:5-23 restated as data: identity pose, pose 2 = 90 degrees about z with translation
    (1, -1, 0), both bearings (1, 0, 0) -> (1, 0, 0) to 4 float32 ulps (EXPECT_FLOAT_EQ)."""
    poses = np.zeros((2, 3, 4))
    poses[0, :, :3] = np.eye(3)
    poses[1, :, :3] = tv.rotation_about([0, 0, 1], math.pi / 2)
    poses[1, :, 3] = [1.0, -1.0, 0.0]
    p = tv.triangulate(poses, [[0, 1]], [[1.0, 0.0, 0.0]], [[1.0, 0.0, 0.0]])[0]
    want = np.array([1.0, 0.0, 0.0], dtype=np.float32)
    assert np.all(np.abs(p.astype(np.float32) - want) <= 4 * np.spacing(np.float32(1.0))), p


def test_pose_algebra():
    T = tv.random_motions(3, 20, angle=2.0, dist=5.0)
    I = tv.pose_mul(T, tv.pose_inverse(T))
    eye = np.hstack([np.eye(3), np.zeros((3, 1))])
    bound = 8 * 2.0 ** -53 * (1 + np.abs(T[:, :, 3]).max())
    assert np.abs(I - eye).max() <= bound
    p = np.array([0.3, -1.2, 4.0])
    assert np.allclose(tv.pose_apply(tv.pose_mul(T[0], T[1]), p), tv.pose_apply(T[0], tv.pose_apply(T[1], p)), atol=1e-14)


def test_triangulation_recovers_points_and_scores_vanish():
    sc = tv.make_scene(9, n=300, outliers=0.0, noise_px=0.0)
    p = tv.triangulate2(sc["model"], sc["f1"], sc["f2"])
    assert np.abs(p - sc["points"]).max() < 1e-9
    s = tv.scores(sc["model"], sc["f1"], sc["f2"])
    assert s.shape == (300,) and np.abs(s).max() < 1e-14
    assert np.abs(tv.epipolar_residual(sc["model"], sc["f1"], sc["f2"])).max() < 1e-14
    # the essential matrix of a known motion: t along x, no rotation -> hat((1, 0, 0))
    m = np.hstack([np.eye(3), [[2.0], [0.0], [0.0]]])
    assert np.array_equal(tv.essential(m), [[0, 0, 0], [0, 0, -1], [0, 1, 0]])


def test_jacobi_against_lapack():
    rng = np.random.default_rng(0)
    A = rng.normal(size=(50, 3, 3))
    M = A @ A.transpose(0, 2, 1)
    d, V = tv.jacobi(M, tv.JACOBI_SWEEPS_3)
    w = np.linalg.eigvalsh(M)
    assert np.abs(np.sort(d, axis=1) - w).max() <= 1e-12 * np.abs(w).max()
    assert np.abs(V.transpose(0, 2, 1) @ V - np.eye(3)).max() < 1e-13
    assert np.abs(M @ V - V * d[:, None, :]).max() <= 1e-12 * np.abs(w).max()
    # the one-sided iteration on an 8 x 9 matrix: squared singular values (one of them zero: rank 8), orthogonal V
    A = rng.normal(size=(50, 8, 9))
    d, V = tv.hestenes(A, tv.JACOBI_SWEEPS_9)
    sv = np.linalg.svd(A, compute_uv=False)
    assert np.abs(np.sort(d, axis=1)[:, 1:] - np.sort(sv ** 2, axis=1)).max() <= 1e-12 * (sv ** 2).max()
    assert np.sort(d, axis=1)[:, 0].max() <= 1e-24 * (sv ** 2).max()
    assert np.abs(V.transpose(0, 2, 1) @ V - np.eye(9)).max() < 1e-13
    null = V[np.arange(50), :, np.argmin(d, axis=1)]
    assert np.abs(np.einsum("bij,bj->bi", A, null)).max() < 1e-13


def test_noise_free_scene_is_solved_by_the_first_hypothesis():
    """check 2: hypothesis 0 has all n inliers, the walk stops after 1, and the model equals the ground truth
    (R12, t12 / |t12|) to the accuracy the LAPACK solve reaches on the same sample, x 10.  One scene and one sample,
    at the default seeds (scene 0, RANSAC seed 0): the comparison is a single draw.  Over the 200 samples of each of
    six such scenes the ratio of the two solvers' errors has median 0.8-1.1 and exceeds 10 for 1.5-4.5 % of the
    samples (LAPACK's exceeds ten times this solve's about as often): both are backward stable and each sample's
    error is its condition number times a factor of either sign."""
    sc = tv.make_scene(0, n=200, outliers=0.0, noise_px=0.0)
    run = tv.ransac(sc["f1"], sc["f2"], seed=0, pair=0, max_iterations=20)
    assert run["counts"][0] == 200
    assert (run["found"], run["winner"], run["iterations"], run["n_inliers"]) == (True, 0, 1, 200)
    assert np.array_equal(run["inliers"], np.arange(200))
    gt = sc["model"].copy()
    gt[:, 3] /= np.linalg.norm(gt[:, 3])
    s0 = run["samples"][:1]
    lap, ok = tv.solve_samples_lapack(sc["f1"][s0], sc["f2"][s0])
    assert ok[0]
    bound = 10 * np.abs(lap[0] - gt).max()
    err = np.abs(run["models"][0] - gt).max()
    print("|restatement - truth| = %.3g, |lapack - truth| x 10 = %.3g" % (err, bound))
    assert err <= bound


def test_sampler():
    """check 3: 8 distinct indices in range for n = 8 .. 65535; (seed, p, h) alone determines a sample."""
    for n in (8, 9, 10, 17, 75, 200, 500, 4096, 65535):
        s = tv.samples(5, 3, np.arange(2000), n)
        assert s.min() >= 0 and s.max() < n
        assert all(len(set(row)) == 8 for row in s.tolist())
        if n == 8:
            assert np.array_equal(np.sort(s, axis=1), np.tile(np.arange(8), (2000, 1)))
        # a hypothesis does not depend on which others are evaluated
        assert np.array_equal(tv.samples(5, 3, [1999, 7], n), s[[1999, 7]])
        assert not np.array_equal(tv.samples(6, 3, np.arange(2000), n), s) or n == 8
        assert not np.array_equal(tv.samples(5, 4, np.arange(2000), n), s) or n == 8
    # every index can be drawn, roughly evenly
    s = tv.samples(0, 0, np.arange(4000), 40)
    hist = np.bincount(s.ravel(), minlength=40)
    assert hist.min() > 600 and hist.max() < 1000   # 800 expected
    # the hash is the one the header writes out (splitmix64's finaliser chained over seed, pair, hypothesis, draw)
    def mix(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & (2 ** 64 - 1)
        return z ^ (z >> 31)
    G = 0x9E3779B97F4A7C15
    x = mix((11 + G) & (2 ** 64 - 1))
    for v in (2, 33, 4):
        x = mix(((x ^ v) + G) & (2 ** 64 - 1))
    assert int(tv.draw_hash(11, 2, 33, 4)) == x


def test_serial_walk():
    """check 4: rule 6 on hand-made count arrays."""
    # earliest of equal counts wins
    c = np.array([10, 50, 50, 20] + [0] * 96)
    found, winner, it, best = tv.ransac_walk(c, 100, 0.99, 100)
    assert (found, winner, best) == (True, 1, 50)
    # w = 0.5: k = log(0.01) / log(1 - 2^-8) = 1176.6 > 100 -> runs to the end
    assert it == 100 and math.log(0.01) / math.log(1 - 0.5 ** 8) > 100
    # all inliers at hypothesis 0: 1 - w^8 clamps to 1e-15, k = 0.133 -> stops after 1
    assert tv.ransac_walk(np.array([100] * 10), 100, 0.99, 10) == (True, 0, 1, 100)
    # w = 0.9 at h = 2: k = log(0.01) / log(1 - 0.9^8) = 8.16 -> stops after 9
    c = np.array([0, 0, 90] + [0] * 97)
    assert tv.ransac_walk(c, 100, 0.99, 100) == (True, 2, 9, 90)
    # ... unless a better one arrives first: w = 1 at h = 5 -> stops after 6
    c[5] = 100
    assert tv.ransac_walk(c, 100, 0.99, 100) == (True, 5, 6, 100)
    # best < 8: not found, every hypothesis walked
    assert tv.ransac_walk(np.array([7] * 30), 100, 0.99, 30) == (False, 0, 30, 7)
    assert tv.ransac_walk(np.array([0] * 30), 100, 0.99, 30) == (False, 0, 30, 0)
    # max_iterations = 1
    assert tv.ransac_walk(np.array([3]), 100, 0.99, 1) == (False, 0, 1, 3)
    # fewer than 8 correspondences: no hypothesis at all
    r = tv.ransac(np.zeros((7, 3)), np.zeros((7, 3)))
    assert (r["found"], r["winner"], r["iterations"]) == (False, -1, 0)


def test_gpu_test_inputs_keep_clear_of_the_threshold():
    """check 5: for every scene the GPU tests use, no restatement score lies within 1e-6 relative of the threshold
    and none is non-finite, so that an exact comparison of counts cannot pass or fail by a coin toss."""
    for i in range(len(tv.SCENES)):
        sc = tv.scene(i)
        run = tv.ransac(sc["f1"], sc["f2"], seed=tv.RANSAC_SEED, pair=i)
        s = run["scores"]
        rel = np.abs(s - tv.THRESHOLD) / tv.THRESHOLD
        print("scene %d: valid %d, nearest score %.3g relative, %d within 1e-3; winner %d after %d with %d inliers (%d true)" % (
            i, int(run["valid"].sum()), rel.min(), int((rel < 1e-3).sum()), run["winner"], run["iterations"], run["n_inliers"],
            int((~sc["is_outlier"]).sum())))
        assert np.isfinite(s).all()
        assert run["valid"].all()
        assert rel.min() > 1e-6
        assert run["found"]
        # the yardstick finds the scene: most of the true inliers are the winner's
        good = ~sc["is_outlier"]
        assert good[run["inliers"]].sum() >= 0.6 * good.sum()


def test_facade_scene_keeps_clear_of_the_threshold():
    """check 5 for the scene of test_gpu_twoview_facade.py: the RANSAC scores and the scores at the ground-truth
    motion (which the refinement callback of that test returns)."""
    fs = tv.make_facade_scene()
    f1, f2 = tv.facade_bearings(fs)
    run = tv.ransac(f1, f2, seed=tv.RANSAC_SEED, pair=0)
    gt = tv.scores(fs["model"], f1, f2)
    for name, s in (("ransac", run["scores"]), ("ground truth", gt)):
        rel = np.abs(s - tv.THRESHOLD) / tv.THRESHOLD
        print("facade scene, %s: nearest score %.3g relative" % (name, rel.min()))
        assert np.isfinite(s).all() and rel.min() > 1e-6
    print("winner %d after %d with %d inliers; %d inliers at the ground truth; %d true" % (
        run["winner"], run["iterations"], run["n_inliers"], int(tv.inliers(gt).sum()), int((~fs["is_outlier"]).sum())))
    assert run["found"] and run["valid"].all()
    assert run["n_inliers"] >= 55 and tv.inliers(gt).sum() >= 55   # VisualOdometryParams::numOfInliers


def test_facade_host_parts(ebo, tmp_path):
    """check 5b: common::Pose3d, Keyframe::getSharedTracks, computeEssential and the conformance tables of
    tests/cpp/two_view_lines_test.cpp, compiled under -Wall -Wextra and run without a GPU."""
    ebo.lib()
    cpp = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
    exe = tmp_path / "two_view_lines_test"
    subprocess.check_call(["make", "-s", "-C", cpp, "-f", "twoview.mk", "OUT=" + str(tmp_path), str(exe)])
    out = subprocess.run([str(exe), "self"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert json.loads(out.stdout.strip().splitlines()[-1])["self"] == "ok"
