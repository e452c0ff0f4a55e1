"""GPU: the odometry front end end to end through the camera layer (tests/cpp/localize_lines_test.cpp `run`): world
points seen by six keyframes along a known trajectory, projected with CameraModel::project under the DAVIS240C
distortion, Keyframes built from patches at those corners, visual_odometry::VisualOdometryFrontEnd run as the body of a
keyframe hook -- against abspose_ref.FrontEndReplay, the same statements on the restatements of the device entries
(tests/test_abspose_cpu.py checks that the scene keeps clear of the thresholds)."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import abspose_ref as ap
import camera_ref
import twoview_ref as tv

pytestmark = pytest.mark.gpu

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
ACTIVE = 3


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def same(a, b):
    """Bit equality, a NaN matching a NaN whatever its sign and payload (which are not part of any rule)."""
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and bool(((bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))).all())


@pytest.fixture(scope="module")
def driver(ebo, tmp_path_factory):
    ebo.lib()
    out = tmp_path_factory.mktemp("odometry")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "abspose.mk", "OUT=" + str(out), str(out / "localize_lines_test")])
    fs = ap.make_facade_scene()
    fs["x"].tofile(str(out / "x.f64"))
    fs["visible"].astype(np.float64).tofile(str(out / "visible.f64"))

    def run(num_of_inliers=55, refine=None):
        cmd = ["timeout", "-k", "10", "300", str(out / "localize_lines_test"), "run"] + [repr(float(v)) for v in camera_ref.DAVIS]
        cmd += [str(out / "x.f64"), str(out / "visible.f64"), str(len(fs["x"])), str(num_of_inliers), str(ACTIVE), str(ap.FACADE_SEED)]
        if refine is not None:
            np.ascontiguousarray(refine, dtype=np.float64).tofile(str(out / "refine.f64"))
            cmd.append(str(out / "refine.f64"))
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        # printf writes a landmark triangulated from one keyframe twice (the fall-back branch) as nan or inf
        line = re.sub(r"(?<![\w.])(-?)nan\b", "NaN", r.stdout.strip().splitlines()[-1])
        line = re.sub(r"(?<![\w.])(-?)inf\b", r"\1Infinity", line)
        return json.loads(line)

    return fs, run


def replay(fs, got, num_of_inliers=55, refine=None):
    assert got["threshold"] == ap.localize_threshold(3.0)
    rp = ap.FrontEndReplay(got["threshold"], num_of_inliers=num_of_inliers, num_of_active_frames=ACTIVE, seed=ap.FACADE_SEED,
                           refine=refine)
    for t, lm in ap.facade_frames(fs):
        rp.new_keyframe_candidate(t, lm)
    return rp


def check_against_replay(got, rp):
    """Poses and landmarks bit for bit, the rest as integers."""
    assert len(got["candidates"]) == len(rp.log)
    for k, (c, want) in enumerate(zip(got["candidates"], rp.log)):
        loc = want["localize"]
        print("keyframe %d: added %s, %d inliers; localize %s / restatement %s" % (
            k, c["added"], len(c["inliers"]), c["localize"],
            None if loc is None else [int(loc["found"]), loc["winner"], loc["iterations"], loc["n_inliers"]]))
        assert c["added"] == want["added"], k
        assert same(np.array(c["pose"]).reshape(3, 4), want["pose"]), k
        # the first keyframe and the fall-back branch list a keyframe's landmarks in hash-map order: compare as multisets
        assert sorted(c["inliers"]) == sorted(want["inliers"]), k
        if loc is not None:
            assert c["localize"] == [int(loc["found"]), loc["winner"], loc["iterations"], loc["n_inliers"]], k
        else:
            assert c["localize"] == [0, 0, 0, 0], k
    assert [a[0] for a in got["active"]] == sorted(rp.active)
    for ts, pose in got["active"]:
        assert same(np.array(pose).reshape(3, 4), rp.active[ts]["pose"])
    assert [s[0] for s in got["stored_frames"]] == [s[0] for s in rp.stored_frames]
    for (_, pose), (_, want) in zip(got["stored_frames"], rp.stored_frames):
        assert same(np.array(pose).reshape(3, 4), want)
    lm = np.array(got["landmarks"], dtype=np.float64).reshape(-1, 4)
    assert lm[:, 0].astype(np.int64).tolist() == sorted(rp.landmarks)
    want = np.array([rp.landmarks[t] for t in sorted(rp.landmarks)]).reshape(-1, 3)
    print("landmarks: %d of %d differ, %d not finite" % (
        int(((bits(lm[:, 1:]) != bits(want)) & ~(np.isnan(lm[:, 1:]) & np.isnan(want))).any(axis=1).sum()), len(want),
        int((~np.isfinite(want)).any(axis=1).sum())))
    assert same(lm[:, 1:], want)
    assert [[t, seen] for t, seen in got["observations"]] == [[t, rp.observations[t]] for t in sorted(rp.observations)]
    assert [s[0] for s in got["stored_landmarks"]] == [s[0] for s in rp.stored_landmarks]
    if rp.stored_landmarks:
        assert same(np.array([s[1:] for s in got["stored_landmarks"]]), np.array([s[1] for s in rp.stored_landmarks]))
    # the optimizer hook: once per added keyframe, with the active set
    assert got["optimizer_calls"] == rp.optimizer_calls
    assert len(got["optimizer_calls"]) == sum(c["added"] for c in got["candidates"])


def test_front_end_against_the_restatement(driver):
    fs, run = driver
    got = run()
    rp = replay(fs, got)
    check_against_replay(got, rp)
    # the scene does what it was built for: two-view on keyframes 1-2, keyframes 3-6 localised against the map, the
    # two oldest keyframes and the landmarks only they saw stored
    assert [c["added"] for c in got["candidates"]] == [True] * 6
    assert got["candidates"][1]["localize"] == [0, 0, 0, 0]
    for c in got["candidates"][2:]:
        assert c["localize"][0] == 1 and len(c["inliers"]) > 55
    assert [s[0] for s in got["stored_frames"]] == [1000, 51000] and len(got["active"]) == ACTIVE + 1
    assert len(got["stored_landmarks"]) > 0
    # against the ground truth up to the scale of the unit baseline: within the restatement's own error plus the model
    # bound (10 x the restatement's A3-vs-LAPACK difference on the samples of that keyframe's RANSAC)
    scale = np.linalg.norm(fs["poses"][1][:, 3])
    for k, (c, want) in enumerate(zip(got["candidates"], rp.log)):
        truth = fs["poses"][k].copy()
        truth[:, 3] /= scale
        bound = 0.0
        loc = want["localize"]
        if loc is not None:
            smp = ap.samples(ap.FACADE_SEED, 0, np.arange(ap.MAX_ITERATIONS), loc["n"])
            m, v = ap.solve_samples(loc["f"][smp], loc["p"][smp])
            ml, vl = ap.solve_samples_lapack(loc["f"][smp], loc["p"][smp])
            bound = 10.0 * float(np.abs(m[v & vl] - ml[v & vl]).max())
        err_dev = float(np.abs(np.array(c["pose"]).reshape(3, 4) - truth).max())
        err_ref = float(np.abs(want["pose"] - truth).max())
        print("keyframe %d against the truth: device %.4g, restatement %.4g, model bound %.3g" % (k, err_dev, err_ref, bound))
        assert err_dev <= err_ref + bound
        # the trajectory is followed: within a tenth of the distance travelled (no bundle adjustment: the error grows)
        assert err_ref <= 0.1 * (1.0 + np.linalg.norm(truth[:, 3]))


def test_localize_refinement_and_reselection(ebo, driver):
    """With a refinement that returns a given pose, Tw2c is that pose and the re-selected inliers are those of
    ebo_absolute_pose_scores at it.  Two sets of given poses: the true ones in the map's scale (the map was
    triangulated from the ESTIMATED first pair, so few points agree with them and the reference's branches fall
    through to initCameras: the whole run still equals the replay), and abspose_ref.refined_poses (the unrefined run's
    poses, nudged), under which the localisation stands and match.inliers are the flags' tracks."""
    fs, run = driver
    scale = np.linalg.norm(fs["poses"][1][:, 3])
    truth = fs["poses"].copy()
    truth[:, :, 3] /= scale
    stands = 0
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        for given in (truth, ap.refined_poses(fs, ACTIVE)):
            got = run(refine=given)
            rp = replay(fs, got, refine={t: given[k] for k, t in enumerate(fs["timestamps"])})
            check_against_replay(got, rp)
            for k, (cand, want) in enumerate(zip(got["candidates"], rp.log)):
                loc = want["localize"]
                if loc is None or not loc["found"]:
                    continue
                sc, flags = c.absolute_pose_scores(given[k], loc["f"], loc["p"], got["threshold"])
                assert np.array_equal(flags, ap.inliers(ap.scores(given[k], loc["f"], loc["p"]), got["threshold"]))
                print("keyframe %d: %d of %d points within the threshold at the given pose" % (k, int(flags.sum()), loc["n"]))
                if flags.sum() > 55:      # otherwise initCameras or the fall-back branch has replaced the match
                    assert np.array_equal(bits(np.array(cand["Tw2c"]).reshape(3, 4)), bits(given[k]))
                    assert cand["inliers"] == [int(t) for t in loc["tracks"][flags]]
                    stands += 1
    assert stands >= 3


def test_too_few_map_points_fall_through_the_references_branches(driver):
    """numOfInliers = 85: the two-view pair still initialises, the later keyframes localise with too few inliers, fail
    initCameras against the last active frame and take the fall-back branch (pose of the last frame, the keyframe's
    landmarks APPENDED to the match), as the restatement does."""
    fs, run = driver
    got = run(num_of_inliers=85)
    rp = replay(fs, got, num_of_inliers=85)
    check_against_replay(got, rp)
    assert [c["added"] for c in got["candidates"]] == [True] * 6
    late = got["candidates"][2:]
    assert any(len(c["inliers"]) != len(set(c["inliers"])) for c in late)      # appended without clearing
    assert any(c["localize"][0] == 1 and c["localize"][3] <= 85 for c in late)
