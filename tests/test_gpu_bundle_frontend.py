"""GPU: the odometry front end with BOTH device hooks installed (useDeviceBundleAdjustment, useDeviceLocalizeRefinement)
on the six-keyframe scene of tests/cpp/localize_lines_test.cpp, the keyframes going through newKeyframeCandidate
(tests/cpp/bundle_lines_test.cpp `frontend`), against the replay of the same statements: abspose_ref.FrontEndReplay
with the refinement and optimize() restated on bundle_ref.py.  Decisions (added, inliers, the localisation, iterations
and terminations of every refinement and adjustment, the map's bookkeeping) as equal integers; every pose and landmark
within 10 x delta, delta being the largest difference between that replay and itself with every stated sum of the
bundle adjustment reversed (the bound of test_gpu_bundle.py, over the whole run).  The count of bit-equal doubles is
printed.  Two windows: 3 active frames (4 at the moment optimize() runs, the oldest keyframes stored) and 20 (all six
active).  On the noisy scene (0.5 px) the summed squared reprojection error of the active window is lower with the
optimiser than without: asserted as a sign, both numbers printed."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

import abspose_ref as ap
import bundle_ref as B
import camera_ref

pytestmark = pytest.mark.gpu
CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
HUBER, MAX_ITERATIONS = 0.8, 50      # VisualOdometryParams::huberLoss, maxNumIterations


class BundleReplay(ap.FrontEndReplay):
    """FrontEndReplay with the two hooks as visual_odometry/bundle_adjustment.h states them."""

    def __init__(self, *a, hooks=True, reverse_sums=False, **kw):
        super().__init__(*a, **kw)
        self.hooks, self.rev = hooks, reverse_sums
        self.last_refine, self.last_bundle = [0, 0], [0, 0]

    def refine_pose(self, pose, f, p, inliers):
        keep = [i for i in inliers if f[i, 2] > 0.0]
        pr = dict(poses=pose.reshape(1, 3, 4), fixed=np.zeros(1, np.uint8), points=p[keep], of=np.zeros(len(keep), np.int32),
                  op=np.arange(len(keep), dtype=np.int32), uv=np.stack([f[keep, 0] / f[keep, 2], f[keep, 1] / f[keep, 2]], axis=1),
                  cam=B.IDENTITY_CAM)
        r = B.solve(pr, HUBER, True, B.default_opts(max_num_iterations=MAX_ITERATIONS), reverse_sums=self.rev)
        self.last_refine = [r["summary"]["iterations"], r["summary"]["termination"]]
        return r["poses"][0]

    def localize_camera(self, kf, match, timestamp):
        # FrontEndReplay.localize_camera with the refinement computed from the RANSAC inliers instead of given
        match["inliers"] = []
        tracks = np.array(sorted(t for t in kf["landmarks"] if t in self.landmarks), dtype=np.int64)
        f = self._unproject([kf["landmarks"][t] for t in tracks]) if len(tracks) else np.zeros((0, 3))
        p = np.array([self.landmarks[t] for t in tracks], dtype=np.float64).reshape(-1, 3)
        run = ap.ransac(f, p, seed=self.seed, frame=0, threshold=self.threshold)
        info = dict(n=len(tracks), found=bool(run["found"]), winner=run["winner"], iterations=run["iterations"],
                    n_inliers=run["n_inliers"], model=run["model"], f=f, p=p, tracks=tracks)
        if not run["found"]:
            return info
        model = run["model"]
        if self.hooks:
            model = self.refine_pose(np.array(model, dtype=np.float64), f, p, [int(i) for i in run["inliers"]])
        match["Tw2c"] = model.copy()
        flags = ap.inliers(ap.scores(model, f, p), self.threshold)
        match["inliers"] = [int(t) for t in tracks[flags]]
        return info

    def window_problem(self):
        """optimize() as bundleAdjust states it: frames in map order, the first two constant, landmarks in ascending
        track id, the observation filter of visual_odometry.cpp:445-474."""
        keys = sorted(self.active)
        tracks = sorted(self.landmarks)
        of, op, uv = [], [], []
        for l, t in enumerate(tracks):
            seen = self.observations.get(t)
            if seen is None or len(seen) < 2:
                continue
            for ts in seen:
                if ts in self.active and t in self.active[ts]["landmarks"]:
                    of.append(keys.index(ts))
                    op.append(l)
                    uv.append(self.active[ts]["landmarks"][t])
        return keys, tracks, dict(poses=np.array([self.active[k]["pose"] for k in keys]).reshape(-1, 3, 4),
                                  fixed=np.array([i < 2 for i in range(len(keys))], np.uint8),
                                  points=np.array([self.landmarks[t] for t in tracks], dtype=np.float64).reshape(-1, 3),
                                  of=np.array(of, np.int32), op=np.array(op, np.int32), uv=np.array(uv, np.float64).reshape(-1, 2),
                                  cam=camera_ref.DAVIS)

    def new_keyframe_candidate(self, timestamp, landmarks):
        added = super().new_keyframe_candidate(timestamp, landmarks)
        if added and self.hooks:
            keys, tracks, pr = self.window_problem()
            r = B.solve(pr, HUBER, False, B.default_opts(max_num_iterations=MAX_ITERATIONS), reverse_sums=self.rev)
            self.last_bundle = [r["summary"]["iterations"], r["summary"]["termination"]]
            for i, k in enumerate(keys):
                self.active[k]["pose"] = r["poses"][i].copy()     # the log keeps the pose the candidate left
            for l, t in enumerate(tracks):
                self.landmarks[t] = r["points"][l].copy()
        self.log[-1]["refine"], self.log[-1]["bundle"] = list(self.last_refine), list(self.last_bundle)
        return added

    def window_error(self):
        _, _, pr = self.window_problem()
        return squared_error(pr)


def squared_error(pr):
    if len(pr["of"]) == 0:
        return 0.0
    q = np.einsum("nji,nj->ni", pr["poses"][pr["of"], :, :3], pr["points"][pr["op"]] - pr["poses"][pr["of"], :, 3])
    return float(((B.project_np(pr["cam"], q) - pr["uv"]) ** 2).sum())


def replay(fs, active, hooks=True, reverse_sums=False):
    rp = BundleReplay(ap.localize_threshold(3.0), num_of_inliers=55, num_of_active_frames=active, seed=ap.FACADE_SEED, hooks=hooks,
                      reverse_sums=reverse_sums)
    for t, lm in ap.facade_frames(fs):
        rp.new_keyframe_candidate(t, lm)
    return rp


def doubles(rp):
    """Every pose and landmark a replay ends with or logged, in a fixed order."""
    parts = [e["pose"].reshape(-1) for e in rp.log] + [rp.active[k]["pose"].reshape(-1) for k in sorted(rp.active)]
    parts += [p.reshape(-1) for _, p in rp.stored_frames] + [np.asarray(rp.landmarks[t]).reshape(-1) for t in sorted(rp.landmarks)]
    parts += [np.asarray(p).reshape(-1) for _, p in rp.stored_landmarks]
    return np.concatenate(parts)


def decisions(rp):
    return ([(e["added"], sorted(e["inliers"]), e["refine"], e["bundle"],
              None if e["localize"] is None else (e["localize"]["found"], e["localize"]["winner"], e["localize"]["iterations"],
                                                  e["localize"]["n_inliers"])) for e in rp.log],
            sorted(rp.active), [s[0] for s in rp.stored_frames], sorted(rp.landmarks), [s[0] for s in rp.stored_landmarks],
            {t: list(v) for t, v in rp.observations.items()})


@pytest.fixture(scope="module")
def driver(ebo, tmp_path_factory):
    ebo.lib()
    out = tmp_path_factory.mktemp("bundle_frontend")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "bundle.mk", "OUT=" + str(out), str(out / "bundle_lines_test")])

    def run(fs, active, hooks):
        fs["x"].tofile(str(out / "x.f64"))
        fs["visible"].astype(np.float64).tofile(str(out / "visible.f64"))
        cmd = ["timeout", "-k", "10", "300", str(out / "bundle_lines_test"), "frontend"] + [repr(float(v)) for v in camera_ref.DAVIS]
        cmd += [str(out / "x.f64"), str(out / "visible.f64"), str(len(fs["x"])), "55", str(active), str(ap.FACADE_SEED), "1" if hooks else "0"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        line = re.sub(r"(?<![\w.])(-?)nan\b", "NaN", r.stdout.strip().splitlines()[-1])
        return json.loads(re.sub(r"(?<![\w.])(-?)inf\b", r"\1Infinity", line))

    return run


def got_as_replay_view(got):
    """The driver's line in the shape of doubles() / decisions()."""
    parts = [np.array(c["pose"]) for c in got["candidates"]] + [np.array(p) for _, p in got["active"]]
    parts += [np.array(p) for _, p in got["stored_frames"]] + [np.array(l[1:]) for l in got["landmarks"]]
    parts += [np.array(l[1:]) for l in got["stored_landmarks"]]
    dec = ([(c["added"], sorted(c["inliers"]), c["refine"], c["bundle"], c["localize"]) for c in got["candidates"]],
           [a[0] for a in got["active"]], [s[0] for s in got["stored_frames"]], [int(l[0]) for l in got["landmarks"]],
           [int(l[0]) for l in got["stored_landmarks"]], {int(t): list(v) for t, v in got["observations"]})
    return np.concatenate(parts), dec


@pytest.mark.parametrize("active", [3, 20])
def test_front_end_with_both_hooks_equals_the_replay(driver, active):
    fs = ap.make_facade_scene()
    got = driver(fs, active, True)
    fwd, rev = replay(fs, active), replay(fs, active, reverse_sums=True)
    assert decisions(fwd) == decisions(rev)            # no decision of this run is a coin toss of rounding order
    delta = B.difference(doubles(rev), doubles(fwd))
    have, dec = got_as_replay_view(got)
    want_dec = decisions(fwd)
    for k, (g, w) in enumerate(zip(dec[0], want_dec[0])):
        loc = [0, 0, 0, 0] if w[4] is None else [int(w[4][0]), w[4][1], w[4][2], w[4][3]]
        assert (g[0], g[1], g[2], g[3], g[4]) == (w[0], w[1], w[2], w[3], loc), k
    assert dec[1:] == tuple(want_dec[1:])
    want = doubles(fwd)
    assert have.shape == want.shape
    worst = B.difference(have, want)
    print("active %d: %d of %d doubles bit-equal, largest difference %.3g, delta %.3g; refinements %s, adjustments %s" % (
        active, int((have.view(np.uint64) == want.view(np.uint64)).sum()), have.size, worst, delta,
        [c["refine"] for c in got["candidates"]], [c["bundle"] for c in got["candidates"]]))
    assert worst <= 10 * delta
    # the hooks ran: keyframes 3-6 were refined, every added keyframe adjusted, and they changed the answer
    assert [c["added"] for c in got["candidates"]] == [True] * 6
    assert all(c["localize"][0] == 1 and c["refine"][0] > 0 for c in got["candidates"][2:])
    assert all(c["bundle"][0] > 0 for c in got["candidates"][2:])
    assert len(got["active"]) == min(6, active + 1)
    plain = replay(fs, active, hooks=False)
    assert not np.array_equal(doubles(plain)[:72], want[:72])


def test_the_optimiser_lowers_the_windows_error_on_a_noisy_scene(driver):
    fs = ap.make_facade_scene(noise_px=0.5)
    err = {}
    for hooks in (False, True):
        got = driver(fs, 20, hooks)
        rp = replay(fs, 20, hooks=hooks)
        # the driver's final window, put into the replay's bookkeeping (which the decisions above tie to the device's)
        assert [a[0] for a in got["active"]] == sorted(rp.active)
        for ts, pose in got["active"]:
            rp.active[ts]["pose"] = np.array(pose).reshape(3, 4)
        assert [int(l[0]) for l in got["landmarks"]] == sorted(rp.landmarks)
        for l in got["landmarks"]:
            rp.landmarks[int(l[0])] = np.array(l[1:])
        err[hooks] = rp.window_error()
    print("summed squared reprojection error of the active window: %.6g without the optimiser, %.6g with" % (err[False], err[True]))
    assert err[True] < err[False]
