"""GPU: the facade's map maintenance end to end (tests/cpp/map_maintenance_test.cpp) on the six-keyframe scene of
tests/test_gpu_odometry_facade.py.  With useDeviceMapMaintenance an optimizer hook, which runs just before the
maintenance, plants the damage at the fifth keyframe -- five tracks whose corners are moved by 40, 80 and 120 px, up and
down in turn, in the active keyframes after their first, two landmarks mirrored behind the cameras -- and records what the
maintenance is about to see; at every keyframe the summary and the map afterwards equal landmark_ref.maintain on that
record, bit for bit: the corrupted landmarks are gone while their observations remain, the mirrored ones are
triangulated again.  Without the call every output equals the existing driver's (tests/cpp/rpe_facade_test.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import abspose_ref as ap
import camera_ref
import landmark_ref as L
from test_gpu_align_facade import ACTIVE, loads, same_json

pytestmark = pytest.mark.gpu

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")
CANDIDATE = ("timestamp", "pose", "Tw2c", "inliers", "localize")
PLANT_AT = 4


@pytest.fixture(scope="module")
def driver(ebo, tmp_path_factory):
    ebo.lib()
    out = tmp_path_factory.mktemp("map_maintenance")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "map_maintenance.mk", "OUT=" + str(out), str(out / "map_maintenance_test")])
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "rpe.mk", "OUT=" + str(out), str(out / "rpe_facade_test")])
    fs = ap.make_facade_scene()
    fs["x"].tofile(str(out / "x.f64"))
    fs["visible"].astype(np.float64).tofile(str(out / "visible.f64"))
    np.zeros(0).tofile(str(out / "samples.f64"))
    scene = [repr(float(v)) for v in camera_ref.DAVIS] + [str(out / "x.f64"), str(out / "visible.f64"), str(len(fs["x"])), "55",
                                                          str(ACTIVE), str(ap.FACADE_SEED)]

    def call(cmd):
        r = subprocess.run(["timeout", "-k", "10", "300"] + cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return loads(r.stdout)

    def run(mode, edits=()):
        np.asarray(edits, np.float64).reshape(-1).tofile(str(out / "edits.f64"))
        return call([str(out / "map_maintenance_test")] + scene + [str(mode), str(out / "edits.f64")])

    def existing():
        return call([str(out / "rpe_facade_test"), "frontend"] + scene + [str(out / "samples.f64"), "0"])

    return fs, run, existing


def state(js):
    active = [(kid, np.array(p).reshape(3, 4), {int(t): np.array([u, v]) for t, u, v in corners}) for kid, p, corners in js["active"]]
    return active, {int(t): ids for t, ids in js["observations"]}, {int(t): np.array(p) for t, *p in js["landmarks"]}


def check_against_the_policy(got):
    prm = dict(threshold=got["threshold"], min_parallax=got["min_parallax"], min_inliers=got["min_inliers"],
               max_hypotheses=got["max_hypotheses"], seed=got["seed"])
    assert L.same_bits(prm["threshold"], L.THRESHOLD) and L.same_bits(prm["min_parallax"], L.MIN_PARALLAX)
    summaries = []
    for c in got["candidates"]:
        active, observations, landmarks = state(c["input"])
        summary, after = L.maintain(camera_ref.DAVIS, active, observations, landmarks, prm)
        assert c["summary"] == [summary[k] for k in L.SUMMARY], (c["timestamp"], c["summary"], summary)
        want = [[t] + [float(v) for v in after[t]] for t in sorted(after)]
        assert same_json(c["landmarks_after"], want), c["timestamp"]
        assert c["observations_after"] == c["input"]["observations"]
        summaries.append(summary)
    return summaries


def test_without_the_call_every_output_is_the_existing_drivers(driver):
    _, run, existing = driver
    plain, old = run(0), existing()
    for key in ("active", "stored_frames", "landmarks"):
        assert same_json(plain[key], old[key]), key
    assert len(plain["candidates"]) == len(old["candidates"]) == 6
    for c, e in zip(plain["candidates"], old["candidates"]):
        assert same_json({k: c[k] for k in CANDIDATE}, {k: e[k] for k in CANDIDATE}), c["timestamp"]
        assert c["summary"] == [0] * 6 and c["input"] is None


def test_the_maintained_map_equals_the_policy_keyframe_by_keyframe(driver):
    fs, run, _ = driver
    clean = run(1)
    summaries = check_against_the_policy(clean)
    assert summaries[0]["candidates"] == 0 and summaries[-1]["candidates"] > 50
    # what to damage at the fifth keyframe: tracks that have a landmark there and at least three active observations
    active, observations, landmarks = state(clean["candidates"][PLANT_AT]["input"])
    index = {kid: i for i, (kid, _, _) in enumerate(active)}
    full = [t for t in sorted(landmarks) if sum(k in index and t in active[index[k]][2] for k in observations[t]) >= 3]
    assert len(full) >= 20
    corrupted, mirrored = full[2:12:2], full[13:17:2]
    edits = []
    for j, t in enumerate(corrupted):
        seen = [k for k in sorted(observations[t]) if k in index and t in active[index[k]][2]]
        # up 40, down 80, up 120 px, across the epipolar lines of a camera that moves sideways: no two of a track's
        # moved corners agree with each other or with the first
        for i, k in enumerate(seen[1:]):
            edits.append([0, PLANT_AT, t, fs["timestamps"].index(k), 5.0 * j, 40.0 * (i + 1) * (-1.0) ** i])
    first = active[0][1]
    for t in mirrored:
        edits.append([1, PLANT_AT, t] + list(2.0 * first[:, 3] - landmarks[t] - [0.0, 0.0, 1.0]))
    got = run(1, edits)
    summaries = check_against_the_policy(got)
    for k in range(PLANT_AT):
        assert same_json(got["candidates"][k]["landmarks_after"], clean["candidates"][k]["landmarks_after"])
    s = summaries[PLANT_AT]
    print("at the fifth keyframe:", s)
    assert s["culled"] >= len(corrupted) and s["retriangulated"] >= len(mirrored), s
    after = {int(t) for t, *_ in got["candidates"][PLANT_AT]["landmarks_after"]}
    observed = {int(t) for t, _ in got["candidates"][PLANT_AT]["observations_after"]}
    assert not after & set(corrupted) and set(corrupted) <= observed and set(mirrored) <= after
    # the mirrored landmarks are back in front of the cameras, near where they were
    fixed = {int(t): np.array(p) for t, *p in got["candidates"][PLANT_AT]["landmarks_after"]}
    for t in mirrored:
        assert np.linalg.norm(fixed[t] - landmarks[t]) <= 0.05 * np.linalg.norm(landmarks[t] - first[:, 3])
