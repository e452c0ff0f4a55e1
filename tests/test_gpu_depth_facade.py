"""GPU: the facade's depth-map side end to end.  tools/track_recording --depth-map runs tools::Evaluator with
visual_odometry::DepthMapper over a synth.make_recording directory -- a textured plane at depth 1 seen by a camera that
translates parallel to it -- and depth.txt / points.txt equal the restatement (tests/depth_ref.py) run on the same
windows and poses, unbatched and under --window-batch 4 with the same bytes; the median of the kept depths lies within
one plane of 1.0; a distorted recording without --rectify is refused; a recording's other files are written as without
the flag."""
import json
import os
import subprocess

import numpy as np
import pytest

import depth_ref as D

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CSRC = os.path.join(ROOT, "event-based-odomety_amd", "csrc")
TOOL = os.path.join(ROOT, "event-based-odomety_amd", "tools", "track_recording")
W, H, FOCAL = 240, 180, 200.0
CAM = (FOCAL, FOCAL, W / 2.0, H / 2.0)


def run_tool(d, out, flags, expect=0):
    out.mkdir()
    r = subprocess.run(["timeout", "-k", "10", "600", TOOL, "--dataset", d, "--out", str(out), "--tracker-experiment"] + flags,
                       capture_output=True, text=True)
    assert (r.returncode == 0) == (expect == 0), r.stdout[-2000:] + r.stderr[-2000:]
    return r


@pytest.fixture(scope="module")
def tool(ebo):
    ebo.lib()
    subprocess.check_call(["make", "-s", "-C", CSRC, "track_recording"])
    return TOOL


@pytest.fixture(scope="module")
def plane(synth, tmp_path_factory):
    """The default threshold, 0.25: a window of 15 000 events spans about 36 ms, 1.7 px of the scene's 47 px/s, and
    half a second holds 13 of them and about 23 px of parallax at depth 1."""
    d = tmp_path_factory.mktemp("plane") / "rec"
    info = synth.make_recording(str(d), seed=1, duration_s=0.5)
    return str(d), info


def read_windows(path):
    lines = open(path).read().splitlines()
    assert lines[0].startswith("reference ")
    ref = np.array([float(v) for v in lines[0].split()[1:]])
    rows = np.array([[float(v) for v in ln.split()] for ln in lines[1:]]).reshape(-1, 15)
    return ref, rows


def test_the_depth_map_of_a_plane_equals_the_restatement(ebo, tool, plane, tmp_path):
    d, info = plane
    ev = ebo.read_events_txt(os.path.join(d, "events.txt"), cap=info["events"] + 16)
    gt = np.loadtxt(os.path.join(d, "groundtruth.txt"))
    files = {}
    for name, flags in (("one", []), ("batch", ["--window-batch", "4"])):
        out = tmp_path / name
        r = run_tool(d, out, ["--depth-map"] + flags)
        js = json.loads(r.stdout.strip().splitlines()[-1])
        files[name] = {f: (out / f).read_bytes() for f in ("depth.txt", "points.txt", "depth_windows.txt")}
        assert js["depth_pixels"] == len(files[name]["depth.txt"].splitlines()) > 0
        assert os.path.exists(out / "trajectory.txt")
    # batched under --window-batch, on the batch context: the same bytes
    assert files["batch"] == files["one"]
    ref, rows = read_windows(tmp_path / "one" / "depth_windows.txt")
    n = len(rows)
    assert js["depth_windows"] == n >= js["windows"] >= 1 and np.all(rows[:, 2] == 1)
    # the windows are the whole 15 000-event chunks of the stream up to the last frame
    assert 8 <= n <= len(ev) // 15000
    wins = [ev[k * 15000:(k + 1) * 15000] for k in range(n)]
    t_refs = [int(float(int(w["t_us"][0]) + int(w["t_us"][-1])) * 0.5) for w in wins]
    assert np.array_equal(rows[:, 0].astype(np.int64), np.array(t_refs)) and np.all(rows[:, 1] == 15000)
    # the poses are the ground truth's, interpolated: identity rotation, the translation linear between the samples
    poses = rows[:, 3:]

    def truth(t_us):
        return D.pose(t=(np.interp(t_us * 1e-6, gt[:, 0], gt[:, 1]), np.interp(t_us * 1e-6, gt[:, 0], gt[:, 2]), 0.0))
    mid = (int(round(gt[0, 0] * 1e6)) + int(round(gt[-1, 0] * 1e6))) // 2
    # syncGroundTruth takes the interpolation parameter in float: 2^-24 of a 10 ms step at 0.24 units/s is 1.4e-10; the
    # middle of the span may round by a microsecond, 2.4e-7
    assert np.abs(ref - truth(mid)).max() <= 5e-7
    for k in range(n):
        assert np.abs(poses[k] - truth(t_refs[k])).max() <= 1e-9, k
    assert np.abs(poses[-1][9:] - poses[0][9:]).max() * FOCAL >= 10.0  # pixels of parallax at depth 1
    # the restatement on the same windows and poses, with the defaults
    p = D.DEFAULTS
    z = D.planes(p["nz"], p["z_near"], p["z_far"])
    Hq = D.volume(wins, poses, ref, CAM, W, H, z)
    index, conf, depth, points = D.extract(Hq, z, CAM, p["box_radius"], p["min_excess"], p["median_radius"])
    ys, xs = np.nonzero(index >= 0)
    got = np.loadtxt(tmp_path / "one" / "depth.txt", ndmin=2)
    assert np.array_equal(got[:, 0].astype(int), xs) and np.array_equal(got[:, 1].astype(int), ys)
    assert np.array_equal(got[:, 2], depth[ys, xs]) and np.array_equal(got[:, 3].astype(np.uint32), conf[ys, xs])
    # the points, taken to the world frame by the reference pose: ((r0 x + r1 y) + r2 z) + t per row
    R, t = ref[:9].reshape(3, 3), ref[9:]
    world = np.stack([((R[i, 0] * points[:, 0] + R[i, 1] * points[:, 1]) + R[i, 2] * points[:, 2]) + t[i] for i in range(3)], axis=1)
    assert np.array_equal(np.loadtxt(tmp_path / "one" / "points.txt", ndmin=2), world)
    # the plane is at depth 1: plane 34 of 64.  Measured with the restatement alone: 3440 pixels kept, their median plane
    # 34, 90 % of them within one plane of it
    k_true = D.true_plane(1.0, p["nz"], p["z_near"], p["z_far"])
    k_med = np.median(index[index >= 0])
    print("kept %d, median plane %.1f (true %d), median depth %.4f, within one plane %.3f"
          % (len(ys), k_med, k_true, np.median(depth[ys, xs]), np.mean(np.abs(index[ys, xs] - k_true) <= 1)))
    assert abs(k_med - k_true) <= 1
    assert z[k_true - 1] <= np.median(got[:, 2]) <= z[k_true + 1]  # plane 0 is the nearest


def test_a_distorted_recording_needs_rectify(ebo, tool, synth, tmp_path):
    d = tmp_path / "lens"
    synth.make_recording(str(d), seed=2, duration_s=0.1, distortion=(-0.368, 0.151, 0.0, 0.0))
    r = run_tool(str(d), tmp_path / "refused", ["--depth-map"], expect=1)
    assert "--rectify" in r.stderr + r.stdout
    assert not os.path.exists(tmp_path / "refused" / "depth.txt")
    run_tool(str(d), tmp_path / "rectified", ["--rectify", "--depth-map"])
    assert os.path.exists(tmp_path / "rectified" / "depth.txt") and os.path.exists(tmp_path / "rectified" / "points.txt")
    # without the flag the other files are what they are with it
    run_tool(str(d), tmp_path / "plain", ["--rectify"])
    for name in ("trajectory.txt", "final_cost.txt"):
        assert (tmp_path / "plain" / name).read_bytes() == (tmp_path / "rectified" / name).read_bytes(), name
    assert not os.path.exists(tmp_path / "plain" / "depth.txt")
