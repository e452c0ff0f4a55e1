"""GPU: tools/track_recording --track-error end to end on a synth.make_recording directory.  The run writes
groundtruth_tracks.txt and track_errors.txt; recomputing from the written trajectory.txt, the recording's frames and the
Python bindings (track_seeds, Context.reference_tracks, Context.track_errors, track_error_summary) reproduces
groundtruth_tracks.txt, track_errors.txt's integers exactly and its doubles to the printed digits (17 significant, so
bit for bit), and the JSON line's four fields.  Once on a plain recording and once through a lens with --rectify-frames,
where the frames KLT sees are the rectified ones."""
import json
import os
import subprocess

import numpy as np
import pytest

import trackerr_ref as V

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "event-based-odomety_amd", "csrc")
TOOL = os.path.join(ROOT, "event-based-odomety_amd", "tools", "track_recording")
LENS = (-0.368, 0.151, 0.0, 0.0)
CAM = (200.0, 200.0, 120.0, 90.0, LENS[0], LENS[1], 0.0, LENS[2], LENS[3])
W, H = 240, 180


@pytest.fixture(scope="module")
def tool():
    subprocess.check_call(["make", "-s", "-C", CSRC, "track_recording"])
    return TOOL


def run(cmd):
    out = subprocess.run(["timeout", "-k", "10", "300"] + [str(c) for c in cmd], capture_output=True, text=True)
    print(out.stdout[-3000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


def tracks_of(points):
    """Track records -> (ids in the order of their first point, [(t_us, xy), ..]), each track in time order (stable) as
    tools::TrackEvaluator puts it: a patch's first two points carry the first two frames' times, the event-based points
    that follow begin inside that interval."""
    ids, groups = [], {}
    for p in points:
        k = int(p["id"])
        if k not in groups:
            ids.append(k)
            groups[k] = []
        groups[k].append((int(p["t_us"]), float(p["x"]), float(p["y"])))
    for k in ids:
        groups[k].sort(key=lambda s: s[0])                    # list.sort is stable
    return ids, [(np.array([s[0] for s in groups[k]], np.int64), np.array([s[1:] for s in groups[k]], np.float64).reshape(-1, 2))
                 for k in ids]


def recompute(ebo, data, out, tau, rectified):
    ids, ests = tracks_of(ebo.read_tracks_txt(out / "trajectory.txt"))
    stamps, frames = [], []
    for line in open(os.path.join(data, "images.txt")):
        sec, name = line.split()
        stamps.append(int(float(sec) * 1e6))                  # the reader's truncation
        frames.append(ebo.read_png8(os.path.join(data, name)))
    with ebo.Context(image_w=W, image_h=H) as c:
        if rectified is not None:
            c.set_rectification_camera(CAM, rectified)
            frames = [c.rectify_image(f) for f in frames]
        frames = np.stack(frames)
        seed_frame, seed_xy = ebo.track_seeds(ests, stamps)
        first, last, xy = c.reference_tracks(frames, stamps, seed_frame, seed_xy)
        gts = [(np.array(stamps[first[k]:last[k] + 1], np.int64), xy[k, first[k]:last[k] + 1]) if first[k] >= 0 else
               (np.zeros(0, np.int64), np.zeros((0, 2))) for k in range(len(ids))]
        results = c.track_errors(ests, gts, [tau])
    return ids, ests, gts, results, frames


def check_run(ebo, data, out, line, tau, rectified=None):
    assert os.path.exists(out / "groundtruth_tracks.txt") and os.path.exists(out / "track_errors.txt")
    ids, ests, gts, results, frames = recompute(ebo, data, out, tau, rectified)
    # the reference tracks as written: the same ids, frame times and positions.  The file has 8 decimals: half a unit
    # of the last, plus the rounding of the parsed number and of the difference, each within an ulp of a coordinate < 256
    gt_ids, gt_file = tracks_of(ebo.read_tracks_txt(out / "groundtruth_tracks.txt"))
    assert gt_ids == [k for k, g in zip(ids, gts) if len(g[0])]
    for (t, xy), (wt, wxy) in zip(gt_file, [g for g in gts if len(g[0])]):
        assert np.array_equal(t, wt) and np.abs(xy - wxy).max() <= 0.5e-8 + 2 * np.spacing(256.0)
    rows = [ln.split() for ln in open(out / "track_errors.txt").read().splitlines()]
    assert len(rows) == len(ids) <= line["tracks"] and all(len(r) == 8 for r in rows)
    for r, k, w in zip(rows, ids, results):
        assert (int(r[0]), int(r[1]), int(r[6]), int(r[7])) == (k, w["n_inliers"], w["cut"], w["status"]), (r, w)
        for got, want in zip(r[2:6], (w["err_mean"], w["err_rmse"], w["err_max"], np.float64(w["age_us"]) * 1e-6)):
            assert V.same_bits(float(got), want), (r, w)
    s = ebo.track_error_summary(results)
    assert V.same_bits(line["track_error_mean"], s["mean_error"]) and V.same_bits(line["feature_age_mean_s"], s["mean_age_s"])
    assert line["tracks_counted"] == s["counted"] and line["tracks_discarded"] == s["discarded"]
    # the device against the restatement on the same inputs, and not vacuous: tracks were judged
    want, _ = V.track_errors(ests, gts, [tau])
    assert all(V.same_result(g, w) for g, w in zip(results, want))
    print("tracks %d, counted %d, discarded %d, mean error %.3f px, mean age %.3f s" %
          (len(ids), s["counted"], s["discarded"], s["mean_error"], s["mean_age_s"]))
    assert s["counted"] >= 1
    return frames


def test_track_error_of_a_tracker_experiment(ebo, synth, tool, tmp_path):
    data = tmp_path / "rec"
    synth.make_recording(str(data), seed=1, duration_s=0.4)
    out = tmp_path / "out"
    out.mkdir()
    line = run([tool, "--dataset", data, "--out", out, "--tracker-experiment", "--track-error"])
    check_run(ebo, str(data), out, line, 5.0)
    # the threshold is the flag's; the tracker's own files do not depend on it
    out2 = tmp_path / "out2"
    out2.mkdir()
    line2 = run([tool, "--dataset", data, "--out", out2, "--tracker-experiment", "--track-error", "--track-error-threshold", "0.75"])
    check_run(ebo, str(data), out2, line2, 0.75)
    assert open(out / "trajectory.txt", "rb").read() == open(out2 / "trajectory.txt", "rb").read()

def test_track_error_with_rectified_frames(ebo, synth, tool, tmp_path):
    data = tmp_path / "rec"
    synth.make_recording(str(data), seed=1, duration_s=0.4, distortion=LENS)
    out = tmp_path / "out"
    out.mkdir()
    line = run([tool, "--dataset", data, "--out", out, "--tracker-experiment", "--rectify-frames", "--track-error"])
    rectified = [float(v) for v in open(out / "calib_rectified.txt").read().split()]
    rectified = rectified[:6] + [rectified[8], rectified[6], rectified[7]]         # calib.txt's order -> the struct's
    frames = check_run(ebo, str(data), out, line, 5.0, rectified)
    raw = ebo.read_png8(os.path.join(str(data), "images", "frame_00000000.png"))
    assert (frames[0] != raw).mean() > 0.3                                         # KLT saw the rectified frames
