"""GPU: rectified frames through the C++ facade and the tools -- FeatureDetector::rectifyFrames,
tools::EvaluatorParams::rectifyFrames (tests/cpp/rectify_frames_test.cpp), tools/track_recording --rectify-frames --
against tests/rectify_ref.py, and the physical check of tests/test_gpu_camera_facade.py with the fitted camera."""
import json
import os
import subprocess

import numpy as np
import pytest

import frontend_ref
import rectify_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CPP = os.path.join(HERE, "cpp")
CSRC = os.path.join(ROOT, "event-based-odomety_amd", "csrc")
TOOL = os.path.join(ROOT, "event-based-odomety_amd", "tools", "track_recording")

LENS = (-0.368, 0.151, 0.0, 0.0)
CAM = (200.0, 200.0, 120.0, 90.0, LENS[0], LENS[1], 0.0, LENS[2], LENS[3])
W, H = 240, 180


@pytest.fixture(scope="module")
def driver(ebo, tmp_path_factory):
    ebo.lib()
    out = tmp_path_factory.mktemp("rectify_bin")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "rectify.mk", "OUT=" + str(out), str(out / "rectify_frames_test")])
    return str(out / "rectify_frames_test")


def test_rectify_frames_driver_compiles(driver):
    """CPU: rectifyFrames, the setRectification overload, projectBatch and fitRectifiedCamera compile under -Wall
    -Wextra against the library."""
    assert os.path.exists(driver)


@pytest.fixture(scope="module")
def distorted_recording(synth, tmp_path_factory):
    d = tmp_path_factory.mktemp("lens") / "rec"
    info = synth.make_recording(str(d), seed=1, duration_s=0.25, distortion=LENS)
    return str(d), info


def run(cmd):
    out = subprocess.run(["timeout", "-k", "10", "300"] + cmd, capture_output=True, text=True)
    print(out.stdout[-3000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-2000:]
    return out.stdout


@pytest.mark.gpu
def test_identity_rectification_changes_nothing(synth, driver, tmp_path):
    """Zero distortion and rectifiedCamera = K: the remap returns every frame byte for byte and the table is the
    identity, so patches, tracks and trajectory are those of the plain run, bit for bit."""
    d = tmp_path / "rec"
    synth.make_recording(str(d))
    files = {}
    for mode in ("plain", "null"):
        out = tmp_path / mode
        out.mkdir()
        run([driver, "replay", str(d), str(out), mode])
        files[mode] = {n: open(out / n, "rb").read() for n in ("trajectory.txt", "final_cost.txt", "patches.txt")}
    assert len(files["plain"]["trajectory.txt"].splitlines()) > 10 and len(files["plain"]["patches.txt"].splitlines()) > 2
    for n in files["plain"]:
        assert files["null"][n] == files["plain"][n], n


@pytest.mark.gpu
def test_hooks_see_the_rectified_frame_and_patches_the_rectified_events(driver, distorted_recording, tmp_path):
    d, info = distorted_recording
    stdout = run([driver, "hooks", d, str(tmp_path)])
    assert "all passed" in stdout
    first = sorted(os.listdir(os.path.join(d, "images")))[0]
    raw = frontend_ref.read_png_gray8(os.path.join(d, "images", first))
    r = rectify_ref.fit(CAM, W, H)
    want = rectify_ref.rectify_image(CAM, r, raw)
    assert (want != raw).mean() > 0.3  # the lens moves the picture
    for hook in ("detect", "gradients", "add"):
        got = np.fromfile(tmp_path / ("hook_%s.bin" % hook), dtype=np.uint8).reshape(H, W)
        assert np.array_equal(got, want), hook
    # the events added to the first patch: the table's images of the raw events, newest first, capped
    lines = open(tmp_path / "patch_events.txt").read().splitlines()
    x0, y0, pw, ph, cap = (float(v) for v in lines[0].split())
    got = np.array([[int(v) for v in ln.split()] for ln in lines[1:]], dtype=np.int64).reshape(-1, 4)
    ev = np.loadtxt(tmp_path / "raw_events.txt", dtype=np.int64).reshape(-1, 4)
    _, lut, ok = rectify_ref.forward_map(CAM, r, W, H)
    assert ok
    inside = (ev[:, 0] >= 0) & (ev[:, 0] < W) & (ev[:, 1] >= 0) & (ev[:, 1] < H)
    rect = ev.copy()
    rect[inside, 0] = lut[ev[inside, 1], ev[inside, 0], 0]
    rect[inside, 1] = lut[ev[inside, 1], ev[inside, 0], 1]
    in_patch = (rect[:, 0] >= x0) & (rect[:, 0] < x0 + pw) & (rect[:, 1] >= y0) & (rect[:, 1] < y0 + ph)
    want_ev = rect[in_patch][::-1][:int(cap)]
    raw_in_patch = ev[(ev[:, 0] >= x0) & (ev[:, 0] < x0 + pw) & (ev[:, 1] >= y0) & (ev[:, 1] < y0 + ph)][::-1][:int(cap)]
    print("patch at (%.1f, %.1f): %d events, %d of them moved by the table" % (
        x0, y0, len(got), int((want_ev[:, :2] != ev[in_patch][::-1][:int(cap)][:, :2]).any(axis=1).sum())))
    assert len(got) > 0 and np.array_equal(got, want_ev)
    assert not np.array_equal(got, raw_in_patch)  # not the raw events of that rect


@pytest.mark.gpu
def test_track_recording_rectify_frames_with_odometry(ebo, distorted_recording, tmp_path):
    d, info = distorted_recording
    subprocess.check_call(["make", "-s", "-C", CSRC, "track_recording"])
    out = tmp_path / "out"
    out.mkdir()
    stdout = run([TOOL, "--dataset", d, "--out", str(out), "--rectify-frames", "--odometry"])
    line = json.loads(stdout.strip().splitlines()[-1])
    assert line["frames"] > 2 and line["events"] > 0 and line["odometry"] is True
    calib = [float(v) for v in open(out / "calib_rectified.txt").read().split()]
    want = rectify_ref.fit(CAM, W, H)
    assert len(calib) == 9 and np.array_equal(np.array(calib).view(np.uint64), np.array(want).view(np.uint64))
    tracks = np.loadtxt(out / "trajectory.txt").reshape(-1, 4)
    assert len(tracks) > 10
    assert np.isfinite(tracks).all()
    assert (tracks[:, 2] >= 0).all() and (tracks[:, 2] <= W - 1).all() and (tracks[:, 3] >= 0).all() and (tracks[:, 3] <= H - 1).all()
    assert os.path.exists(out / "keyframe_poses.txt")


@pytest.mark.gpu
def test_contrast_of_a_rigidly_translating_scene_with_the_fitted_camera(ebo, distorted_recording):
    """The physical check of tests/test_gpu_camera_facade.py (measured there on an MI355X, six windows: warped count-image
    variance 2.2256 without rectification, 1.8146 with the rectified camera that keeps K) recomputed with the fitted
    camera, which keeps every event on the sensor.  Reported (the figures belong in DESIGN.md 4.12), not
    asserted: the fitted camera shrinks the picture, so more events share a pixel and the figures of the three
    geometries are not on one scale."""
    d, info = distorted_recording
    ev = ebo.read_events_txt(os.path.join(d, "events.txt"), cap=info["events"] + 16)
    offsets = np.arange(0, len(ev) + 1, 15000, dtype=np.uint64)
    assert len(offsets) >= 5
    opts = ebo.default_solver(mode=ebo.SOLVE_INDEPENDENT, max_num_iterations=30)
    sums = {}
    with ebo.Context(loss=ebo.LOSS_VARIANCE, max_windows=8, max_events=8 * 15000) as c:
        fitted = c.fit_rectified_camera(CAM)
        for name, r in (("raw", None), ("same K", rectify_ref.same_k(CAM)), ("fitted", fitted)):
            if r is not None:
                c.set_rectification_camera(CAM, r)
            flows, warped, integrated, summ, status = c.compensate_windows(ev, offsets, opts)
            assert not status.any()
            sums[name] = (float(sum(w.var() for w in warped)), float(sum(w.var() for w in integrated)),
                          float(sum(w.sum() for w in integrated)))
    print("count-image variance over %d windows (warped / un-warped / events on the sensor): " % (len(offsets) - 1) +
          "; ".join("%s %.4f / %.4f / %.0f" % ((k,) + v) for k, v in sums.items()) + "  [2.2256 -> 1.8146 before]")
    assert all(np.isfinite(v) for s in sums.values() for v in s)
