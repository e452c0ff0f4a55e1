"""CPU: a whole DAVIS240C recording directory through the facade -- tools::Davis240cRecording (images with their frames,
ground truth, calibration) and tools::Replayer (events and decoded frames merged by time), driven by
tests/cpp/recording_test.cpp, built plain and with the facade's OpenCV branch (test-only declarations).

The reference's reader scenario is rebuilt in tmp_path from the three frames under tests/golden/frontend (byte-identical
to the reference's test frames) and text files written here; its known answers are the data below."""
import json
import os
import shutil
import subprocess

import numpy as np
import pytest

import frontend_ref

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")
GOLDEN = os.path.join(HERE, "golden")

# the reference reader scenario: files and known answers
IMAGES_TXT = ("0.028046000 images/frame_00000000.png\n0.072111000 images/frame_00000001.png\n"
              "0.116176001 images/frame_00000002.png\n")
IMAGE_TIMES = [28046, 72111, 116176]
GROUNDTRUTH_TXT = ("0.072111000 1.0 0.0 0.0 0.707 0.0 0.0 0.707\n"
                   "0.116176001 0.0 0.0 1.0 0.0 0.707 0.0 0.707\n")
GT_TIMES = [72111, 116176]
GT_MATRICES = [
    [[1, 0, 0, 1], [0, 0, -1, 0], [0, 1, 0, 0], [0, 0, 0, 1]],
    [[0, 0, 1, 0], [0, 1, 0, 0], [-1, 0, 0, 1], [0, 0, 0, 1]],
]
CALIB_TXT = "501 499 249 251 0.11 0.011 0.0011 0.123 0.321\n"
CALIBRATION = dict(fx=501, fy=499, cx=249, cy=251, k1=0.11, k2=0.011, p1=0.0011, p2=0.123, k3=0.321)
EVENTS_TXT = ("0.000000000 33 39 1\n0.000011001 158 145 1\n0.000050000 88 143 0\n0.000055000 174 154 0\n"
              "0.000080001 112 139 1\n")


@pytest.fixture(scope="module")
def drivers(tmp_path_factory):
    out = tmp_path_factory.mktemp("recording_bin")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "recording.mk", "OUT=" + str(out),
                           str(out / "recording_test"), str(out / "recording_opencv_test")])
    return [str(out / "recording_test"), str(out / "recording_opencv_test")]


def _scenario(root, images_txt=IMAGES_TXT, frames=True):
    os.makedirs(os.path.join(root, "images"), exist_ok=True)
    if frames:
        for p in frontend_ref.FRAMES:
            shutil.copy(p, os.path.join(root, "images", os.path.basename(p)))
    for name, text in (("images.txt", images_txt), ("groundtruth.txt", GROUNDTRUTH_TXT), ("calib.txt", CALIB_TXT),
                       ("events.txt", EVENTS_TXT)):
        with open(os.path.join(root, name), "w") as f:
            f.write(text)
    return str(root)


def _run(cmd):
    out = subprocess.run(cmd, capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-3000:] + out.stderr[-3000:]
    return json.loads(out.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("flavour", [0, 1], ids=["plain", "opencv_branch"])
def test_reference_reader_scenario(drivers, tmp_path, flavour):
    d = _scenario(tmp_path / "data")
    dump = tmp_path / "dump"
    dump.mkdir()
    r = _run([drivers[flavour], "reader", d, str(dump)])
    assert [im["t_us"] for im in r["images"]] == IMAGE_TIMES
    for i, im in enumerate(r["images"]):
        assert (im["rows"], im["cols"]) == (180, 240)
        px = np.fromfile(dump / ("frame_%d.raw" % i), dtype=np.uint8).reshape(180, 240)
        assert np.array_equal(px, frontend_ref.read_png_gray8(frontend_ref.FRAMES[i]))
    assert [g["t_us"] for g in r["groundtruth"]] == GT_TIMES
    for g, m in zip(r["groundtruth"], GT_MATRICES):
        np.testing.assert_allclose(np.array(g["matrix"]).reshape(4, 4), np.array(m, dtype=float), rtol=0, atol=1e-9)
        np.testing.assert_allclose(g["translation"], np.array(m, dtype=float)[:3, 3], rtol=0, atol=1e-12)
    assert r["calibration"] == pytest.approx(CALIBRATION, rel=1e-15)
    assert r["events"] == 5


def test_only_newline_terminated_lines_count(drivers, tmp_path):
    d = _scenario(tmp_path / "data", images_txt=IMAGES_TXT.rstrip("\n"))
    r = _run([drivers[0], "reader", d, str(tmp_path)])
    assert [im["t_us"] for im in r["images"]] == IMAGE_TIMES[:2]


def test_a_missing_frame_file_is_an_error_naming_it(drivers, tmp_path):
    d = _scenario(tmp_path / "data", images_txt=IMAGES_TXT + "0.2 images/frame_00000009.png\n")
    r = _run([drivers[0], "reader", d, str(tmp_path)])
    assert "images" not in r
    assert "frame_00000009.png" in r["images_error"]
    # a file that is no PNG names the file too
    with open(os.path.join(d, "images", "frame_00000001.png"), "wb") as f:
        f.write(b"not a png")
    r = _run([drivers[0], "reader", _scenario(tmp_path / "data", frames=False), str(tmp_path)])
    assert "frame_00000001.png" in r["images_error"] and "signature" in r["images_error"]


def test_replayer_delivery_order(drivers, tmp_path):
    """The reference's replayer scenario (events at 0 and 3 us, frames at 1 and 4 us): the deliveries of next(),
    nextImage() twice, nextInterval(3), next() after reset(), and nextChunk; tools::StreamPump agrees."""
    d = tmp_path / "data"
    os.makedirs(d / "images")
    shutil.copy(os.path.join(GOLDEN, "replayer", "events.txt"), d / "events.txt")
    shutil.copy(os.path.join(GOLDEN, "replayer", "images.txt"), d / "images.txt")
    for p in frontend_ref.FRAMES[:2]:
        shutil.copy(p, d / "images" / os.path.basename(p))
    for exe in drivers:
        r = _run([exe, "replay", str(d)])
        order = [[0, "E"], [1, "I"], [3, "E"], [4, "I"]]
        assert r["next"] == order
        assert r["nextImage2"] == order
        assert r["nextInterval3"] == order[:3]
        assert r["afterReset"] == order[:1]
        assert r["chunks"] == order and r["chunkEvents"] == [1, 1]
        assert (r["pumpNext"], r["pumpNextImage2"], r["pumpNextInterval3"]) == (r["next"], r["nextImage2"],
                                                                                r["nextInterval3"])
        assert r["groundTruth"] == 0 and r["groundTruthCallbacks"] == 0  # no groundtruth.txt: empty, as the reference


def test_replayer_on_a_synthetic_recording_matches_the_stream_pump(drivers, synth, tmp_path):
    d = str(tmp_path / "rec")
    info = synth.make_recording(d, seed=3, duration_s=0.2, velocity=(30.0, 10.0))
    r = _run([drivers[0], "replay", d])
    kinds = [k for _, k in r["next"]]
    assert kinds.count("I") == info["frames"] and kinds.count("E") > 1000
    times = [t for t, _ in r["next"]]
    assert times == sorted(times)
    assert r["next"] == r["pumpNext"] and r["chunks"] == r["next"]
    assert r["nextImage2"] == r["pumpNextImage2"] and r["nextInterval3"] == r["pumpNextInterval3"]
    assert sum(r["chunkEvents"]) == kinds.count("E")
    assert r["groundTruth"] > 0 and r["groundTruthCallbacks"] == 0
