"""CPU: the camera model -- tests/camera_ref.py (the numpy restatement of include/ebo.h's rules) and the facade's host
common::CameraModel<double>, driven by tests/cpp/camera_model_lines_test.cpp (built by tests/cpp/camera.mk with
-ffp-contract=off).

The reference's own camera test enters as data: the DAVIS240C calibration, the 19 x 19 grid of points (x, y, 10),
x, y in [-9, 9], and its bound, Eigen's isApprox(., 0.01): |a - b| <= 0.01 * min(|a|, |b|)."""
import ctypes as C
import hashlib
import json
import os
import re
import subprocess

import numpy as np
import pytest

import camera_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CPP = os.path.join(HERE, "cpp")

CAMERAS = {"davis": camera_ref.DAVIS, "reader": camera_ref.READER, "pinhole": camera_ref.PINHOLE}
IS_APPROX = 0.01

# sha256 of synth.make_recording(path, seed=3, duration_s=0.1) as written BEFORE the `distortion` keyword existed
RECORDING_HASHES = {
    "calib.txt": "1c746c6178607eb14f9d9df6ef70ee02f3d3bc02aa7577ca6949fac53c792550",
    "events.txt": "c4d5057c9b428f6bbaef621683c9fabbdc533608f337990dc2539b566bc33b2a",
    "groundtruth.txt": "10ec1668260e277986e885f90c980560aeb55adfd938c191bc46caac90de3f8e",
    "images.txt": "89e150689c7b3b08ebaa0890e5d56e4136337b8268d60c721e82f06fdfcca13b",
    "images/frame_00000000.png": "bcef468338e1a452f2078b6a5eaf50ac53927ed59fe8cc4b5c5ae4ae0da9ef47",
    "images/frame_00000001.png": "bfd8c7edb06c22d94888f76a0e8c6fa401688a847adfb27ff86e37476fde2f82",
}


@pytest.fixture(scope="module")
def driver(tmp_path_factory):
    out = tmp_path_factory.mktemp("camera_bin")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "camera.mk", "OUT=" + str(out),
                           str(out / "camera_model_lines_test")])
    return str(out / "camera_model_lines_test")


def _facade(driver, tmp_path, mode, cam, pts):
    src, dst = tmp_path / (mode + "_in.f64"), tmp_path / (mode + "_out.f64")
    np.ascontiguousarray(pts, dtype="<f8").tofile(src)
    out = subprocess.run([driver, mode] + [repr(float(v)) for v in cam] + [str(src), str(dst)], capture_output=True,
                         text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    return np.fromfile(dst, dtype="<f8").reshape(len(pts), 2 if mode == "project" else 3)


def reference_grid():
    xs, ys = np.meshgrid(np.arange(-9, 10), np.arange(-9, 10), indexing="ij")
    return np.stack([xs.ravel(), ys.ravel(), np.full(xs.size, 10)], axis=1).astype(np.float64)


def assert_is_approx(a, b):
    """Eigen's a.isApprox(b, 0.01), row by row."""
    d = np.linalg.norm(a - b, axis=1)
    bound = IS_APPROX * np.minimum(np.linalg.norm(a, axis=1), np.linalg.norm(b, axis=1))
    worst = int(np.argmax(d - bound))
    assert (d <= bound).all(), (worst, a[worst], b[worst], d[worst], bound[worst])


def seeded_points(seed, n):
    """Points in front of the camera and pixels around a DAVIS-sized sensor, corners and beyond included."""
    rng = np.random.default_rng(seed)
    p3 = np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(0.5, 20, n)], axis=1)
    uv = np.stack([rng.uniform(-40, 400, n), rng.uniform(-40, 300, n)], axis=1)
    uv[:8] = [[0, 0], [239, 0], [0, 179], [239, 179], [132.192071378, 110.712660011], [120, 90], [-40, -40], [0.5, 179.5]]
    return p3, uv


def test_reference_scenario_in_camera_ref():
    p = reference_grid()
    assert len(p) == 361
    back = camera_ref.unproject(camera_ref.DAVIS, camera_ref.project(camera_ref.DAVIS, p))
    assert_is_approx(back, p / np.linalg.norm(p, axis=1, keepdims=True))


def test_reference_scenario_in_the_facade(driver, tmp_path):
    p = reference_grid()
    px = _facade(driver, tmp_path, "project", camera_ref.DAVIS, p)
    back = _facade(driver, tmp_path, "unproject", camera_ref.DAVIS, px)
    assert_is_approx(back, p / np.linalg.norm(p, axis=1, keepdims=True))


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_facade_is_bit_equal_to_camera_ref(driver, tmp_path, name):
    cam = CAMERAS[name]
    p3, uv = seeded_points(11, 4096)
    got = _facade(driver, tmp_path, "project", cam, p3)
    want = camera_ref.project(cam, p3)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))
    got = _facade(driver, tmp_path, "unproject", cam, uv)
    want = camera_ref.unproject(cam, uv)
    assert np.array_equal(got.view(np.uint64), want.view(np.uint64))


def test_facade_caller_statements_and_dual_scalar(driver):
    out = subprocess.run([driver, "self"], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    assert json.loads(out.stdout.strip().splitlines()[-1]) == {"self": "ok"}


def test_zero_distortion_rectifies_to_the_identity():
    for w, h in ((240, 180), (346, 260)):
        m, lut, ok = camera_ref.rectify_map(camera_ref.PINHOLE, w, h)
        assert ok
        ys, xs = np.mgrid[0:h, 0:w]
        assert np.array_equal(lut[..., 0], xs) and np.array_equal(lut[..., 1], ys)
        assert np.abs(m[..., 0] - xs).max() < 1e-9 and np.abs(m[..., 1] - ys).max() < 1e-9


def test_davis_corners_leave_the_sensor():
    """The hand calculation of the design note: with k1 = -0.368 the corner pixels rectify to outside 240 x 180."""
    _, lut, ok = camera_ref.rectify_map(camera_ref.DAVIS, 240, 180)
    assert ok
    assert lut[0, 0, 0] < 0 and lut[0, 0, 1] < 0
    assert lut[179, 239, 0] > 239 and lut[179, 239, 1] > 179
    assert tuple(lut[111, 132]) == (132, 111)  # the principal point stays


def test_round_is_half_away_from_zero():
    a = np.array([0.5, -0.5, 1.5, -1.5, 2.5, 0.49999999999999994, -0.49999999999999994, -0.2, 7.0])
    assert camera_ref.round_half_away(a).tolist() == [1.0, -1.0, 2.0, -2.0, 3.0, 0.0, -0.0, -0.0, 7.0]


def test_rectify_events_leaves_strays_alone(ebo):
    ev = ebo.make_events([0, 120, -3, 240, 239], [0, 90, 10, 10, 179], [1, 2, 3, 4, 5])
    out = camera_ref.rectify_events(camera_ref.DAVIS, 240, 180, ev)
    _, lut, _ = camera_ref.rectify_map(camera_ref.DAVIS, 240, 180)
    assert (out["x"][0], out["y"][0]) == tuple(lut[0, 0])
    assert (out["x"][2], out["y"][2]) == (-3, 10) and (out["x"][3], out["y"][3]) == (240, 10)
    assert np.array_equal(out["t_us"], ev["t_us"]) and np.array_equal(out["sign"], ev["sign"])


# ---- ABI ---------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("ebo_camera_unproject", "ebo_camera_unproject_device", "ebo_set_rectification", "ebo_clear_rectification",
               "ebo_rectification_map")


def test_header_declares_the_camera_entries():
    text = open(os.path.join(ROOT, "include", "ebo.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name
    m = re.search(r"typedef struct ebo_camera\s*\{(.*?)\}\s*ebo_camera;", code, flags=re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)).strip() == "double fx, fy, cx, cy, k1, k2, k3, p1, p2;"


def test_library_exports_the_camera_entries(ebo):
    lib = ebo.lib()
    assert [n for n in NEW_ENTRIES if not hasattr(lib, n)] == []
    assert C.sizeof(ebo.Camera) == 72
    assert [f[0] for f in ebo.Camera._fields_] == ["fx", "fy", "cx", "cy", "k1", "k2", "k3", "p1", "p2"]
    c = ebo.camera(camera_ref.READER)
    assert (c.k3, c.p1, c.p2) == (0.321, 0.0011, 0.123)


# ---- synth.make_recording(distortion=...) ---------------------------------------------------------------------------
def _hashes(d):
    out = {}
    for root, _, files in os.walk(d):
        for f in files:
            p = os.path.join(root, f)
            out[os.path.relpath(p, d).replace(os.sep, "/")] = hashlib.sha256(open(p, "rb").read()).hexdigest()
    return out


def test_default_recording_is_byte_identical_to_before(synth, tmp_path):
    synth.make_recording(str(tmp_path / "rec"), seed=3, duration_s=0.1)
    assert _hashes(tmp_path / "rec") == RECORDING_HASHES


def test_distorted_recording_carries_its_calibration(synth, driver, tmp_path):
    coeff = (-0.368436311798, 0.150947243557, -0.000296130534385, -0.000759431726241)
    d = tmp_path / "rec"
    info = synth.make_recording(str(d), seed=3, duration_s=0.05, distortion=coeff)
    assert info["events"] > 0
    out = subprocess.run([driver, "calib", str(d)], capture_output=True, text=True, timeout=600)
    assert out.returncode == 0, out.stdout[-2000:] + out.stderr[-2000:]
    c = json.loads(out.stdout.strip().splitlines()[-1])
    assert c == dict(fx=200.0, fy=200.0, cx=120.0, cy=90.0, k1=coeff[0], k2=coeff[1], p1=coeff[2], p2=coeff[3], k3=0.0)
    # the lens compresses the scene towards the centre: the distorted recording differs from the plain one
    plain = tmp_path / "plain"
    synth.make_recording(str(plain), seed=3, duration_s=0.05)
    assert open(d / "events.txt", "rb").read() != open(plain / "events.txt", "rb").read()
