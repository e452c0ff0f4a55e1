"""CPU tests of the image front end (include/ebo.h, "image front end"): the ABI and the bindings exist, the
PNG fixtures read back, and the CPU restatement (tests/frontend_ref.py) the GPU tests compare against behaves
as the reference's detector and flow estimator are expected to."""
import ctypes
import os
import zlib

import numpy as np
import pytest

import frontend_ref as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["ebo_image_gradients", "ebo_good_features", "ebo_lk_add_image", "ebo_lk_track"]


def test_library_exports_front_end_and_bindings(ebo):
    lib = ctypes.CDLL(os.path.join(ROOT, "event-based-odomety_amd", "libebo_hip.so"))
    for s in SYMBOLS:
        assert hasattr(lib, s), s
    for m in ("image_gradients", "good_features", "lk_add_image", "lk_track"):
        assert callable(getattr(ebo.Context, m, None)), m


def test_png_fixtures_read_back():
    crcs = [2802912075, 3624776616, 1811180222]
    for path, crc in zip(F.FRAMES, crcs):
        img = F.read_png_gray8(path)
        assert img.shape == (180, 240) and img.dtype == np.uint8
        assert zlib.crc32(img.tobytes()) == crc


def test_harris_finds_the_four_corners_of_a_rectangle():
    img = np.zeros((50, 60), dtype=np.uint8)
    img[15:35, 20:40] = 200
    c = F.good_features(img, None, max_corners=50, quality_level=0.01, min_distance=5, block_size=3)
    assert len(c) == 4
    got = sorted((int(x), int(y)) for x, y in c)
    want = sorted([(20, 15), (39, 15), (20, 34), (39, 34)])
    for (gx, gy), (wx, wy) in zip(got, want):
        assert abs(gx - wx) <= 1 and abs(gy - wy) <= 1, (got, want)


def test_greedy_minimum_distance_is_strict():
    w = 100
    first, other = 10 * w + 10, 14 * w + 13  # (10, 10) and (13, 14): 5 apart
    d = 5.0
    assert len(F.greedy(np.array([first, other]), w, 10, d)) == 2  # exactly min_distance: accepted
    assert len(F.greedy(np.array([first, other]), w, 10, np.nextafter(d, 10.0))) == 1  # min_distance - eps: rejected
    assert len(F.greedy(np.array([first, other]), w, 1, 0.0)) == 1  # max_corners


def test_ties_go_to_the_larger_raster_index():
    # two identical squares: equal responses at mirrored / translated corners
    img = np.zeros((40, 80), dtype=np.uint8)
    img[10:20, 10:20] = 180
    img[10:20, 50:60] = 180
    R = F.harris_response(img)
    best = F.good_features(img, None, max_corners=1, quality_level=0.01, min_distance=1)
    x, y = int(best[0, 0]), int(best[0, 1])
    cand = np.argwhere(R[1:-1, 1:-1] == R[1:-1, 1:-1].max()) + 1
    assert len(cand) > 1, "the image must tie"
    assert (y, x) == tuple(max(cand.tolist(), key=lambda p: p[0] * 80 + p[1]))


def test_reference_detector_properties_on_fixture_frame():
    # the reference's featureDetectorTest (feature_detector_test.cpp:10-26) with patchExtent = 5
    img = F.read_png_gray8(F.FRAMES[0])
    h, w = img.shape
    pe = 5
    c = F.good_features(img, F.reference_mask(w, h, pe), F.reference_max_corners(w, h, pe), 0.01, 10, 3, 0.04)
    assert len(c) > 10
    assert np.all((c[:, 0] > pe + 1) & (c[:, 0] < w - pe - 1) & (c[:, 1] > pe + 1) & (c[:, 1] < h - pe - 1))


@pytest.mark.parametrize("shift,tol", [((3, -2), 0.02), ((0.4, 1.7), 0.02), ((10, 0), 0.02)])
def test_restated_lk_recovers_shifts(shift, tol):
    big = F.textured(180, 240, seed=1, sigma=3.0)
    a, b = F.shifted(big, 180, 240, *shift)
    lk = F.LK()
    lk.add_image(a)
    lk.add_image(b)
    pts = np.array([[120, 90], [60, 50], [180, 130], [100.5, 70.25]], dtype=np.float32)
    nxt, st, _ = lk.track(pts)
    assert st.all()
    np.testing.assert_allclose(nxt - pts, np.tile(np.float32(shift), (len(pts), 1)), atol=tol)


def test_restated_lk_status_zero_on_flat_image_and_outside():
    flat = np.full((180, 240), 90, dtype=np.uint8)
    lk = F.LK()
    lk.add_image(flat)
    lk.add_image(flat)
    _, st, _ = lk.track(np.array([[120, 90]], dtype=np.float32))
    assert st[0] == 0  # minimum-eigenvalue test
    big = F.textured(180, 240, seed=2, sigma=3.0)
    a, b = F.shifted(big, 180, 240, 1, 1)
    lk = F.LK()
    lk.add_image(a)
    lk.add_image(b)
    _, st, _ = lk.track(np.array([[-40, 90], [120, 300], [120, 90]], dtype=np.float32))
    assert st.tolist() == [0, 0, 1]
