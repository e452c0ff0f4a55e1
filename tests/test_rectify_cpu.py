"""CPU: the rectified-frame rules of include/ebo.h (C1-C5) as tests/rectify_ref.py restates them -- the fit keeps
every sensor pixel in view for the calibrations in use, the remap is the identity for an identity camera, shifts
with the principal point, and reproduces an analytic scene within a bound derived below -- and the ABI."""
import os
import re

import numpy as np
import pytest

import camera_ref
import frontend_ref
import rectify_ref

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)

DAVIS_346 = tuple(v * 346.0 / 240.0 for v in camera_ref.DAVIS[:4]) + camera_ref.DAVIS[4:]
# (camera, w, h, sensor pixels that leave the sensor when the rectified camera keeps K)
FIT_CASES = {"davis": (camera_ref.DAVIS, 240, 180, 9869), "davis346": (DAVIS_346, 346, 260, 20532),
             "reader": (camera_ref.READER, 500, 500, 23685)}


def golden_frames():
    return [frontend_ref.read_png_gray8(os.path.join(frontend_ref.GOLDEN, "frame_%08d.png" % i)) for i in range(3)]


@pytest.mark.parametrize("name", sorted(FIT_CASES))
def test_fitted_camera_keeps_every_pixel_in_view(name):
    cam, w, h, outside_same_k = FIT_CASES[name]
    r = rectify_ref.fit(cam, w, h)
    assert r is not None and rectify_ref.check_rectified(r) is None
    _, lut, ok = rectify_ref.forward_map(cam, r, w, h)
    assert ok
    _, lut_k, ok_k = rectify_ref.forward_map(cam, rectify_ref.same_k(cam), w, h)
    assert ok_k
    print("%s %dx%d: fitted fx fy cx cy = %.4f %.4f %.4f %.4f; outside: fitted %d, same K %d" % (
        (name, w, h) + r[:4] + (rectify_ref.outside_count(lut, w, h), rectify_ref.outside_count(lut_k, w, h))))
    assert rectify_ref.outside_count(lut, w, h) == 0
    assert rectify_ref.outside_count(lut_k, w, h) == outside_same_k
    # C2 with r = K is the existing rule
    m0, lut0, ok0 = camera_ref.rectify_map(cam, w, h)
    assert ok0 and np.array_equal(lut0, lut_k)
    # the border carries the extremes of the whole sensor
    ys, xs = np.mgrid[0:h, 0:w]
    xo, yo = camera_ref.undistort(cam, np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float64))
    assert rectify_ref.border_extremes(cam, w, h) == (xo.min(), xo.max(), yo.min(), yo.max())


def test_fitted_values_of_the_design_note():
    got = rectify_ref.fit(camera_ref.DAVIS, 240, 180)[:4]
    assert np.allclose(got, (155.30, 155.10, 132.55, 111.43), atol=0.006), got
    got = rectify_ref.fit(DAVIS_346, 346, 260)[:4]
    assert np.allclose(got, (223.86, 223.57, 191.06, 160.62), atol=0.006), got
    got = rectify_ref.fit(camera_ref.READER, 500, 500)[:4]
    assert np.allclose(got, (463.99, 462.14, 297.04, 251.57), atol=0.006), got


def test_pinhole_fits_to_itself():
    r = rectify_ref.fit(camera_ref.PINHOLE, 240, 180)
    assert r[4:] == (0.0,) * 5
    assert np.allclose(r[:4], camera_ref.PINHOLE[:4], rtol=1e-12, atol=0.0), r
    _, lut, ok = rectify_ref.forward_map(camera_ref.PINHOLE, r, 240, 180)
    assert ok and rectify_ref.outside_count(lut, 240, 180) == 0


def test_fit_and_rectified_camera_refusals():
    assert rectify_ref.fit(camera_ref.DAVIS, 1, 180) is None and rectify_ref.fit(camera_ref.DAVIS, 240, 1) is None
    assert rectify_ref.fit((0.0,) + camera_ref.DAVIS[1:], 240, 180) is None
    assert rectify_ref.fit(camera_ref.DAVIS[:1] + (-3.0,) + camera_ref.DAVIS[2:], 240, 180) is None
    assert rectify_ref.fit((float("nan"),) + camera_ref.DAVIS[1:], 240, 180) is None
    assert rectify_ref.fit(camera_ref.DAVIS, 2, 2) is not None
    assert rectify_ref.check_rectified(camera_ref.DAVIS) == rectify_ref.ERR_ARG
    assert rectify_ref.check_rectified(camera_ref.PINHOLE[:8] + (float("nan"),)) == rectify_ref.ERR_ARG
    assert rectify_ref.check_rectified(camera_ref.PINHOLE[:6] + (0.7, 0.0, 0.0)) is None  # k3 is ignored
    assert rectify_ref.check_rectified((0.0,) + camera_ref.PINHOLE[1:]) == rectify_ref.ERR_RANGE
    assert rectify_ref.check_rectified(camera_ref.PINHOLE[:1] + (float("inf"),) + camera_ref.PINHOLE[2:]) == rectify_ref.ERR_RANGE


def test_identity_camera_returns_the_frame_byte_for_byte():
    images = golden_frames() + [np.random.default_rng(7).integers(0, 256, (180, 240), dtype=np.uint8)]
    for cam in (camera_ref.PINHOLE, rectify_ref.same_k(camera_ref.DAVIS)):
        for img in images:
            assert img.shape == (180, 240)
            out = rectify_ref.rectify_image(cam, rectify_ref.same_k(cam), img)
            assert out.dtype == np.uint8 and np.array_equal(out, img)


def test_principal_point_shift_shifts_the_frame():
    img = np.random.default_rng(8).integers(1, 256, (180, 240), dtype=np.uint8)
    cam = camera_ref.PINHOLE
    r = rectify_ref.rectified(cam[0], cam[1], cam[2] + 3.0, cam[3])
    out = rectify_ref.rectify_image(cam, r, img)
    assert np.array_equal(out[:, 3:], img[:, :-3])
    assert not out[:, :3].any()


def test_a_wild_map_reads_nothing_and_gives_zero():
    img = np.full((29, 37), 200, dtype=np.uint8)
    src = np.zeros((29, 37, 2))
    src[0, 0] = (np.nan, 3.0)
    src[0, 1] = (1e300, 3.0)
    src[0, 2] = (-1e300, 3.0)
    src[0, 3] = (np.inf, -np.inf)
    src[0, 4] = (-1.0, 3.0)   # not > -1
    src[0, 5] = (37.0, 3.0)   # not < w
    src[0, 6] = (-0.5, 3.0)   # half of the left neighbour, which is the border's 0
    src[0, 7] = (36.5, 28.5)  # a quarter of the last pixel
    out, inside = rectify_ref.remap(img, src)
    assert out[0, :8].tolist() == [0, 0, 0, 0, 0, 0, 100, 50]
    assert not inside[0, :8].any() and inside[1:].all()


# ---- physical check -----------------------------------------------------------------------------------------------
# the scene, a function of the normalised pinhole coordinates: 128 + sum A sin(kx * x + ky * y + phase)
SCENE = ((40.0, 10.0, 3.0, 0.3), (30.0, -8.0, 18.0, 1.1), (20.0, 20.0, 15.0, 2.0))
ROUND_TRIP_PX = 5.8e-5  # project(undistort(.)) of the ten-iteration fixed point for DAVIS, in pixels


def scene(x, y):
    s = np.full(np.shape(x), 128.0)
    for a, kx, ky, ph in SCENE:
        s = s + a * np.sin(kx * x + ky * y + ph)
    return s


def converged_undistort(cam, uv, iterations=200):
    """The model's fixed point iterated to convergence (camera_ref.undistort stops after ten steps)."""
    fx, fy, cx, cy, k1, k2, _k3, p1, p2 = (np.float64(v) for v in cam)
    xd, yd = (uv[:, 0] - cx) / fx, (uv[:, 1] - cy) / fy
    xo, yo = xd.copy(), yd.copy()
    for _ in range(iterations):
        r2 = xo * xo + yo * yo
        rad = camera_ref._radial(k1, k2, r2)
        dx = camera_ref._tangential(p1, p2, xo, yo, r2)
        dy = camera_ref._tangential(p2, p1, yo, xo, r2)
        xo, yo = (xd - dx) / rad, (yd - dy) / rad
    return xo, yo


def test_remapped_analytic_scene_is_the_pinhole_render():
    """raw(u, v) = uint8(round(R(u, v))), R = scene o g, g = the converged inverse of the lens; rect = remap(raw) at
    (us, vs) = project(xn, yn); ideal = scene(xn, yn) = R(us, vs) because g inverts project.  Where all four taps are
    in the frame:
      |rect - ideal| <= 0.5 (rounding rect to uint8) + 0.5 (rounding raw: a bilinear sample is a convex combination)
                      + (Muu + Mvv) / 8 (bilinear interpolation over a unit cell; Muu, Mvv bound |R_uu|, |R_vv|)
                      + G_px * ROUND_TRIP_PX (the scene's gradient per raw pixel times the model's round-trip error).
    Chain rule: R_uu = g_u^T H g_u + grad . g_uu, so |R_uu| <= Hmax |g_u|^2 + Gmax |g_uu| with the analytic
    Gmax = sum A |k| >= |grad scene| and Hmax = sum A |k|^2 >= ||Hessian of the scene||; |g_u|, |g_uu| (and v) are
    the largest central first and second differences of g over the sensor's pixel grid, widened by 10 % for what
    lies between grid points (g is the smooth lens inverse: it varies by far less than that from pixel to pixel)."""
    cam, w, h = camera_ref.DAVIS, 240, 180
    ys, xs = np.mgrid[0:h, 0:w]
    px = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float64)
    gx, gy = converged_undistort(cam, px)
    back = camera_ref.project(cam, np.stack([gx, gy, np.ones_like(gx)], axis=1))
    assert np.abs(back - px).max() < 1e-9  # converged: g inverts project on the whole sensor
    ten = camera_ref.undistort(cam, px)
    back10 = camera_ref.project(cam, np.stack([ten[0], ten[1], np.ones_like(gx)], axis=1))
    assert np.abs(back10 - px).max() <= ROUND_TRIP_PX
    raw = camera_ref.round_half_away(scene(gx, gy)).reshape(h, w)
    assert raw.min() >= 0 and raw.max() <= 255
    raw = raw.astype(np.uint8)

    r = rectify_ref.fit(cam, w, h)
    src = rectify_ref.source_map(cam, r, w, h)
    rect, inside = rectify_ref.remap(raw, src)
    xn = (xs - r[2]) / r[0]
    yn = (ys - r[3]) / r[1]
    ideal = scene(xn, yn)

    g = np.stack([gx.reshape(h, w), gy.reshape(h, w)], axis=-1)
    norm = lambda d: np.sqrt((d * d).sum(axis=-1)).max()
    gu = 1.1 * norm((g[:, 2:] - g[:, :-2]) / 2.0)
    gv = 1.1 * norm((g[2:] - g[:-2]) / 2.0)
    guu = 1.1 * norm(g[:, 2:] - 2.0 * g[:, 1:-1] + g[:, :-2])
    gvv = 1.1 * norm(g[2:] - 2.0 * g[1:-1] + g[:-2])
    gmax = sum(a * np.hypot(kx, ky) for a, kx, ky, _ in SCENE)
    hmax = sum(a * (kx * kx + ky * ky) for a, kx, ky, _ in SCENE)
    muu = hmax * gu * gu + gmax * guu
    mvv = hmax * gv * gv + gmax * gvv
    bound = 1.0 + (muu + mvv) / 8.0 + gmax * max(gu, gv) * ROUND_TRIP_PX
    err = np.abs(rect.astype(np.float64) - ideal)[inside]
    print("physical: %d of %d pixels with all taps inside; |rect - ideal| mean %.4f max %.4f, bound %.4f "
          "(bilinear %.4f, round trip %.2e)" % (inside.sum(), w * h, err.mean(), err.max(), bound, (muu + mvv) / 8.0,
                                                gmax * max(gu, gv) * ROUND_TRIP_PX))
    assert inside.sum() > 0.8 * w * h  # the rectified frame is wider than the lens image at its waist
    assert 1.0 < bound < 2.0  # the bound says something: the scene is neither flat nor finer than the pixel grid
    assert err.max() <= bound


# ---- ABI ---------------------------------------------------------------------------------------------------------
NEW_ENTRIES = ("ebo_fit_rectified_camera", "ebo_set_rectification_camera", "ebo_rectified_camera",
               "ebo_rectification_source_map", "ebo_rectify_image", "ebo_rectify_image_device", "ebo_camera_project",
               "ebo_camera_project_device")


def test_header_declares_the_rectification_entries():
    text = open(os.path.join(ROOT, "include", "ebo.h")).read()
    code = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    for name in NEW_ENTRIES:
        assert re.search(r"\bint\s+%s\s*\(" % name, code), name


def test_library_exports_the_rectification_entries(ebo):
    lib = ebo.lib()
    assert [n for n in NEW_ENTRIES if not hasattr(lib, n)] == []
    for method in ("camera_project", "camera_project_device", "fit_rectified_camera", "set_rectification_camera",
                   "rectified_camera", "rectification_source_map", "rectify_image", "rectify_image_device"):
        assert callable(getattr(ebo.Context, method)), method
