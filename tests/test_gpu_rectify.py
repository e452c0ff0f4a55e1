"""GPU: rectified frames, the fitted rectified camera and project on the device against tests/rectify_ref.py and
tests/camera_ref.py.  Every double and every byte is bit-equal to the restatement."""
import os

import numpy as np
import pytest

import camera_ref
import frontend_ref
import rectify_ref

pytestmark = pytest.mark.gpu

CAMERAS = {"davis": camera_ref.DAVIS, "reader": camera_ref.READER, "pinhole": camera_ref.PINHOLE}
DAVIS_346 = tuple(v * 346.0 / 240.0 for v in camera_ref.DAVIS[:4]) + camera_ref.DAVIS[4:]
DAVIS_1280 = (camera_ref.DAVIS[0] * 1280 / 240.0, camera_ref.DAVIS[1] * 720 / 180.0, camera_ref.DAVIS[2] * 1280 / 240.0,
              camera_ref.DAVIS[3] * 720 / 180.0) + camera_ref.DAVIS[4:]
# project overflows: k1 * r2 is ~1e307 away from the axis, so fx * xDist is infinite there and finite but ~1e300 near it
OVERFLOW = (200.0, 200.0, 120.0, 90.0, 1e308, 0.0, 0.0, 0.0, 0.0)
# (camera, w, h, patch) of the fit and map cases
SIZES = {"240x180": (camera_ref.DAVIS, 240, 180, (30, 20)), "346x260": (DAVIS_346, 346, 260, (40, 20)),
         "37x29": (camera_ref.DAVIS, 37, 29, (37, 29)), "2x2": (camera_ref.DAVIS, 2, 2, (2, 2))}


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def nine(cam):
    return np.array([cam.fx, cam.fy, cam.cx, cam.cy, cam.k1, cam.k2, cam.k3, cam.p1, cam.p2])


def ctx(ebo, w, h, patch, **kw):
    return ebo.Context(image_w=w, image_h=h, patch_w=patch[0], patch_h=patch[1], loss=ebo.LOSS_VARIANCE, **kw)


def code_of(ebo, call):
    try:
        call()
    except ebo.EboError as e:
        return e.code
    return 0


def seeded_points(seed, n):
    rng = np.random.default_rng(seed)
    p = np.stack([rng.uniform(-2, 2, n), rng.uniform(-2, 2, n), rng.uniform(0.5, 20, n)], axis=1)
    p[:40, 2] = 0.0             # z = 0: infinities and NaN, as the rule gives them
    p[40:44] = 0.0              # 0 / 0
    p[100:400, 2] *= -1.0       # behind the camera
    p[400] = (0.0, 0.0, 1.0)    # the principal point
    return p


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_project_is_bit_equal_to_camera_ref(ebo, name):
    import torch
    cam = CAMERAS[name]
    p = seeded_points(17, 10_000)
    want = camera_ref.project(cam, p)
    assert not np.isfinite(want[:44]).all(axis=1).any() and np.isfinite(want[44:]).all()
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = c.camera_project(cam, p)
        d_p = torch.from_numpy(p).to("cuda")
        d_out = torch.zeros((len(p), 2), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        c.camera_project_device(cam, len(p), d_p.data_ptr(), d_out.data_ptr())
        c.synchronize()
        got_dev = d_out.cpu().numpy()
        few = c.camera_project(cam, p[:3])
        assert c.camera_project(cam, np.zeros((0, 3))).shape == (0, 2)
    # a NaN's payload and sign are not part of the rule: compare NaN as NaN, everything else by its bits
    for g in (got, got_dev):
        nan = np.isnan(want)
        assert np.array_equal(np.isnan(g), nan)
        assert np.array_equal(bits(g)[~nan], bits(want)[~nan])
    assert np.array_equal(np.isnan(few), np.isnan(want[:3]))


@pytest.mark.parametrize("size", sorted(SIZES))
def test_fit_is_bit_equal_to_the_restatement(ebo, size):
    cam, w, h, patch = SIZES[size]
    want = rectify_ref.fit(cam, w, h)
    assert want is not None
    with ctx(ebo, w, h, patch) as c:
        got = nine(c.fit_rectified_camera(cam))
        assert code_of(ebo, lambda: c.fit_rectified_camera((0.0,) + cam[1:])) == ebo.ERR_RANGE
        assert code_of(ebo, lambda: c.fit_rectified_camera(cam[:1] + (-2.0,) + cam[2:])) == ebo.ERR_RANGE
        assert code_of(ebo, lambda: c.fit_rectified_camera((float("nan"),) + cam[1:])) == ebo.ERR_RANGE
    print("fit %s:" % size, got[:4], "want", want[:4])
    assert np.array_equal(bits(got), bits(np.array(want)))


def test_fit_refuses_a_one_pixel_side(ebo):
    for w, h in ((1, 29), (37, 1)):
        assert rectify_ref.fit(camera_ref.DAVIS, w, h) is None
        with ctx(ebo, w, h, (w, h)) as c:
            assert code_of(ebo, lambda: c.fit_rectified_camera(camera_ref.DAVIS)) == ebo.ERR_RANGE


@pytest.mark.parametrize("size", sorted(SIZES))
def test_forward_map_with_a_rectified_camera(ebo, size):
    cam, w, h, patch = SIZES[size]
    r = rectify_ref.fit(cam, w, h)
    m, lut, ok = rectify_ref.forward_map(cam, r, w, h)
    assert ok
    with ctx(ebo, w, h, patch) as c:
        # r = K: exactly ebo_set_rectification
        c.set_rectification(cam)
        m0, lut0 = c.rectification_map()
        k0 = nine(c.rectified_camera())
        c.set_rectification_camera(cam, rectify_ref.same_k(cam))
        m1, lut1 = c.rectification_map()
        assert np.array_equal(bits(m0), bits(m1)) and np.array_equal(lut0, lut1)
        assert np.array_equal(bits(k0), bits(np.array(rectify_ref.same_k(cam))))
        assert np.array_equal(bits(nine(c.rectified_camera())), bits(k0))
        mk, lutk, okk = camera_ref.rectify_map(cam, w, h)
        assert okk and np.array_equal(bits(m0), bits(mk)) and np.array_equal(lut0, lutk)
        # the fitted camera
        fitted = c.fit_rectified_camera(cam)
        c.set_rectification_camera(cam, fitted)
        gm, glut = c.rectification_map()
        assert np.array_equal(bits(nine(c.rectified_camera())), bits(np.array(r)))
    print("forward map %s: %d map words, %d table entries differ; %d pixels outside" % (
        size, int((bits(gm) != bits(m)).sum()), int((glut != lut).sum()), rectify_ref.outside_count(glut, w, h)))
    assert np.array_equal(bits(gm), bits(m))
    assert np.array_equal(glut, lut)
    assert rectify_ref.outside_count(glut, w, h) == 0


def test_rectified_camera_refusals(ebo):
    cam = camera_ref.DAVIS
    k = rectify_ref.same_k(cam)
    img = np.zeros((180, 240), dtype=np.uint8)
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        nothing_set = (c.rectified_camera, c.rectification_source_map, lambda: c.rectify_image(img), c.rectification_map)
        assert [code_of(ebo, f) for f in nothing_set] == [ebo.ERR_STATE] * 4
        for bad, code in ((cam, ebo.ERR_ARG), (k[:4] + (1e-9, 0.0, 0.0, 0.0, 0.0), ebo.ERR_ARG),
                          (k[:8] + (float("nan"),), ebo.ERR_ARG), ((0.0,) + k[1:], ebo.ERR_RANGE),
                          (k[:1] + (float("inf"),) + k[2:], ebo.ERR_RANGE)):
            c.set_rectification_camera(cam, k)
            assert code_of(ebo, c.rectified_camera) == 0
            assert code_of(ebo, lambda: c.set_rectification_camera(cam, bad)) == code, bad
            assert rectify_ref.check_rectified(bad) == (rectify_ref.ERR_ARG if code == ebo.ERR_ARG else rectify_ref.ERR_RANGE)
            # a refused call leaves nothing set
            assert [code_of(ebo, f) for f in nothing_set] == [ebo.ERR_STATE] * 4
        c.set_rectification_camera(cam, k[:6] + (0.7, 0.0, 0.0))  # k3 is ignored
        assert nine(c.rectified_camera())[6] == 0.0
        # still refused while a rectification is set
        ev = ebo.make_events([1, 2], [3, 4], [10, 20])
        assert code_of(ebo, lambda: c.set_patches(ev, [0, 2], [[0, 0, 30, 22]])) == ebo.ERR_UNSUPPORTED
        c.clear_rectification()
        assert [code_of(ebo, f) for f in nothing_set] == [ebo.ERR_STATE] * 4


def test_new_entries_are_refused_while_recording(ebo, synth):
    import torch
    cam = camera_ref.DAVIS
    img = np.zeros((180, 240), dtype=np.uint8)
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        c.set_rectification(cam)
        ev, gt = synth.make_window(0, n_events=3000)
        c.set_window(ev)
        d_flows = torch.zeros((c.P, 2), dtype=torch.float64, device="cuda")
        d_out = torch.zeros(3 * c.P, dtype=torch.float64, device="cuda")
        d_a = torch.zeros(240 * 180, dtype=torch.uint8, device="cuda")
        d_b = torch.zeros(240 * 180, dtype=torch.uint8, device="cuda")
        d_p = torch.ones(6, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())
        c.synchronize()
        codes = []

        def body():
            for call in (lambda: c.fit_rectified_camera(cam), lambda: c.set_rectification_camera(cam, rectify_ref.same_k(cam)),
                         c.rectified_camera, c.rectification_source_map, lambda: c.rectify_image(img),
                         lambda: c.rectify_image_device(d_a.data_ptr(), d_b.data_ptr()),
                         lambda: c.camera_project(cam, [[1.0, 2.0, 3.0]]),
                         lambda: c.camera_project_device(cam, 2, d_p.data_ptr(), d_p.data_ptr())):
                codes.append(code_of(ebo, call))
            c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())

        g = c.record(body)
        assert codes == [ebo.ERR_STATE] * 8
        g.launch()
        c.synchronize()
        g.close()
        assert code_of(ebo, c.rectified_camera) == 0  # the refused calls changed nothing


def golden_and_noise():
    frames = [frontend_ref.read_png_gray8(os.path.join(frontend_ref.GOLDEN, "frame_%08d.png" % i)) for i in range(3)]
    return frames + [np.random.default_rng(21).integers(0, 256, (180, 240), dtype=np.uint8)]


def noise(seed, w, h):
    return [np.random.default_rng(seed).integers(0, 256, (h, w), dtype=np.uint8)]


def _remap_case(name):
    """-> (camera, rectified camera or None for the fit, w, h, patch, images)"""
    if name == "davis-240x180":
        return camera_ref.DAVIS, None, 240, 180, (30, 20), golden_and_noise()
    if name == "davis-37x29":
        return camera_ref.DAVIS, None, 37, 29, (37, 29), noise(22, 37, 29)
    if name == "davis-2x2":
        return camera_ref.DAVIS, None, 2, 2, (2, 2), noise(23, 2, 2)
    if name == "davis-1280x720":
        return DAVIS_1280, None, 1280, 720, (40, 20), noise(24, 1280, 720)
    if name == "reader-same-K":
        return camera_ref.READER, rectify_ref.same_k(camera_ref.READER), 500, 500, (50, 50), noise(25, 500, 500)
    if name == "overflow":
        return OVERFLOW, rectify_ref.same_k(OVERFLOW), 240, 180, (30, 20), noise(26, 240, 180)
    if name == "identity":
        return camera_ref.PINHOLE, rectify_ref.same_k(camera_ref.PINHOLE), 240, 180, (30, 20), golden_and_noise()
    raise KeyError(name)


@pytest.mark.parametrize("name", ["davis-240x180", "davis-37x29", "davis-2x2", "davis-1280x720", "reader-same-K",
                                  "overflow", "identity"])
def test_source_map_and_remap_are_bit_equal_to_the_restatement(ebo, name):
    import torch
    cam, r, w, h, patch, images = _remap_case(name)
    if r is None:
        r = rectify_ref.fit(cam, w, h)
    assert rectify_ref.forward_map(cam, r, w, h)[2]
    src = rectify_ref.source_map(cam, r, w, h)
    with np.errstate(all="ignore"):
        no_source = ~((src[..., 0] > -1) & (src[..., 0] < w) & (src[..., 1] > -1) & (src[..., 1] < h))
    with ctx(ebo, w, h, patch) as c:
        c.set_rectification_camera(cam, r)
        got_src = c.rectification_source_map()
        nan = np.isnan(src)
        assert np.array_equal(np.isnan(got_src), nan)
        assert np.array_equal(bits(got_src)[~nan], bits(src)[~nan])
        for img in images:
            want, _ = rectify_ref.remap(img, src)
            got = c.rectify_image(img)
            d_in = torch.from_numpy(img).to("cuda")
            d_out = torch.full((h, w), 77, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()
            c.rectify_image_device(d_in.data_ptr(), d_out.data_ptr())
            c.synchronize()
            print("remap %s: %d of %d bytes differ, %d pixels have no source" % (name, int((got != want).sum()), w * h,
                                                                                int(no_source.sum())))
            assert got.dtype == np.uint8 and np.array_equal(got, want)
            assert np.array_equal(d_out.cpu().numpy(), want)
            assert np.array_equal(d_in.cpu().numpy(), img)  # the source frame is untouched
            assert not got[no_source].any()
            assert code_of(ebo, lambda: c.rectify_image_device(d_in.data_ptr(), d_in.data_ptr())) == ebo.ERR_ARG
    if name == "reader-same-K":
        assert 0 < no_source.sum() < w * h
    if name == "overflow":
        # everything but the principal point's row and column overflows or lands far outside the frame
        assert no_source.sum() >= (w - 1) * (h - 1) and not np.isfinite(src).all() and np.isfinite(src).any()
    if name == "identity":
        assert all(np.array_equal(rectify_ref.remap(img, src)[0], img) for img in images)


def _every_pixel_once(ebo, w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return ebo.make_events(xs.ravel(), ys.ravel(), 1_000_000 + np.arange(w * h))


def test_fitted_camera_leaves_no_stray(ebo):
    """One event on every pixel of a 240 x 180 sensor under DAVIS: the patch grid (30 x 20) tiles the sensor, so the
    events in no patch are exactly the stray unit's."""
    w, h = 240, 180
    ev = _every_pixel_once(ebo, w, h)
    with ctx(ebo, w, h, (30, 20), max_events=len(ev)) as c:
        stray = {}
        for which, r in (("fitted", rectify_ref.fit(camera_ref.DAVIS, w, h)), ("same K", rectify_ref.same_k(camera_ref.DAVIS))):
            c.set_rectification_camera(camera_ref.DAVIS, r)
            c.set_window(ev)
            stray[which] = len(ev) - sum(c.patch_info(p)[0] for p in range(c.P))
    print("stray events of %d:" % len(ev), stray)
    assert stray["fitted"] == 0
    assert stray["same K"] == 9869  # the pixels camera_ref sends outside (tests/test_rectify_cpu.py)


def test_load_under_the_fitted_camera_equals_load_of_rectified_events(ebo, synth):
    cam, (w, h) = camera_ref.DAVIS, synth.CONFIGS[2]["image"]
    pw, ph = synth.CONFIGS[2]["patch"]
    n_windows = 3
    ev, offsets, gt = synth.make_stream(2, n_windows, n_events=9000)
    ev = ev.copy()
    ev["x"][3] = -2  # strays stay strays
    ev["y"][11] = 15000
    for i, (x, y) in enumerate(((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1))):
        ev["x"][30 + i], ev["y"][30 + i] = x, y
    r = rectify_ref.fit(cam, w, h)
    rect = rectify_ref.rectify_events(cam, r, w, h, ev)
    rect_k = camera_ref.rectify_events(cam, w, h, ev)
    assert ((rect["x"] != rect_k["x"]) | (rect["y"] != rect_k["y"])).mean() > 0.3  # not the table of the same K

    def snapshot(c):
        info = [[c.patch_info(p, k) for p in range(c.P)] for k in range(n_windows)]
        rr, J = c.eval(gt * 0.5)
        return info, rr, J, c.count_image(ebo.COUNT_WARPED, gt * 0.7)

    kw = dict(max_windows=n_windows, max_events=len(ev))
    with ctx(ebo, w, h, (pw, ph), **kw) as plain:
        plain.set_windows(rect, offsets)
        want = snapshot(plain)
    with ctx(ebo, w, h, (pw, ph), **kw) as c:
        c.set_rectification_camera(cam, c.fit_rectified_camera(cam))
        c.set_windows(ev, offsets)
        got = snapshot(c)
    assert got[0] == want[0]
    for k in (1, 2, 3):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
