"""The image front end on the MI355X (include/ebo.h, "image front end") against the CPU restatement of its
rules (tests/frontend_ref.py): gradients, corners and LK (positions, status, err) bit for bit,
the gradients installed for the per-feature objective, and the C++ facade's FeatureDetector::useDeviceFrontEnd
driven through newImage (tests/cpp/front_end_device_test.cpp)."""
import os
import subprocess

import numpy as np
import pytest

import frontend_ref as F

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def ctx(ebo, w, h):
    return ebo.Context(image_w=w, image_h=h)


def random_images(h, w, seed):
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, size=(h, w), dtype=np.uint8), F.textured(h, w, seed=seed, sigma=1.5)[32:32 + h, 32:32 + w]]


def test_gradients_bit_equal(ebo):
    cases = [(f, "frame%d" % i) for i, f in enumerate(F.frames())]
    for (h, w) in ((180, 240), (260, 346), (23, 37)):
        cases += [(im, "random %dx%d" % (w, h)) for im in random_images(h, w, w)]
        cases += [(np.zeros((h, w), np.uint8), "zeros"), (np.full((h, w), 255, np.uint8), "255")]
    for img, name in cases:
        h, w = img.shape
        with ctx(ebo, w, h) as c:
            gx, gy = c.image_gradients(img)
        rx, ry = F.image_gradients(img)
        assert np.array_equal(gx.view(np.uint64), rx.view(np.uint64)), name
        assert np.array_equal(gy.view(np.uint64), ry.view(np.uint64)), name


def _check_corners(c, img, **kw):
    got = c.good_features(img, **kw)
    want = F.good_features(img, **kw)
    assert got.shape == want.shape, (got.shape, want.shape, kw.get("max_corners"))
    assert np.array_equal(got, want)
    assert np.array_equal(c.good_features(img, **kw), got)  # deterministic
    return got


def test_corners_fixture_frames(ebo):
    with ctx(ebo, 240, 180) as c:
        for img in F.frames():
            for pe in (12, 5):
                kw = dict(mask=F.reference_mask(240, 180, pe), max_corners=F.reference_max_corners(240, 180, pe),
                          quality_level=0.01, min_distance=10.0, block_size=3, harris_k=0.04)
                assert len(_check_corners(c, img, **kw)) > 10


def test_corners_random_ties_and_limits(ebo):
    yy, xx = np.indices((180, 240))
    checker = (((xx // 6 + yy // 6) % 2) * 200 + 20).astype(np.uint8)
    with ctx(ebo, 240, 180) as c:
        imgs = random_images(180, 240, 7) + [checker]
        for img in imgs:
            _check_corners(c, img, max_corners=500, quality_level=0.01, min_distance=10.0)
            _check_corners(c, img, mask=F.reference_mask(240, 180, 12), max_corners=69, min_distance=10.0)
            _check_corners(c, img, max_corners=1, min_distance=10.0)
            _check_corners(c, img, max_corners=2000, min_distance=0.0)
            _check_corners(c, img, max_corners=300, block_size=5, min_distance=4.0)
    # a candidate list longer than the LDS sort: the global bitonic path
    with ctx(ebo, 346, 260) as c:
        img = random_images(260, 346, 3)[0]
        n = np.count_nonzero(F.good_features(img, max_corners=8192, quality_level=0.0, min_distance=0.0))
        assert n > 4096
        _check_corners(c, img, max_corners=8192, quality_level=0.0, min_distance=0.0)
        _check_corners(c, img, max_corners=1000, quality_level=0.0, min_distance=3.0)


def _lk_pair(c, a, b, pts, **kw):
    c.lk_add_image(a)
    c.lk_add_image(b)
    got = c.lk_track(pts, **kw)
    lk = F.LK()
    lk.add_image(a)
    lk.add_image(b)
    want = lk.track(pts, **kw)
    return got, want


def test_lk_fixture_frames_against_restatement(ebo):
    fr = F.frames()
    with ctx(ebo, 240, 180) as c:
        for k in (0, 1):
            pts = F.good_features(fr[k], F.reference_mask(240, 180, 5), F.reference_max_corners(240, 180, 5))
            (n, s, e), (rn, rs, re) = _lk_pair(c, fr[k], fr[k + 1], pts)
            assert np.array_equal(s, rs)
            ok = s == 1
            assert ok.sum() > 5
            assert np.array_equal(n.view(np.uint32), rn.view(np.uint32))
            assert np.array_equal(e.view(np.uint32), re.view(np.uint32))


def test_lk_synthetic_shifts_and_status(ebo):
    big = F.textured(180, 240, seed=1, sigma=3.0)
    pts = np.array([[120, 90], [60, 50], [180, 130], [100.5, 70.25]], dtype=np.float32)
    with ctx(ebo, 240, 180) as c:
        for shift in ((3, -2), (0.4, 1.7), (10, 0)):
            a, b = F.shifted(big, 180, 240, *shift)
            (n, s, _), (rn, rs, _) = _lk_pair(c, a, b, pts)
            assert s.all() and np.array_equal(s, rs)
            np.testing.assert_allclose(n - pts, np.tile(np.float32(shift), (len(pts), 1)), atol=0.05)
            assert np.array_equal(n.view(np.uint32), rn.view(np.uint32))
        a, b = F.shifted(big, 180, 240, 1, 1)
        edge = np.array([[-40, 90], [120, 300], [239.5, 90], [0, 0], [-5, -5], [120, 90]], dtype=np.float32)
        (n, s, _), (rn, rs, _) = _lk_pair(c, a, b, edge)
        assert np.array_equal(s, rs)
        assert s[0] == 0 and s[1] == 0 and s[-1] == 1
        flat = np.full((180, 240), 90, np.uint8)
        (n, s, _), (rn, rs, _) = _lk_pair(c, flat, flat, pts)
        assert not s.any() and not rs.any()


def test_lk_track_needs_two_images(ebo):
    with ctx(ebo, 240, 180) as c:
        with pytest.raises(ebo.EboError) as ei:
            c.lk_track(np.array([[10, 10]], np.float32))
        assert ei.value.code == ebo.ERR_STATE
        c.lk_add_image(F.frames()[0])
        with pytest.raises(ebo.EboError) as ei:
            c.lk_track(np.array([[10, 10]], np.float32))
        assert ei.value.code == ebo.ERR_STATE


def test_gradients_installed_for_the_objective(ebo):
    img = F.frames()[0]
    rects = np.array([[50, 40, 11, 11], [120, 90, 11, 11], [200, 150, 11, 11]], dtype=np.float64)
    rng = np.random.default_rng(5)
    nablas = [rng.standard_normal((11, 11)) for _ in rects]
    poses = np.array([[1, 0, 0.3, -0.2], [np.cos(0.1), np.sin(0.1), -1.0, 0.5], [1, 0, 0, 0]], dtype=np.float64)
    fds = np.array([0.3, -1.2, 2.0])
    out = []
    with ctx(ebo, 240, 180) as c:
        gx, gy = c.image_gradients(img)
        for grads in ((gx, gy), F.image_gradients(img)):
            c.optimizer_set_grad(*grads)
            res, jp, jf = c.optimizer_eval(rects, nablas, poses, fds)
            ne = c.estimate_num_events(rects, poses, fds)
            out.append((np.concatenate(res), np.concatenate(jp), np.concatenate(jf), ne))
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_facade_device_front_end(tmp_path):
    src = os.path.join(ROOT, "tests", "cpp", "front_end_device_test.cpp")
    exe = str(tmp_path / "front_end_device_test")
    inc = os.path.join(ROOT, "event-based-odomety_amd", "include")
    libdir = os.path.join(ROOT, "event-based-odomety_amd")
    # the flags of tests/cpp/Makefile's front_end_lines_test
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-I" + inc, "-o", exe, src, "-L" + libdir,
                           "-lebo_hip", "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib"], timeout=300)
    # the frames as PGM, and the restatement's results for the sequence: what the second detector's hooks return
    fr = F.frames()
    pe, w, h = 5, 240, 180
    mask, maxc = F.reference_mask(w, h, pe), F.reference_max_corners(w, h, pe)
    corners = [F.good_features(img, mask, maxc) for img in fr]
    pgms = []
    lk = F.LK()
    lines = []
    for k, img in enumerate(fr):
        pgm = tmp_path / ("frame%d.pgm" % k)
        pgm.write_bytes(b"P5\n%d %d\n255\n" % (w, h) + img.tobytes())
        pgms.append(str(pgm))
        grad = tmp_path / ("grad%d.bin" % k)
        gx, gy = F.image_gradients(img)
        grad.write_bytes(gx.tobytes() + gy.tobytes())
        lines.append("corners %d %s" % (len(corners[k]), " ".join("%.9g %.9g" % (x, y) for x, y in corners[k])))
        lines.append("grad %s" % grad)
        lk.add_image(img)
        if k > 0:
            pts = np.unique(np.concatenate([corners[k - 1], corners[k]]), axis=0)
            n, s, _ = lk.track(pts)
            lines.append("flow %d %s" % (len(pts), " ".join("%.9g %.9g %.9g %.9g %d" % (p[0], p[1], q[0], q[1], t)
                                                             for p, q, t in zip(pts, n, s))))
    ref = tmp_path / "ref.txt"
    ref.write_text("\n".join(lines) + "\n")
    r = subprocess.run([exe] + pgms + [os.path.join(ROOT, "tests", "golden", "replayer", "events.txt"), str(ref)],
                       capture_output=True, text=True, timeout=300)
    print(r.stdout[-4000:], r.stderr[-4000:])
    assert r.returncode == 0
    assert "front_end_device_test: ok" in r.stdout
