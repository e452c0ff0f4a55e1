"""The image front end on the MI355X over its whole admitted parameter range (include/ebo.h, "image front end"),
bit for bit against the CPU restatement (tests/frontend_ref.py): gradients and corner lists as arrays, LK next_xy,
status and err as raw bits.  The cases are tests/frontend_cases.py's; tests/test_front_end_cpu.py checks that
they reach every branch of the restatement."""
import ctypes
import math

import numpy as np
import pytest

import frontend_cases as FC
import frontend_ref as F

pytestmark = pytest.mark.gpu


class Contexts:
    """One context per image size (patch no larger than the image), closed at the end of the test."""

    def __init__(self, ebo):
        self.ebo, self.open = ebo, {}

    def __call__(self, w, h):
        if (w, h) not in self.open:
            self.open[(w, h)] = self.ebo.Context(image_w=w, image_h=h, patch_w=min(20, w), patch_h=min(20, h))
        return self.open[(w, h)]

    def close(self):
        for c in self.open.values():
            c.close()


@pytest.fixture
def ctxs(ebo):
    c = Contexts(ebo)
    yield c
    c.close()


def fresh(ebo, w, h):
    return ebo.Context(image_w=w, image_h=h, patch_w=min(20, w), patch_h=min(20, h))


def assert_lk_bits(got, want, name):
    (n, s, e), (rn, rs, re) = got, want
    assert np.array_equal(s, rs), (name, np.flatnonzero(s != rs)[:10])
    bad = np.flatnonzero(np.any(n.view(np.uint32) != rn.view(np.uint32), axis=1))
    assert len(bad) == 0, (name, bad[:10], n[bad[:3]].tolist(), rn[bad[:3]].tolist())
    bad = np.flatnonzero(e.view(np.uint32) != re.view(np.uint32))
    assert len(bad) == 0, (name, bad[:10], e[bad[:3]].tolist(), re[bad[:3]].tolist())


def test_gradients_sweep(ctxs):
    for name, img in FC.gradient_cases():
        h, w = img.shape
        gx, gy = ctxs(w, h).image_gradients(img)
        rx, ry = F.image_gradients(img)
        assert np.array_equal(gx.view(np.uint64), rx.view(np.uint64)), name
        assert np.array_equal(gy.view(np.uint64), ry.view(np.uint64)), name


def _corners(c, img, mask, kw, name):
    got = c.good_features(img, mask=mask, **kw)
    want = F.good_features(img, mask, **kw)
    assert got.shape == want.shape and np.array_equal(got, want), (name, got.shape, want.shape)
    return got


def test_corners_sweep(ctxs):
    for name, img, mask, kw in FC.corner_cases():
        h, w = img.shape
        _corners(ctxs(w, h), img, mask, kw, name)


def test_selection_at_candidate_count_boundaries(ctxs):
    # the greedy pick with max_corners = m is the first m corners of the pick with 8192
    c = ctxs(FC.SELECT_W, FC.SELECT_H)
    for kind in ("noise", "checker"):
        img, _ = FC.select_base(kind)
        for n in FC.SELECT_COUNTS:
            mask = FC.select_mask(kind, n)
            cand = F.candidates(img, mask, 0.0, 3, 0.04)
            assert len(cand) == n, (kind, n)
            for md in (0.0, 3.0, 10.0):
                full = F.greedy(cand, img.shape[1], 8192, md)
                for mc in FC.select_max_corners(n):
                    got = c.good_features(img, mask=mask, max_corners=mc, quality_level=0.0, min_distance=md,
                                          block_size=3, harris_k=0.04)
                    assert np.array_equal(got, full[:mc]), (kind, n, md, mc, got.shape, full[:mc].shape)


def test_selection_distance_ties(ctxs):
    for name, img, mask, kw in FC.tie_cases():
        h, w = img.shape
        _corners(ctxs(w, h), img, mask, kw, name)


def test_lk_sweep(ebo):
    for kind in dict.fromkeys(k for _, k, _, _ in FC.lk_cases()):
        a, b = FC.lk_pair(kind)
        h, w = a.shape
        with fresh(ebo, w, h) as c:
            c.lk_add_image(a)
            c.lk_add_image(b)
            for name, k, pts, kw in FC.lk_cases():
                if k == kind:
                    assert_lk_bits(c.lk_track(pts, **kw), FC.lk_restated(kind).track(pts, **kw), name)


def _batch_points():
    a, _ = FC.lk_pair("tex640s")
    h, w = a.shape
    pts = FC.interior_points(w, h, 40, 77) + FC.bound_points(w, h, (21, 21), 3)[:16]
    pts += FC.special_points(w, h, (21, 21))
    return np.array(pts, dtype=np.float32)


def test_lk_batch_invariance(ebo):
    # k_fe_lk runs 4 points per workgroup: a point's result depends on nothing but the point
    uniq = _batch_points()
    want = FC.lk_restated("tex640s").track(uniq)
    a, b = FC.lk_pair("tex640s")
    h, w = a.shape
    with fresh(ebo, w, h) as c:
        c.lk_add_image(a)
        c.lk_add_image(b)
        for i in range(len(uniq)):
            assert_lk_bits(c.lk_track(uniq[i:i + 1]), tuple(v[i:i + 1] for v in want), "single point %d" % i)
        for n in (1, 3, 4, 5, 257, 4099):
            idx = (np.arange(n) * 37 + n) % len(uniq)  # every point at several positions of the batch
            got = c.lk_track(uniq[idx])
            assert_lk_bits(got, tuple(v[idx] for v in want), "batch of %d" % n)


def _lk_track_raw(ebo, c, pts, with_err):
    n = len(pts)
    nxt = np.zeros((n, 2), np.float32)
    st = np.zeros(n, np.uint8)
    err = np.zeros(n, np.float32)
    lib = ebo.lib()
    rc = lib.ebo_lk_track(c._h, n, ebo._vp(pts), ebo._vp(nxt), ebo._vp(st), ebo._vp(err) if with_err else None,
                          21, 21, 3, 30, ctypes.c_double(0.01), ctypes.c_double(1e-4))
    assert rc == 0, lib.ebo_last_error(c._h)
    return nxt, st, err


def test_lk_without_err(ebo):
    pts = _batch_points()
    a, b = FC.lk_pair("tex640s")
    h, w = a.shape
    with fresh(ebo, w, h) as c:
        c.lk_add_image(a)
        c.lk_add_image(b)
        n1, s1, e1 = _lk_track_raw(ebo, c, pts, True)
        n0, s0, e0 = _lk_track_raw(ebo, c, pts, False)
    assert np.array_equal(n0.view(np.uint32), n1.view(np.uint32)) and np.array_equal(s0, s1)
    assert not e0.any()
    rn, rs, re = FC.lk_restated("tex640s").track(pts)
    assert_lk_bits((n1, s1, e1), (rn, rs, re), "err passed")
    assert s1.any() and not s1.all()  # points with either status


def test_lk_keeps_the_last_two_images(ebo):
    a, b = FC.lk_pair("tex640")
    cimg = FC.lk_pair("tex640s")[0]
    pts = _batch_points()
    h, w = a.shape
    with fresh(ebo, w, h) as c:
        for im in (a, b, cimg):
            c.lk_add_image(im)
        got = c.lk_track(pts)
    with fresh(ebo, w, h) as c:
        c.lk_add_image(b)
        c.lk_add_image(cimg)
        again = c.lk_track(pts)
    lk = F.LK()
    lk.add_image(b)
    lk.add_image(cimg)
    want = lk.track(pts)
    assert_lk_bits(got, want, "a, b, c")
    assert_lk_bits(again, want, "b, c")


def test_interleaved_calls_share_the_workspace(ebo):
    # gradients, corners and LK grow and reuse the same device buffers (ensure()): each result is a fresh context's
    a, b = FC.lk_pair("tex640")
    h, w = a.shape
    pts = _batch_points()
    add_a, add_b = (lambda c: c.lk_add_image(a)), (lambda c: c.lk_add_image(b))
    calls = [
        ("gradients", lambda c: c.image_gradients(a)),
        ("corners 8192", lambda c: (c.good_features(b, max_corners=8192, quality_level=0.0, min_distance=0.0),)),
        ("lk add a", add_a),
        ("gradients b", lambda c: c.image_gradients(b)),
        ("corners 1", lambda c: (c.good_features(a, max_corners=1),)),
        ("lk add b", add_b),
        ("lk track", lambda c: c.lk_track(pts)),
        ("corners 8192 masked", lambda c: (c.good_features(a, mask=F.reference_mask(w, h, 12), max_corners=8192,
                                                           quality_level=0.001, min_distance=2.0, block_size=7),)),
        ("lk track 1", lambda c: c.lk_track(pts[:1], win=(32, 32))),
        ("gradients again", lambda c: c.image_gradients(a)),
    ]
    with fresh(ebo, w, h) as shared:
        got = [f(shared) for _, f in calls]
    for k, (name, f) in enumerate(calls):
        if f in (add_a, add_b):
            continue
        with fresh(ebo, w, h) as c:
            for _, g in calls[:k]:  # the only state a call sees is the images added before it
                if g in (add_a, add_b):
                    g(c)
            want = f(c)
        for x, y in zip(got[k], want):
            assert np.array_equal(np.asarray(x).view(np.uint8), np.asarray(y).view(np.uint8)), name
    assert np.array_equal(got[1][0], F.good_features(b, max_corners=8192, quality_level=0.0, min_distance=0.0))
    gx, gy = F.image_gradients(a)
    assert np.array_equal(got[-1][0].view(np.uint64), gx.view(np.uint64))
    assert_lk_bits(got[6], FC.lk_restated("tex640").track(pts), "interleaved lk track")


def test_rejected_arguments_leave_the_context_usable(ebo):
    a, b = FC.lk_pair("small16x12")
    h, w = a.shape
    pts = np.array([[8, 6], [3.5, 2.25]], np.float32)
    lk = F.LK()
    lk.add_image(a)
    lk.add_image(b)
    bad_corners = [dict(max_corners=0), dict(max_corners=8193), dict(block_size=0), dict(block_size=8),
                   dict(quality_level=math.nan), dict(quality_level=-0.01), dict(min_distance=math.nan),
                   dict(min_distance=-1.0)]
    bad_lk = [dict(win=(2, 21)), dict(win=(21, 2)), dict(win=(33, 32)), dict(max_level=8), dict(max_count=0),
              dict(epsilon=-1.0), dict(epsilon=math.nan), dict(min_eig_threshold=math.nan)]
    with fresh(ebo, w, h) as c:
        c.lk_add_image(a)
        c.lk_add_image(b)
        for kw in bad_corners:
            with pytest.raises(ebo.EboError) as ei:
                c.good_features(a, **kw)
            assert ei.value.code == ebo.ERR_ARG, kw
            assert np.array_equal(c.good_features(a, min_distance=1.0), F.good_features(a, min_distance=1.0)), kw
        for kw in bad_lk:
            with pytest.raises(ebo.EboError) as ei:
                c.lk_track(pts, **kw)
            assert ei.value.code == ebo.ERR_ARG, kw
            assert_lk_bits(c.lk_track(pts), lk.track(pts), "after %s" % kw)
