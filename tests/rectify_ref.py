"""numpy restatement of the rectified-frame rules of include/ebo.h ("camera model", C1-C5): the yardstick of the
rectification tests.  Built on camera_ref's undistort / project / round_half_away; float64 throughout, ONE operation
per statement in the association the header writes out.  A camera is nine numbers in ebo_camera's order; a
rectified camera is one whose k1 k2 p1 p2 are zero."""
import numpy as np

import camera_ref

ERR_ARG, ERR_RANGE = "arg", "range"


def rectified(fx, fy, cx, cy):
    return (float(fx), float(fy), float(cx), float(cy), 0.0, 0.0, 0.0, 0.0, 0.0)


def same_k(cam):
    """The rectified camera ebo_set_rectification uses: it keeps fx fy cx cy."""
    return rectified(*cam[:4])


def check_rectified(r):
    """C1 -> None, ERR_ARG or ERR_RANGE."""
    if not (r[4] == 0.0 and r[5] == 0.0 and r[7] == 0.0 and r[8] == 0.0):
        return ERR_ARG
    if not (np.isfinite(r[0]) and np.isfinite(r[1])) or r[0] == 0.0 or r[1] == 0.0:
        return ERR_RANGE
    return None


def _pixels(w, h):
    ys, xs = np.mgrid[0:h, 0:w]
    return np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float64)


def forward_map(cam, r, w, h):
    """C2 -> (map float64 [h][w][2], table int16 [h][w][2], ok)."""
    rfx, rfy, rcx, rcy = (np.float64(v) for v in r[:4])
    xo, yo = camera_ref.undistort(cam, _pixels(w, h))
    with np.errstate(all="ignore"):
        fu = rfx * xo
        fv = rfy * yo
        u = fu + rcx
        v = fv + rcy
    m = np.stack([u, v], axis=1).reshape(h, w, 2)
    ok = check_rectified(r) is None and bool(np.isfinite(cam[0]) and np.isfinite(cam[1]) and cam[0] != 0 and cam[1] != 0)
    ok = ok and bool(np.isfinite(m).all())
    lut = np.zeros((h, w, 2), dtype=np.int16)
    if ok:
        q = camera_ref.round_half_away(m)
        ok = bool((q >= camera_ref.COORD_MIN).all() and (q <= camera_ref.COORD_MAX).all())
        if ok:
            lut = q.astype(np.int16)
    return m, lut, ok


def border_pixels(w, h):
    xs = np.arange(w, dtype=np.float64)
    ys = np.arange(h, dtype=np.float64)
    return np.concatenate([np.stack([xs, np.zeros(w)], axis=1), np.stack([xs, np.full(w, h - 1.0)], axis=1),
                           np.stack([np.zeros(h), ys], axis=1), np.stack([np.full(h, w - 1.0), ys], axis=1)])


def border_extremes(cam, w, h):
    """-> (xmin, xmax, ymin, ymax) of undistort over rows 0, h-1 and columns 0, w-1 (NaN if any is NaN)."""
    xo, yo = camera_ref.undistort(cam, border_pixels(w, h))
    return np.min(xo), np.max(xo), np.min(yo), np.max(yo)


def fit(cam, w, h):
    """C3 -> the fitted rectified camera (nine floats), or None where ebo_fit_rectified_camera refuses."""
    fx, fy = np.float64(cam[0]), np.float64(cam[1])
    if w < 2 or h < 2 or not fx > 0 or not fy > 0:
        return None
    xo, yo = camera_ref.undistort(cam, border_pixels(w, h))
    if not (np.isfinite(xo).all() and np.isfinite(yo).all()):
        return None
    xmin, xmax, ymin, ymax = np.min(xo), np.max(xo), np.min(yo), np.max(yo)
    wm, hm = np.float64(w - 1), np.float64(h - 1)
    ex = xmax - xmin
    ey = ymax - ymin
    if not ex > 0 or not ey > 0:
        return None
    dx = fx * ex
    dy = fy * ey
    sx = wm / dx
    sy = hm / dy
    s = sx if sx < sy else sy
    rfx = s * fx
    rfy = s * fy
    tx = xmax + xmin
    ty = ymax + ymin
    mx = rfx * tx
    my = rfy * ty
    nx = wm - mx
    ny = hm - my
    rcx = nx / np.float64(2.0)
    rcy = ny / np.float64(2.0)
    return rectified(rfx, rfy, rcx, rcy)


def source_map(cam, r, w, h):
    """C4 -> float64 [h][w][2] = (us, vs)."""
    rfx, rfy, rcx, rcy = (np.float64(v) for v in r[:4])
    px = _pixels(w, h)
    with np.errstate(all="ignore"):
        xs = px[:, 0] - rcx
        ys = px[:, 1] - rcy
        xn = xs / rfx
        yn = ys / rfy
    return camera_ref.project(cam, np.stack([xn, yn, np.ones_like(xn)], axis=1)).reshape(h, w, 2)


def remap(image, src):
    """C5: image uint8 [h][w], src float64 [h][w][2] -> (uint8 [h][w], all_taps_inside bool [h][w])."""
    image = np.ascontiguousarray(image, dtype=np.uint8)
    h, w = image.shape
    us, vs = src[..., 0], src[..., 1]
    with np.errstate(all="ignore"):
        ok = (us > -1.0) & (us < np.float64(w)) & (vs > -1.0) & (vs < np.float64(h))
    us = np.where(ok, us, 0.0)
    vs = np.where(ok, vs, 0.0)
    x0f = np.floor(us)
    y0f = np.floor(vs)
    a = us - x0f
    b = vs - y0f
    ia = np.float64(1.0) - a
    ib = np.float64(1.0) - b
    x0 = x0f.astype(np.int64)
    y0 = y0f.astype(np.int64)

    def tap(x, y):
        inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        return np.where(inside, image[np.clip(y, 0, h - 1), np.clip(x, 0, w - 1)], 0).astype(np.float64), inside

    p00, i00 = tap(x0, y0)
    p10, i10 = tap(x0 + 1, y0)
    p01, i01 = tap(x0, y0 + 1)
    p11, i11 = tap(x0 + 1, y0 + 1)
    t0 = ia * p00
    t1 = a * p10
    top = t0 + t1
    b0 = ia * p01
    b1 = a * p11
    bot = b0 + b1
    v0 = ib * top
    v1 = b * bot
    val = v0 + v1
    out = np.where(ok, camera_ref.round_half_away(val), 0.0).astype(np.uint8)
    return out, ok & i00 & i10 & i01 & i11


def rectify_image(cam, r, image):
    h, w = np.asarray(image).shape
    return remap(image, source_map(cam, r, w, h))[0]


def rectify_events(cam, r, w, h, ev):
    """camera_ref.rectify_events through the table of C2."""
    _, lut, ok = forward_map(cam, r, w, h)
    assert ok
    out = ev.copy()
    x, y = ev["x"].astype(np.int64), ev["y"].astype(np.int64)
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    out["x"][inside] = lut[y[inside], x[inside], 0]
    out["y"][inside] = lut[y[inside], x[inside], 1]
    return out


def outside_count(lut, w, h):
    return int(((lut[..., 0] < 0) | (lut[..., 0] >= w) | (lut[..., 1] < 0) | (lut[..., 1] >= h)).sum())
