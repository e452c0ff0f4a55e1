"""numpy restatement of the camera model of include/ebo.h ("camera model"): the yardstick of the camera tests.

Float64 throughout, ONE operation per statement, in the association the header writes out, so that every
intermediate is rounded exactly once (numpy's + - * / sqrt on float64 arrays are correctly rounded and never
fused).  A camera is nine numbers in ebo_camera's order: fx fy cx cy k1 k2 k3 p1 p2 (k3 is carried, never used)."""
import numpy as np

# the calibration of the reference's own camera test (a DAVIS240C), in ebo_camera's order
DAVIS = (199.092366542, 198.82882047, 132.192071378, 110.712660011, -0.368436311798, 0.150947243557, 0.0,
         -0.000296130534385, -0.000759431726241)
# the recording reader test's calib.txt (fx fy cx cy k1 k2 p1 p2 k3 = 501 499 249 251 0.11 0.011 0.0011 0.123 0.321)
READER = (501.0, 499.0, 249.0, 251.0, 0.11, 0.011, 0.321, 0.0011, 0.123)
PINHOLE = (200.0, 200.0, 120.0, 90.0, 0.0, 0.0, 0.0, 0.0, 0.0)
COORD_MIN, COORD_MAX = -16384, 16383


def _f64(a):
    return np.asarray(a, dtype=np.float64)


def _tangential(pa, pb, a, b, r2):
    t0 = np.float64(2.0) * pa
    t1 = t0 * a
    lhs = t1 * b
    t2 = np.float64(2.0) * a
    t3 = t2 * a
    t4 = r2 + t3
    rhs = pb * t4
    return lhs + rhs


def _radial(k1, k2, r2):
    t0 = k1 * r2
    t1 = np.float64(1.0) + t0
    t2 = k2 * r2
    t3 = t2 * r2
    return t1 + t3


def _r2(x, y):
    xx = x * x
    yy = y * y
    return xx + yy


def project(cam, p):
    """p: [n][3] points in the camera frame -> [n][2] pixels."""
    fx, fy, cx, cy, k1, k2, _k3, p1, p2 = (np.float64(v) for v in cam)
    p = _f64(p).reshape(-1, 3)
    with np.errstate(all="ignore"):
        xp = p[:, 0] / p[:, 2]
        yp = p[:, 1] / p[:, 2]
        r2 = _r2(xp, yp)
        rad = _radial(k1, k2, r2)
        xr = xp * rad
        yr = yp * rad
        xd = xr + _tangential(p1, p2, xp, yp, r2)
        yd = yr + _tangential(p2, p1, yp, xp, r2)
        fxd = fx * xd
        fyd = fy * yd
        u = fxd + cx
        v = fyd + cy
    return np.stack([u, v], axis=1)


def undistort(cam, uv):
    """uv: [n][2] pixels -> (xOpt, yOpt), the ten-iteration fixed point in normalised coordinates."""
    fx, fy, cx, cy, k1, k2, _k3, p1, p2 = (np.float64(v) for v in cam)
    uv = _f64(uv).reshape(-1, 2)
    with np.errstate(all="ignore"):
        xs = uv[:, 0] - cx
        ys = uv[:, 1] - cy
        xd = xs / fx
        yd = ys / fy
        xo, yo = xd.copy(), yd.copy()
        for _ in range(10):
            r2 = _r2(xo, yo)
            rad = _radial(k1, k2, r2)
            dx = _tangential(p1, p2, xo, yo, r2)
            dy = _tangential(p2, p1, yo, xo, r2)
            nx = xd - dx
            ny = yd - dy
            xo = nx / rad
            yo = ny / rad
    return xo, yo


def unproject(cam, uv):
    """uv: [n][2] pixels -> [n][3] unit bearing vectors."""
    xo, yo = undistort(cam, uv)
    with np.errstate(all="ignore"):
        s = _r2(xo, yo)
        s1 = s + np.float64(1.0)
        norm = np.sqrt(s1)
        bx = xo / norm
        by = yo / norm
        bz = np.float64(1.0) / norm
    return np.stack([bx, by, bz], axis=1)


def round_half_away(a):
    """std::round: half away from zero (np.round is half to even)."""
    a = _f64(a)
    m = np.abs(a)
    f = np.floor(m)
    frac = m - f  # exact: f <= m < f + 1
    return np.copysign(np.where(frac >= 0.5, f + 1.0, f), a)


def rectify_map(cam, w, h):
    """-> (map float64 [h][w][2], table int16 [h][w][2], ok).  ok is False where ebo_set_rectification refuses:
    fx / fy not finite or zero, a map that is not finite, a rounded coordinate outside the record range (the
    table is then not meaningful)."""
    fx, fy, cx, cy = (np.float64(v) for v in cam[:4])
    ys, xs = np.mgrid[0:h, 0:w]
    uv = np.stack([xs.ravel(), ys.ravel()], axis=1).astype(np.float64)
    xo, yo = undistort(cam, uv)
    with np.errstate(all="ignore"):
        fu = fx * xo
        fv = fy * yo
        u = fu + cx
        v = fv + cy
    m = np.stack([u, v], axis=1).reshape(h, w, 2)
    ok = bool(np.isfinite(fx) and np.isfinite(fy) and fx != 0 and fy != 0 and np.isfinite(m).all())
    lut = np.zeros((h, w, 2), dtype=np.int16)
    if ok:
        r = round_half_away(m)
        ok = bool((r >= COORD_MIN).all() and (r <= COORD_MAX).all())
        if ok:
            lut = r.astype(np.int16)
    return m, lut, ok


def rectify_events(cam, w, h, ev):
    """A copy of the event records with every in-sensor (x, y) replaced by its table entry; events whose raw
    coordinate lies outside the sensor are left as they are."""
    _, lut, ok = rectify_map(cam, w, h)
    assert ok
    out = ev.copy()
    x, y = ev["x"].astype(np.int64), ev["y"].astype(np.int64)
    inside = (x >= 0) & (x < w) & (y >= 0) & (y < h)
    out["x"][inside] = lut[y[inside], x[inside], 0]
    out["y"][inside] = lut[y[inside], x[inside], 1]
    return out
