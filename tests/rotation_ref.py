"""The rules of include/ebo.h's "angular velocity from events" (V1-V9, N1-N5) restated in numpy, one operation per
statement: the vote image of events warped by a first-order rotation, its blur, the variance and its exact gradient,
and the three-variable solver.  numpy's elementwise float64 operations round once each, which is the rules' discipline;
sums are numpy's own (pairwise) sums, which V9's bounds allow for.  Test infrastructure: nothing here is the product."""
import math

import numpy as np

EVENT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("sign", "<i4"), ("reserved", "<i4"), ("t_us", "<i8")])

CAM = (200.0, 200.0, 119.5, 89.5)  # fx fy cx cy of the test scenes
W, H = 240, 180
Q = 1073741824.0  # 2^30

RUNNING, CONVERGED_STEP, CONVERGED_GRADIENT, MAX_ITERATIONS, NO_PROGRESS, NONFINITE = -1, 0, 1, 2, 3, 4
DEFAULT_OPTS = dict(first_rate=0.5, c1=1e-4, step_tol=1e-4, max_backtracks=20, max_iterations=100)


def events(x, y, t_us):
    ev = np.zeros(len(x), dtype=EVENT_DTYPE)
    ev["x"], ev["y"], ev["t_us"], ev["sign"] = x, y, t_us, 1
    return ev


def ref_time(ev):
    """The window's reference time as ebo_window_info reports it: the mid of the first and last LISTED stamp, truncated."""
    return int(float(int(ev["t_us"][0]) + int(ev["t_us"][-1])) * 0.5)


def blur_weights(sigma):
    """V5: seven weights divided by their sum taken in the order d = -3 .. 3; sigma 0: the identity."""
    if sigma == 0.0:
        return [0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0]
    g = [math.exp(-float(d * d) / (2.0 * sigma * sigma)) for d in range(-3, 4)]
    s = 0.0
    for v in g:
        s = s + v
    return [v / s for v in g]


def blur(img, g):
    """Horizontal then vertical pass; an output is the sum from 0 in tap order of g_d * value, taps outside skipped."""
    h, w = img.shape
    t = np.zeros_like(img)
    for d in range(-3, 4):
        lo, hi = max(0, -d), min(w, w - d)
        if lo < hi:
            t[:, lo:hi] = t[:, lo:hi] + g[d + 3] * img[:, lo + d:hi + d]
    o = np.zeros_like(img)
    for d in range(-3, 4):
        lo, hi = max(0, -d), min(h, h - d)
        if lo < hi:
            o[lo:hi, :] = o[lo:hi, :] + g[d + 3] * t[lo + d:hi + d, :]
    return o


def warp(ev, t_ref, cam, w, h, omega):
    """V1-V3 for the in-sensor events -> dict of per-voting-event arrays (x0, y0, al, be, ial, ibe, a, b, X, Y, Z, tau, and
    the source pixel x, y)."""
    fx, fy, cx, cy = [np.float64(v) for v in cam]
    wx, wy, wz = [np.float64(v) for v in omega]
    inside = (ev["x"] >= 0) & (ev["x"] < w) & (ev["y"] >= 0) & (ev["y"] < h)  # the stray unit takes no part
    x = ev["x"][inside].astype(np.float64)
    y = ev["y"][inside].astype(np.float64)
    dt = (np.int64(t_ref) - ev["t_us"][inside]).astype(np.float64)
    with np.errstate(all="ignore"):
        a = (x - cx) / fx
        b = (y - cy) / fy
        tau = dt * 1e-6
        thx = tau * wx
        thy = tau * wy
        thz = tau * wz
        X = (a - thy) + thz * b
        Y = (b - thz * a) + thx
        Z = (np.float64(1.0) - thx * b) + thy * a
        ok = Z > 0.0
        u = fx * (X / Z) + cx
        v = fy * (Y / Z) + cy
        ok &= (u > -1.0) & (u < float(w)) & (v > -1.0) & (v < float(h))
    k = {n: arr[ok] for n, arr in dict(a=a, b=b, X=X, Y=Y, Z=Z, tau=tau, u=u, v=v, x=x, y=y).items()}
    fx0 = np.floor(k["u"])
    fy0 = np.floor(k["v"])
    k["x0"] = fx0.astype(np.int64)
    k["y0"] = fy0.astype(np.int64)
    k["al"] = k["u"] - fx0
    k["be"] = k["v"] - fy0
    k["ial"] = 1.0 - k["al"]
    k["ibe"] = 1.0 - k["be"]
    return k


def taps(k):
    """The four taps in the rule's order: (dx, dy, weight)."""
    return [(0, 0, k["ial"] * k["ibe"]), (1, 0, k["al"] * k["ibe"]), (0, 1, k["ial"] * k["be"]), (1, 1, k["al"] * k["be"])]


def votes(k, w, h):
    Hq = np.zeros((h, w), dtype=np.int64)
    for dx, dy, wt in taps(k):
        q = np.rint(wt * Q).astype(np.int64)  # ties to even
        px = k["x0"] + dx
        py = k["y0"] + dy
        ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
        np.add.at(Hq, (py[ok], px[ok]), q[ok])
    return Hq


def eval(ev, t_ref, cam, w, h, omega, sigma_blur=1.0, scale=Q):  # noqa: A001 (the issue's name)
    """-> H int64 [h][w], r, g [3], A [3] (V9's scale of g), sum(B^2) / Np (V9's scale of r).  `scale` other than 2^30 is
    for the quantisation study of tests/test_rotation_cpu.py only."""
    k = warp(ev, t_ref, cam, w, h, omega)
    if scale == Q:
        Hq = votes(k, w, h)
        F = Hq.astype(np.float64) * 2.0 ** -30
    else:
        Hq = None
        F = np.zeros((h, w))
        for dx, dy, wt in taps(k):
            px, py = k["x0"] + dx, k["y0"] + dy
            ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
            np.add.at(F, (py[ok], px[ok]), (np.rint(wt * scale) / scale)[ok])
    g7 = blur_weights(sigma_blur)
    B = blur(F, g7)
    Np = float(w * h)
    mu = B.sum() / Np
    D = B - mu
    r = (D * D).sum() / Np
    C = blur(D, g7)
    c = []
    for dx, dy, _ in taps(k):
        px, py = k["x0"] + dx, k["y0"] + dy
        ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
        cv = np.zeros(len(px))
        cv[ok] = C[py[ok], px[ok]]
        c.append(cv)
    c00, c10, c01, c11 = c
    Du = k["ibe"] * (c10 - c00) + k["be"] * (c11 - c01)
    Dv = k["ial"] * (c01 - c00) + k["al"] * (c11 - c10)
    a, b, X, Y, Z, tau = k["a"], k["b"], k["X"], k["Y"], k["Z"], k["tau"]
    zero, one = np.zeros_like(a), np.ones_like(a)
    dX = (zero, -one, b)
    dY = (one, zero, -a)
    dZ = (-b, a, zero)
    fx, fy = float(cam[0]), float(cam[1])
    g = np.zeros(3)
    A = np.zeros(3)
    for i in range(3):
        du = fx * (dX[i] * Z - X * dZ[i]) / (Z * Z)
        dv = fy * (dY[i] * Z - Y * dZ[i]) / (Z * Z)
        g[i] = (2.0 / Np) * (tau * (Du * du + Dv * dv)).sum()
        A[i] = (2.0 / Np) * (np.abs(tau) * (np.abs(Du * du) + np.abs(Dv * dv))).sum()
    return Hq, float(r), g, A, float((B * B).sum() / Np)


# ---- the solver (N1-N5) --------------------------------------------------------------------------

def _dot(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _finite(f, gf):
    return math.isfinite(f) and all(math.isfinite(v) for v in gf)


def solve(fun, omega0=(0.0, 0.0, 0.0), opts=None):
    """fun(omega [3 floats]) -> (r, g [3]).  -> (omega [3], summary dict, the list of requested omegas)."""
    o = dict(DEFAULT_OPTS)
    o.update(opts or {})
    om = [float(v) for v in omega0]
    requests = [list(om)]
    r, g = fun(om)
    f, gf = -float(r), [-float(v) for v in g]
    s = dict(status=RUNNING, iterations=0, evaluations=1, r_initial=float(r), r_final=float(r))

    def done(status):
        s["status"] = status
        s["r_final"] = -f
        return om, s, requests

    # N1
    if not _finite(f, gf):
        return done(NONFINITE)
    gmax = max(abs(gf[0]), abs(gf[1]), abs(gf[2]))
    if gmax == 0.0:
        return done(CONVERGED_GRADIENT)
    alpha = o["first_rate"] / gmax
    backtracks = 0
    while True:
        # N2
        slope = -_dot(gf, gf)
        om_t = [om[i] + alpha * (-gf[i]) for i in range(3)]
        requests.append(list(om_t))
        r, g = fun(om_t)
        f_t, gf_t = -float(r), [-float(v) for v in g]
        s["evaluations"] += 1
        # N3
        if not (_finite(f_t, gf_t) and f_t <= f + (o["c1"] * alpha) * slope):
            alpha = alpha / 2.0
            backtracks += 1
            if backtracks >= o["max_backtracks"]:
                return done(NO_PROGRESS)
            continue
        # N4
        sv = [om_t[i] - om[i] for i in range(3)]
        yv = [gf_t[i] - gf[i] for i in range(3)]
        om, f, gf = om_t, f_t, gf_t
        s["iterations"] += 1
        backtracks = 0
        if max(abs(sv[0]), abs(sv[1]), abs(sv[2])) < o["step_tol"]:
            return done(CONVERGED_STEP)
        if s["iterations"] == o["max_iterations"]:
            return done(MAX_ITERATIONS)
        sy = _dot(sv, yv)
        alpha = _dot(sv, sv) / sy if sy > 0.0 else 2.0 * alpha


def solve_window(ev, cam=CAM, w=W, h=H, sigma_blur=1.0, omega0=(0.0, 0.0, 0.0), opts=None, t_ref=None):
    t_ref = ref_time(ev) if t_ref is None else t_ref

    def fun(om):
        _, r, g, _, _ = eval(ev, t_ref, cam, w, h, om, sigma_blur)
        return r, g
    return solve(fun, omega0, opts)


# ---- scenes --------------------------------------------------------------------------------------

def rodrigues(rv):
    th = float(np.linalg.norm(rv))
    if th == 0.0:
        return np.eye(3)
    kx, ky, kz = np.asarray(rv, dtype=np.float64) / th
    K = np.array([[0.0, -kz, ky], [kz, 0.0, -kx], [-ky, kx, 0.0]])
    return np.eye(3) + math.sin(th) * K + (1.0 - math.cos(th)) * (K @ K)


def scene(seed, omega, n_events=15000, duration_us=30000, n_segments=25, noise=0.4, cam=CAM, w=W, h=H, t0=0):
    """25 random straight segments, 20-70 px long, as they look at the reference time; every event is a point of a
    segment rotated exactly (Rodrigues) by -omega * (t - t_ref) and projected, plus Gaussian pixel noise, rounded;
    events off the sensor are dropped.  Times are uniform over the duration, sorted."""
    rng = np.random.default_rng(seed)
    fx, fy, cx, cy = cam
    p0 = np.stack([rng.uniform(0, w, n_segments), rng.uniform(0, h, n_segments)], axis=1)
    ang = rng.uniform(0, 2 * math.pi, n_segments)
    length = rng.uniform(20.0, 70.0, n_segments)
    p1 = p0 + length[:, None] * np.stack([np.cos(ang), np.sin(ang)], axis=1)
    t = np.sort(rng.integers(0, duration_us + 1, n_events)).astype(np.int64) + t0
    t[0], t[-1] = t0, t0 + duration_us
    t_ref = int(float(int(t[0]) + int(t[-1])) * 0.5)
    seg = rng.integers(0, n_segments, n_events)
    s = rng.uniform(0.0, 1.0, n_events)
    p = p0[seg] + s[:, None] * (p1[seg] - p0[seg])
    Xr = np.stack([(p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy, np.ones(n_events)], axis=1)
    om = np.asarray(omega, dtype=np.float64)
    out = np.zeros((n_events, 2))
    for i in range(n_events):
        Xt = rodrigues(-om * ((t[i] - t_ref) * 1e-6)) @ Xr[i]
        out[i] = (fx * Xt[0] / Xt[2] + cx, fy * Xt[1] / Xt[2] + cy)
    out = np.rint(out + rng.normal(0.0, noise, out.shape)).astype(np.int64)
    keep = (out[:, 0] >= 0) & (out[:, 0] < w) & (out[:, 1] >= 0) & (out[:, 1] < h)
    keep[0] = keep[-1] = True  # the first and last stamp fix the reference time
    out[0] = np.clip(out[0], 0, [w - 1, h - 1])
    out[-1] = np.clip(out[-1], 0, [w - 1, h - 1])
    return events(out[keep, 0], out[keep, 1], t[keep])


RECOVERY_SEEDS = tuple(range(1, 13))


def recovery_truths():
    """The 12 scenes' angular velocities: uniform in +-5 rad/s per component."""
    return np.random.default_rng(99).uniform(-5.0, 5.0, (len(RECOVERY_SEEDS), 3))


_SCENES = {}


def recovery_scene(i):
    if i not in _SCENES:
        _SCENES[i] = scene(RECOVERY_SEEDS[i], recovery_truths()[i])
    return _SCENES[i]


# ---- the GPU test's cases ------------------------------------------------------------------------

SMALL = dict(w=37, h=29, patch_w=8, patch_h=8, cam=(30.0, 31.0, 18.0, 14.25))  # 4 x 3 patches, the last of each axis wider
LARGE = dict(w=W, h=H, patch_w=20, patch_h=20, cam=CAM)

OMEGAS = {
    "zero": (0.0, 0.0, 0.0),
    "small": (0.3, -0.2, 0.5),
    "x40": (40.0, 0.0, 0.0),
    "y40": (0.0, 40.0, 0.0),
    "z40": (0.0, 0.0, 40.0),
    "huge": (1e9, -1e9, 1e9),
    "nan": (0.3, float("nan"), 0.5),
    "inf": (float("inf"), 0.1, 0.0),
}


def random_window(seed, n, w, h, duration_us=30000, strays=0):
    """n events uniform over the sensor and the duration (sorted), `strays` of them outside the sensor."""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, w, n)
    y = rng.integers(0, h, n)
    t = np.sort(rng.integers(0, duration_us + 1, n)).astype(np.int64)
    if strays:
        idx = rng.choice(n, strays, replace=False)
        x[idx] = rng.choice([-3, -1, w, w + 5], strays)
        y[idx[::2]] = rng.choice([-2, h, h + 7], len(idx[::2]))
    return events(x, y, t)


def border_window(w, h):
    """Events along the four borders and corners with times either side of the reference time: under a small rotation
    x0 = -1, x0 = w - 1, y0 = -1 and y0 = h - 1 occur, with taps half outside; at omega = 0 every event is on an integer."""
    xs, ys = [], []
    for x in range(w):
        xs += [x, x]
        ys += [0, h - 1]
    for y in range(h):
        xs += [0, w - 1]
        ys += [y, y]
    n = len(xs)
    t = (np.arange(n, dtype=np.int64) * 30000) // (n - 1)
    return events(np.array(xs), np.array(ys), t)


def gpu_cases():
    """name -> dict(geo, windows [list of event arrays], omegas [Wn][3], sigma).  Built once, read only."""
    cases = {}
    for gname, geo in (("small", SMALL), ("large", LARGE)):
        w, h = geo["w"], geo["h"]
        one = random_window(5, 1, w, h)
        r300 = random_window(6, 300, w, h, strays=20)
        pile = events(np.full(15000, w // 3), np.full(15000, h // 2), np.full(15000, 777, dtype=np.int64))
        border = border_window(w, h)
        for oname, om in OMEGAS.items():
            wins = [one, r300, border, pile]
            cases["%s_%s" % (gname, oname)] = dict(geo=geo, windows=wins, omegas=np.tile(np.array(om), (len(wins), 1)), sigma=1.0)
    big = scene(3, (1.0, -2.0, 3.0))
    for sigma in (0.0, 1.0, 2.5):
        cases["scene_sigma_%g" % sigma] = dict(geo=LARGE, windows=[big], omegas=np.array([[0.8, -1.5, 2.0]]), sigma=sigma)
    cases["scene_strays"] = dict(geo=LARGE, windows=[random_window(8, 15000, W, H, strays=500)],
                                 omegas=np.array([[2.0, 1.0, -4.0]]), sigma=1.0)
    return cases


def batch_windows(n):
    """n different windows of 37 x 29 with their omegas, for the batch tests."""
    rng = np.random.default_rng(1234)
    wins = [random_window(100 + i, int(rng.integers(3, 600)), SMALL["w"], SMALL["h"], strays=int(i % 3)) for i in range(n)]
    return wins, rng.uniform(-8.0, 8.0, (n, 3))


def same_bits(a, b):
    a = np.ascontiguousarray(a, dtype=np.float64)
    b = np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


# ---- the launch shapes: k_rot_vote's tile and eval_windows' chunks (tests/test_gpu_rotation_shapes.py) ----

MARGIN, TILE_PX = 8, 4096  # kRotMargin and kRotTilePx of csrc/ebo_rotation.inc
CHUNK_MAX, BLOCK = 64, 256  # kRotChunkMax and kRotBlock of csrc/ebo_rotation.h

T150 = dict(w=150, h=128, patch_w=48, patch_h=48, cam=(140.0, 141.0, 74.5, 63.25))  # 48 x 48, 54 x 48, 48 x 80 and 54 x 80
T64 = dict(w=64, h=64, patch_w=64, patch_h=64, cam=(60.0, 61.0, 31.5, 32.25))  # one unit of 4096 px: the last tile
T65 = dict(w=64, h=65, patch_w=64, patch_h=64, cam=(60.0, 61.0, 31.5, 32.25))  # one unit of 4160 px: no tile
T40 = dict(w=40, h=40, patch_w=20, patch_h=20, cam=(38.0, 39.0, 19.5, 20.25))  # four grown tiles, each clipped at two edges
DAVIS346 = dict(w=346, h=260, patch_w=20, patch_h=20, cam=(260.0, 261.0, 172.5, 129.25))  # 352 pixel blocks, 221 patches
TILE_GEOS = dict(t150=T150, t64=T64, t65=T65, t40=T40)
SLOW = (0.006, -0.004, 0.01)  # OMEGAS["small"] / 50: over a 1.5 s window the events stay in view


def grid(geo):
    return geo["w"] // geo["patch_w"], geo["h"] // geo["patch_h"]


def rects(geo):
    """The units' rects (rx, ry, rw, rh) in unit order, as the loader's rect_of: the last patch of an axis takes the rest."""
    npx, npy = grid(geo)
    out = []
    for py in range(npy):
        for px in range(npx):
            rw = geo["w"] - px * geo["patch_w"] if px == npx - 1 else geo["patch_w"]
            rh = geo["h"] - py * geo["patch_h"] if py == npy - 1 else geo["patch_h"]
            out.append((px * geo["patch_w"], py * geo["patch_h"], rw, rh))
    return out


def unit_of(geo, x, y):
    """The unit of in-sensor pixels, as the loader's bucket_of."""
    npx, npy = grid(geo)
    return np.minimum(y // geo["patch_h"], npy - 1) * npx + np.minimum(x // geo["patch_w"], npx - 1)


def tile_margin(rect):
    rx, ry, rw, rh = rect
    return 0 if (rw + 2 * MARGIN) * (rh + 2 * MARGIN) > TILE_PX else MARGIN


def tile_of(rect, w, h):
    """k_rot_vote's LDS tile of a unit (tx0, ty0, tw, th): the margin rule, then the clip to the image, then the size
    rule; tw = th = 0: no tile."""
    rx, ry, rw, rh = rect
    m = tile_margin(rect)
    tx0, ty0 = max(rx - m, 0), max(ry - m, 0)
    tw, th = min(rx + rw + m, w) - tx0, min(ry + rh + m, h) - ty0
    if tw <= 0 or th <= 0 or tw * th > TILE_PX:
        tw = th = 0
    return tx0, ty0, tw, th


def tile_form(rect, w, h):
    """"grown": the rect with its margin; "bare": the rect alone; "none": no tile."""
    if tile_of(rect, w, h)[2] == 0:
        return "none"
    return "grown" if tile_margin(rect) else "bare"


def tap_census(case):
    """form -> dict(units: the (window, unit) pairs of that form with a voting event, inside: their taps that land in the
    unit's tile, direct: their taps that go straight to H).  A tap counts as in k_rot_vote: in the image, weight not 0."""
    geo = case["geo"]
    w, h = geo["w"], geo["h"]
    rs = rects(geo)
    tiles = np.array([tile_of(r, w, h) for r in rs])
    forms = [tile_form(r, w, h) for r in rs]
    out = {f: dict(units=set(), inside=0, direct=0) for f in ("grown", "bare", "none")}
    for i, (ev, om) in enumerate(zip(case["windows"], case["omegas"])):
        k = warp(ev, ref_time(ev), geo["cam"], w, h, om)
        unit = unit_of(geo, k["x"].astype(np.int64), k["y"].astype(np.int64))
        for b in np.unique(unit):
            out[forms[b]]["units"].add((i, int(b)))
        tx0, ty0, tw, th = tiles[unit].T
        for dx, dy, wt in taps(k):
            px, py = k["x0"] + dx, k["y0"] + dy
            counted = (np.rint(wt * Q) != 0) & (px >= 0) & (px < w) & (py >= 0) & (py < h)
            inside = counted & (px - tx0 >= 0) & (px - tx0 < tw) & (py - ty0 >= 0) & (py - ty0 < th)
            for f in out:
                of_form = np.array([forms[b] == f for b in unit], dtype=bool)
                out[f]["inside"] += int((inside & of_form).sum())
                out[f]["direct"] += int((counted & ~inside & of_form).sum())
    return out


_SHAPES = {}


def tile_cases():
    """The four tile geometries at OMEGAS "small" (taps land in the margin) and "x40" (taps leave the tile): 4000 uniform
    events with strays, and the border window.  Built once, read only."""
    if "tile" not in _SHAPES:
        cases = {}
        for gname, geo in TILE_GEOS.items():
            wins = [random_window(21, 4000, geo["w"], geo["h"], strays=20), border_window(geo["w"], geo["h"])]
            for oname in ("small", "x40"):
                cases["%s_%s" % (gname, oname)] = dict(geo=geo, windows=wins, omegas=np.tile(np.array(OMEGAS[oname]), (2, 1)), sigma=1.0)
        _SHAPES["tile"] = cases
    return _SHAPES["tile"]


def davis_cases():
    """346 x 260 with 20 x 20 patches: a scene window of 15 000 events and 15 000 uniform events with 500 strays."""
    if "davis" not in _SHAPES:
        geo = DAVIS346
        wins = [scene(5, (1.0, -2.0, 3.0), cam=geo["cam"], w=geo["w"], h=geo["h"]), random_window(9, 15000, geo["w"], geo["h"], strays=500)]
        om = np.array([[0.8, -1.5, 2.0], [2.0, 1.0, -4.0]])
        _SHAPES["davis"] = {"davis_sigma_%g" % s: dict(geo=geo, windows=wins, omegas=om, sigma=s) for s in (1.0, 2.5)}
    return _SHAPES["davis"]


def long_window(seed, t0):
    """1.5 s of 37 x 29 from t0: the first patch column falls silent after 0.5 s and the last patch of the first row
    wakes after 1.0 s, so their units' own reference times lie far from the window's."""
    ev = random_window(seed, 1500, SMALL["w"], SMALL["h"], duration_us=1500000, strays=10)
    early = (ev["x"] < 8) & (ev["t_us"] > 500000)
    late = (ev["x"] >= 24) & (ev["y"] < 8) & (ev["t_us"] < 1000000)
    ev = ev[~(early | late)]
    ev["t_us"] += t0
    return ev


def long_cases():
    """Two windows of 1.5 s, one from 0 and one from 2 000 000 000 us, at omega 0 and at SLOW."""
    if "long" not in _SHAPES:
        wins = [long_window(31, 0), long_window(32, 2000000000)]
        _SHAPES["long"] = {"long_" + n: dict(geo=SMALL, windows=wins, omegas=np.tile(np.array(om), (2, 1)), sigma=1.0)
                           for n, om in (("zero", OMEGAS["zero"]), ("slow", SLOW))}
    return _SHAPES["long"]


def unit_dt_win(ev, geo):
    """unit -> the loader's dt_win = t_ref(window) - t_ref(unit) of the units that hold events: a unit's reference time
    is the mid of its earliest and latest stamp, truncated."""
    inside = (ev["x"] >= 0) & (ev["x"] < geo["w"]) & (ev["y"] >= 0) & (ev["y"] < geo["h"])
    unit = unit_of(geo, ev["x"][inside].astype(np.int64), ev["y"][inside].astype(np.int64))
    t = ev["t_us"][inside]
    return {int(b): ref_time(ev) - int(float(int(t[unit == b].min()) + int(t[unit == b].max())) * 0.5) for b in np.unique(unit)}


def carve_bytes(geo):
    """The scratch of one chunk slot, as csrc/ebo_rotation.cpp's RotCarve(1, w, h, P): every piece ends on 256 bytes."""
    npx, npy = grid(geo)
    npix = geo["w"] * geo["h"]
    img, part = npix * 8, ((npix + BLOCK - 1) // BLOCK) * 8
    at = 0
    for piece in (img, img, img, part, part, 8, npx * npy * 3 * 8):
        at = (at + piece + 255) & ~255
    return at


def chunk_slots(geo, budget_mb, n):
    """eval_windows' windows per chunk for n windows under EBO_ROTATION_SCRATCH_MB = budget_mb (None: unset, 256)."""
    budget = (256 if budget_mb is None else int(budget_mb)) << 20
    return min(max(1, budget // carve_bytes(geo)), CHUNK_MAX, max(n, 1))
