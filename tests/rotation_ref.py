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
    """V1-V3 for the in-sensor events -> dict of per-voting-event arrays (x0, y0, al, be, ial, ibe, a, b, X, Y, Z, tau)."""
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
    k = {n: arr[ok] for n, arr in dict(a=a, b=b, X=X, Y=Y, Z=Z, tau=tau, u=u, v=v).items()}
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
