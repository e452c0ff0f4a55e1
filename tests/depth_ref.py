"""The rules of include/ebo.h's "depth from events" (M1-M9) restated in numpy, one operation per statement: the planes
of a reference view, the relative pose of a window, the ray of an event through every plane, the bilinear vote in exact
fixed point into the uint32 volume, and the extraction (confidence, adaptive threshold, median, point list).  numpy's
elementwise float64 operations round once each, which is the rules' discipline.  Test infrastructure: nothing here is
the product."""
import math

import numpy as np

EVENT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("sign", "<i4"), ("reserved", "<i4"), ("t_us", "<i8")])
Q = 1024.0  # 2^10
MAX_EVENTS = 1 << 21
DEFAULTS = dict(nz=64, z_near=0.5, z_far=8.0, box_radius=2, min_excess=3.0, median_radius=2)


def events(x, y, t_us=None):
    ev = np.zeros(len(x), dtype=EVENT_DTYPE)
    ev["x"], ev["y"], ev["sign"] = x, y, 1
    ev["t_us"] = np.arange(len(x), dtype=np.int64) * 7 if t_us is None else t_us
    return ev


def pose(R=None, t=(0.0, 0.0, 0.0)):
    """12 doubles (R row-major, t), camera to world."""
    R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64)
    return np.concatenate([R.reshape(9), np.asarray(t, dtype=np.float64)])


def rot(axis, deg):
    c, s = math.cos(math.radians(deg)), math.sin(math.radians(deg))
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def planes(nz, z_near, z_far):
    """M1"""
    rho0 = 1.0 / z_near
    drho = (1.0 / z_far - rho0) / float(nz - 1)
    return np.array([1.0 / (rho0 + float(k) * drho) for k in range(nz)])


def relative_pose(ref, win):
    """M2's host part -> (Rr [3][3], tr [3])"""
    with np.errstate(all="ignore"):
        Rf, tf = np.asarray(ref[:9], dtype=np.float64).reshape(3, 3), np.asarray(ref[9:], dtype=np.float64)
        Rw, tw = np.asarray(win[:9], dtype=np.float64).reshape(3, 3), np.asarray(win[9:], dtype=np.float64)
        Rr = np.zeros((3, 3))
        tr = np.zeros(3)
        e = tw - tf
        for i in range(3):
            for j in range(3):
                Rr[i, j] = (Rf[0, i] * Rw[0, j] + Rf[1, i] * Rw[1, j]) + Rf[2, i] * Rw[2, j]
            tr[i] = (Rf[0, i] * e[0] + Rf[1, i] * e[1]) + Rf[2, i] * e[2]
    return Rr, tr


def in_sensor(ev, w, h):
    return (ev["x"] >= 0) & (ev["x"] < w) & (ev["y"] >= 0) & (ev["y"] < h)  # the stray unit takes no part


def project(x, y, Rr, tr, cam, w, h, zk):
    """M2's ray and M3 for arrays of integer pixels on one plane -> (voting mask, u, v)"""
    fx, fy, cx, cy = [np.float64(v) for v in cam]
    x = np.asarray(x).astype(np.float64)
    y = np.asarray(y).astype(np.float64)
    with np.errstate(all="ignore"):
        a = (x - cx) / fx
        b = (y - cy) / fy
        d0 = (Rr[0, 0] * a + Rr[0, 1] * b) + Rr[0, 2]
        d1 = (Rr[1, 0] * a + Rr[1, 1] * b) + Rr[1, 2]
        d2 = (Rr[2, 0] * a + Rr[2, 1] * b) + Rr[2, 2]
        lam = (np.float64(zk) - tr[2]) / d2
        ok = lam > 0.0
        X = tr[0] + lam * d0
        Y = tr[1] + lam * d1
        u = fx * (X / np.float64(zk)) + cx
        v = fy * (Y / np.float64(zk)) + cy
        ok &= (u > -1.0) & (u < float(w)) & (v > -1.0) & (v < float(h))
    return ok, u, v


def vote_plane(Hk, u, v, w, h):
    """M4 for the voting events of one plane, in place -> the x0 and y0 seen"""
    fx0 = np.floor(u)
    fy0 = np.floor(v)
    x0 = fx0.astype(np.int64)
    y0 = fy0.astype(np.int64)
    al = u - fx0
    be = v - fy0
    ial = 1.0 - al
    ibe = 1.0 - be
    for dx, dy, wt in ((0, 0, ial * ibe), (1, 0, al * ibe), (0, 1, ial * be), (1, 1, al * be)):
        q = np.rint(wt * Q).astype(np.int64)  # ties to even
        px, py = x0 + dx, y0 + dy
        ok = (px >= 0) & (px < w) & (py >= 0) & (py < h)
        # float64 sums of integers below 2^53 are exact
        Hk += np.bincount(py[ok] * w + px[ok], weights=q[ok], minlength=h * w).astype(np.int64).reshape(h, w)
    return x0, y0


def volume(windows, poses, ref_pose, cam, w, h, z, use=None, H=None, seen=None):
    """H uint32 [nz][h][w] of the windows' in-sensor events (added to H when given).  `seen`: a dict that collects the
    set of x0 and of y0 that occurred."""
    acc = np.zeros((len(z), h, w), dtype=np.int64) if H is None else H.astype(np.int64)
    for i, ev in enumerate(windows):
        if use is not None and not use[i]:
            continue
        Rr, tr = relative_pose(ref_pose, poses[i])
        keep = in_sensor(ev, w, h)
        x, y = ev["x"][keep], ev["y"][keep]
        for k, zk in enumerate(z):
            ok, u, v = project(x, y, Rr, tr, cam, w, h, zk)
            x0, y0 = vote_plane(acc[k], u[ok], v[ok], w, h)
            if seen is not None:
                seen.setdefault("x0", set()).update(np.unique(x0).tolist())
                seen.setdefault("y0", set()).update(np.unique(y0).tolist())
    assert acc.max(initial=0) < 2 ** 32
    return acc.astype(np.uint32)


def counted_events(windows, w, h, use=None):
    """M4's count: the in-sensor events of the windows a call votes"""
    return int(sum(in_sensor(ev, w, h).sum() for i, ev in enumerate(windows) if use is None or use[i]))


def offset(min_excess):
    """M6's off"""
    return int(np.rint(min(float(min_excess), 4194304.0) * Q))


def extract(H, z, cam, box_radius=2, min_excess=3.0, median_radius=2):
    """M5-M8 -> index int32 [h][w], conf uint32 [h][w], depth [h][w], points [n][3]"""
    nz, h, w = H.shape
    conf = H.max(axis=0)
    kbest = H.argmax(axis=0)  # the first maximum
    c = conf.astype(np.int64)
    r = box_radius
    S = np.zeros((h, w), dtype=np.int64)
    cnt = np.zeros((h, w), dtype=np.int64)
    for dy in range(-r, r + 1):
        for dx in range(-r, r + 1):
            ys, ye = max(0, -dy), min(h, h - dy)
            xs, xe = max(0, -dx), min(w, w - dx)
            if ys < ye and xs < xe:
                S[ys:ye, xs:xe] += c[ys + dy:ye + dy, xs + dx:xe + dx]
                cnt[ys:ye, xs:xe] += 1
    keep = (c > 0) & (c * cnt > S + offset(min_excess) * cnt)
    index = np.where(keep, kbest, -1).astype(np.int32)
    m = median_radius
    if m > 0:
        for y, x in zip(*np.nonzero(keep)):
            ya, yb, xa, xb = max(y - m, 0), min(y + m, h - 1), max(x - m, 0), min(x + m, w - 1)
            box = kbest[ya:yb + 1, xa:xb + 1][keep[ya:yb + 1, xa:xb + 1]]
            index[y, x] = np.sort(box)[(len(box) - 1) // 2]
    depth = np.where(keep, z[np.maximum(index, 0)], 0.0)
    fx, fy, cx, cy = [np.float64(v) for v in cam]
    ys, xs = np.nonzero(keep)  # row-major
    zz = depth[ys, xs]
    a = (xs.astype(np.float64) - cx) / fx
    b = (ys.astype(np.float64) - cy) / fy
    points = np.stack([a * zz, b * zz, zz], axis=1) if len(zz) else np.zeros((0, 3))
    return index, conf.astype(np.uint32), depth, points


# ---- the recovery scene --------------------------------------------------------------------------

SCENE = dict(w=64, h=48, patch_w=16, patch_h=16, cam=(60.0, 60.0, 32.0, 24.0))
SCENE_PARAMS = dict(nz=32, z_near=1.0, z_far=8.0, box_radius=2, min_excess=3.0, median_radius=0)
SCENE_SEEDS = (0, 1, 2, 3)


def recovery_scene(seed, two_depths):
    """40 points with X, Y = U(+-0.8, +-0.6) * Z / 2 at Z = 2 (two_depths: every second one at Z = 4), seen from nine
    poses with identity rotation and centres x = -0.5 .. 0.5, the middle one the reference; one window per pose, its
    events the rounded projections of the points, deduplicated.  -> (windows, poses, reference pose, points [40][3])"""
    rng = np.random.default_rng(seed)
    w, h = SCENE["w"], SCENE["h"]
    fx, fy, cx, cy = SCENE["cam"]
    Z = np.full(40, 2.0)
    if two_depths:
        Z[1::2] = 4.0
    X = rng.uniform(-0.8, 0.8, 40) * Z / 2.0
    Y = rng.uniform(-0.6, 0.6, 40) * Z / 2.0
    pts = np.stack([X, Y, Z], axis=1)
    centres = np.linspace(-0.5, 0.5, 9)
    poses = [pose(t=(c, 0.0, 0.0)) for c in centres]
    windows = []
    for c in centres:
        u = np.rint(fx * (X - c) / Z + cx).astype(np.int64)
        v = np.rint(fy * Y / Z + cy).astype(np.int64)
        ok = (u >= 0) & (u < w) & (v >= 0) & (v < h)
        uv = np.unique(np.stack([v[ok], u[ok]], axis=1), axis=0)
        windows.append(events(uv[:, 1], uv[:, 0]))
    return windows, poses, poses[4], pts


def true_plane(Z, nz, z_near, z_far):
    """The plane nearest to depth Z in inverse depth"""
    rho0 = 1.0 / z_near
    drho = (1.0 / z_far - rho0) / float(nz - 1)
    return int(np.rint((1.0 / Z - rho0) / drho))


def recovery_figures(index, pts):
    """-> (pixels kept, kept pixels NOT within 1.5 px and +-1 plane of a point, points whose rounded reference pixel is
    kept with a plane within +-1 of the true one)"""
    fx, fy, cx, cy = SCENE["cam"]
    p = SCENE_PARAMS
    up = fx * pts[:, 0] / pts[:, 2] + cx
    vp = fy * pts[:, 1] / pts[:, 2] + cy
    kp = np.array([true_plane(zz, p["nz"], p["z_near"], p["z_far"]) for zz in pts[:, 2]])
    recovered = 0
    for u, v, k in zip(np.rint(up).astype(int), np.rint(vp).astype(int), kp):
        if 0 <= u < SCENE["w"] and 0 <= v < SCENE["h"] and index[v, u] >= 0 and abs(int(index[v, u]) - k) <= 1:
            recovered += 1
    ys, xs = np.nonzero(index >= 0)
    off = 0
    for y, x in zip(ys, xs):
        near = (np.hypot(up - x, vp - y) <= 1.5) & (np.abs(kp - int(index[y, x])) <= 1)
        off += 0 if near.any() else 1
    return len(ys), off, recovered


def check_recovery(index, pts):
    """The two conditions of the recovery test, on a plane-index map"""
    kept, off, recovered = recovery_figures(index, pts)
    assert recovered >= 36, (kept, off, recovered)
    assert kept - off >= 0.95 * kept, (kept, off, recovered)
    return kept, off, recovered


# ---- the GPU test's cases ------------------------------------------------------------------------

SMALL = dict(w=37, h=29, patch_w=8, patch_h=8, cam=(30.0, 31.0, 18.0, 14.25))  # 4 x 3 patches, the last of each axis wider
MEDIUM = dict(w=64, h=48, patch_w=16, patch_h=16, cam=(60.0, 60.0, 32.0, 24.0))
GEOS = dict(small=SMALL, medium=MEDIUM)
NZS = (2, 5, 32)
Z_RANGE = (1.0, 8.0)
REF_POSE = pose(rot(1, 3.0) @ rot(0, -2.0), (0.1, -0.2, 0.3))  # not the identity: M2's products are exercised


def _rel(R=None, t=(0.0, 0.0, 0.0)):
    """The world pose of a camera whose pose RELATIVE to the reference view is (R, t)"""
    R = np.eye(3) if R is None else R
    Rf, tf = REF_POSE[:9].reshape(3, 3), REF_POSE[9:]
    return pose(Rf @ R, Rf @ np.asarray(t, dtype=np.float64) + tf)


def _with(p, i, v):
    p = p.copy()
    p[i] = v
    return p


POSES = {
    "reference": REF_POSE,                       # every plane is 1024 x the count image
    "identity": pose(),
    "tx": _rel(t=(0.3, 0.0, 0.0)),
    "tx_neg": _rel(t=(-0.011, 0.0, 0.0)),         # border events: x0 = -1 on the left, x0 = w - 1 with "tx_pos"
    "tx_pos": _rel(t=(0.011, 0.0, 0.0)),
    "ty_neg": _rel(t=(0.0, -0.013, 0.0)),
    "ty_pos": _rel(t=(0.0, 0.012, 0.0)),
    "ty": _rel(t=(0.0, 0.2, 0.0)),
    "tz": _rel(t=(0.0, 0.0, 0.4)),
    "tz_near": _rel(t=(0.0, 0.0, 2.5)),           # beyond the near planes: lam <= 0 on some planes only
    "tz_beyond": _rel(t=(0.0, 0.0, 20.0)),        # beyond all of them, looking away: no vote
    "behind": _rel(rot(1, 180.0), (0.0, 0.0, 10.0)),  # behind the volume, looking back at it
    "rx5": _rel(rot(0, 5.0), (0.05, 0.0, 0.0)),
    "ry5": _rel(rot(1, 5.0), (0.0, 0.05, 0.0)),
    "rz5": _rel(rot(2, 5.0), (0.02, -0.02, 0.1)),
    "nan": _with(_rel(t=(0.1, 0.0, 0.0)), 4, float("nan")),
    "inf": _with(_rel(t=(0.1, 0.0, 0.0)), 9, float("inf")),
    "inf_rotation": _with(_rel(t=(0.1, 0.0, 0.0)), 8, float("-inf")),
}
NO_VOTE = ("tz_beyond", "nan", "inf", "inf_rotation")


def random_window(seed, n, w, h, strays=0):
    """n events uniform over the sensor, `strays` of them outside it"""
    rng = np.random.default_rng(seed)
    x = rng.integers(0, w, n)
    y = rng.integers(0, h, n)
    if strays:
        idx = rng.choice(n, strays, replace=False)
        x[idx] = rng.choice([-3, -1, w, w + 5], strays)
        y[idx[::2]] = rng.choice([-2, h, h + 7], len(idx[::2]))
    return events(x, y)


def border_window(w, h):
    """Every pixel of the four borders, corners twice"""
    xs = list(range(w)) * 2 + [0] * h + [w - 1] * h
    ys = [0] * w + [h - 1] * w + list(range(h)) * 2
    return events(np.array(xs), np.array(ys))


_WINDOWS = {}


def case_windows(gname):
    """The five windows of a sensor: 1 event, 300 with strays, the borders, 5000 on one pixel, 5000 spread.  Built
    once, read only."""
    if gname not in _WINDOWS:
        w, h = GEOS[gname]["w"], GEOS[gname]["h"]
        _WINDOWS[gname] = [random_window(5, 1, w, h), random_window(6, 300, w, h, strays=20), border_window(w, h),
                           events(np.full(5000, w // 3), np.full(5000, h // 2)), random_window(7, 5000, w, h, strays=100)]
    return _WINDOWS[gname]


def batch(n, gname="small"):
    """n different windows of a sensor with a pose each, for the order and batching tests"""
    rng = np.random.default_rng(4321)
    w, h = GEOS[gname]["w"], GEOS[gname]["h"]
    wins = [random_window(200 + i, int(rng.integers(3, 400)), w, h, strays=int(i % 3)) for i in range(n)]
    names = [k for k in POSES if k not in NO_VOTE]
    return wins, [POSES[names[i % len(names)]] for i in range(n)]


# ---- the launch shapes: dsi_tile's outcomes, the plane split and the point list's scan (tests/test_gpu_depth_shapes.py) ----

TILE_MARGIN, TILE_PX, WAVES, BLOCK = 1, 1024, 4, 256  # kDsiMargin, kDsiTilePx, kDsiWaves and kDsiBlock of csrc/ebo_depth.inc
OUTCOMES = ("tile", "lam", "far", "off", "large")

# a view turned by 90 degrees about y, 4 units along -x: d2 = cos(90 deg) - sin(90 deg) * a changes sign where x passes
# cx, so lam is of either sign and of any size; the rays left of cx come back into the image
SHAPE_POSE_TABLE = dict(POSES)  # POSES itself stays as tests/test_gpu_depth.py's parameters
SHAPE_POSE_TABLE["ry90"] = _rel(rot(1, 90.0), (-4.0, 0.0, 0.0))
SHAPE_POSE_TABLE["drift_a"] = _rel(t=(0.02, 0.01, 0.0))  # a few pixels: a region without events stays without votes
SHAPE_POSE_TABLE["drift_b"] = _rel(rot(2, 1.0), (-0.015, 0.02, 0.0))
SHAPE_POSES = ("rz5", "tz_near", "behind", "tx", "ry5", "ry90")  # test_gpu_depth.py's A/B list and the near-90-degree view
BIG_PATCH = dict(w=64, h=48, patch_w=32, patch_h=32, cam=(60.0, 60.0, 32.0, 24.0))  # two units of 32 x 48: no box fits a tile
FINE = dict(w=37, h=29, patch_w=4, patch_h=4, cam=SMALL["cam"])  # 63 units: 17 windows are 1071 (patch, window) pairs
SCAN_GEOS = {
    "255_blocks": dict(w=256, h=255, patch_w=20, patch_h=20, cam=(240.0, 241.0, 127.5, 127.25), hole_x=64),
    "256_blocks": dict(w=256, h=256, patch_w=20, patch_h=20, cam=(240.0, 241.0, 127.5, 127.25), hole_x=64),
    "257_blocks": dict(w=257, h=256, patch_w=20, patch_h=20, cam=(240.0, 241.0, 128.0, 127.25), hole_x=20),
    "352_blocks": dict(w=346, h=260, patch_w=20, patch_h=20, cam=(260.0, 261.0, 172.5, 129.25), hole_x=120),
}
SCAN_POSES = ("tx_neg", "tx_pos", "ty_neg", "ty_pos", "drift_a", "drift_b")
SCAN_NZ, SCAN_EXCESS = 5, 0.125
PLANE_COUNTS = (253, 255, 256)


def rects(geo):
    """The units' rects (rx, ry, rw, rh) in unit order, as the loader's rect_of: the last patch of an axis takes the rest."""
    npx, npy = geo["w"] // geo["patch_w"], geo["h"] // geo["patch_h"]
    out = []
    for py in range(npy):
        for px in range(npx):
            rw = geo["w"] - px * geo["patch_w"] if px == npx - 1 else geo["patch_w"]
            rh = geo["h"] - py * geo["patch_h"] if py == npy - 1 else geo["patch_h"]
            out.append((px * geo["patch_w"], py * geo["patch_h"], rw, rh))
    return out


def tile_of(geo, rect, Rr, tr, zk):
    """dsi_tile of one (unit, plane) -> (outcome, (tx0, ty0, tw, th)): "tile"; "lam": a corner with lam <= 0; "far": a
    corner mapped beyond 1e6 or not finite; "off": the box misses the image; "large": more than kDsiTilePx pixels.  The
    corners go through M2 and M3 in their written order, one rounding per operation, and are tested in the kernel's order."""
    fx, fy, cx, cy = [np.float64(v) for v in geo["cam"]]
    w, h = geo["w"], geo["h"]
    rx, ry, rw, rh = rect
    zk = np.float64(zk)
    us, vs = [], []
    with np.errstate(all="ignore"):
        for c in range(4):
            x = np.float64(rx + (rw - 1 if c & 1 else 0))
            y = np.float64(ry + (rh - 1 if c >> 1 else 0))
            a = (x - cx) / fx
            b = (y - cy) / fy
            d0 = (Rr[0, 0] * a + Rr[0, 1] * b) + Rr[0, 2]
            d1 = (Rr[1, 0] * a + Rr[1, 1] * b) + Rr[1, 2]
            d2 = (Rr[2, 0] * a + Rr[2, 1] * b) + Rr[2, 2]
            lam = (zk - tr[2]) / d2
            if not lam > 0.0:
                return "lam", (0, 0, 0, 0)
            X = tr[0] + lam * d0
            Y = tr[1] + lam * d1
            u = fx * (X / zk) + cx
            v = fy * (Y / zk) + cy
            if not (u > -1e6 and u < 1e6 and v > -1e6 and v < 1e6):
                return "far", (0, 0, 0, 0)
            us.append(u)
            vs.append(v)
    x0, x1 = max(int(math.floor(min(us))) - TILE_MARGIN, 0), min(int(math.floor(max(us))) + 1 + TILE_MARGIN, w - 1)
    y0, y1 = max(int(math.floor(min(vs))) - TILE_MARGIN, 0), min(int(math.floor(max(vs))) + 1 + TILE_MARGIN, h - 1)
    if x1 < x0 or y1 < y0:
        return "off", (0, 0, 0, 0)
    if (x1 - x0 + 1) * (y1 - y0 + 1) > TILE_PX:
        return "large", (0, 0, 0, 0)
    return "tile", (x0, y0, x1 - x0 + 1, y1 - y0 + 1)


def tile_census(geo, nz, pose_names, planes=None):
    """Over (unit, plane, pose): outcome -> count, the poses seen per outcome, and "mixed": the rounds of four consecutive
    planes of a workgroup (that walks `planes` planes from a multiple of it; None: all nz) in which a tile and a non-tile
    outcome meet."""
    z = planes_table(nz)
    planes = nz if planes is None else planes
    count = {o: 0 for o in OUTCOMES}
    poses = {o: set() for o in OUTCOMES}
    mixed = 0
    for pname in pose_names:
        Rr, tr = relative_pose(REF_POSE, SHAPE_POSE_TABLE[pname])
        for rect in rects(geo):
            got = [tile_of(geo, rect, Rr, tr, zk)[0] for zk in z]
            for o in got:
                count[o] += 1
                poses[o].add(pname)
            for k0 in range(0, nz, planes):
                k1 = min(k0 + planes, nz)
                for kr in range(k0, k1, WAVES):
                    kinds = {o == "tile" for o in got[kr:min(kr + WAVES, k1)]}
                    mixed += len(kinds) == 2
    return dict(count=count, poses=poses, mixed=mixed)


def planes_table(nz):
    return planes(nz, *Z_RANGE)


def planes_per_group(n_cus, pairs, nz):
    """csrc/ebo_depth.cpp's planes_per_group of the shipped build"""
    want = 4 * (n_cus if n_cus > 0 else 256)
    chunks = min(nz, max(1, (want + pairs - 1) // max(pairs, 1)))
    return (nz + chunks - 1) // chunks


def shape_windows(gname):
    """Six windows of a sensor, one for each of SHAPE_POSES: case_windows and 2000 more spread events"""
    key = "shape_" + gname
    if key not in _WINDOWS:
        _WINDOWS[key] = case_windows(gname) + [random_window(8, 2000, GEOS[gname]["w"], GEOS[gname]["h"], strays=30)]
    return _WINDOWS[key]


def scan_windows(gname):
    """Six windows of 20 000 uniform events of a SCAN_GEOS sensor, one for each of SCAN_POSES, less the events from
    column hole_x on within 24 rows of the middle row (fewer than 256 pixels a row, so every workgroup keeps some): under SCAN_POSES' few pixels of motion no ray reaches the middle of
    that region, so whole waves of k_dsi_count's workgroups keep nothing there."""
    key = "scan_" + gname
    if key not in _WINDOWS:
        w, h = SCAN_GEOS[gname]["w"], SCAN_GEOS[gname]["h"]
        wins = [random_window(300 + i, 20000, w, h) for i in range(len(SCAN_POSES))]
        _WINDOWS[key] = [ev[~((ev["x"] >= SCAN_GEOS[gname]["hole_x"]) & (np.abs(ev["y"] - h // 2) <= 24))] for ev in wins]
    return _WINDOWS[key]


def block_census(index):
    """Of k_dsi_count's workgroups of 256 consecutive pixels: (kept pixels per block, kept pixels in each block's last
    wave, the exclusive offsets)"""
    kept = (np.asarray(index).reshape(-1) >= 0).astype(np.int64)
    nb = (len(kept) + BLOCK - 1) // BLOCK
    pad = np.concatenate([kept, np.zeros(nb * BLOCK - len(kept), dtype=np.int64)]).reshape(nb, BLOCK)
    per = pad.sum(axis=1)
    return per, pad[:, BLOCK - 64:].sum(axis=1), np.concatenate([[0], np.cumsum(per)[:-1]])
