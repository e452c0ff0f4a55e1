"""numpy restatement of the trajectory-alignment rules of include/ebo.h (S1-S7): float64, one rounding per operation in
the association written there, every sum in R6's tree (relpose_ref.tree64), jacobi and the descending order those of
twoview_ref.py.  `align` is the restatement; `lapack_align` is an independent statement of the same least-squares
problem (Umeyama's closed form with numpy.linalg.svd, the steps aligner.cpp takes), the yardstick's own error bar and
not a rule.  The scenes and batches of the CPU and GPU tests live here so that both test what the other measured."""
import numpy as np

import relpose_ref as RP
import twoview_ref as TV

LANES = 64
SWEEPS = 8
MIN_POINTS = 3
RANK2_FLOOR = 2.0 ** -46       # S4: d1 > d0 * 2^-46
DBL_MAX = np.finfo(np.float64).max


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def _cross(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]])


def _tree(v):
    return RP.tree64(np.asarray(v, np.float64).reshape(-1, 1))


def _tree_extreme(e, start, smaller):
    """S7's min / max: partial l starts at `start` and takes e[l], e[l + 64], .. when strictly smaller / larger; then
    partial[i] takes partial[i + s] likewise for s = 32 .. 1."""
    n = len(e)
    chunks = max((n + LANES - 1) // LANES, 1)
    pad = np.full(chunks * LANES, np.nan)          # a comparison with a NaN is false: a missing point changes nothing
    pad[:n] = e
    pad = pad.reshape(chunks, LANES)
    acc = np.full(LANES, start)
    with np.errstate(all="ignore"):
        for r in range(chunks):
            take = pad[r] < acc if smaller else pad[r] > acc
            acc = np.where(take, pad[r], acc)
        s = LANES // 2
        while s:
            a, b = acc[:s].copy(), acc[s:2 * s].copy()
            acc[:s] = np.where(b < a if smaller else b > a, b, a)
            s //= 2
    return acc[0]


def _not_aligned(status, n):
    return dict(scale=np.float64(1.0), R=np.eye(3), t=np.zeros(3), rmse=np.float64(0.0), mean=np.float64(0.0),
                min=np.float64(0.0), max=np.float64(0.0), count=int(n), status=int(status))


def align(data, model, fix_scale=False):
    """One segment: data, model (n, 3) -> dict(scale, R, t, rmse, mean, min, max, count, status)."""
    d = np.asarray(data, np.float64).reshape(-1, 3)
    m = np.asarray(model, np.float64).reshape(-1, 3)
    n = len(d)
    assert len(m) == n
    if n < MIN_POINTS:                                                    # S1
        return _not_aligned(1, n)
    if not (np.isfinite(d).all() and np.isfinite(m).all()):
        return _not_aligned(2, n)
    with np.errstate(all="ignore"):
        nd = np.float64(n)
        cd = np.array([_tree(d[:, a]) / nd for a in range(3)])            # S2
        cm = np.array([_tree(m[:, a]) / nd for a in range(3)])
        dc = d - cd                                                       # S3
        mc = m - cm
        W = np.array([[_tree(dc[:, a] * mc[:, b]) for b in range(3)] for a in range(3)])
        nm = _tree((mc[:, 0] * mc[:, 0] + mc[:, 1] * mc[:, 1]) + mc[:, 2] * mc[:, 2])
        G = np.array([[_dot3(W[:, j], W[:, k]) for k in range(3)] for j in range(3)])      # S4
        dd, V = TV.jacobi(G[None], SWEEPS)
        dd = [dd[0, c] for c in range(3)]
        vv = [V[0, :, c].copy() for c in range(3)]
        for a, b in ((0, 1), (1, 2), (0, 1)):
            if dd[a] < dd[b]:
                dd[a], dd[b] = dd[b], dd[a]
                vv[a], vv[b] = vv[b], vv[a]
        ok = dd[1] > 0.0 and np.isfinite(dd[1]) and dd[1] > dd[0] * RANK2_FLOOR and nm > 0.0 and np.isfinite(nm)
        v0, v1 = vv[0], vv[1]
        u0 = np.array([_dot3(W[i], v0) for i in range(3)])                # S5
        n0 = np.sqrt(_dot3(u0, u0))
        u0 = u0 / n0
        u1 = np.array([_dot3(W[i], v1) for i in range(3)])
        h = _dot3(u0, u1)
        u1 = u1 - h * u0
        n1 = np.sqrt(_dot3(u1, u1))
        u1 = u1 / n1
        ok = ok and n0 > 0.0 and np.isfinite(n0) and n1 > 0.0 and np.isfinite(n1)
        if not ok:
            return _not_aligned(3, n)
        u2 = _cross(u0, u1)
        v2 = _cross(v0, v1)
        R = np.array([[(u0[i] * v0[j] + u1[i] * v1[j]) + u2[i] * v2[j] for j in range(3)] for i in range(3)])
        s = np.float64(1.0)                                               # S6
        if not fix_scale:
            dots = np.float64(0.0)
            for a in range(3):
                for b in range(3):
                    dots = dots + R[a, b] * W[a, b]
            s = dots / nm
        t = np.array([cd[i] - s * _dot3(R[i], cm) for i in range(3)])
        r = np.stack([d[:, k] - (s * _dot3(R[k], [m[:, 0], m[:, 1], m[:, 2]]) + t[k]) for k in range(3)], axis=1)   # S7
        q = (r[:, 0] * r[:, 0] + r[:, 1] * r[:, 1]) + r[:, 2] * r[:, 2]
        e = np.sqrt(q)
        return dict(scale=s, R=R, t=t, rmse=np.sqrt(_tree(q) / nd), mean=_tree(e) / nd,
                    min=_tree_extreme(e, DBL_MAX, True), max=_tree_extreme(e, 0.0, False), count=n, status=0)


def align_segments(data, model, segments, fix_scale=False):
    data = np.asarray(data, np.float64).reshape(-1, 3)
    model = np.asarray(model, np.float64).reshape(-1, 3)
    return [align(data[b:e], model[b:e], fix_scale) for b, e in segments]


def lapack_align(data, model, fix_scale=False):
    """The least-squares similarity with data ~ s R model + t by an SVD of the cross-covariance (Umeyama 1991; Arun et
    al. 1987 for the rotation), LAPACK through numpy.  -> (s, R, t, errors per point)."""
    d = np.asarray(data, np.float64)
    m = np.asarray(model, np.float64)
    cd, cm = d.mean(axis=0), m.mean(axis=0)
    dc, mc = d - cd, m - cm
    W = dc.T @ mc
    U, _, Vt = np.linalg.svd(W)
    S = np.diag([1.0, 1.0, -1.0 if np.linalg.det(U) * np.linalg.det(Vt) < 0 else 1.0])
    R = U @ S @ Vt
    s = 1.0 if fix_scale else float((dc * (mc @ R.T)).sum() / (mc * mc).sum())
    t = cd - s * (R @ cm)
    err = np.linalg.norm(d - (s * (m @ R.T) + t), axis=1)
    return s, R, t, err


def top_two_ratio(data, model):
    d = np.asarray(data, np.float64)
    m = np.asarray(model, np.float64)
    sv = np.linalg.svd((d - d.mean(axis=0)).T @ (m - m.mean(axis=0)), compute_uv=False)
    return sv[0] / sv[1] if sv[1] > 0 else np.inf


# ---- scenes -------------------------------------------------------------------------------------------------------
def rotation(rng):
    q = rng.normal(0, 1, 4)
    q /= np.linalg.norm(q)
    w, x, y, z = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                     [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                     [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])


def scene(kind, seed, n, noise=0.0, mirror=False):
    """A cloud and its image under a known similarity.  kind: "generic" (extents 1 : 0.7 : 0.4), "planar" (z exactly
    0 in the model), "offset" (generic, 1e4 away from the origin in every coordinate).  The cloud is redrawn from the
    same seeded stream until the two largest singular values of W are within 10 : 1, so every scene returned is one the
    comparison with LAPACK covers.  -> dict(data, model, s, R, t, size)."""
    rng = np.random.default_rng([seed, n, {"generic": 0, "planar": 1, "offset": 2}[kind]])
    while True:
        m = rng.normal(0, 1, (n, 3)) * np.array([1.0, 0.7, 0.0 if kind == "planar" else 0.4])
        if kind == "offset":
            m = m + np.array([1e4, -1e4, 1e4])
        s = float(rng.uniform(0.5, 2.0))
        R = rotation(rng)
        t = rng.normal(0, 1, 3) * (1e4 if kind == "offset" else 1.0)
        src = m * np.array([-1.0, 1.0, 1.0]) if mirror else m
        d = s * (src @ R.T) + t + (rng.normal(0, noise, (n, 3)) if noise else 0.0)
        if top_two_ratio(d, m) <= 10.0:
            return dict(data=d, model=m, s=s, R=R, t=t, size=float(np.linalg.norm(d - d.mean(axis=0), axis=1).max()))


def lapack_scenes():
    """The seeded scenes of the comparison with LAPACK: three kinds x three noise levels x sizes 3 .. 80."""
    sizes = (3, 4, 5, 6, 7, 9, 12, 17, 24, 33, 47, 63, 64, 65, 80)
    out = []
    for kind in ("generic", "planar", "offset"):
        for noise in (0.0, 1e-3, 0.3):
            for k, n in enumerate(sizes):
                out.append((kind, noise, n, scene(kind, 100 + k, n, noise)))
    return out


def collinear(n, axis=(1.0, 2.0, -0.5)):
    i = np.arange(n, dtype=np.float64)[:, None]
    m = i * np.asarray(axis) + np.array([0.25, -1.0, 3.0])
    return dict(data=2.0 * m + 1.0, model=m)


def gpu_cases():
    """name -> (data, model, segments, fix_scale): the shapes at which the kernel can go wrong, each small."""
    c = {}
    for n in (3, 63, 64, 65, 128, 129):                      # the lane-stride tails
        sc = scene("generic", 7, n, 1e-3)
        c["n%d" % n] = (sc["data"], sc["model"], [(0, n)], False)
    sc = scene("generic", 8, 10, 0.0)
    c["short"] = (sc["data"], sc["model"], [(4, 4), (4, 5), (4, 6), (0, 0), (10, 10)], False)   # 0, 1, 2 points
    d = sc["data"].copy()
    d[5, 1] = np.nan
    c["nan"] = (d, sc["model"], [(0, 10), (0, 5), (6, 10), (5, 6)], False)   # inside; just outside, twice; alone
    m = sc["model"].copy()
    m[0, 2] = np.inf
    c["inf_model"] = (sc["data"], m, [(0, 10), (1, 10)], False)
    col = collinear(20)
    c["collinear"] = (col["data"], col["model"], [(0, 20), (3, 9)], False)
    c["coincident"] = (np.ones((5, 3)) * 2.0, np.ones((5, 3)) * 3.0, [(0, 5)], False)
    sc = scene("planar", 9, 40, 0.0)
    c["planar"] = (sc["data"], sc["model"], [(0, 40)], False)
    sc = scene("generic", 10, 33, 1e-3, mirror=True)
    c["mirrored"] = (sc["data"], sc["model"], [(0, 33)], False)
    sc = scene("offset", 11, 70, 1e-3)
    c["offset"] = (sc["data"], sc["model"], [(0, 70)], False)
    sc = scene("generic", 12, 50, 0.3)
    c["fix_scale"] = (sc["data"], sc["model"], [(0, 50)], True)
    return c


def batch70():
    """70 segments over one pair of arrays, mixing every case of gpu_cases: -> (data, model, segments)."""
    datas, models, segs, at = [], [], [], 0
    for name, (d, m, ss, fix) in gpu_cases().items():
        if fix:
            continue
        datas.append(d)
        models.append(m)
        segs += [(at + b, at + e) for b, e in ss]
        at += len(d)
    data, model = np.concatenate(datas), np.concatenate(models)
    rng = np.random.default_rng(70)
    while len(segs) < 70:                                    # overlapping segments, across the cases' borders too
        b = int(rng.integers(0, at - 3))
        segs.append((b, min(at, b + int(rng.integers(0, 140)))))
    return data, model, segs


def trajectory(K=40, seed=5, span=3.0):
    """A K-pose trajectory and its ground truth: a noisy, scaled, rotated helix of `span` radians.
    -> (gt centres, estimated centres)."""
    rng = np.random.default_rng(seed)
    a = np.linspace(0.0, span, K)
    est = np.stack([np.cos(a), np.sin(a), 0.2 * a], axis=1) + rng.normal(0, 0.01, (K, 3))
    gt = 1.7 * (np.stack([np.cos(a), np.sin(a), 0.2 * a], axis=1) @ rotation(rng).T) + np.array([3.0, -2.0, 0.5])
    return gt, est


# ---- files of tools/align_sim3_serial.cpp ----------------------------------------------------------------------------
def write_problem(path, data, model, segments, fix_scale):
    data = np.asarray(data, np.float64).reshape(-1, 3)
    model = np.asarray(model, np.float64).reshape(-1, 3)
    seg = np.asarray(segments, np.float64).reshape(-1, 2)
    np.concatenate([[len(data), len(seg), 1.0 if fix_scale else 0.0], seg[:, 0], seg[:, 1], data.ravel(),
                    model.ravel()]).astype(np.float64).tofile(path)


def read_result(path, n_segments):
    v = np.fromfile(path, np.float64).reshape(n_segments, 19)
    return [dict(scale=r[0], R=r[1:10].reshape(3, 3).copy(), t=r[10:13].copy(), rmse=r[13], mean=r[14], min=r[15],
                 max=r[16], count=int(r[17]), status=int(r[18])) for r in v]


def same_bits(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


def same_result(a, b):
    return (a["status"] == b["status"] and a["count"] == b["count"]
            and all(same_bits(a[k], b[k]) for k in ("scale", "R", "t", "rmse", "mean", "min", "max")))


# ---- syncGroundTruth's interpolation (visual_odometry/aligner.h): prev * exp(p * log(prev^-1 * next)) on SE3 ----------
def _hat(w):
    return np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])


def se3_log(T):
    """T (3, 4) -> (upsilon, omega): the unit quaternion of R, omega = 2 atan2(|v|, w) / |v| * v, upsilon = V^-1 t."""
    R, t = T[:, :3], T[:, 3]
    tr = R[0, 0] + R[1, 1] + R[2, 2]
    q = np.zeros(4)
    if tr > 0.0:
        s = 2.0 * np.sqrt(tr + 1.0)
        q[:] = (0.25 * s, (R[2, 1] - R[1, 2]) / s, (R[0, 2] - R[2, 0]) / s, (R[1, 0] - R[0, 1]) / s)
    else:
        i = int(np.argmax(np.diag(R)))
        j, k = (i + 1) % 3, (i + 2) % 3
        s = 2.0 * np.sqrt(R[i, i] - R[j, j] - R[k, k] + 1.0)
        q[1 + i], q[0] = 0.25 * s, (R[k, j] - R[j, k]) / s
        q[1 + j], q[1 + k] = (R[j, i] + R[i, j]) / s, (R[k, i] + R[i, k]) / s
        if q[0] < 0.0:
            q = -q
    n2 = q[1:] @ q[1:]
    n = np.sqrt(n2)
    k = 2.0 / q[0] - (2.0 / 3.0) * n2 / q[0] ** 3 if n < 1e-10 else 2.0 * np.arctan2(n, q[0]) / n
    omega, theta = k * q[1:], k * n
    c = 1.0 / 12.0 if abs(theta) < 1e-10 else (1.0 - theta * np.cos(0.5 * theta) / (2.0 * np.sin(0.5 * theta))) / (theta * theta)
    W = _hat(omega)
    return t - 0.5 * (W @ t) + c * (W @ (W @ t)), omega


def se3_exp(upsilon, omega):
    theta2 = omega @ omega
    theta = np.sqrt(theta2)
    small = theta < 1e-10
    imag = 0.5 - theta2 / 48.0 + theta2 * theta2 / 3840.0 if small else np.sin(0.5 * theta) / theta
    real = 1.0 - theta2 / 8.0 + theta2 * theta2 / 384.0 if small else np.cos(0.5 * theta)
    w, x, y, z = np.array([real, *(imag * omega)]) / np.sqrt(real * real + imag * imag * theta2)
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    W = _hat(omega)
    V = R if small else np.eye(3) + (1.0 - np.cos(theta)) / theta2 * W + (theta - np.sin(theta)) / (theta2 * theta) * (W @ W)
    return np.concatenate([R, (V @ upsilon)[:, None]], axis=1)


def _mul(A, B):
    return np.concatenate([A[:, :3] @ B[:, :3], (A[:, :3] @ B[:, 3] + A[:, 3])[:, None]], axis=1)


def _inv(A):
    return np.concatenate([A[:, :3].T, (-(A[:, :3].T @ A[:, 3]))[:, None]], axis=1)


def interpolate(prev, nxt, p):
    """Poses (3, 4); p in [0, 1]."""
    ups, om = se3_log(_mul(_inv(prev), nxt))
    return _mul(prev, se3_exp(p * ups, p * om))


def sync_fraction(t, t_prev, t_next):
    """The reference's p: a float quotient of the two durations, widened."""
    return float(np.float32(t - t_prev) / np.float32(t_next - t_prev))


def pose_of(rng, centre):
    return np.concatenate([rotation(rng), np.asarray(centre, np.float64)[:, None]], axis=1)
