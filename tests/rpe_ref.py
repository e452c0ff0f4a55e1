"""numpy restatement of the relative-pose-error rules of include/ebo.h (T1-T7): float64, one rounding per operation in
the association written there, every sum in R6's tree (relpose_ref.tree64), the extrema over the same tree
(align_ref._tree_extreme).  `rpe` is the restatement; `tum_rpe` is an independent statement of the same quantities (4 x 4
homogeneous matrices, numpy.linalg.inv, numpy.arctan2), the yardstick's own error bar and not a rule.  The scenes and
batches of the CPU and GPU tests live here so that both test what the other measured."""
import numpy as np

import align_ref as A

DBL_MAX = A.DBL_MAX
PI = np.float64(np.pi)
HALVINGS = 2
TERMS = 13
MAX_DELTAS = 16
FIELDS = ("trans_rmse", "trans_mean", "trans_min", "trans_max", "rot_rmse", "rot_mean", "rot_min", "rot_max")


def _dot3(a, b):
    return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]


def angle(sn, cs):
    """T5, entry by entry: the angle in [0, pi] with sine : cosine = sn : cs, from + - * / sqrt alone."""
    sn = np.asarray(sn, np.float64)
    cs = np.asarray(cs, np.float64)
    with np.errstate(all="ignore"):
        h = np.sqrt(sn * sn + cs * cs)
        u = sn / (h + np.abs(cs))
        for _ in range(HALVINGS):
            u = u / (1.0 + np.sqrt(1.0 + u * u))
        z = u * u
        p = np.full(z.shape, np.float64(1.0) / np.float64(2 * (TERMS - 1) + 1))
        for k in range(TERMS - 2, -1, -1):
            p = p * z + np.float64(-1.0 if k % 2 else 1.0) / np.float64(2 * k + 1)
        phi = 8.0 * (u * p)
        theta = np.where(cs >= 0.0, phi, PI - phi)
        return np.where(h > 0.0, theta, 0.0)


def sine_cosine(E):
    """T4: E (m, 3, 3) -> (sn, cs)."""
    v = [0.5 * (E[:, 2, 1] - E[:, 1, 2]), 0.5 * (E[:, 0, 2] - E[:, 2, 0]), 0.5 * (E[:, 1, 0] - E[:, 0, 1])]
    return np.sqrt(_dot3(v, v)), (((E[:, 0, 0] + E[:, 1, 1]) + E[:, 2, 2]) - 1.0) / 2.0


def _rel_rot(Xi, Xj):
    """M[r][c] = dot(column r of Xi, column c of Xj), for stacks (m, 3, 4)."""
    M = np.empty((len(Xi), 3, 3))
    for r in range(3):
        for c in range(3):
            M[:, r, c] = _dot3([Xi[:, 0, r], Xi[:, 1, r], Xi[:, 2, r]], [Xj[:, 0, c], Xj[:, 1, c], Xj[:, 2, c]])
    return M


def _none(status, count):
    out = {f: np.float64(0.0) for f in FIELDS}
    out.update(count=int(count), status=int(status))
    return out


def pair_errors(gt, est, delta, scale=1.0):
    """T2-T5 of every pair of one segment: -> (q, e, theta), each (n - delta,)."""
    s = np.float64(scale)
    Qi, Qj, Pi, Pj = gt[:-delta], gt[delta:], est[:-delta], est[delta:]
    with np.errstate(all="ignore"):
        dp = [Pj[:, k, 3] - Pi[:, k, 3] for k in range(3)]
        dg = [Qj[:, k, 3] - Qi[:, k, 3] for k in range(3)]
        r = []
        for k in range(3):
            a = s * _dot3([Pi[:, 0, k], Pi[:, 1, k], Pi[:, 2, k]], dp)
            b = _dot3([Qi[:, 0, k], Qi[:, 1, k], Qi[:, 2, k]], dg)
            r.append(a - b)
        q = _dot3(r, r)
        e = np.sqrt(q)
        Am, Bm = _rel_rot(Pi, Pj), _rel_rot(Qi, Qj)
        E = np.empty_like(Am)
        for a in range(3):
            for c in range(3):
                E[:, a, c] = _dot3([Bm[:, 0, a], Bm[:, 1, a], Bm[:, 2, a]], [Am[:, 0, c], Am[:, 1, c], Am[:, 2, c]])
        sn, cs = sine_cosine(E)
        return q, e, angle(sn, cs)


def rpe(gt, est, delta, scale=1.0):
    """One unit: gt, est (n, 3, 4) the segment's poses -> dict(FIELDS.., count, status)."""
    gt = np.asarray(gt, np.float64).reshape(-1, 3, 4)
    est = np.asarray(est, np.float64).reshape(-1, 3, 4)
    n, delta = len(gt), int(delta)
    assert len(est) == n and delta >= 1
    if n <= delta:                                                        # T1
        return _none(1, 0)
    pairs = n - delta
    if not (np.isfinite(gt).all() and np.isfinite(est).all() and np.isfinite(scale)):
        return _none(2, pairs)
    q, e, th = pair_errors(gt, est, delta, scale)
    with np.errstate(all="ignore"):
        nd = np.float64(pairs)                                            # T6
        out = dict(trans_rmse=np.sqrt(A._tree(q) / nd), trans_mean=A._tree(e) / nd,
                   trans_min=A._tree_extreme(e, DBL_MAX, True), trans_max=A._tree_extreme(e, 0.0, False),
                   rot_rmse=np.sqrt(A._tree(th * th) / nd), rot_mean=A._tree(th) / nd,
                   rot_min=A._tree_extreme(th, DBL_MAX, True), rot_max=A._tree_extreme(th, 0.0, False),
                   count=pairs, status=0)
    return {k: (v if k in ("count", "status") else np.float64(v)) for k, v in out.items()}


def rpe_units(gt, est, segments, deltas, scales=None):
    """Every (segment, delta) of a call, segment-major, as Context.trajectory_rpe returns them."""
    gt = np.asarray(gt, np.float64).reshape(-1, 3, 4)
    est = np.asarray(est, np.float64).reshape(-1, 3, 4)
    out = []
    for g, (b, e) in enumerate(segments):
        for d in deltas:
            r = rpe(gt[b:e], est[b:e], d, 1.0 if scales is None else scales[g])
            r.update(segment=g, delta=int(d))
            out.append(r)
    return out


def tum_rpe(gt, est, delta, scale=1.0):
    """The TUM benchmark's relative pose error with homogeneous matrices: err = (Q_i^-1 Q_j)^-1 (P_i^-1 P_j) with the
    estimate's translations scaled; -> (|trans(err)|, angle(rot(err)) by arctan2), each (n - delta,)."""
    def hom(X, s):
        H = np.tile(np.eye(4), (len(X), 1, 1))
        H[:, :3, :3] = X[:, :, :3]
        H[:, :3, 3] = s * X[:, :, 3]
        return H
    Q, P = hom(np.asarray(gt, np.float64), 1.0), hom(np.asarray(est, np.float64), float(scale))
    et, er = [], []
    for i in range(len(Q) - delta):
        err = np.linalg.inv(np.linalg.inv(Q[i]) @ Q[i + delta]) @ (np.linalg.inv(P[i]) @ P[i + delta])
        et.append(np.linalg.norm(err[:3, 3]))
        R = err[:3, :3]
        v = 0.5 * np.array([R[2, 1] - R[1, 2], R[0, 2] - R[2, 0], R[1, 0] - R[0, 1]])
        er.append(np.arctan2(np.linalg.norm(v), 0.5 * (np.trace(R) - 1.0)))
    return np.array(et), np.array(er)


# ---- scenes -------------------------------------------------------------------------------------------------------
def rot(axis, a):
    """Rodrigues' rotation by `a` radians about `axis`."""
    k = np.asarray(axis, np.float64)
    k = k / np.linalg.norm(k)
    K = np.array([[0.0, -k[2], k[1]], [k[2], 0.0, -k[0]], [-k[1], k[0], 0.0]])
    return np.eye(3) + np.sin(a) * K + (1.0 - np.cos(a)) * (K @ K)


def poses(Rs, ts):
    return np.concatenate([np.asarray(Rs, np.float64), np.asarray(ts, np.float64)[:, :, None]], axis=2)


def helix(n, seed, noise=0.0, offset=0.0, span=3.0):
    """A ground-truth helix whose camera turns as it goes, and an estimate of it: every pose off by a rotation of about
    `noise` radians and a shift of about `noise`.  `offset` moves both away from the origin.  -> (gt, est) (n, 3, 4)."""
    rng = np.random.default_rng([seed, n])
    a = np.linspace(0.0, span, n)
    c = np.stack([np.cos(a), np.sin(a), 0.2 * a], axis=1) + offset * np.array([1.0, -1.0, 1.0])
    G = np.array([rot((0.0, 0.0, 1.0), x) @ rot((1.0, 0.2, 0.0), 0.4 * x) for x in a])
    gt = poses(G, c)
    if not noise:
        return gt, gt.copy()
    w = rng.normal(0, 1, (n, 3))
    R = np.array([G[i] @ rot(w[i], noise * np.linalg.norm(w[i])) for i in range(n)])
    return gt, poses(R, c + rng.normal(0, noise, (n, 3)))


def moved(gt, s, R0, t0):
    """gt moved by one similarity from the left: [R0 G_i | s R0 g_i + t0]."""
    return poses(np.einsum("ab,nbc->nac", R0, gt[:, :, :3]), s * (gt[:, :, 3] @ R0.T) + t0)


def tum_scenes():
    """The seeded trajectories of the comparison with tum_rpe: -> list of (n, noise, offset, gt, est, scale)."""
    out = []
    for k, n in enumerate((3, 4, 9, 33, 64, 65, 130, 200)):
        for noise in (0.0, 1e-3, 0.3):
            for offset in (0.0, 1e4):
                gt, est = helix(n, 200 + k, noise, offset)
                out.append((n, noise, offset, gt, est, 1.0 if noise == 0.0 else 1.0 + noise))
    return out


ANGLES = (0.0, 1e-9, np.pi / 2, np.pi - 1e-9, np.pi)


def angle_pairs():
    """Five two-pose segments whose relative rotation is exactly 0, 1e-9, pi / 2, pi - 1e-9 and exactly pi (the ground
    truth does not turn): -> (gt, est, segments)."""
    rng = np.random.default_rng(31)
    second = [np.eye(3), rot((0.0, 0.0, 1.0), 1e-9), np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]]),
              rot((0.0, 0.0, 1.0), np.pi - 1e-9), np.diag([1.0, -1.0, -1.0])]
    Rs, segs = [], []
    for k, X in enumerate(second):
        Rs += [np.eye(3), X]
        segs.append((2 * k, 2 * k + 2))
    c = rng.normal(0, 1, (10, 3))
    return poses([np.eye(3)] * 10, c), poses(Rs, c + rng.normal(0, 0.01, (10, 3))), segs


def gpu_cases():
    """name -> (gt, est, segments, deltas, scales or None): the shapes at which the kernel can go wrong, each small."""
    c = {}
    gt, est = helix(130, 7, 1e-3)
    c["pairs"] = (gt, est, [(0, p + 1) for p in (1, 63, 64, 65, 128, 129)], [1], None)    # the lane stride's tails
    gt, est = helix(20, 8, 1e-2)
    c["deltas"] = (gt, est, [(0, 20), (3, 20)], [1, 2, 7, 19, 20, 23], None)              # n - 1: one pair; n, n + 3: none
    c["angles"] = angle_pairs() + ([1], None)
    gt, est = helix(40, 9, 1e-2)
    c["scale"] = (gt, est, [(0, 40), (5, 30), (0, 40)], [1, 3], [1.7, 0.25, 1.0])
    gt, est = helix(70, 10, 1e-3, offset=1e4)
    c["offset"] = (gt, est, [(0, 70)], [1, 7], None)
    gt, est = helix(12, 11, 1e-2)
    bad = est.copy()
    bad[5, 1, 2] = np.nan                                                                 # a rotation entry of the estimate
    c["nan_rot"] = (gt, bad, [(0, 12), (5, 6), (0, 5), (6, 12)], [1, 2], None)            # inside, alone; just outside, twice
    bad = gt.copy()
    bad[6, 0, 3] = np.inf                                                                 # a translation entry of the ground truth
    c["inf_trans"] = (bad, est, [(0, 12), (6, 12), (0, 6), (7, 12)], [1, 4], None)
    c["bad_scale"] = (gt, est, [(0, 12), (0, 12), (0, 12), (4, 5)], [1, 11], [np.nan, np.inf, 2.0, -np.inf])
    return c


BATCH_DELTAS = (1, 2, 7, 19, 64)


def batch70():
    """14 segments x 5 deltas over one pair of arrays, mixing the cases of gpu_cases: -> (gt, est, segments, deltas,
    scales)."""
    take = {"pairs": [4, 5], "angles": [0, 1, 2, 3, 4], "nan_rot": [0, 2], "inf_trans": [1], "offset": [0], "scale": [0]}
    gts, ests, segs, scales, at = [], [], [], [], 0
    for name, (gt, est, ss, _, sc) in gpu_cases().items():
        if name in take:
            gts.append(gt)
            ests.append(est)
            for k in take[name]:
                segs.append((at + ss[k][0], at + ss[k][1]))
                scales.append(1.0 if sc is None else sc[k])
            at += len(gt)
    gt, est = np.concatenate(gts), np.concatenate(ests)
    segs += [(100, 215), (60, 132)]                          # overlapping, across the cases' borders
    scales += [0.5, np.inf]
    assert len(segs) * len(BATCH_DELTAS) == 70 and segs[-2][1] <= at
    return gt, est, segs, list(BATCH_DELTAS), scales


# ---- files of tools/rpe_serial.cpp -----------------------------------------------------------------------------------
def write_problem(path, gt, est, segments, deltas, scales=None):
    gt = np.asarray(gt, np.float64).reshape(-1, 12)
    est = np.asarray(est, np.float64).reshape(-1, 12)
    seg = np.asarray(segments, np.float64).reshape(-1, 2)
    parts = [[len(gt), len(seg), len(deltas), 0.0 if scales is None else 1.0], seg[:, 0], seg[:, 1]]
    if scales is not None:
        parts.append(np.asarray(scales, np.float64))
    parts += [np.asarray(deltas, np.float64), gt.ravel(), est.ravel()]
    np.concatenate(parts).astype(np.float64).tofile(path)


def read_result(path, n_units):
    v = np.fromfile(path, np.float64).reshape(n_units, 10)
    out = []
    for r in v:
        d = {f: np.float64(r[k]) for k, f in enumerate(FIELDS)}
        d.update(count=int(r[8]), status=int(r[9]))
        out.append(d)
    return out


same_bits = A.same_bits


def same_result(a, b):
    return a["status"] == b["status"] and a["count"] == b["count"] and all(same_bits(a[f], b[f]) for f in FIELDS)
