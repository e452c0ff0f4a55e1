"""numpy restatement of the two-view rules of include/ebo.h ("two-view geometry"): the yardstick of the two-view tests.

Float64 throughout, ONE operation per statement, in the association the header writes out, so that every
intermediate is rounded exactly once (numpy's + - * / sqrt on float64 arrays are correctly rounded and never fused).
Everything is batched: a leading axis runs over hypotheses (or points) and every statement acts on whole arrays, so
that a statement is the same operation for every element.  A model is (R12, t12) as a [3][4] array taking camera-2
coordinates to camera-1 coordinates.  The sampler is integer arithmetic on uint64 (wrap-around intended)."""
import math

import numpy as np

JACOBI_SWEEPS_9 = 10
JACOBI_SWEEPS_3 = 8
THRESHOLD = 5e-5          # VisualOdometryParams::ransacThreshold
PROBABILITY = 0.99
MAX_ITERATIONS = 1000
GOLDEN = np.uint64(0x9E3779B97F4A7C15)
_M1 = np.uint64(0xBF58476D1CE4E5B9)
_M2 = np.uint64(0x94D049BB133111EB)


def _f64(a):
    return np.asarray(a, dtype=np.float64)


# ---- small closed forms ---------------------------------------------------------------------------------------
def _dot3(a, b):
    """(a0 * b0 + a1 * b1) + a2 * b2 on sequences of three arrays."""
    p0 = a[0] * b[0]
    p1 = a[1] * b[1]
    p2 = a[2] * b[2]
    s = p0 + p1
    return s + p2


def _cols(a):
    """[..., 3] -> three arrays."""
    return [a[..., 0], a[..., 1], a[..., 2]]


def _model_parts(model):
    """[..., 3, 4] -> R as 3 rows of 3 arrays, t as 3 arrays."""
    model = _f64(model)
    R = [[model[..., i, j] for j in range(3)] for i in range(3)]
    t = [model[..., i, 3] for i in range(3)]
    return R, t


def _triangulate2(R, t, f1, f2):
    """Rule 1 on component lists; returns the three components of p (camera-1 coordinates)."""
    g = [_dot3(R[i], f2) for i in range(3)]
    b0 = _dot3(t, f1)
    b1 = _dot3(t, g)
    a00 = _dot3(f1, f1)
    fg = _dot3(f1, g)
    a01 = -fg
    a10 = fg
    gg = _dot3(g, g)
    a11 = -gg
    m0 = a00 * a11
    m1 = a01 * a10
    det = m0 - m1
    n00 = a11 * b0
    n01 = a01 * b1
    n0 = n00 - n01
    n10 = a00 * b1
    n11 = a10 * b0
    n1 = n10 - n11
    l0 = n0 / det
    l1 = n1 / det
    p = []
    for i in range(3):
        x = l0 * f1[i]
        y = l1 * g[i]
        z = t[i] + y
        w = x + z
        p.append(w / np.float64(2.0))
    return p


def _score(R, t, f1, f2):
    """Rule 2 on component lists."""
    p = _triangulate2(R, t, f1, f2)
    n1 = np.sqrt(_dot3(p, p))
    r1 = [p[i] / n1 for i in range(3)]
    d = [p[i] - t[i] for i in range(3)]
    q = []
    for j in range(3):
        x0 = R[0][j] * d[0]
        x1 = R[1][j] * d[1]
        x2 = R[2][j] * d[2]
        s = x0 + x1
        q.append(s + x2)
    n2 = np.sqrt(_dot3(q, q))
    r2 = [q[i] / n2 for i in range(3)]
    c1 = _dot3(f1, r1)
    c2 = _dot3(f2, r2)
    s1 = np.float64(1.0) - c1
    s2 = np.float64(1.0) - c2
    return s1 + s2


def triangulate2(model, f1, f2):
    """model [3][4] (or [n][3][4]), f1 f2 [n][3] -> [n][3] points in camera-1 coordinates."""
    R, t = _model_parts(model)
    with np.errstate(all="ignore"):
        p = _triangulate2(R, t, _cols(_f64(f1).reshape(-1, 3)), _cols(_f64(f2).reshape(-1, 3)))
    return np.stack(np.broadcast_arrays(*p), axis=-1)


def scores(model, f1, f2):
    """model [3][4], f1 f2 [n][3] -> [n] scores.  model [B][3][4] -> [B][n]."""
    model = _f64(model)
    f1 = _f64(f1).reshape(-1, 3)
    f2 = _f64(f2).reshape(-1, 3)
    if model.ndim == 3:
        model = model[:, None, :, :]
    R, t = _model_parts(model)
    with np.errstate(all="ignore"):
        return _score(R, t, _cols(f1), _cols(f2)) + np.zeros(len(f1))


def inliers(score, threshold=THRESHOLD):
    """A NaN score is not an inlier."""
    with np.errstate(all="ignore"):
        return score < threshold


# ---- poses ----------------------------------------------------------------------------------------------------
def pose_inverse(T):
    """(R, t) -> (R^T, -(R^T t)); [..., 3, 4]."""
    R, t = _model_parts(T)
    out = np.zeros(np.broadcast(R[0][0]).shape + (3, 4))
    for i in range(3):
        for j in range(3):
            out[..., i, j] = R[j][i]
        out[..., i, 3] = -_dot3([R[0][i], R[1][i], R[2][i]], t)
    return out


def pose_mul(A, B):
    """(Ra, ta)(Rb, tb) = (Ra Rb, Ra tb + ta)."""
    Ra, ta = _model_parts(A)
    Rb, tb = _model_parts(B)
    shape = np.broadcast(Ra[0][0], Rb[0][0]).shape
    out = np.zeros(shape + (3, 4))
    for i in range(3):
        for j in range(3):
            out[..., i, j] = _dot3(Ra[i], [Rb[0][j], Rb[1][j], Rb[2][j]])
        out[..., i, 3] = _dot3(Ra[i], tb) + ta[i]
    return out


def pose_apply(T, p):
    """R p + t; T [..., 3, 4], p [..., 3]."""
    R, t = _model_parts(T)
    pc = _cols(_f64(p))
    return np.stack(np.broadcast_arrays(*[_dot3(R[i], pc) + t[i] for i in range(3)]), axis=-1)


def triangulate(poses, pose_pair, f1, f2):
    """ebo_triangulate: world points pose1 * triangulate2(pose1^-1 * pose2, f1, f2), one pose pair per point."""
    poses = _f64(poses).reshape(-1, 3, 4)
    pose_pair = np.asarray(pose_pair, dtype=np.int64).reshape(-1, 2)
    P1 = poses[pose_pair[:, 0]]
    P2 = poses[pose_pair[:, 1]]
    with np.errstate(all="ignore"):
        T12 = pose_mul(pose_inverse(P1), P2)
        p = triangulate2(T12, f1, f2)
        return pose_apply(P1, p)


def essential(model):
    """Rule 7: hat(t / |t|) * R, each entry a difference of two products."""
    R, t = _model_parts(model)
    with np.errstate(all="ignore"):
        n = np.sqrt(_dot3(t, t))
        tx, ty, tz = t[0] / n, t[1] / n, t[2] / n
        E = np.zeros(np.broadcast(R[0][0]).shape + (3, 3))
        for j in range(3):
            a = ty * R[2][j]
            b = tz * R[1][j]
            E[..., 0, j] = a - b
            a = tz * R[0][j]
            b = tx * R[2][j]
            E[..., 1, j] = a - b
            a = tx * R[1][j]
            b = ty * R[0][j]
            E[..., 2, j] = a - b
    return E


def epipolar_residual(model, f1, f2):
    """|f1^T E f2| per correspondence."""
    E = essential(model)
    f1c = _cols(_f64(f1).reshape(-1, 3))
    f2c = _cols(_f64(f2).reshape(-1, 3))
    with np.errstate(all="ignore"):
        w = [_dot3([E[i, 0], E[i, 1], E[i, 2]], f2c) for i in range(3)]
        return np.abs(_dot3(f1c, w))


# ---- rule 3: the sampler ----------------------------------------------------------------------------------------
def _mix(z):
    z = (z ^ (z >> np.uint64(30))) * _M1
    z = (z ^ (z >> np.uint64(27))) * _M2
    return z ^ (z >> np.uint64(31))


def draw_hash(seed, pair, h, d):
    """The 64-bit hash of (seed, pair, hypothesis, draw); h may be an array."""
    with np.errstate(over="ignore"):
        x = _mix(np.uint64(seed & 0xFFFFFFFFFFFFFFFF) + GOLDEN)
        x = _mix((x ^ np.uint64(pair)) + GOLDEN)
        x = _mix((x ^ np.asarray(h, dtype=np.uint64)) + GOLDEN)
        return _mix((x ^ np.uint64(d)) + GOLDEN)


def samples(seed, pair, hyps, n):
    """8 distinct indices of 0 .. n-1 for each hypothesis in `hyps`: the first 8 steps of a Fisher-Yates shuffle,
    draw d swapping position d with position d + (hash >> 32) mod (n - d).  -> int32 [len(hyps)][8]."""
    hyps = np.asarray(hyps, dtype=np.int64).reshape(-1)
    B = len(hyps)
    assert n >= 8
    pos = np.full((B, 8), -1, dtype=np.int64)   # positions whose content is no longer their own index
    val = np.zeros((B, 8), dtype=np.int64)
    out = np.zeros((B, 8), dtype=np.int32)

    def get(x, upto):
        v = x.copy()
        for e in range(upto):       # later records override earlier ones
            v = np.where(pos[:, e] == x, val[:, e], v)
        return v

    for d in range(8):
        r = draw_hash(seed, pair, hyps, d)
        j = d + ((r >> np.uint64(32)) % np.uint64(n - d)).astype(np.int64)
        vj = get(j, d)
        vd = get(np.full(B, d, dtype=np.int64), d)
        out[:, d] = vj
        pos[:, d] = j
        val[:, d] = vd
    return out


# ---- rule 4: Jacobi, eight-point ------------------------------------------------------------------------------------
def jacobi(M, sweeps):
    """Cyclic-by-row Jacobi on symmetric [B][n][n]: -> (diagonal [B][n], eigenvector columns [B][n][n])."""
    M = _f64(M).copy()
    B, n, _ = M.shape
    V = np.zeros_like(M)
    for i in range(n):
        V[:, i, i] = 1.0
    one = np.float64(1.0)
    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p in range(n - 1):
                for q in range(p + 1, n):
                    apq = M[:, p, q].copy()
                    app = M[:, p, p].copy()
                    aqq = M[:, q, q].copy()
                    act = apq != 0.0
                    d = aqq - app
                    two = np.float64(2.0) * apq
                    th = d / two
                    ath = np.abs(th)
                    th2 = th * th
                    th21 = th2 + one
                    rt = np.sqrt(th21)
                    den = ath + rt
                    sg = np.where(th < 0.0, -one, one)
                    t = sg / den
                    t2 = t * t
                    t21 = t2 + one
                    rc = np.sqrt(t21)
                    c = one / rc
                    s = t * c
                    tapq = t * apq
                    for X, sym in ((M, True), (V, False)):
                        xp = X[:, :, p].copy()
                        xq = X[:, :, q].copy()
                        a0 = c[:, None] * xp
                        a1 = s[:, None] * xq
                        np_ = a0 - a1
                        b0 = s[:, None] * xp
                        b1 = c[:, None] * xq
                        nq = b0 + b1
                        if sym:
                            np_[:, p] = app - tapq
                            np_[:, q] = 0.0
                            nq[:, q] = aqq + tapq
                            nq[:, p] = 0.0
                        np_ = np.where(act[:, None], np_, xp)
                        nq = np.where(act[:, None], nq, xq)
                        X[:, :, p] = np_
                        X[:, :, q] = nq
                        if sym:
                            X[:, p, :] = np_
                            X[:, q, :] = nq
    return np.stack([M[:, i, i] for i in range(n)], axis=1), V


def hestenes(A, sweeps):
    """One-sided (Hestenes) Jacobi on the columns of A [B][m][n], cyclic by row: -> (squared column norms [B][n],
    V [B][n][n]) with A V = the rotated columns; the squared norms are the eigenvalues of A^T A and the columns of V
    its eigenvectors, without ever forming A^T A (whose condition number is the square of A's)."""
    A = _f64(A).copy()
    B, m, n = A.shape
    V = np.zeros((B, n, n))
    for i in range(n):
        V[:, i, i] = 1.0
    one = np.float64(1.0)

    def coldot(p, q):
        acc = A[:, 0, p] * A[:, 0, q]
        for i in range(1, m):
            pr = A[:, i, p] * A[:, i, q]
            acc = acc + pr
        return acc

    with np.errstate(all="ignore"):
        for _ in range(sweeps):
            for p in range(n - 1):
                for q in range(p + 1, n):
                    app = coldot(p, p)
                    aqq = coldot(q, q)
                    apq = coldot(p, q)
                    act = apq != 0.0
                    d = aqq - app
                    two = np.float64(2.0) * apq
                    th = d / two
                    ath = np.abs(th)
                    th2 = th * th
                    th21 = th2 + one
                    rt = np.sqrt(th21)
                    den = ath + rt
                    sg = np.where(th < 0.0, -one, one)
                    t = sg / den
                    t2 = t * t
                    t21 = t2 + one
                    rc = np.sqrt(t21)
                    c = one / rc
                    s = t * c
                    for X in (A, V):
                        xp = X[:, :, p].copy()
                        xq = X[:, :, q].copy()
                        a0 = c[:, None] * xp
                        a1 = s[:, None] * xq
                        np_ = a0 - a1
                        b0 = s[:, None] * xp
                        b1 = c[:, None] * xq
                        nq = b0 + b1
                        X[:, :, p] = np.where(act[:, None], np_, xp)
                        X[:, :, q] = np.where(act[:, None], nq, xq)
        d = np.stack([coldot(j, j) for j in range(n)], axis=1)
    return d, V


def _cross(a, b):
    x0 = a[1] * b[2]
    x1 = a[2] * b[1]
    y0 = a[2] * b[0]
    y1 = a[0] * b[2]
    z0 = a[0] * b[1]
    z1 = a[1] * b[0]
    return [x0 - x1, y0 - y1, z0 - z1]


def _det3(R):
    a0 = R[1][1] * R[2][2]
    a1 = R[1][2] * R[2][1]
    a = a0 - a1
    b0 = R[1][0] * R[2][2]
    b1 = R[1][2] * R[2][0]
    b = b0 - b1
    c0 = R[1][0] * R[2][1]
    c1 = R[1][1] * R[2][0]
    c = c0 - c1
    x = R[0][0] * a
    y = R[0][1] * b
    z = R[0][2] * c
    w = x - y
    return w + z


def _candidates(u0, u1, u2, v0, v1, v2):
    """Rule 5: the four (R, t) in the fixed order (Ra,+) (Ra,-) (Rb,+) (Rb,-)."""
    Ra = [[None] * 3 for _ in range(3)]
    Rb = [[None] * 3 for _ in range(3)]
    for i in range(3):
        for j in range(3):
            a = u1[i] * v0[j]
            b = u0[i] * v1[j]
            c = u2[i] * v2[j]
            d = a - b
            Ra[i][j] = d + c
            e = b - a
            Rb[i][j] = e + c
    out = []
    for R in (Ra, Rb):
        neg = _det3(R) < 0.0
        R = [[np.where(neg, -R[i][j], R[i][j]) for j in range(3)] for i in range(3)]
        out.append((R, [u2[0], u2[1], u2[2]]))
        out.append((R, [-u2[0], -u2[1], -u2[2]]))
    return out


def _select(cands, f1s, f2s, B):
    """The first candidate with the smallest sum of the 8 sample scores (not finite = +inf); -> model, valid."""
    best = np.full(B, np.inf)
    model = np.zeros((B, 3, 4))
    valid = np.zeros(B, dtype=bool)
    for R, t in cands:
        tot = None
        for i in range(8):
            s = _score(R, t, [f1s[:, i, k] for k in range(3)], [f2s[:, i, k] for k in range(3)])
            tot = s if tot is None else tot + s
        tot = np.where(np.isfinite(tot), tot, np.inf)
        take = tot < best
        best = np.where(take, tot, best)
        valid |= take
        for i in range(3):
            for j in range(3):
                model[:, i, j] = np.where(take, R[i][j], model[:, i, j])
            model[:, i, 3] = np.where(take, t[i], model[:, i, 3])
    return model, valid


def _sample_matrix(f1s, f2s):
    """The 8 x 9 matrix whose row i is (f2x * f1, f2y * f1, f2z * f1)."""
    B = len(f1s)
    A = np.zeros((B, 8, 9))
    for a in range(3):
        for b in range(3):
            A[:, :, 3 * a + b] = f2s[:, :, a] * f1s[:, :, b]
    return A


def solve_samples(f1s, f2s):
    """Rules 4 and 5 for B samples: f1s f2s [B][8][3] -> (models [B][3][4], valid [B])."""
    f1s = _f64(f1s)
    f2s = _f64(f2s)
    B = len(f1s)
    with np.errstate(all="ignore"):
        A = _sample_matrix(f1s, f2s)
        d, V = hestenes(A, JACOBI_SWEEPS_9)
        jmin = np.zeros(B, dtype=np.int64)
        dmin = d[:, 0].copy()
        for j in range(1, 9):
            take = d[:, j] < dmin
            dmin = np.where(take, d[:, j], dmin)
            jmin = np.where(take, j, jmin)
        e = V[np.arange(B), :, jmin]                   # [B][9]
        F = [[e[:, 3 * a + b] for a in range(3)] for b in range(3)]   # F[b][a] = e[3a + b]
        G = np.zeros((B, 3, 3))
        for j in range(3):
            for k in range(3):
                G[:, j, k] = _dot3([F[0][j], F[1][j], F[2][j]], [F[0][k], F[1][k], F[2][k]])
        d3, V3 = jacobi(G, JACOBI_SWEEPS_3)
        dd = [d3[:, 0].copy(), d3[:, 1].copy(), d3[:, 2].copy()]
        vv = [[V3[:, k, c].copy() for k in range(3)] for c in range(3)]     # vv[c] = column c
        for a, b in ((0, 1), (1, 2), (0, 1)):          # stable descending: swap only when strictly smaller
            sw = dd[a] < dd[b]
            dd[a], dd[b] = np.where(sw, dd[b], dd[a]), np.where(sw, dd[a], dd[b])
            for k in range(3):
                vv[a][k], vv[b][k] = np.where(sw, vv[b][k], vv[a][k]), np.where(sw, vv[a][k], vv[b][k])
        s0 = np.sqrt(dd[0])
        s1 = np.sqrt(dd[1])
        ok = (s0 > 0.0) & (s1 > 0.0)
        v0, v1 = vv[0], vv[1]
        u0 = [_dot3(F[i], v0) / s0 for i in range(3)]
        n0 = np.sqrt(_dot3(u0, u0))
        u0 = [u0[i] / n0 for i in range(3)]
        u1 = [_dot3(F[i], v1) / s1 for i in range(3)]
        h = _dot3(u0, u1)
        u1 = [u1[i] - h * u0[i] for i in range(3)]
        n1 = np.sqrt(_dot3(u1, u1))
        u1 = [u1[i] / n1 for i in range(3)]
        u2 = _cross(u0, u1)
        v2 = _cross(v0, v1)
        model, valid = _select(_candidates(u0, u1, u2, v0, v1, v2), f1s, f2s, B)
    valid &= ok
    model[~valid] = 0.0
    return model, valid


def solve_samples_lapack(f1s, f2s):
    """The same samples solved with LAPACK (SVD of A, SVD of F): the yardstick's own error bar, not a rule."""
    f1s = _f64(f1s)
    f2s = _f64(f2s)
    B = len(f1s)
    with np.errstate(all="ignore"):
        A = _sample_matrix(f1s, f2s)
        e = np.linalg.svd(A)[2][:, 8, :]
        Fm = e.reshape(B, 3, 3).transpose(0, 2, 1)
        U, _, Vt = np.linalg.svd(Fm)
        u0 = [U[:, i, 0] for i in range(3)]
        u1 = [U[:, i, 1] for i in range(3)]
        v0 = [Vt[:, 0, i] for i in range(3)]
        v1 = [Vt[:, 1, i] for i in range(3)]
        u2 = _cross(u0, u1)
        v2 = _cross(v0, v1)
        return _select(_candidates(u0, u1, u2, v0, v1, v2), f1s, f2s, B)


# ---- rule 6: the serial walk ------------------------------------------------------------------------------------
def ransac_walk(counts, n, probability=PROBABILITY, max_iterations=MAX_ITERATIONS):
    """-> (found, winner, iterations, best)."""
    best, winner, k, h = -1, -1, float(max_iterations), 0
    for h in range(max_iterations):
        if int(counts[h]) > best:
            best = int(counts[h])
            winner = h
            w = best / n
            w2 = w * w
            w4 = w2 * w2
            w8 = w4 * w4
            x = min(max(1.0 - w8, 1e-15), 1.0 - 1e-15)
            k = math.log(1.0 - probability) / math.log(x)
        if h + 1 >= k or h + 1 == max_iterations:
            break
    return best >= 8, winner, h + 1, best


def ransac(f1, f2, seed=0, pair=0, threshold=THRESHOLD, probability=PROBABILITY, max_iterations=MAX_ITERATIONS):
    """Rules 3-6 for one pair.  -> dict(found, model, winner, iterations, n_inliers, inliers, counts, models, valid,
    samples, scores [H][n])."""
    f1 = _f64(f1).reshape(-1, 3)
    f2 = _f64(f2).reshape(-1, 3)
    n, H = len(f1), int(max_iterations)
    out = dict(found=False, model=np.zeros((3, 4)), winner=-1, iterations=0, n_inliers=0,
               inliers=np.zeros(0, dtype=np.int32), counts=np.zeros(H, dtype=np.int32), models=np.zeros((H, 3, 4)),
               valid=np.zeros(H, dtype=bool), samples=np.zeros((H, 8), dtype=np.int32), scores=np.zeros((H, n)))
    if n < 8:
        return out
    smp = samples(seed, pair, np.arange(H), n)
    models, valid = solve_samples(f1[smp], f2[smp])
    sc = scores(models, f1, f2)
    inl = inliers(sc, threshold) & valid[:, None]
    counts = inl.sum(axis=1).astype(np.int32)
    found, winner, iterations, best = ransac_walk(counts, n, probability, H)
    out.update(found=found, winner=winner, iterations=iterations, n_inliers=best, counts=counts, models=models,
               valid=valid, samples=smp, scores=sc, model=models[winner].copy(),
               inliers=np.flatnonzero(inl[winner]).astype(np.int32))
    return out


# ---- test scenes ------------------------------------------------------------------------------------------------
def rotation_about(axis, angle):
    axis = _f64(axis) / np.linalg.norm(axis)
    K = np.array([[0, -axis[2], axis[1]], [axis[2], 0, -axis[0]], [-axis[1], axis[0], 0]])
    return np.eye(3) + math.sin(angle) * K + (1 - math.cos(angle)) * (K @ K)


def random_motions(seed, count, angle=0.5, dist=1.0):
    """count rigid motions [count][3][4] with rotation angles up to `angle` and translations of length up to `dist`."""
    rng = np.random.default_rng(seed)
    out = np.zeros((count, 3, 4))
    for i in range(count):
        out[i, :, :3] = rotation_about(rng.normal(size=3), rng.uniform(-angle, angle))
        d = rng.normal(size=3)
        out[i, :, 3] = d / np.linalg.norm(d) * rng.uniform(0.05, dist)
    return out


def make_scene(seed, n=200, outliers=0.3, noise_px=0.3, angle=0.08, baseline=0.3):
    """n points at depth 2-8 seen through a 240 x 180, f = 200 pinhole by two cameras `angle` rad and `baseline`
    apart in a random direction; Gaussian pixel noise; a share of correspondences replaced by uniform random
    bearings.  -> dict(f1, f2 [n][3] unit, model [3][4] = (R12, t12), is_outlier [n], points [n][3] in camera 1)."""
    rng = np.random.default_rng(seed)
    f, cx, cy, w, h = 200.0, 120.0, 90.0, 240.0, 180.0
    R12 = rotation_about(rng.normal(size=3), angle)
    d = rng.normal(size=3)
    t12 = d / np.linalg.norm(d) * baseline
    # points visible in camera 1; camera 2 sees x2 = R12^T (x1 - t12)
    u1 = np.stack([rng.uniform(0, w, n), rng.uniform(0, h, n)], axis=1)
    z = rng.uniform(2.0, 8.0, n)
    X1 = np.stack([(u1[:, 0] - cx) / f * z, (u1[:, 1] - cy) / f * z, z], axis=1)
    X2 = (X1 - t12) @ R12
    u2 = np.stack([f * X2[:, 0] / X2[:, 2] + cx, f * X2[:, 1] / X2[:, 2] + cy], axis=1)
    u1n = u1 + rng.normal(size=(n, 2)) * noise_px
    u2n = u2 + rng.normal(size=(n, 2)) * noise_px

    def bearing(uv):
        b = np.stack([(uv[:, 0] - cx) / f, (uv[:, 1] - cy) / f, np.ones(len(uv))], axis=1)
        return b / np.linalg.norm(b, axis=1)[:, None]

    f1, f2 = bearing(u1n), bearing(u2n)
    n_out = int(round(outliers * n))
    is_out = np.zeros(n, dtype=bool)
    if n_out:
        idx = rng.choice(n, n_out, replace=False)
        is_out[idx] = True
        ru = np.stack([rng.uniform(0, w, n_out), rng.uniform(0, h, n_out)], axis=1)
        f2[idx] = bearing(ru)
    model = np.zeros((3, 4))
    model[:, :3] = R12
    model[:, 3] = t12
    return dict(f1=np.ascontiguousarray(f1), f2=np.ascontiguousarray(f2), model=model, is_outlier=is_out, points=X1)


# the five scenes of the GPU tests: (scene seed, n, outlier share, noise in pixels)
SCENES = [(1, 200, 0.3, 0.3), (2, 200, 0.3, 0.3), (3, 200, 0.3, 0.3), (4, 75, 0.2, 0.3), (5, 500, 0.4, 0.5)]
RANSAC_SEED = 7


def scene(i):
    s, n, o, px = SCENES[i]
    return make_scene(s, n, o, px)


# ---- the facade's end-to-end scene --------------------------------------------------------------------------------
FACADE_SEED = 21
FACADE_PATCH_EXTENT = 4


def make_facade_scene(seed=FACADE_SEED, n=200, outliers=0.3, noise_px=0.3):
    """The scene of tests/test_gpu_twoview_facade.py: the same n points in the frames of camera 1 (x1) and camera 2
    (x2), which the C++ driver projects through the DAVIS240C lens (camera_ref.DAVIS); the noise and the outliers
    are put into x2.  -> dict(x1, x2 [n][3], model [3][4] = (R12, t12), corners1, corners2 [n][2]: the pixels the
    keyframes hold, i.e. camera_ref.project followed by the round trip through a patch rectangle of extent 4)."""
    import camera_ref
    sc = make_scene(seed, n, outliers=0.0, noise_px=0.0)
    rng = np.random.default_rng(seed + 1000)
    R12, t12 = sc["model"][:, :3], sc["model"][:, 3]
    x1 = sc["points"].copy()
    x2 = (x1 - t12) @ R12
    x2[:, :2] += rng.normal(size=(n, 2)) * (noise_px / 200.0) * x2[:, 2:3]
    idx = rng.choice(n, int(round(outliers * n)), replace=False)
    z = rng.uniform(2.0, 8.0, len(idx))
    x2[idx] = np.stack([rng.uniform(-0.5, 0.5, len(idx)) * z, rng.uniform(-0.4, 0.4, len(idx)) * z, z], axis=1)
    e = np.float64(FACADE_PATCH_EXTENT)
    corners = []
    for x in (x1, x2):
        uv = camera_ref.project(camera_ref.DAVIS, x)
        low = uv - e           # Patch(corner, extent): the rectangle starts at corner - extent, 2 * extent + 1 wide
        corners.append(low + e)  # Patch::toCorner(): x + (width - 1) / 2
    is_out = np.zeros(n, dtype=bool)
    is_out[idx] = True
    return dict(x1=np.ascontiguousarray(x1), x2=np.ascontiguousarray(x2), model=sc["model"], corners1=corners[0],
                corners2=corners[1], is_outlier=is_out)


def facade_bearings(fs):
    import camera_ref
    return camera_ref.unproject(camera_ref.DAVIS, fs["corners1"]), camera_ref.unproject(camera_ref.DAVIS, fs["corners2"])
