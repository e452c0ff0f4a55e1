"""numpy restatement of the absolute-pose rules A1-A5 of include/ebo.h ("absolute pose"): the yardstick of the
absolute-pose tests.

Float64 throughout; numpy's + - * / sqrt on float64 arrays are correctly rounded and never fused, so an expression
written with its parentheses is rounded once per operation in exactly that association.  Everything is batched: a
leading axis runs over hypotheses (or points), a dropped candidate is a False in a mask and its lanes compute on
with whatever they hold.  A pose is (R, t) as a [3][4] array taking camera coordinates to world coordinates.  The
shared rules (dot, cross, mix / hash, rotation, jacobi) are those of twoview_ref.py."""
import math

import numpy as np

import twoview_ref as tv
from twoview_ref import _cols, _cross, _dot3, _f64, _model_parts

NEWTON_STEPS = 32
POLISH_STEPS = 3
JACOBI_SWEEPS = 8
PROBABILITY = 0.99
MAX_ITERATIONS = 1000
REPROJECTION_ERROR = 2.0


def localize_threshold(reprojection_error=REPROJECTION_ERROR):
    """visual_odometry.cpp:232-233: the reference's float, widened."""
    return float(np.float32(1.0 - math.cos(math.atan2(reprojection_error, 200.0))))


THRESHOLD = localize_threshold()
_INF = np.float64(np.inf)
_ONE = np.float64(1.0)
_TWO = np.float64(2.0)
_THREE = np.float64(3.0)
_FOUR = np.float64(4.0)


# ---- A1 -----------------------------------------------------------------------------------------------------------
def _score(R, t, f, p):
    d = [p[i] - t[i] for i in range(3)]
    q = [((R[0][j] * d[0]) + (R[1][j] * d[1])) + (R[2][j] * d[2]) for j in range(3)]
    n = np.sqrt(_dot3(q, q))
    r = [q[i] / n for i in range(3)]
    return _ONE - _dot3(f, r)


def scores(pose, f, p):
    """pose [3][4], f p [n][3] -> [n] scores.  pose [B][3][4] -> [B][n]."""
    pose = _f64(pose)
    f = _f64(f).reshape(-1, 3)
    p = _f64(p).reshape(-1, 3)
    if pose.ndim == 3:
        pose = pose[:, None, :, :]
    R, t = _model_parts(pose)
    with np.errstate(all="ignore"):
        return _score(R, t, _cols(f), _cols(p)) + np.zeros(len(f))


def inliers(score, threshold=THRESHOLD):
    """A NaN score is not an inlier."""
    with np.errstate(all="ignore"):
        return score < threshold


# ---- A2 -----------------------------------------------------------------------------------------------------------
def samples(seed, frame, hyps, n):
    """4 distinct indices of 0 .. n-1 per hypothesis: the first 4 steps of rule 3's shuffle.  -> int32 [len(hyps)][4]."""
    hyps = np.asarray(hyps, dtype=np.int64).reshape(-1)
    B = len(hyps)
    assert n >= 4
    pos = np.full((B, 4), -1, dtype=np.int64)
    val = np.zeros((B, 4), dtype=np.int64)
    out = np.zeros((B, 4), dtype=np.int32)

    def get(x, upto):
        v = x.copy()
        for e in range(upto):       # later records override earlier ones
            v = np.where(pos[:, e] == x, val[:, e], v)
        return v

    for d in range(4):
        r = tv.draw_hash(seed, frame, hyps, d)
        j = d + ((r >> np.uint64(32)) % np.uint64(n - d)).astype(np.int64)
        vj = get(j, d)
        vd = get(np.full(B, d, dtype=np.int64), d)
        out[:, d] = vj
        pos[:, d] = j
        val[:, d] = vd
    return out


# ---- A3 -----------------------------------------------------------------------------------------------------------
def _cof(M):
    """Cofactors with cyclic indices: C[i][j] = M[i+1][j+1] * M[i+2][j+2] - M[i+1][j+2] * M[i+2][j+1]; det = dot(M[0], C[0])."""
    C = [[None] * 3 for _ in range(3)]
    for i in range(3):
        i1, i2 = (i + 1) % 3, (i + 2) % 3
        for j in range(3):
            j1, j2 = (j + 1) % 3, (j + 2) % 3
            C[i][j] = (M[i1][j1] * M[i2][j2]) - (M[i1][j2] * M[i2][j1])
    return C, _dot3(M[0], C[0])


def _rows_dot(A, B):
    return (_dot3(A[0], B[0]) + _dot3(A[1], B[1])) + _dot3(A[2], B[2])


def _cubic(r, b, c, d):
    return ((((r + b) * r) + c) * r) + d


def cubic_root(b, c, d, steps=NEWTON_STEPS):
    """One real root of x^3 + b x^2 + c x + d by `steps` Newton steps from the start A3 states."""
    q = (b * b) - (_THREE * c)
    v = np.sqrt(q)
    nb = -b
    t1 = (nb - v) / _THREE
    k1 = _cubic(t1, b, c, d)
    t2 = (nb + v) / _THREE
    k2 = _cubic(t2, b, c, d)
    rl = t1 - np.sqrt(k1 / v)
    rr = t2 + np.sqrt(np.abs(k2) / v)
    ri = nb / _THREE
    r = np.where(q > 0.0, np.where(k1 > 0.0, rl, rr), ri)
    for _ in range(steps):
        fx = _cubic(r, b, c, d)
        fp = ((((_THREE * r) + (_TWO * b)) * r) + c)
        r = np.where(fp != 0.0, r - (fx / fp), r)
    return r


def solve_samples(fs, ps, newton_steps=NEWTON_STEPS, polish_steps=POLISH_STEPS, all_candidates=False):
    """A3 + A4 for B samples: fs ps [B][4][3] (three points to solve, the fourth to choose) -> (poses [B][3][4],
    valid [B]).  all_candidates=True: -> list of four (pose [B][3][4], kept [B]) in A3's order instead."""
    fs = _f64(fs)
    ps = _f64(ps)
    B = len(fs)
    f = [[fs[:, i, k] for k in range(3)] for i in range(4)]
    p = [[ps[:, i, k] for k in range(3)] for i in range(4)]
    zero = np.zeros(B)
    cands = []
    with np.errstate(all="ignore"):
        b12, b13, b23 = _dot3(f[0], f[1]), _dot3(f[0], f[2]), _dot3(f[1], f[2])
        d12 = [p[0][k] - p[1][k] for k in range(3)]
        d13 = [p[0][k] - p[2][k] for k in range(3)]
        d23 = [p[1][k] - p[2][k] for k in range(3)]
        a12, a13, a23 = _dot3(d12, d12), _dot3(d13, d13), _dot3(d23, d23)
        ww = _cross(d12, d13)
        ok = _dot3(ww, ww) > 0.0
        for i in range(4):
            ok = ok & (_dot3(f[i], f[i]) > 0.0)
        m12 = -(b12 * a23)
        m13 = -(b13 * a23)
        x1 = b23 * a12
        x2 = b23 * a13
        D1 = [[a23 + zero, m12, zero], [m12, a23 - a12, x1], [zero, x1, -a12]]
        D2 = [[a23 + zero, zero, m13], [zero, -a13, x2], [m13, x2, a23 - a13]]
        C1, c0 = _cof(D1)
        C2, c3 = _cof(D2)
        c1 = _rows_dot(C1, D2)
        c2 = _rows_dot(C2, D1)
        ok &= c3 != 0.0
        g = cubic_root(c2 / c3, c1 / c3, c0 / c3, newton_steps)
        D0 = np.zeros((B, 3, 3))
        for i in range(3):
            for j in range(3):
                D0[:, i, j] = D1[i][j] + (g * D2[i][j])
        e, V = tv.jacobi(D0, JACOBI_SWEEPS)
        # drop the eigenvalue of smallest magnitude, the first of equals
        ae = np.abs(e)
        m = np.zeros(B, dtype=np.int64)
        am = ae[:, 0].copy()
        for j in (1, 2):
            take = ae[:, j] < am
            am = np.where(take, ae[:, j], am)
            m = np.where(take, j, m)
        ea = np.where(m == 0, e[:, 1], e[:, 0])
        eb = np.where(m == 2, e[:, 1], e[:, 2])
        va = [np.where(m == 0, V[:, k, 1], V[:, k, 0]) for k in range(3)]
        vb = [np.where(m == 2, V[:, k, 1], V[:, k, 2]) for k in range(3)]
        ok &= ((ea > 0.0) & (eb < 0.0)) | ((ea < 0.0) & (eb > 0.0))
        s = np.sqrt((-eb) / ea)
        Bw = [[d12[r], d13[r], ww[r]] for r in range(3)]
        tb12, tb13, tb23 = _TWO * b12, _TWO * b13, _TWO * b23
        for sg in (s, -s):
            n = [va[k] - (sg * vb[k]) for k in range(3)]
            okp = ok & (n[0] != 0.0)
            w0 = (-n[1]) / n[0]
            w1 = (-n[2]) / n[0]
            qa = (a23 * (w1 * w1)) - a12
            qb = (a23 * (((_TWO * w0) * w1) - (tb12 * w1))) + ((_TWO * a12) * b23)
            qc = (a23 * (((w0 * w0) + _ONE) - (tb12 * w0))) - a12
            okp &= qa != 0.0
            disc = (qb * qb) - ((_FOUR * qa) * qc)
            okp &= disc >= 0.0
            sq = np.sqrt(disc)
            nqb = -qb
            ta = _TWO * qa
            for num in (nqb + sq, nqb - sq):
                tau = num / ta
                okc = okp & (tau > 0.0)
                den = (_ONE + (tau * tau)) - (tb23 * tau)
                okc &= den > 0.0
                l2 = np.sqrt(a23 / den)
                l3 = tau * l2
                l1 = (w0 * l2) + (w1 * l3)
                okc &= l1 > 0.0
                L = [l1, l2, l3]
                for _ in range(polish_steps):
                    r0 = (((L[0] * L[0]) + (L[1] * L[1])) - ((tb12 * L[0]) * L[1])) - a12
                    r1 = (((L[0] * L[0]) + (L[2] * L[2])) - ((tb13 * L[0]) * L[2])) - a13
                    r2 = (((L[1] * L[1]) + (L[2] * L[2])) - ((tb23 * L[1]) * L[2])) - a23
                    J = [[(_TWO * L[0]) - (tb12 * L[1]), (_TWO * L[1]) - (tb12 * L[0]), zero],
                         [(_TWO * L[0]) - (tb13 * L[2]), zero, (_TWO * L[2]) - (tb13 * L[0])],
                         [zero, (_TWO * L[1]) - (tb23 * L[2]), (_TWO * L[2]) - (tb23 * L[1])]]
                    Cj, dj = _cof(J)
                    rr = [r0, r1, r2]
                    go = dj != 0.0
                    L = [np.where(go, L[i] - (_dot3([Cj[0][i], Cj[1][i], Cj[2][i]], rr) / dj), L[i]) for i in range(3)]
                X = [[L[i] * f[i][k] for k in range(3)] for i in range(3)]
                u = [X[0][k] - X[1][k] for k in range(3)]
                v = [X[0][k] - X[2][k] for k in range(3)]
                w = _cross(u, v)
                Bc = [[u[r], v[r], w[r]] for r in range(3)]
                Cc, dc = _cof(Bc)
                okc &= dc != 0.0
                inv = [[Cc[j][i] / dc for j in range(3)] for i in range(3)]
                pose = np.zeros((B, 3, 4))
                R = [[None] * 3 for _ in range(3)]
                for i in range(3):
                    for j in range(3):
                        R[i][j] = _dot3(Bw[i], [inv[0][j], inv[1][j], inv[2][j]])
                        pose[:, i, j] = R[i][j]
                t = [p[0][i] - _dot3(R[i], X[0]) for i in range(3)]
                for i in range(3):
                    pose[:, i, 3] = t[i]
                cands.append((pose, okc, R, t))
        if all_candidates:
            return [(c[0], c[1]) for c in cands]
        # A4: the first candidate with the smallest score of the fourth point
        best = np.full(B, _INF)
        model = np.zeros((B, 3, 4))
        valid = np.zeros(B, dtype=bool)
        for pose, okc, R, t in cands:
            sc = _score(R, t, f[3], p[3])
            sc = np.where(np.abs(sc) < _INF, sc, _INF)
            take = okc & (sc < best)
            best = np.where(take, sc, best)
            valid |= take
            model = np.where(take[:, None, None], pose, model)
    model[~valid] = 0.0
    return model, valid


def solve_samples_lapack(fs, ps):
    """The same three-point problem by another road, sharing no code with A3: the quartic in u = s2 / s1 (the
    resultant of the two ratio equations) through np.roots, the distances from it, and the rigid motion by the SVD of the 3 x 3 cross-covariance (Arun /
    Kabsch).  The fourth point chooses as in A4.  -> (poses [B][3][4], valid [B])."""
    fs = _f64(fs)
    ps = _f64(ps)
    B = len(fs)
    out = np.zeros((B, 3, 4))
    valid = np.zeros(B, dtype=bool)
    for h in range(B):
        f, p = fs[h], ps[h]
        if not (np.isfinite(f).all() and np.isfinite(p).all()):
            continue
        d12, d13, d23 = p[0] - p[1], p[0] - p[2], p[1] - p[2]
        a12, a13, a23 = float(d12 @ d12), float(d13 @ d13), float(d23 @ d23)
        if min(a12, a13, a23) == 0.0:
            continue
        cg, cb, ca = float(f[0] @ f[1]), float(f[0] @ f[2]), float(f[1] @ f[2])
        # with u = s2 / s1, v = s3 / s1:  P(v) = a12 v^2 + p1 v + p0(u) = 0 and Q(v) = a12 v^2 + q1(u) v + q0(u) = 0;
        # their difference is linear in v, and putting it back into P leaves a quartic in u
        K = np.poly1d([1.0, -2.0 * cg, 1.0])
        p1 = np.poly1d([-2.0 * a12 * cb])
        p0 = np.poly1d([a12]) - K * a13
        q1 = np.poly1d([-2.0 * a12 * ca, 0.0])
        q0 = np.poly1d([a12, 0.0, 0.0]) - K * a23
        dl, dc = p1 - q1, p0 - q0
        quartic = dc * dc * a12 - p1 * dc * dl + p0 * dl * dl
        co = quartic.coeffs
        if not np.isfinite(co).all() or len(co) < 2:
            continue
        best = np.inf
        for u in np.roots(co):
            if abs(u.imag) > 1e-7 * max(1.0, abs(u.real)) or u.real <= 0:
                continue
            u = u.real
            den = dl(u)
            if den == 0.0:
                continue
            v = -dc(u) / den
            if not v > 0:
                continue
            s1sq = a12 / K(u)
            if not s1sq > 0:
                continue
            s1 = math.sqrt(s1sq)
            a, b, c = math.sqrt(a23), math.sqrt(a13), math.sqrt(a12)
            L = np.array([s1, u * s1, v * s1])
            for _ in range(5):     # the same polish the LAPACK way: Newton on the three distance equations
                r = np.array([L[0] ** 2 + L[1] ** 2 - 2 * cg * L[0] * L[1] - c * c,
                              L[0] ** 2 + L[2] ** 2 - 2 * cb * L[0] * L[2] - b * b,
                              L[1] ** 2 + L[2] ** 2 - 2 * ca * L[1] * L[2] - a * a])
                J = np.array([[2 * L[0] - 2 * cg * L[1], 2 * L[1] - 2 * cg * L[0], 0],
                              [2 * L[0] - 2 * cb * L[2], 0, 2 * L[2] - 2 * cb * L[0]],
                              [0, 2 * L[1] - 2 * ca * L[2], 2 * L[2] - 2 * ca * L[1]]])
                try:
                    L = L - np.linalg.solve(J, r)
                except np.linalg.LinAlgError:
                    break
            if not (np.isfinite(L).all() and (L > 0).all()):
                continue
            X = L[:, None] * f[:3]
            mc, mw = X.mean(axis=0), p[:3].mean(axis=0)
            Hm = (X - mc).T @ (p[:3] - mw)
            U, _, Vt = np.linalg.svd(Hm)
            Dg = np.diag([1.0, 1.0, np.sign(np.linalg.det(Vt.T @ U.T)) or 1.0])
            R = Vt.T @ Dg @ U.T
            t = mw - R @ mc
            q = R.T @ (p[3] - t)
            nq = np.linalg.norm(q)
            if not nq > 0:
                continue
            sc = 1.0 - f[3] @ (q / nq)
            if np.isfinite(sc) and sc < best:
                best = sc
                out[h, :, :3] = R
                out[h, :, 3] = t
                valid[h] = True
    return out, valid


# ---- A5 -----------------------------------------------------------------------------------------------------------
def ransac_walk(counts, n, probability=PROBABILITY, max_iterations=MAX_ITERATIONS):
    """Rule 6 with w^4.  -> (found, winner, iterations, best)."""
    best, winner, k, h = -1, -1, float(max_iterations), 0
    for h in range(max_iterations):
        if int(counts[h]) > best:
            best = int(counts[h])
            winner = h
            w = best / n
            w2 = w * w
            w4 = w2 * w2
            x = min(max(1.0 - w4, 1e-15), 1.0 - 1e-15)
            k = math.log(1.0 - probability) / math.log(x)
        if h + 1 >= k or h + 1 == max_iterations:
            break
    return best >= 4, winner, h + 1, best


def ransac(f, p, seed=0, frame=0, threshold=THRESHOLD, probability=PROBABILITY, max_iterations=MAX_ITERATIONS):
    """A2-A5 for one frame.  -> dict(found, model, winner, iterations, n_inliers, inliers, counts, models, valid,
    samples, scores [H][n])."""
    f = _f64(f).reshape(-1, 3)
    p = _f64(p).reshape(-1, 3)
    n, H = len(f), int(max_iterations)
    out = dict(found=False, model=np.zeros((3, 4)), winner=-1, iterations=0, n_inliers=0,
               inliers=np.zeros(0, dtype=np.int32), counts=np.zeros(H, dtype=np.int32), models=np.zeros((H, 3, 4)),
               valid=np.zeros(H, dtype=bool), samples=np.zeros((H, 4), dtype=np.int32), scores=np.zeros((H, n)))
    if n < 4:
        return out
    smp = samples(seed, frame, np.arange(H), n)
    models, valid = solve_samples(f[smp], p[smp])
    sc = scores(models, f, p)
    inl = inliers(sc, threshold) & valid[:, None]
    counts = inl.sum(axis=1).astype(np.int32)
    found, winner, iterations, best = ransac_walk(counts, n, probability, H)
    out.update(found=found, winner=winner, iterations=iterations, n_inliers=best, counts=counts, models=models,
               valid=valid, samples=smp, scores=sc, model=models[winner].copy(),
               inliers=np.flatnonzero(inl[winner]).astype(np.int32))
    return out


# ---- test scenes --------------------------------------------------------------------------------------------------
def make_scene(seed, n=200, outliers=0.3, noise_px=0.3, angle=0.4, dist=1.0):
    """n landmarks at depth 1-8 in front of a DAVIS240C camera (camera_ref.DAVIS, distortion included) at a known pose
    (rotation up to `angle` rad, translation up to `dist`); the corners are the projections plus Gaussian pixel noise,
    the bearings their unprojection; a share of the corners is replaced by uniform random pixels.
    -> dict(f [n][3] unit, points [n][3] world, pose [3][4] camera-to-world, is_outlier [n], corners [n][2])."""
    import camera_ref
    rng = np.random.default_rng(seed)
    pose = tv.random_motions(int(rng.integers(1 << 30)), 1, angle=angle, dist=dist)[0]
    uv = np.stack([rng.uniform(20.0, 220.0, n), rng.uniform(20.0, 160.0, n)], axis=1)
    z = rng.uniform(1.0, 8.0, n)
    Xc = camera_ref.unproject(camera_ref.DAVIS, uv)
    Xc = Xc / Xc[:, 2:3] * z[:, None]
    points = Xc @ pose[:, :3].T + pose[:, 3]
    corners = camera_ref.project(camera_ref.DAVIS, Xc) + rng.normal(size=(n, 2)) * noise_px
    n_out = int(round(outliers * n))
    is_out = np.zeros(n, dtype=bool)
    if n_out:
        idx = rng.choice(n, n_out, replace=False)
        is_out[idx] = True
        corners[idx] = np.stack([rng.uniform(20.0, 220.0, n_out), rng.uniform(20.0, 160.0, n_out)], axis=1)
    f = camera_ref.unproject(camera_ref.DAVIS, corners)
    if noise_px == 0.0:      # noise-free: the exact bearings, not the lens model's round trip (good to 1e-7 only)
        f[~is_out] = (Xc / np.linalg.norm(Xc, axis=1)[:, None])[~is_out]
    return dict(f=np.ascontiguousarray(f), points=np.ascontiguousarray(points), pose=pose, is_outlier=is_out,
                corners=corners)


# the scenes of the GPU tests: (scene seed, n, outlier share, noise in pixels)
SCENES = [(1, 200, 0.0, 0.3), (2, 200, 0.2, 0.3), (3, 200, 0.3, 0.3), (4, 40, 0.2, 0.3)]
RANSAC_SEED = 7
# the sizes of the score tests (wave and tile edges of the counting kernel's shape), scene seed = 100 + n
SCORE_SIZES = (1, 63, 64, 65, 1023, 1024, 1025, 2049, 10000)
# the frames of the batched call: sizes, with one of 3 points and one of exactly 4; scene seed = 200 + position
BATCH_SIZES = (200, 3, 75, 4, 130, 64)


def scene(i):
    s, n, o, px = SCENES[i]
    return make_scene(s, n, o, px)


def degenerate_samples():
    """Samples [B][4][3] that must give "no model": collinear landmarks, coincident landmarks, a zero bearing, a NaN
    bearing, a NaN landmark, all zeros.  Built on one good sample."""
    sc = make_scene(50, n=4, outliers=0.0, noise_px=0.0)
    f0, p0 = sc["f"], sc["points"]
    fs, ps = [], []

    def add(f, p):
        fs.append(f)
        ps.append(p)

    p = p0.copy()
    p[:3] = [[0.0, 0.0, 4.0], [1.0, 1.0, 5.0], [2.0, 2.0, 6.0]]
    add(f0, p)
    p = p0.copy()
    p[1] = p[0]
    add(f0, p)
    p = p0.copy()
    p[1] = p[2]
    add(f0, p)
    for k in range(3):
        f = f0.copy()
        f[k] = 0.0
        add(f, p0)
    for k in range(4):
        f = f0.copy()
        f[k, 1] = np.nan
        add(f, p0)
    p = p0.copy()
    p[2, 0] = np.nan
    add(f0, p)
    add(np.zeros((4, 3)), np.zeros((4, 3)))
    add(f0, p0)      # the good one, last: it has a model
    return np.array(fs), np.array(ps)


# ---- the front end's bookkeeping (visual_odometry/visual_odometry.h) ----------------------------------------------
FACADE_SEED = 31
FACADE_PATCH_EXTENT = 4
IDENTITY = np.hstack([np.eye(3), np.zeros((3, 1))])


def make_facade_scene(seed=FACADE_SEED, n=120, frames=6, noise_px=0.05):
    """The scene of tests/test_gpu_odometry_facade.py: n world points seen by `frames` keyframes along a smooth known
    trajectory (the first camera is the world frame; the camera moves sideways and forward and turns slowly).
    -> dict(points [n][3], poses [frames][3][4] camera-to-world, x [frames][n][3] the points in each camera's frame
    with the pixel noise put into them, visible [frames][n] bool: every frame misses some tracks, ten tracks first
    appear in frame 2 and eight are seen by frames 0 and 1 only, timestamps)."""
    rng = np.random.default_rng(seed)
    uv = np.stack([rng.uniform(40.0, 200.0, n), rng.uniform(40.0, 140.0, n)], axis=1)
    z = rng.uniform(2.0, 6.0, n)
    points = np.stack([(uv[:, 0] - 120.0) / 200.0 * z, (uv[:, 1] - 90.0) / 200.0 * z, z], axis=1)
    poses = np.zeros((frames, 3, 4))
    x = np.zeros((frames, n, 3))
    for k in range(frames):
        poses[k, :, :3] = tv.rotation_about([0.1, 1.0, 0.05], -0.012 * k)
        poses[k, :, 3] = [0.25 * k, 0.02 * k * k, 0.04 * k]
        xc = (points - poses[k, :, 3]) @ poses[k, :, :3]
        xc[:, :2] += rng.normal(size=(n, 2)) * (noise_px / 200.0) * xc[:, 2:3]
        x[k] = xc
    visible = rng.uniform(size=(frames, n)) > 0.08
    late = rng.choice(n, 10, replace=False)
    visible[:2, late] = False
    visible[2:4, late] = True
    early = rng.choice(np.setdiff1d(np.arange(n), late), 8, replace=False)
    visible[:2, early] = True
    visible[2:, early] = False
    return dict(points=points, poses=poses, x=np.ascontiguousarray(x), visible=visible,
                timestamps=[1000 + 50000 * k for k in range(frames)])


def facade_frames(fs):
    """What the driver builds from the scene: per keyframe (timestamp, {track id: corner}); track ids 3 i + 5, corners
    = camera_ref.project followed by the round trip through a patch rectangle of extent 4."""
    import camera_ref
    e = np.float64(FACADE_PATCH_EXTENT)
    out = []
    for k, t in enumerate(fs["timestamps"]):
        uv = (camera_ref.project(camera_ref.DAVIS, fs["x"][k]) - e) + e
        out.append((t, {3 * i + 5: uv[i] for i in range(len(uv)) if fs["visible"][k, i]}))
    return out


def _unit_translation(model):
    out = np.array(model, dtype=np.float64).reshape(3, 4).copy()
    t = out[:, 3]
    s = t[0] * t[0] + t[1] * t[1]
    s = s + t[2] * t[2]
    ln = np.sqrt(s)
    if not (ln > 0.0 and np.isfinite(ln)):
        return None
    out[:, 3] = t / ln
    return out


class FrontEndReplay:
    """visual_odometry::VisualOdometryFrontEnd statement by statement on the restatements of the device entries."""

    def __init__(self, threshold, num_of_inliers=55, num_of_active_frames=20, seed=0, ransac_min_inliers=15,
                 max_num_without_add=4, ransac_threshold=5e-5, refine=None):
        import camera_ref
        self.cam = camera_ref
        self.threshold = threshold
        self.num_of_inliers = num_of_inliers
        self.num_of_active_frames = num_of_active_frames
        self.seed = seed
        self.ransac_min_inliers = ransac_min_inliers
        self.max_num_without_add = max_num_without_add
        self.ransac_threshold = ransac_threshold
        self.refine = refine            # frame timestamp -> pose [3][4], or None
        self.active = {}                # timestamp -> dict(landmarks, pose)
        self.stored_frames = []
        self.landmarks = {}
        self.observations = {}
        self.stored_landmarks = []
        self.without_add = 0
        self.optimizer_calls = []
        self.log = []                   # per candidate: dict(added, pose, inliers, localize)

    def _unproject(self, corners):
        return self.cam.unproject(self.cam.DAVIS, np.array(corners, dtype=np.float64).reshape(-1, 2))

    def init_cameras(self, kf, match):
        start = self.active[max(self.active)]
        tracks = np.array(sorted(t for t in start["landmarks"] if t in kf["landmarks"]), dtype=np.int64)
        match["inliers"] = []
        if len(tracks) == 0:
            return False
        f1 = self._unproject([start["landmarks"][t] for t in tracks])
        f2 = self._unproject([kf["landmarks"][t] for t in tracks])
        run = tv.ransac(f1, f2, seed=self.seed, pair=0, threshold=self.ransac_threshold)
        if not run["found"] or run["n_inliers"] < self.ransac_min_inliers:
            return False
        tw2c = _unit_translation(run["model"])
        if tw2c is None:
            return False
        match["Tw2c"] = tw2c
        flags = tv.inliers(tv.scores(run["model"], f1, f2), self.ransac_threshold)
        match["inliers"] = [int(t) for t in tracks[flags]]
        if len(match["inliers"]) < self.num_of_inliers:
            return False
        kf["pose"] = tv.pose_mul(start["pose"], tw2c)
        return True

    def localize_camera(self, kf, match, timestamp):
        match["inliers"] = []
        tracks = np.array(sorted(t for t in kf["landmarks"] if t in self.landmarks), dtype=np.int64)
        f = self._unproject([kf["landmarks"][t] for t in tracks]) if len(tracks) else np.zeros((0, 3))
        p = np.array([self.landmarks[t] for t in tracks], dtype=np.float64).reshape(-1, 3)
        run = ransac(f, p, seed=self.seed, frame=0, threshold=self.threshold)
        info = dict(n=len(tracks), found=bool(run["found"]), winner=run["winner"], iterations=run["iterations"],
                    n_inliers=run["n_inliers"], model=run["model"], f=f, p=p, tracks=tracks)
        if not run["found"]:
            return info
        model = run["model"]
        if self.refine is not None:
            model = np.array(self.refine[timestamp], dtype=np.float64).reshape(3, 4)
        match["Tw2c"] = model.copy()
        flags = inliers(scores(model, f, p), self.threshold)
        match["inliers"] = [int(t) for t in tracks[flags]]
        return info

    def is_new_keyframe_needed(self, kf, match, timestamp):
        self.last_localize = None
        if not self.active:
            kf["pose"] = IDENTITY.copy()
            match["inliers"].extend(kf["landmarks"].keys())
            return True
        if len(self.active) == 1:
            return self.init_cameras(kf, match)
        self.last_localize = self.localize_camera(kf, match, timestamp)
        kf["pose"] = match["Tw2c"].copy()
        if len(match["inliers"]) > self.num_of_inliers:
            return True
        if self.init_cameras(kf, match):
            return True
        if self.max_num_without_add > self.without_add:
            match["Tw2c"] = self.active[max(self.active)]["pose"].copy()
            match["inliers"].extend(kf["landmarks"].keys())
            return True
        return True

    def add_new_landmarks(self, timestamp, match):
        fresh = []
        for t in match["inliers"]:
            seen = self.observations.setdefault(t, [])
            seen.append(timestamp)
            if len(seen) == 2:
                fresh.append((t, seen[0], seen[1]))
        if not fresh:
            return
        keys = sorted(self.active)
        poses = [self.active[k]["pose"] for k in keys]
        pairs = [[keys.index(a), keys.index(b)] for _, a, b in fresh]
        f1 = self._unproject([self.active[a]["landmarks"][t] for t, a, _ in fresh])
        f2 = self._unproject([self.active[b]["landmarks"][t] for t, _, b in fresh])
        pts = tv.triangulate(poses, pairs, f1, f2)
        for (t, _, _), x in zip(fresh, pts):
            self.landmarks[t] = x

    def delete_keyframe(self):
        if len(self.active) > self.num_of_active_frames:
            first = min(self.active)
            kf = self.active[first]
            self.stored_frames.append((first, kf["pose"]))
            for t in kf["landmarks"]:
                if t in self.observations and first in self.observations[t]:
                    self.observations[t].remove(first)
            for t in sorted(t for t, seen in self.observations.items() if len(seen) == 0):
                if t in self.landmarks:
                    self.stored_landmarks.append((t, self.landmarks.pop(t)))
                del self.observations[t]
            del self.active[first]

    def new_keyframe_candidate(self, timestamp, landmarks):
        kf = dict(landmarks=dict(landmarks), pose=IDENTITY.copy())
        match = dict(Tw2c=IDENTITY.copy(), inliers=[])
        if not self.is_new_keyframe_needed(kf, match, timestamp):
            self.without_add += 1
            self.log.append(dict(added=False, pose=kf["pose"], inliers=list(match["inliers"]), localize=self.last_localize))
            return False
        self.delete_keyframe()
        self.without_add = 0
        self.active[timestamp] = kf
        self.add_new_landmarks(timestamp, match)
        self.optimizer_calls.append(sorted(self.active))
        self.log.append(dict(added=True, pose=kf["pose"], inliers=list(match["inliers"]), localize=self.last_localize))
        return True


def refined_poses(fs, num_of_active_frames, num_of_inliers=55):
    """Given poses for the refinement test: the poses of the unrefined replay, each followed by a small motion."""
    rp = FrontEndReplay(localize_threshold(3.0), num_of_inliers=num_of_inliers, num_of_active_frames=num_of_active_frames,
                        seed=FACADE_SEED)
    for t, lm in facade_frames(fs):
        rp.new_keyframe_candidate(t, lm)
    nudge = np.zeros((3, 4))
    nudge[:, :3] = tv.rotation_about([0.0, 1.0, 0.0], 2e-4)
    nudge[:, 3] = [1e-3, 0.0, 0.0]
    return np.array([tv.pose_mul(entry["pose"], nudge) for entry in rp.log])
