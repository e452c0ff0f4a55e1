"""numpy restatement of the landmark-maintenance rules of include/ebo.h (L1-L7): float64, one rounding per operation in
the association written there.  dot, cof / det, the score A1, the hash and jacobi(M, sweeps) are the restatements the
two-view and absolute-pose sections already have (twoview_ref, abspose_ref).  `triangulate` and `audit` are the rules
for a whole call; `maintain` is the facade's policy on top of them.  The scenes and batches of the CPU and GPU tests
live here so that both test what the other measured."""
import math

import numpy as np

import abspose_ref as ap
import twoview_ref as tv
from twoview_ref import _dot3

PARTIALS = 16
SWEEPS = 8
THRESHOLD = ap.localize_threshold()
MIN_PARALLAX = 1.0 - math.cos(math.radians(1.0))
_ZERO = np.float64(0.0)
_ONE = np.float64(1.0)
_TWO = np.float64(2.0)


def default_params(**kw):
    p = dict(threshold=THRESHOLD, min_parallax=MIN_PARALLAX, min_inliers=2, max_hypotheses=300, seed=0)
    p.update(kw)
    return p


# ---- L1, L2, L3 ------------------------------------------------------------------------------------------------------
def rays(P, f):
    """L1 for one landmark: P (m, 3, 4) the poses of its observations, f (m, 3) -> d (m, 3), e (m, 3), c_ref (3)."""
    d = np.stack([_dot3([P[:, i, 0], P[:, i, 1], P[:, i, 2]], [f[:, 0], f[:, 1], f[:, 2]]) for i in range(3)], axis=1)
    cref = P[0, :, 3].copy()
    e = P[:, :, 3] - cref
    return d, e, cref


def terms(d, e):
    """L2's nine terms per observation: (.., 3), (.., 3) -> (.., 9) = M00 M01 M02 M11 M12 M22 b0 b1 b2."""
    d0, d1, d2 = d[..., 0], d[..., 1], d[..., 2]
    ev = [e[..., 0], e[..., 1], e[..., 2]]
    dd = _dot3([d0, d1, d2], [d0, d1, d2])
    a00 = dd - d0 * d0
    a11 = dd - d1 * d1
    a22 = dd - d2 * d2
    a01 = -(d0 * d1)
    a02 = -(d0 * d2)
    a12 = -(d1 * d2)
    return np.stack([a00, a01, a02, a11, a12, a22, _dot3([a00, a01, a02], ev), _dot3([a01, a11, a12], ev),
                     _dot3([a02, a12, a22], ev)], axis=-1)


def _fold(part):
    """(.., 16, 9) -> (.., 9): partial[i] += partial[i + s] for s = 8, 4, 2, 1."""
    s = PARTIALS // 2
    while s > 0:
        part[..., :s, :] = part[..., :s, :] + part[..., s:2 * s, :]
        s //= 2
    return part[..., 0, :].copy()


def tree_sums(T, member):
    """L2's sums over the observations o with member[o]: T (m, 9) -> (9)."""
    part = np.zeros((PARTIALS, 9))
    for o in range(len(T)):
        if member[o]:
            part[o % PARTIALS] = part[o % PARTIALS] + T[o]
    return _fold(part)


def pair_sums(T, a, b):
    """L2's sums over the sets {a[h], b[h]}, the rule taken literally: (H, 9)."""
    H = len(a)
    lo, hi = np.minimum(a, b), np.maximum(a, b)
    idx = np.arange(H)
    part = np.zeros((H, PARTIALS, 9))
    part[idx, lo % PARTIALS] = part[idx, lo % PARTIALS] + T[lo]
    part[idx, hi % PARTIALS] = part[idx, hi % PARTIALS] + T[hi]
    return _fold(part)


def _matrix(S):
    return [[S[..., 0], S[..., 1], S[..., 2]], [S[..., 1], S[..., 3], S[..., 4]], [S[..., 2], S[..., 4], S[..., 5]]]


def solve(S, cref):
    """L2: sums (.., 9) -> X (.., 3), has_point (..)."""
    with np.errstate(all="ignore"):
        C, D = ap._cof(_matrix(S))
        b = [S[..., 6], S[..., 7], S[..., 8]]
        X = np.stack([cref[i] + _dot3([C[0][i], C[1][i], C[2][i]], b) / D for i in range(3)], axis=-1)
        return X, D > 0.0


def parallax(S, count):
    """L3: sums (B, 9) (only M is read), count (B) -> (B)."""
    S = np.asarray(S, np.float64).reshape(-1, 9)
    M = np.empty((len(S), 3, 3))
    rows = _matrix(S)
    for i in range(3):
        for j in range(3):
            M[:, i, j] = rows[i][j]
    lam, _ = tv.jacobi(M, SWEEPS)
    with np.errstate(all="ignore"):
        lo = lam[:, 0].copy()
        lo = np.where(lam[:, 1] < lo, lam[:, 1], lo)
        lo = np.where(lam[:, 2] < lo, lam[:, 2], lo)
        return (_TWO * lo) / np.asarray(count, np.float64)


def scores_under(P, f, X):
    """A1 of every observation of a landmark under the points X (.., 3): (.., m)."""
    X = np.asarray(X, np.float64)
    R = [[P[:, i, j] for j in range(3)] for i in range(3)]
    t = [P[:, i, 3] for i in range(3)]
    p = [X[..., i, None] for i in range(3)]
    with np.errstate(all="ignore"):
        return ap._score(R, t, [f[:, 0], f[:, 1], f[:, 2]], p) + np.zeros(len(f))


# ---- L4 --------------------------------------------------------------------------------------------------------------
def hypotheses(m, max_hypotheses, seed):
    """-> a (H), b (H): the pairs of L4."""
    n_pairs = m * (m - 1) // 2
    if n_pairs <= max_hypotheses:
        a, b = np.triu_indices(m, 1)   # lexicographic
        return a.astype(np.int64), b.astype(np.int64)
    h = np.arange(max_hypotheses, dtype=np.int64)
    j0 = ((tv.draw_hash(seed, 0, h, 0) >> np.uint64(32)) % np.uint64(m)).astype(np.int64)
    j1 = 1 + ((tv.draw_hash(seed, 0, h, 1) >> np.uint64(32)) % np.uint64(m - 1)).astype(np.int64)
    # Fisher-Yates: after the first draw position j0 holds 0
    return j0, np.where(j1 == j0, 0, j1)


def _empty(m, status, **kw):
    r = dict(point=np.zeros(3), parallax=_ZERO, score_max=_ZERO, status=status, n_obs=m, n_inliers=0, winner=-1, hypotheses=0,
             scores=np.zeros(m), flags=np.zeros(m, np.uint8))
    r.update(kw)
    return r


def _finite_max(sc):
    fin = sc[np.isfinite(sc)]
    return np.float64(fin.max()) if len(fin) else _ZERO


def _scan_bad(poses, k, f, point=None):
    if np.any(k < 0) or np.any(k >= len(poses)):
        return True
    if not (np.all(np.isfinite(poses[k])) and np.all(np.isfinite(f))):
        return True
    return point is not None and not np.all(np.isfinite(point))


def triangulate_one(poses, k, f, prm):
    """L1-L6 for one landmark: k (m) pose indices, f (m, 3)."""
    m = len(k)
    if _scan_bad(poses, k, f):
        return _empty(m, 2)
    if m < 2:
        return _empty(m, 1)
    thr, minpar = np.float64(prm["threshold"]), np.float64(prm["min_parallax"])
    P = poses[k]
    d, e, cref = rays(P, f)
    T = terms(d, e)
    a, b = hypotheses(m, prm["max_hypotheses"], prm["seed"])
    H = len(a)
    with np.errstate(all="ignore"):
        da, db = [d[a, i] for i in range(3)], [d[b, i] for i in range(3)]
        g = _dot3(da, db)
        n2 = _dot3(da, da) * _dot3(db, db)
        valid = (n2 > 0.0) & (_ONE - g / np.sqrt(n2) >= minpar)
        Xh, has = solve(pair_sums(T, a, b), cref)
        valid &= has
        counts = (scores_under(P, f, Xh) < thr).sum(axis=1)
    counts = np.where(valid, counts, -1)
    w = int(np.argmax(counts))     # the first of the largest
    if counts[w] < 2:
        return _empty(m, 3, hypotheses=H)
    with np.errstate(all="ignore"):
        U = scores_under(P, f, Xh[w]) < thr
    S = tree_sums(T, U)
    X, has = solve(S, cref)
    par = parallax(S, float(counts[w]))[0]
    if not (bool(has) and par >= minpar):
        return _empty(m, 4, hypotheses=H, winner=w, parallax=par)
    sc = scores_under(P, f, X)
    with np.errstate(all="ignore"):
        fl = sc < thr
    n_in = int(fl.sum())
    r = dict(point=X, parallax=par, score_max=_finite_max(sc), status=0, n_obs=m, n_inliers=n_in, winner=w, hypotheses=H, scores=sc,
             flags=fl.astype(np.uint8))
    if n_in < prm["min_inliers"]:
        r.update(status=5, point=np.zeros(3))
    return r


def audit_one(poses, k, f, X, prm):
    """L7 for one landmark."""
    m = len(k)
    X = np.asarray(X, np.float64)
    if _scan_bad(poses, k, f, X):
        return _empty(m, 2)
    if m < 1:
        return _empty(m, 1)
    thr, minpar = np.float64(prm["threshold"]), np.float64(prm["min_parallax"])
    P = poses[k]
    sc = scores_under(P, f, X)
    with np.errstate(all="ignore"):
        fl = sc < thr
    n_in = int(fl.sum())
    par = _ZERO
    if n_in > 0:
        d, e, _ = rays(P, f)
        par = parallax(tree_sums(terms(d, e), fl), float(n_in))[0]
    status = 4 if not par >= minpar else (5 if n_in < prm["min_inliers"] else 0)
    return dict(point=X.copy() if status == 0 else np.zeros(3), parallax=par, score_max=_finite_max(sc), status=status, n_obs=m,
                n_inliers=n_in, winner=-1, hypotheses=0, scores=sc, flags=fl.astype(np.uint8))


RESULT_DOUBLES = ("point", "parallax", "score_max")
RESULT_INTS = ("status", "n_obs", "n_inliers", "winner", "hypotheses")


def _gather(rs):
    out = {k: np.array([r[k] for r in rs]) for k in RESULT_DOUBLES + RESULT_INTS}
    out["point"] = out["point"].reshape(-1, 3)
    out["scores"] = np.concatenate([r["scores"] for r in rs]) if rs else np.zeros(0)
    out["flags"] = np.concatenate([r["flags"] for r in rs]) if rs else np.zeros(0, np.uint8)
    return out


def triangulate(poses, offsets, obs_pose, obs_f, prm):
    """ebo_triangulate_tracks: -> dict of arrays, one row per landmark, scores / flags per observation."""
    poses = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    obs_f = np.asarray(obs_f, np.float64).reshape(-1, 3)
    obs_pose = np.asarray(obs_pose, np.int64)
    return _gather([triangulate_one(poses, obs_pose[offsets[l]:offsets[l + 1]], obs_f[offsets[l]:offsets[l + 1]], prm)
                    for l in range(len(offsets) - 1)])


def audit(poses, offsets, obs_pose, obs_f, points, prm):
    """ebo_landmark_scores."""
    poses = np.asarray(poses, np.float64).reshape(-1, 3, 4)
    obs_f = np.asarray(obs_f, np.float64).reshape(-1, 3)
    obs_pose = np.asarray(obs_pose, np.int64)
    points = np.asarray(points, np.float64).reshape(-1, 3)
    return _gather([audit_one(poses, obs_pose[offsets[l]:offsets[l + 1]], obs_f[offsets[l]:offsets[l + 1]], points[l], prm)
                    for l in range(len(offsets) - 1)])


# ---- scenes ----------------------------------------------------------------------------------------------------------
FOCAL = 200.0
STEP = 0.3        # metres between keyframes
ROW = 24          # keyframes along the baseline before the next row starts, STEP above


def make_keyframes(rng, n, origin=(0.0, 0.0, 0.0), max_angle=0.03):
    """n camera-to-world poses: along the x axis STEP apart (a new row every ROW keyframes), looking down +z, each
    turned by up to max_angle rad about a random axis and jittered by a few centimetres."""
    P = np.zeros((n, 3, 4))
    for i in range(n):
        P[i, :, :3] = tv.rotation_about(rng.normal(size=3), rng.uniform(-max_angle, max_angle))
        P[i, :, 3] = np.asarray(origin) + [STEP * (i % ROW), STEP * (i // ROW), 0.0] + rng.normal(size=3) * 0.02
    return P


def observe(rng, P, X, noise_px=0.3, n_out=0, off_px=0.0):
    """Unit bearing vectors of the world point X in the cameras P (m, 3, 4) with Gaussian pixel noise at f = 200.  The
    LAST n_out observations are planted outliers, a track corrupted from one keyframe on: moved by off_px at right
    angles to the image of the baseline, with a random sign.  (An offset ALONG the epipolar line is a change of depth,
    which a view with a third of the baseline sees at a third of its size, 2 px of 6: such an observation is not an
    outlier to any consensus.  And two outliers of four observations tie with the two good ones at count 2, which only
    L4's "first of the largest" decides: so the corrupted observations are the track's last.)"""
    m = len(P)
    xc = np.einsum("kji,kj->ki", P[:, :, :3], X - P[:, :, 3])
    uv = FOCAL * xc[:, :2] / xc[:, 2:3] + rng.normal(size=(m, 2)) * noise_px
    planted = np.zeros(m, bool)
    if n_out:
        planted[m - n_out:] = True
        base = np.einsum("kji,j->ki", P[:, :, :3], np.array([1.0, 0.0, 0.0]))[:, :2]
        perp = np.stack([-base[:, 1], base[:, 0]], axis=1) / np.linalg.norm(base, axis=1, keepdims=True)
        sign = rng.choice([-1.0, 1.0], size=m)
        uv[planted] += (off_px * sign[:, None] * perp)[planted]
    f = np.concatenate([uv / FOCAL, np.ones((m, 1))], axis=1)
    return f / np.linalg.norm(f, axis=1, keepdims=True), planted


def world_point(rng, P, depth=(2.0, 6.0)):
    """A point in front of the cameras P, over the middle of their centres."""
    c = P[:, :, 3].mean(axis=0)
    return c + [rng.uniform(-0.5, 0.5), rng.uniform(-0.5, 0.5), rng.uniform(*depth)]


def make_track(seed, m, n_out=0, off_px=0.0, noise_px=0.3, origin=(0.0, 0.0, 0.0)):
    """One landmark seen by m keyframes of its own: -> poses (m, 3, 4), f (m, 3), planted (m), X (3)."""
    rng = np.random.default_rng(seed)
    P = make_keyframes(rng, m, origin)
    X = world_point(rng, P)
    f, planted = observe(rng, P, X, noise_px, n_out, off_px)
    return P, f, planted, X


def make_batch(seed, counts, origin=(0.0, 0.0, 0.0), outlier_share=0.0, off_px=40.0, n_keyframes=None):
    """Landmarks with counts[l] observations over ONE set of keyframes, each seen by a run of consecutive keyframes.
    -> dict(poses, offsets, obs_pose, obs_f, planted)."""
    rng = np.random.default_rng(seed)
    K = n_keyframes or max(max(counts), 2)
    P = make_keyframes(rng, K, origin)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    obs_pose, obs_f, planted = [], [], []
    for m in counts:
        first = int(rng.integers(0, K - m + 1))
        k = np.arange(first, first + m)
        n_out = int(m > 3 and rng.uniform() < outlier_share)
        f, pl = observe(rng, P[k], world_point(rng, P[k]) if m else np.zeros(3), 0.3, n_out, off_px)
        obs_pose.append(k)
        obs_f.append(f)
        planted.append(pl)
    return dict(poses=P, offsets=offsets, obs_pose=np.concatenate(obs_pose).astype(np.int32) if counts else np.zeros(0, np.int32),
                obs_f=np.concatenate(obs_f).reshape(-1, 3), planted=np.concatenate(planted))


def concat(batches):
    """Several batches as one call: the pose arrays stacked, the indices shifted."""
    poses, offsets, obs_pose, obs_f = [], [0], [], []
    shift = 0
    for b in batches:
        poses.append(b["poses"])
        obs_pose.append(b["obs_pose"] + shift)
        obs_f.append(b["obs_f"])
        offsets.extend((b["offsets"][1:] + offsets[-1]).tolist())
        shift += len(b["poses"])
    return dict(poses=np.concatenate(poses), offsets=np.asarray(offsets, np.int32), obs_pose=np.concatenate(obs_pose).astype(np.int32),
                obs_f=np.concatenate(obs_f).reshape(-1, 3))


def select(batch, order):
    """The landmarks `order` of a batch, in that order, over the same poses."""
    off = batch["offsets"]
    idx = [np.arange(off[l], off[l + 1]) for l in order]
    flat = np.concatenate(idx) if idx else np.zeros(0, np.int64)
    return dict(poses=batch["poses"], offsets=np.concatenate([[0], np.cumsum([len(i) for i in idx])]).astype(np.int32),
                obs_pose=batch["obs_pose"][flat], obs_f=batch["obs_f"][flat]), flat


def two_rays(theta, depth=5.0):
    """Two exact views of one point whose rays meet at the angle theta."""
    b = 2.0 * depth * math.tan(theta / 2.0)
    P = np.zeros((2, 3, 4))
    P[:, :, :3] = np.eye(3)
    P[1, 0, 3] = b
    X = np.array([b / 2.0, 0.0, depth])
    f = X - P[:, :, 3]
    return P, f / np.linalg.norm(f, axis=1, keepdims=True)


def status_batch():
    """One landmark per way out of L6, and the neighbours of the two that carry a NaN / an Inf.  -> batch, expected."""
    rng = np.random.default_rng(99)
    parts, expected = [], []

    def add(P, f, status):
        parts.append(dict(poses=P, offsets=np.array([0, len(f)], np.int32), obs_pose=np.arange(len(f), dtype=np.int32), obs_f=f))
        expected.append(status)

    one_deg = math.radians(1.0)
    # all centres equal: no pair passes the gate
    P, f, _, _ = make_track(1, 6)
    P[:, :, 3] = P[0, :, 3]
    add(P, observe(rng, P, P[0, :, 3] + [0.3, -0.2, 4.0], noise_px=0.0)[0], 3)
    # two rays just below and just above min_parallax
    add(*two_rays(one_deg * (1.0 - 1e-3)), 3)
    add(*two_rays(one_deg * (1.0 + 1e-3)), 0)
    # every observation an outlier: bearings that have nothing to do with one another
    P, f, _, _ = make_track(2, 6)
    f = rng.normal(size=(6, 3))
    f[:, 2] = np.abs(f[:, 2]) + 0.5
    add(P, f / np.linalg.norm(f, axis=1, keepdims=True), 3)
    # the point behind both cameras; behind one of three
    P, f, _, _ = make_track(3, 2)
    add(P, -f, 3)
    P, f, _, _ = make_track(4, 3)
    f[1] = -f[1]
    add(P, f, 0)
    # a zero bearing vector: one of three, one of two
    P, f, _, _ = make_track(5, 3)
    f[0] = 0.0
    add(P, f, 0)
    P, f, _, _ = make_track(6, 2)
    f[1] = 0.0
    add(P, f, 3)
    # a NaN in a pose entry and an Inf in a bearing vector, each between two landmarks that must not care
    P, f, _, _ = make_track(7, 5)
    add(P, f, 0)
    P, f, _, _ = make_track(8, 5)
    P[3, 1, 2] = np.nan
    add(P, f, 2)
    P, f, _, _ = make_track(9, 17)
    add(P, f, 0)
    P, f, _, _ = make_track(10, 4)
    f[2, 0] = np.inf
    add(P, f, 2)
    P, f, _, _ = make_track(11, 2)
    add(P, f, 0)
    # one observation
    P, f, _, _ = make_track(12, 1)
    add(P, f, 1)
    # status 4: nine exact views from almost one place and a tenth 1.2 degrees away: pairs with the tenth pass the
    # gate, every observation is an inlier, and the ten rays together have a tenth of the pair's parallax
    P = np.zeros((10, 3, 4))
    P[:, :, :3] = np.eye(3)
    P[:9, 0, 3] = np.arange(9) * 1e-4
    P[9, 0, 3] = 2.0 * 5.0 * math.tan(math.radians(1.2) / 2.0)
    X = np.array([0.05, 0.02, 5.0])
    f = X - P[:, :, 3]
    add(P, f / np.linalg.norm(f, axis=1, keepdims=True), 4)
    return concat(parts), expected


OBS_COUNTS = (1, 2, 3, 15, 16, 17, 24, 25, 26, 64, 65, 512)
CALL_SIZES = (1, 3, 4, 5, 63, 64, 65, 1000)
HYPOTHESIS_LIMITS = (1, 64, 65)
FAR_ORIGIN = (1e4, -1e4, 1e4)


def gpu_cases():
    """name -> (batch, params, expected statuses or None).  Everything the GPU tests and the host build of the device
    text are compared on; the restatement is run once per case by the callers."""
    cases = {}
    counts = make_batch(21, list(OBS_COUNTS), n_keyframes=512)
    cases["obs_counts"] = (counts, default_params(), [1] + [0] * (len(OBS_COUNTS) - 1))
    hyp = make_batch(22, [5, 11, 12, 13, 24, 40], outlier_share=0.5)
    for limit in HYPOTHESIS_LIMITS:
        cases["max_hypotheses_%d" % limit] = (hyp, default_params(max_hypotheses=limit, seed=5), None)
    for n in CALL_SIZES:
        rng = np.random.default_rng(100 + n)
        cases["call_%d" % n] = (make_batch(30 + n, rng.integers(2, 11, size=n).tolist(), outlier_share=0.3, n_keyframes=12),
                                default_params(), None)
    statuses, expected = status_batch()
    cases["statuses"] = (statuses, default_params(), expected)
    few = make_batch(23, [2, 3, 4, 4, 8], outlier_share=0.0)
    cases["min_inliers_3"] = (few, default_params(min_inliers=3), [5, 0, 0, 0, 0])
    cases["far"] = (make_batch(24, [2, 3, 7, 16, 24, 33], origin=FAR_ORIGIN, outlier_share=0.5), default_params(), None)
    cases["mixed"] = (concat([counts, hyp, cases["call_65"][0], statuses, few, cases["far"][0]]), default_params(seed=3), None)
    return cases


def moved_points(batch, points, share=0.05):
    """Each point moved sideways (world y: across the baseline and the viewing direction) by `share` of its depth from
    its first camera: 10 px at f = 200 in every view."""
    out = np.array(points, np.float64).copy()
    for l in range(len(out)):
        o = batch["offsets"][l]
        if batch["offsets"][l + 1] > o:
            depth = np.linalg.norm(out[l] - batch["poses"][batch["obs_pose"][o]][:, 3])
            out[l, 1] += share * depth
    return out


# ---- comparing, and the files of tools/landmark_serial ---------------------------------------------------------------
def same_bits(a, b):
    """Element-wise: equal bit patterns, any NaN equal to any NaN."""
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and bool(np.all((a.view(np.uint64) == b.view(np.uint64)) | (np.isnan(a) & np.isnan(b))))


def mismatch(got, want, per_observation=True):
    """None when every double of `got` is bit-equal to `want` and every integer equal; otherwise what differs first."""
    for k in RESULT_INTS:
        if not np.array_equal(np.asarray(got[k], np.int64), np.asarray(want[k], np.int64)):
            l = int(np.flatnonzero(np.asarray(got[k], np.int64) != np.asarray(want[k], np.int64))[0])
            return "%s of landmark %d: %s, want %s" % (k, l, got[k][l], want[k][l])
    for k in RESULT_DOUBLES + (("scores",) if per_observation else ()):
        if not same_bits(got[k], want[k]):
            return "%s: %s, want %s" % (k, np.asarray(got[k]).ravel()[:8], np.asarray(want[k]).ravel()[:8])
    if per_observation and not np.array_equal(np.asarray(got["flags"], np.uint8), np.asarray(want["flags"], np.uint8)):
        return "flags"
    return None


def write_problem(path, batch, prm, points=None):
    n = len(batch["offsets"]) - 1
    head = [0.0 if points is None else 1.0, len(batch["poses"]), n, prm["threshold"], prm["min_parallax"], prm["min_inliers"],
            prm["max_hypotheses"], prm["seed"]]
    parts = [np.asarray(head, np.float64), np.asarray(batch["offsets"], np.float64), np.asarray(batch["obs_pose"], np.float64),
             np.asarray(batch["poses"], np.float64).ravel(), np.asarray(batch["obs_f"], np.float64).ravel()]
    if points is not None:
        parts.append(np.asarray(points, np.float64).ravel())
    np.concatenate(parts).tofile(str(path))


def read_result(path, batch):
    n, total = len(batch["offsets"]) - 1, int(batch["offsets"][-1])
    raw = np.fromfile(str(path), np.float64)
    assert raw.size == 10 * n + 2 * total
    rows = raw[:10 * n].reshape(n, 10)
    out = dict(point=rows[:, :3].copy(), parallax=rows[:, 3].copy(), score_max=rows[:, 4].copy())
    for i, k in enumerate(RESULT_INTS):
        out[k] = rows[:, 5 + i].astype(np.int32)
    out["scores"] = raw[10 * n:10 * n + total].copy()
    out["flags"] = raw[10 * n + total:].astype(np.uint8)
    return out


# ---- the facade's policy (visual_odometry/map_maintenance.h) ---------------------------------------------------------
SUMMARY = ("candidates", "audited", "kept", "retriangulated", "added", "culled")


def maintain(cam, active, observations, landmarks, prm):
    """maintainMap.  active: [(keyframe id, pose [3][4], {track: corner})] in ascending id; observations {track: [keyframe
    ids]}; landmarks {track: point}.  -> (summary dict, the new {track: point})."""
    import camera_ref
    index = {kid: i for i, (kid, _, _) in enumerate(active)}
    poses = np.array([p for _, p, _ in active], np.float64).reshape(-1, 3, 4)
    cand = []
    for track in sorted(observations):
        seen = [(index[k], active[index[k]][2][track]) for k in sorted(set(observations[track]))
                if k in index and track in active[index[k]][2]]
        if len(seen) >= 2:
            cand.append((track, np.array([s[0] for s in seen]), camera_ref.unproject(cam, np.array([s[1] for s in seen]))))
    out = dict(landmarks)
    summary = dict.fromkeys(SUMMARY, 0)
    summary["candidates"] = len(cand)
    again = []
    for track, k, f in cand:
        if track in landmarks:
            summary["audited"] += 1
            if audit_one(poses, k, f, landmarks[track], prm)["status"] == 0:
                summary["kept"] += 1
                continue
        again.append((track, k, f))
    for track, k, f in again:
        r = triangulate_one(poses, k, f, prm)
        if r["status"] == 0:
            out[track] = r["point"]
            summary["retriangulated" if track in landmarks else "added"] += 1
        elif track in landmarks:
            del out[track]
            summary["culled"] += 1
    return summary, out
