"""numpy restatement of the track-evaluation rules of include/ebo.h (V1-V9): float64, one rounding per operation in the
association written there, every sum in R6's tree (align_ref._tree), the maximum over the same tree
(align_ref._tree_extreme).  `track_error` is the restatement; `independent_errors` is an independent statement of V3-V4
(numpy.interp + numpy.hypot), the yardstick's own error bar and not a rule.  `seeds` restates ebo_track_seeds and
`summary` ebo_track_error_summary.  The tracks and batches of the CPU and GPU tests live here so that both test what the
other measured."""
import numpy as np

import align_ref as A

MAX_TAUS = 8
DOUBLES = ("err_mean", "err_rmse", "err_max")
INTS = ("age_us", "t_first_us", "n_inliers", "n_comparable", "first", "cut", "status")
same_bits = A.same_bits


def interp(t, p, T):
    """V3: the track (t (n,) int64, p (n, 2)) at the integer time T, t[0] <= T <= t[-1]."""
    j = int(np.searchsorted(t, T, side="right")) - 1            # the largest j with t[j] <= T
    if t[j] == T:
        return p[j].copy()
    w = np.float64(int(T) - int(t[j])) / np.float64(int(t[j + 1]) - int(t[j]))
    return p[j] + w * (p[j + 1] - p[j])


def sample_errors(est_t, est_xy, gt_t, gt_xy):
    """V2-V4 of one track with at least two ground-truth samples: -> (i0, i1, q, e), q and e over [i0, i1)."""
    i0 = int(np.searchsorted(est_t, gt_t[0], side="left"))
    i1 = int(np.searchsorted(est_t, gt_t[-1], side="right"))
    q = np.zeros(max(i1 - i0, 0))
    for k in range(i0, i1):
        g = interp(gt_t, gt_xy, est_t[k])
        dx = est_xy[k, 0] - g[0]
        dy = est_xy[k, 1] - g[1]
        q[k - i0] = dx * dx + dy * dy
    return i0, i1, q, np.sqrt(q)


def _zero(status):
    out = {f: np.float64(0.0) for f in DOUBLES}
    out.update({f: 0 for f in INTS})
    out["status"] = int(status)
    return out


def _as_track(t, xy):
    return np.asarray(t, np.int64).reshape(-1), np.asarray(xy, np.float64).reshape(-1, 2)


def track_error(est, gt, tau):
    """One unit: est = (t, xy), gt = (t, xy), tau -> (dict(DOUBLES.., INTS..), sample errors (n_est,))."""
    est_t, est_xy = _as_track(*est)
    gt_t, gt_xy = _as_track(*gt)
    none = np.full(len(est_t), -1.0)
    if len(est_t) == 0 or len(gt_t) < 2:                                   # V1
        return _zero(1), none
    if not (np.isfinite(est_xy).all() and np.isfinite(gt_xy).all()):
        return _zero(2), none
    i0, i1, q, e = sample_errors(est_t, est_xy, gt_t, gt_xy)
    if i0 >= i1:
        return _zero(1), none
    per_sample = none.copy()
    per_sample[i0:i1] = e                                                  # V8
    beyond = np.nonzero(e > np.float64(tau))[0]                            # V5
    n = int(beyond[0]) if len(beyond) else i1 - i0
    out = _zero(0)
    out.update(t_first_us=int(est_t[i0]), first=i0, n_comparable=i1 - i0, n_inliers=n,
               cut=i0 + int(beyond[0]) if len(beyond) else -1)
    if n:                                                                  # V6, V7
        nd = np.float64(n)
        out.update(age_us=int(est_t[i0 + n - 1]) - int(est_t[i0]), err_mean=np.float64(A._tree(e[:n]) / nd),
                   err_rmse=np.float64(np.sqrt(A._tree(q[:n]) / nd)), err_max=np.float64(A._tree_extreme(e[:n], 0.0, False)))
    return out, per_sample


def track_errors(ests, gts, taus):
    """Every (track, tau) of a call, track-major, and the per-sample errors of all tracks in one array, as
    Context.track_errors returns them."""
    out, per = [], []
    for k, (est, gt) in enumerate(zip(ests, gts)):
        for j, tau in enumerate(taus):
            r, s = track_error(est, gt, tau)
            r.update(track=k, tau=np.float64(tau))
            out.append(r)
        per.append(track_error(est, gt, 0.0)[1])
    return out, (np.concatenate(per) if per else np.zeros(0))


def independent_errors(est, gt):
    """numpy.interp + numpy.hypot over the comparable samples: -> (i0, i1, e)."""
    est_t, est_xy = _as_track(*est)
    gt_t, gt_xy = _as_track(*gt)
    i0 = int(np.searchsorted(est_t, gt_t[0], side="left"))
    i1 = int(np.searchsorted(est_t, gt_t[-1], side="right"))
    base = gt_t[0]
    tt = (est_t[i0:i1] - base).astype(np.float64)
    gg = (gt_t - base).astype(np.float64)
    gx, gy = np.interp(tt, gg, gt_xy[:, 0]), np.interp(tt, gg, gt_xy[:, 1])
    return i0, i1, np.hypot(est_xy[i0:i1, 0] - gx, est_xy[i0:i1, 1] - gy)


def seeds(ests, frame_t):
    """ebo_track_seeds: -> (seed_frame (n,) int32, seed_xy (n, 2) float32)."""
    frame_t = np.asarray(frame_t, np.int64)
    sf = np.full(len(ests), -1, np.int32)
    sx = np.zeros((len(ests), 2), np.float32)
    for k, est in enumerate(ests):
        t, xy = _as_track(*est)
        if len(t) == 0:
            continue
        f = int(np.searchsorted(frame_t, t[0], side="left"))
        if f == len(frame_t) or frame_t[f] > t[-1]:
            continue
        sf[k] = f
        sx[k] = interp(t, xy, frame_t[f]).astype(np.float32)
    return sf, sx


def summary(results):
    """ebo_track_error_summary over one tau's results, in track order."""
    m = outlived = 0
    se = sa = np.float64(0.0)
    for r in results:
        if r["status"] == 0 and r["n_inliers"] >= 1:
            se = se + np.float64(r["err_mean"])
            sa = sa + np.float64(r["age_us"])
            outlived += 1 if r["cut"] == -1 else 0
            m += 1
    if m == 0:
        return dict(mean_error=np.float64(0.0), mean_age_s=np.float64(0.0), counted=0, discarded=0, outlived=0)
    return dict(mean_error=se / np.float64(m), mean_age_s=(sa / np.float64(m)) * np.float64(1e-6), counted=m,
                discarded=len(results) - m, outlived=outlived)


def same_result(a, b):
    return all(int(a[f]) == int(b[f]) for f in INTS) and all(same_bits(a[f], b[f]) for f in DOUBLES)


# ---- tracks -------------------------------------------------------------------------------------------------------
def pack(tracks):
    """[(t, xy), ..] -> (offsets int32 (n + 1,), t int64, xy float64 (., 2))."""
    tracks = [_as_track(t, xy) for t, xy in tracks]
    off = np.zeros(len(tracks) + 1, np.int32)
    off[1:] = np.cumsum([len(t) for t, _ in tracks])
    t = np.concatenate([t for t, _ in tracks]) if tracks else np.zeros(0, np.int64)
    xy = np.concatenate([xy for _, xy in tracks]) if tracks else np.zeros((0, 2))
    return off, np.ascontiguousarray(t, np.int64), np.ascontiguousarray(xy, np.float64)


def gt_track(n, seed, t0=1_000_000, offset=0.0):
    """A ground-truth track of n samples at irregular frame times, moving smoothly."""
    rng = np.random.default_rng([seed, n, 1])
    t = t0 + np.concatenate([[0], np.cumsum(rng.integers(20_000, 45_000, max(n - 1, 0)))]).astype(np.int64)
    s = (t - t0) * 1e-6
    xy = np.stack([60.0 + 25.0 * s + 3.0 * np.sin(3.0 * s), 90.0 - 12.0 * s + 2.0 * np.cos(2.0 * s)], axis=1) + offset
    return t[:n], xy[:n]


def est_track(gt, n, seed, noise=0.3, on_gt=0.25, lo=None, hi=None):
    """n estimated samples at sorted random times within [lo, hi] (default: the ground truth's span), a share of them
    exactly on ground-truth times, at the ground truth's position plus noise."""
    gt_t, gt_xy = gt
    rng = np.random.default_rng([seed, n, 2])
    lo = int(gt_t[0]) if lo is None else int(lo)
    hi = int(gt_t[-1]) if hi is None else int(hi)
    t = rng.integers(lo, hi + 1, n).astype(np.int64)
    pick = rng.random(n) < on_gt
    t[pick] = rng.choice(gt_t, int(pick.sum()))
    t = np.sort(np.clip(t, lo, hi))
    s = (np.clip(t, gt_t[0], gt_t[-1]) - gt_t[0]).astype(np.float64)
    g = (gt_t - gt_t[0]).astype(np.float64)
    xy = np.stack([np.interp(s, g, gt_xy[:, 0]), np.interp(s, g, gt_xy[:, 1])], axis=1) + rng.normal(0, noise, (n, 2))
    return t, xy


INF = np.float64(np.inf)


def gpu_cases():
    """name -> (ests, gts, taus): the shapes at which the kernel can go wrong, each small."""
    c = {}
    gt = gt_track(40, 1)
    c["inliers"] = ([est_track(gt, n, 10 + n) for n in (1, 63, 64, 65, 128, 129)], [gt] * 6, [1e3])   # the lane stride's tails
    base = est_track(gt, 130, 2, noise=0.2)
    ests = []
    for cut in (0, 1, 63, 64, 65, 129, None):                              # one track, the cut moved along it
        t, xy = base[0].copy(), base[1].copy()
        if cut is not None:
            xy[cut] += (30.0, -40.0)
        ests.append((t, xy))
    c["cuts"] = (ests, [gt] * 7, [3.0])
    still = (np.array([0, 1000, 5000], np.int64), np.array([[10.0, 20.0]] * 3))
    moved = (np.array([0, 250, 1000, 3000, 5000], np.int64), np.array([[13.0, 24.0]] * 5))
    c["tie"] = ([moved], [still], [5.0, np.nextafter(5.0, 0.0), np.nextafter(5.0, 6.0)])                # e == tau: no cut
    gt = gt_track(5, 3)
    a, b = int(gt[0][0]), int(gt[0][-1])
    t = np.array([a - 7000, a - 1, a, a + 31_000, b - 2, b, b + 1, b + 9000], np.int64)
    xy = est_track(gt, 8, 4)[1]
    outside = (np.array([a - 500, a - 1, b + 1, b + 77], np.int64), xy[:4])
    before = (np.array([a - 500, a - 1], np.int64), xy[:2])
    after = (np.array([b + 1, b + 2], np.int64), xy[:2])
    c["span"] = ([(t, xy), outside, before, after, (t[2:6], xy[2:6])], [gt] * 5, [2.0])
    ests, gts = [], []
    for n in (1, 2, 3, 64, 65, 200):                                       # the search's trip counts 0, 1, 2, 6, 7, 8
        g = gt_track(n, 20 + n)
        gts.append(g)
        ests.append(est_track(g, 70, 30 + n, on_gt=0.4))
    c["gt_lengths"] = (ests, gts, [0.5, 50.0])
    gt = gt_track(9, 5)
    t, xy = est_track(gt, 20, 6)
    t[3:7] = t[3]
    t[18:] = gt[0][-1]                                                     # twice on the ground truth's last time
    t[:2] = gt[0][0]
    c["repeats"] = ([(np.sort(t), xy)], [gt], [0.4, 5.0])
    gt = gt_track(30, 7)
    c["taus8"] = ([est_track(gt, 100, 8, noise=0.5), est_track(gt, 17, 9, noise=0.5)], [gt] * 2,
                  [0.0, 0.25, 0.5, 0.75, 1.0, 1.5, 1e300, INF])
    gt = gt_track(6, 11)
    a, b = int(gt[0][0]), int(gt[0][-1])
    t, xy = est_track(gt, 8, 12)                                           # two samples before the span, eight in it, two after
    clean = (np.concatenate([[a - 40_000, a - 10], t, [b + 5, b + 30_000]]).astype(np.int64),
             np.concatenate([xy[:1], xy[:1], xy, xy[-1:], xy[-1:]]))
    ests, gts = [clean], [gt]
    for idx, comp, bad in ((3, 0, np.nan), (0, 1, np.inf), (11, 0, -np.inf)):   # inside, before, after the span
        t, xy = clean[0].copy(), clean[1].copy()
        xy[idx, comp] = bad
        ests.append((t, xy))
        gts.append(gt)
    for idx, comp, bad in ((2, 1, np.nan), (5, 0, np.inf)):                # a ground-truth coordinate
        xy = gt[1].copy()
        xy[idx, comp] = bad
        ests.append(clean)
        gts.append((gt[0], xy))
    ests.append(clean)                                                     # the neighbour after them is clean again
    gts.append(gt)
    c["nonfinite"] = (ests, gts, [1.0, INF])
    gt = gt_track(12, 13, t0=(1 << 50) + 12_345, offset=1e4)
    c["far"] = ([est_track(gt, 66, 14)], [gt], [0.5, 3.0])
    gt = gt_track(4, 15)
    nothing = (np.zeros(0, np.int64), np.zeros((0, 2)))
    c["empty"] = ([nothing, est_track(gt, 5, 16), est_track(gt, 5, 17), nothing], [gt, nothing, gt, nothing], [1.0, INF])
    return c


BATCH_TAUS = (0.0, 0.35, 1.0, 4.0, INF)


def batch70():
    """14 tracks x 5 thresholds mixing the cases of gpu_cases: -> (ests, gts, taus)."""
    take = {"inliers": [3, 5], "cuts": [0, 3, 6], "tie": [0], "span": [0, 1], "gt_lengths": [0, 4], "repeats": [0],
            "nonfinite": [1, 4], "empty": [0]}
    ests, gts = [], []
    for name, (ee, gg, _) in gpu_cases().items():
        for k in take.get(name, []):
            ests.append(ee[k])
            gts.append(gg[k])
    assert len(ests) * len(BATCH_TAUS) == 70
    return ests, gts, list(BATCH_TAUS)


# ---- files of tools/track_errors_serial.cpp --------------------------------------------------------------------------
def write_problem(path, ests, gts, taus):
    """Raw little-endian: int64 header (n_tracks, n_taus, n_est, n_gt), est_off and gt_off as int64 [n_tracks + 1], est_t
    [n_est], gt_t [n_gt] (int64), then float64: taus, est_xy [n_est][2], gt_xy [n_gt][2]."""
    eo, et, exy = pack(ests)
    go, gt, gxy = pack(gts)
    with open(path, "wb") as f:
        np.array([len(ests), len(taus), len(et), len(gt)], np.int64).tofile(f)
        eo.astype(np.int64).tofile(f)
        go.astype(np.int64).tofile(f)
        et.tofile(f)
        gt.tofile(f)
        np.asarray(taus, np.float64).tofile(f)
        exy.tofile(f)
        gxy.tofile(f)


def read_result(path, n_units, n_est):
    """-> (results, sample errors): per unit err_mean, err_rmse, err_max (float64) then the seven integers as int64; the
    per-sample errors [n_est] follow."""
    raw = np.fromfile(path, np.uint8)
    rec = np.dtype([("d", np.float64, 3), ("i", np.int64, 7)])
    units = np.frombuffer(raw[: n_units * rec.itemsize].tobytes(), rec)
    per = np.frombuffer(raw[n_units * rec.itemsize:].tobytes(), np.float64)
    assert len(per) == n_est
    out = []
    for u in units:
        d = {f: np.float64(u["d"][k]) for k, f in enumerate(DOUBLES)}
        d.update({f: int(u["i"][k]) for k, f in enumerate(INTS)})
        out.append(d)
    return out, per
