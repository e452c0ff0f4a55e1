"""A plain restatement of the bucketing of a window's events into units, and the edge cases its tests use.

Written from the rules only -- the header comments of csrc/ebo_bucket.inc, csrc/ebo_internal.h and csrc/order_deal.h,
and what they cite of the reference: feature_detector.cpp:305-306 (a window's reference time), :328-357 (the patch
rects, an event belongs to the rect that contains it, a patch is active with MORE than min_events events),
contrast_functor.h:18-20 (a patch's reference time).  numpy and Python integers; nothing is shared with the library's
own host counting sort.  tests/test_bucket_ref_cpu.py checks this file and its cases without a GPU,
tests/test_gpu_bucket_edges.py compares every loading path of the library with it, integer for integer.
"""
import collections

import numpy as np

EVENT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("sign", "<i4"), ("reserved", "<i4"), ("t_us", "<i8")])
COORD_MIN, COORD_MAX = -16384, 16383
SORT_MAX = 8192        # units above it keep list order
ORDER_STRIDE = 127
RUN_MAX = 32           # k_bucket_canon: runs of equal stamps above it take the bitonic network
I32_MIN, I32_MAX = -(1 << 31), (1 << 31) - 1


class RangeError(ValueError):
    """What the library answers with EBO_ERR_RANGE."""


Grid = collections.namedtuple("Grid", "image_w image_h patch_w patch_h")
G16 = Grid(64, 48, 16, 12)
G16R = Grid(70, 50, 16, 12)   # last column 22 wide, last row 14 high
G576 = Grid(96, 96, 4, 4)     # 577 buckets: three passes of the scan's 256, the last one partial
GRIDS = {"G16": G16, "G16r": G16R, "G576": G576}


def grid_shape(g):
    return g.image_w // g.patch_w, g.image_h // g.patch_h


def grid_rects(g):
    """(x, y, w, h) per patch, row-major; the last column / row absorbs the remainder."""
    npx, npy = grid_shape(g)
    out = []
    for py in range(npy):
        for px in range(npx):
            w = g.image_w - px * g.patch_w if px == npx - 1 else g.patch_w
            h = g.image_h - py * g.patch_h if py == npy - 1 else g.patch_h
            out.append((px * g.patch_w, py * g.patch_h, w, h))
    return out


def gcd(a, b):
    while b:
        a, b = b, a % b
    return a


def order_stride(n):
    """The stride of the deal: coprime to n, the first such at or after 127 mod n (1 where that is 0)."""
    if n < 3:
        return 1
    st = ORDER_STRIDE % n or 1
    while gcd(st, n) != 1:
        st += 1
    return st


def order_inverse(st, n):
    """stride^-1 mod n: the record of rank r sits at position r * inverse mod n."""
    return pow(st, -1, n) if n > 1 else 0


def deal(ranked):
    """Position q holds rank (q * stride) mod n."""
    n = len(ranked)
    if n < 2:
        return ranked.copy()
    st = order_stride(n)
    return ranked[(np.arange(n, dtype=np.int64) * st) % n]


def mid_time(a, b):
    """int32 truncation toward zero of (a + b) * 0.5, computed in float64; RangeError outside int32."""
    half = float(int(a) + int(b)) * 0.5
    if not (-2147483648.0 < half < 2147483648.0):
        raise RangeError("mid time outside int32")
    return int(half)  # int() of a float truncates toward zero


def pack(x, y, sign, dt):
    lo = (x.astype(np.int64) & 0x7FFF) | ((sign > 0).astype(np.int64) << 15) | ((y.astype(np.int64) & 0x7FFF) << 16)
    return (lo | ((dt.astype(np.int64) & 0xFFFFFFFF) << 32)).astype(np.uint64)


def unit_order(rec):
    """Canonical order of a unit's records given in list order."""
    if 2 <= len(rec) <= SORT_MAX:
        return deal(np.sort(rec))
    return rec.copy()


Bucket = collections.namedtuple("Bucket", "count rect t_ref active dt_win flow_idx records")
Window = collections.namedtuple("Window", "t_ref size buckets")


def bucket_windows(ev, offsets, grid, min_events):
    """-> [Window]: buckets 0 .. P-1 are the grid patches, bucket P the stray bucket."""
    npx, npy = grid_shape(grid)
    P = npx * npy
    rects = grid_rects(grid)
    # the rect that contains a point: its column / row begins at or before it, the next one after it
    col0 = np.array([r[0] for r in rects[:npx]], dtype=np.int64)
    row0 = np.array([rects[j * npx][1] for j in range(npy)], dtype=np.int64)
    out = []
    for w in range(len(offsets) - 1):
        e = ev[int(offsets[w]):int(offsets[w + 1])]
        n = len(e)
        x, y, t = e["x"].astype(np.int64), e["y"].astype(np.int64), e["t_us"].astype(np.int64)
        if n and (x.min() < COORD_MIN or x.max() > COORD_MAX or y.min() < COORD_MIN or y.max() > COORD_MAX):
            raise RangeError("coordinate outside the packed range")
        tw = mid_time(t[0], t[-1]) if n else 0
        inside = (x >= 0) & (x < grid.image_w) & (y >= 0) & (y < grid.image_h)
        b = np.full(n, P, dtype=np.int64)
        bx = np.searchsorted(col0, x[inside], side="right") - 1
        by = np.searchsorted(row0, y[inside], side="right") - 1
        b[inside] = by * npx + bx
        order = np.argsort(b, kind="stable")  # list order kept inside a bucket
        cnt = np.bincount(b, minlength=P + 1)
        start = np.concatenate([[0], np.cumsum(cnt)])
        buckets = []
        for k in range(P + 1):
            idx = order[start[k]:start[k + 1]]
            c = int(cnt[k])
            tk = t[idx]
            tu = tw
            if k < P and c:
                tu = mid_time(int(tk.min()), int(tk.max()))
            dwin = tw - tu
            if not I32_MIN <= dwin <= I32_MAX:
                raise RangeError("dt_win outside int32")
            if c:
                dt = tu - tk
                dtw = tw - tk
                if dt.min() < I32_MIN or dt.max() > I32_MAX or dtw.min() < I32_MIN or dtw.max() > I32_MAX:
                    raise RangeError("event further than 2^31 us from a reference time")
                rec = unit_order(pack(x[idx], y[idx], e["sign"][idx], dt))
            else:
                rec = np.zeros(0, dtype=np.uint64)
            buckets.append(Bucket(c, rects[k] if k < P else (0, 0, 1, 1), tu, bool(k < P and c > min_events), dwin,
                                  w * P + min(k, P - 1), rec))
        out.append(Window(tw, n, buckets))
    return out


def patch_units(ev, offsets):
    """ebo_set_patches: unit i = the list ev[offsets[i]:offsets[i+1]]; its reference time is the mid of its first and
    last LISTED stamp (contrast_functor.h:18-20) -> [(t_ref, records)]"""
    out = []
    for i in range(len(offsets) - 1):
        e = ev[int(offsets[i]):int(offsets[i + 1])]
        tu = mid_time(e["t_us"][0], e["t_us"][-1]) if len(e) else 0
        rec = pack(e["x"], e["y"], e["sign"], tu - e["t_us"].astype(np.int64))
        out.append((tu, unit_order(rec)))
    return out


def stamp_runs(records):
    """Lengths of the runs of equal stamps of a unit (from its records: equal hi words)."""
    if len(records) == 0:
        return np.zeros(0, dtype=np.int64)
    return np.unique(records >> np.uint64(32), return_counts=True)[1]


# ---- case builders ---------------------------------------------------------------------------------------------------

Case = collections.namedtuple("Case", "name grid ev offsets min_events eval t_base")


def events(x, y, t, sign=None):
    ev = np.zeros(len(x), dtype=EVENT_DTYPE)
    ev["x"], ev["y"], ev["t_us"] = x, y, t
    ev["sign"] = 1 if sign is None else sign
    return ev


def make_case(name, grid, windows, min_events=10, ev_eval=False, t_base=None):
    offsets = np.zeros(len(windows) + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(w) for w in windows])
    ev = np.concatenate(windows) if windows else np.zeros(0, dtype=EVENT_DTYPE)
    return Case(name, grid, ev, offsets, min_events, ev_eval, t_base)


def random_window(rng, grid, n, t0=1000, quantum=1, span=None, strays=0):
    """n time-ordered events uniform over the sensor, `strays` of them moved outside it."""
    if n == 0:
        return np.zeros(0, dtype=EVENT_DTYPE)
    span = span if span is not None else 2 * n
    t = t0 + (np.sort(rng.integers(0, span, n)) // quantum) * quantum
    ev = events(rng.integers(0, grid.image_w, n), rng.integers(0, grid.image_h, n), t, rng.integers(0, 2, n) * 2 - 1)
    for i in rng.choice(n, min(strays, n), replace=False):
        side = rng.integers(0, 4)
        if side == 0:
            ev["x"][i] = -1 - rng.integers(0, 5)
        elif side == 1:
            ev["x"][i] = grid.image_w + rng.integers(0, 5)
        elif side == 2:
            ev["y"][i] = -1 - rng.integers(0, 5)
        else:
            ev["y"][i] = grid.image_h + rng.integers(0, 5)
    return ev


def in_patch(rng, grid, patch, n):
    """n random pixels of one patch"""
    x0, y0, w, h = grid_rects(grid)[patch]
    return x0 + rng.integers(0, w, n), y0 + rng.integers(0, h, n)


SIZES = (0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 0, 1000, 0)


def case_sizes():
    rng = np.random.default_rng(101)
    return make_case("sizes", G16, [random_window(rng, G16, n, t0=1000 + 7919 * i, strays=2 if n >= 63 else 0) for i, n in enumerate(SIZES)],
                     ev_eval=True)


CHUNK_WINDOWS = (2047, 2048, 2049, 4097)
CHUNK_SWITCH_TOTAL = (1 << 19) + 1


def case_chunk_switch(filler):
    rng = np.random.default_rng(202)
    wins = [random_window(rng, G16R, n, t0=5000 * i, strays=3) for i, n in enumerate(CHUNK_WINDOWS)]
    if filler:
        wins.append(random_window(rng, G16R, CHUNK_SWITCH_TOTAL - sum(CHUNK_WINDOWS), t0=100000, strays=5))
    return make_case("chunk_switch_filler" if filler else "chunk_switch", G16R, wins)


SKEW_SINGLE, SKEW_PAIR = 300, (5, 570)


def case_skew():
    rng = np.random.default_rng(303)
    rects = grid_rects(G576)
    n = 64 * 20 + 17
    i = np.arange(n)
    b = i % 64
    x = np.array([rects[k][0] for k in b]) + (i // 64) % 4
    y = np.array([rects[k][1] for k in b]) + (i // 256) % 4
    walk = events(x, y, 1000 + i, (i % 3 == 0) * 2 - 1)
    sx, sy = in_patch(rng, G576, SKEW_SINGLE, 700)
    single = events(sx, sy, 9000 + np.sort(rng.integers(0, 900, 700)), rng.integers(0, 2, 700) * 2 - 1)
    m = 600
    ax, ay = in_patch(rng, G576, SKEW_PAIR[0], m)
    bx, by = in_patch(rng, G576, SKEW_PAIR[1], m)
    k = np.arange(m) % 3
    alt = events(np.where(k == 0, ax, np.where(k == 1, bx, -3)), np.where(k == 0, ay, np.where(k == 1, by, 200)),
                 20000 + np.arange(m) // 2, rng.integers(0, 2, m) * 2 - 1)
    return make_case("skew", G576, [walk, single, alt])


UNIT_SIZES = (1, 2, 3, 126, 127, 128, 254, 8191, 8192, 8193)


def unit_size_window(rng, sizes, others=5, t0=1000):
    """One G16 window: patch i holds exactly sizes[i] events, every other patch `others`; events interleaved in time."""
    P = 16
    per = list(sizes) + [others] * (P - len(sizes))
    patch = rng.permutation(np.repeat(np.arange(P), per))
    n = len(patch)
    x, y = np.zeros(n, dtype=np.int64), np.zeros(n, dtype=np.int64)
    for p in range(P):
        sel = patch == p
        x[sel], y[sel] = in_patch(rng, G16, p, int(sel.sum()))
    t = t0 + np.cumsum(rng.integers(0, 3, n))
    return events(x, y, t, rng.integers(0, 2, n) * 2 - 1)


def case_unit_sizes():
    rng = np.random.default_rng(404)
    return make_case("unit_sizes", G16, [unit_size_window(rng, UNIT_SIZES)], ev_eval=True)


TIE_MID_RUNS = (2, 31, 32, 33, 64)   # patches 0 .. 4: a run of this length in the middle of the unit
TIE_FIRST, TIE_LAST, TIE_REF, TIE_ALL20, TIE_ALL40 = 5, 6, 7, 8, 9  # the patches of the other sub-cases


def tie_run(rng, patch, length, t):
    """`length` events at stamp t in one patch: a base record, records that differ from it only in x, only in y, only in
    polarity, an exact duplicate, then random ones (more duplicates among them); listed in a random order."""
    x0, y0, w, h = grid_rects(G16)[patch]
    fixed = [(x0 + 3, y0 + 3, 1), (x0 + 3, y0 + 3, -1), (x0 + 3, y0 + 3, 1), (x0 + 4, y0 + 3, 1), (x0 + 3, y0 + 4, 1)]
    rows = fixed[:length]
    while len(rows) < length:
        rows.append((x0 + int(rng.integers(0, 3)), y0 + int(rng.integers(0, 3)), int(rng.integers(0, 2)) * 2 - 1))
    rows = [rows[i] for i in rng.permutation(length)] if length > 2 else rows
    a = np.array(rows)
    return events(a[:, 0], a[:, 1], np.full(length, t), a[:, 2])


def singles(rng, patch, stamps):
    x, y = in_patch(rng, G16, patch, len(stamps))
    return events(x, y, np.asarray(stamps), rng.integers(0, 2, len(stamps)) * 2 - 1)


def ties_window(rng):
    parts = []
    for p, run in enumerate(TIE_MID_RUNS):
        parts += [singles(rng, p, 1000 + 10 * np.arange(20)), tie_run(rng, p, run, 1500 + p),
                  singles(rng, p, 2000 + 10 * np.arange(20))]
    parts += [tie_run(rng, TIE_FIRST, 5, 1000), singles(rng, TIE_FIRST, 1100 + 7 * np.arange(30))]
    parts += [singles(rng, TIE_LAST, 1000 + 7 * np.arange(30)), tie_run(rng, TIE_LAST, 5, 3000)]
    # first stamp 1000, last 3000: the unit's reference time is 2000, where the run of 7 sits (dt == 0)
    parts += [singles(rng, TIE_REF, 1000 + 9 * np.arange(25)), tie_run(rng, TIE_REF, 7, 2000),
              singles(rng, TIE_REF, 3000 - 9 * np.arange(25)[::-1])]
    parts += [tie_run(rng, TIE_ALL20, 20, 1700), tie_run(rng, TIE_ALL40, 40, 1800)]
    for p in range(10, 16):
        parts.append(singles(rng, p, np.sort(rng.integers(1001, 2999, 12))))
    ev = np.concatenate(parts)
    return ev[np.argsort(ev["t_us"], kind="stable")]  # time-ordered; a run keeps the order it was listed in


def case_ties():
    return make_case("ties", G16, [ties_window(np.random.default_rng(505))], ev_eval=True)


STRAY_POINTS = ((-1, 5), (70, 5), (5, -1), (5, 50), (-16384, 16383), (16383, -16384))
LAST_PIXEL = (69, 49)


def case_strays():
    rng = np.random.default_rng(606)
    base = random_window(rng, G16R, 400, t0=1000)
    pts = list(STRAY_POINTS) + [LAST_PIXEL, (69, 0), (0, 49), (47, 35), (48, 36)]
    at = rng.choice(np.arange(1, 399), len(pts), replace=False)
    for i, (x, y) in zip(at, pts):
        base["x"][i], base["y"][i] = x, y
    return make_case("strays", G16R, [base])


def case_min_events(m):
    """patch 0 holds exactly m events (inactive), patch 1 m + 1 (active), patch 2 none; the rest a few each."""
    rng = np.random.default_rng(700 + m)
    sizes = [m, m + 1, 0] + [int(v) for v in rng.integers(0, 2 * m + 4, 13)]
    return make_case("min_events_%d" % m, G16, [unit_size_window(rng, sizes)], min_events=m)


T_WIDE = (1 << 32) - 2


def case_times():
    rng = np.random.default_rng(808)
    neg = random_window(rng, G16, 300, t0=-50000, span=50000)
    neg["t_us"][0], neg["t_us"][-1] = -50000, -1  # odd sum, negative half: -25000.5 truncates to -25000
    wide = events([5, 6], [5, 6], [0, T_WIDE])    # one patch: its reference time is the window's, 2^31 - 1
    return make_case("times", G16, [neg, wide], t_base=np.array([-50000 + 5, I32_MAX], dtype=np.int64))


def case_time_fault():
    """A batch whose middle window spans t = 0 .. 2^32: its mid time is 2^31, outside int32."""
    rng = np.random.default_rng(809)
    return make_case("time_fault", G16, [random_window(rng, G16, 50), events([5, 6], [5, 6], [0, 1 << 32]),
                                         random_window(rng, G16, 50)])


def permute_inside(rng, win):
    """The same events with those between the first and the last one in a random order."""
    idx = np.arange(len(win))
    if len(win) > 2:
        idx[1:-1] = rng.permutation(idx[1:-1])
    return win[idx]


UNORDERED_BIG = 9000   # events of patch 15 of the second window: above 8192, so its records follow the list


def windows_unordered():
    rng = np.random.default_rng(909)
    return [ties_window(np.random.default_rng(505)), unit_size_window(rng, [60] * 15 + [UNORDERED_BIG])]


def case_unordered(permuted=True):
    rng = np.random.default_rng(910)
    wins = windows_unordered()
    if permuted:
        wins = [permute_inside(rng, w) for w in wins]
    return make_case("unordered" if permuted else "unordered_in_order", G16, wins, ev_eval=True)


FINE_FITS, FINE_TOO_FINE = Grid(90, 90, 1, 1), Grid(91, 90, 1, 1)  # 8100 patches: device bucketing; 8190: host only


def case_finest(grid):
    rng = np.random.default_rng(1000 + grid.image_w)
    return make_case("finest_%d" % grid.image_w, grid, [random_window(rng, grid, 1500, strays=3),
                                                        random_window(rng, grid, 700, t0=9000, quantum=100, strays=1)],
                     min_events=0)


SWEEP_SEEDS = tuple(range(40))


def case_sweep(seed):
    rng = np.random.default_rng(5000 + seed)
    name = ("G16", "G16r", "G576")[seed % 3]  # every grid has its share of the seeds
    grid = GRIDS[name]
    quantum = (1, 7, 100, 2000)[(seed // 3) % 4]
    wins = [random_window(rng, grid, int(rng.integers(0, 6001)), t0=int(rng.integers(-100000, 100000)), quantum=quantum,
                          span=10000, strays=int(rng.integers(0, 6)))
            for _ in range(int(rng.integers(1, 7)))]
    return make_case("sweep_%d_%s_q%d" % (seed, name, quantum), grid, wins, min_events=(0, 10, 100)[(seed // 4) % 3])


PATCH_SIZES = (1, 200, 9000)


def patches_case():
    """ebo_set_patches: three lists of 1, 200 and 9000 events, NOT time-ordered -> (ev, offsets, rects)"""
    rng = np.random.default_rng(1111)
    parts = []
    for i, n in enumerate(PATCH_SIZES):
        x, y = in_patch(rng, G16, i, n)
        t = 1000 + rng.permutation(n) // 2 * 3  # pairs of equal stamps, listed in a random order
        parts.append(events(x, y, t, rng.integers(0, 2, n) * 2 - 1))
    offsets = np.concatenate([[0], np.cumsum(PATCH_SIZES)]).astype(np.uint64)
    return np.concatenate(parts), offsets, np.array(grid_rects(G16)[:3], dtype=np.int32)


_cache = {}


def reference(case):
    """bucket_windows of a case, computed once per process and shared (treat it as read-only)."""
    if case.name not in _cache:
        _cache[case.name] = bucket_windows(case.ev, case.offsets, case.grid, case.min_events)
    return _cache[case.name]
