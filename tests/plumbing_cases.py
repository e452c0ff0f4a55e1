"""Hand-built scenes for the per-feature tracker's plumbing: event routing (k_route), the patch count images
(k_patch_integrate) and the initial motion field (k_field_fixed / k_field_fill).  Every scene is deterministic and named
after the edge it reaches; tests/test_plumbing_cases_cpu.py checks with the oracle alone that it reaches it, the three
tests/test_gpu_*_edges.py files hold the device to the oracle on it.  No RandomState but in field_many_points().

Routing scenes are "calls": dict(name, chunk, rects [P][4], start [P], take [P], cap).  Patch scenes are lists of
patches: (events, rect) and, motion compensated, (events, rect, prelast, last, mid_time).  Field scenes are
(name, timestamp, trajectories)."""
import ctypes as C
import math

import numpy as np

import orc

EVENT_DTYPE = orc.EVENT_DTYPE


def events(x, y, t=None, sign=None):
    x = np.asarray(x, dtype=np.int64).ravel()
    ev = np.zeros(len(x), dtype=EVENT_DTYPE)
    ev["x"] = x
    ev["y"] = np.asarray(y, dtype=np.int64).ravel() if np.ndim(y) else int(y)
    ev["t_us"] = (1000 + np.arange(len(x))) if t is None else t
    ev["sign"] = 1 if sign is None else sign
    return ev


# ---- k_route ------------------------------------------------------------------------------------------------------------
# one wave per patch, 256 events per step in four sub-steps of 64

ROUTE_LENGTHS = (1, 63, 64, 65, 255, 256, 257, 511, 512, 513, 1025)
ROUTE_CAP = 1100            # above every chunk length: a quota of ROUTE_CAP is never filled
DENSE_RECT = (95.0, 95.0, 30.0, 30.0)   # holds every event of dense_chunk()
FILLING = (1, 63, 64, 65, 255, 256, 257)  # the filling event is the q-th from start


def dense_chunk(n):
    """n events, all inside DENSE_RECT (x, y in 100..119): every ballot of a walk over it is full."""
    i = np.arange(n)
    return events(100 + i % 20, 100 + (i // 20) % 20)


def sparse_chunk(n, lane):
    """n events outside DENSE_RECT but one per sub-step of 64, at `lane` of it (for a walk that starts at a multiple
    of 64)."""
    i = np.arange(n)
    ev = events(10 + i % 20, 10 + (i // 20) % 20)
    inside = i % 64 == lane
    ev["x"][inside] = 100 + (i[inside] // 64) % 20
    ev["y"][inside] = 110
    return ev


COORD_ENDS = (-16384, -1, 0, 16383)


def coords_chunk():
    """Every (x, y) pair of the packed range's ends, five times over (80 events)."""
    xs = [x for _ in range(5) for x in COORD_ENDS for _y in COORD_ENDS]
    ys = [y for _ in range(5) for _x in COORD_ENDS for y in COORD_ENDS]
    return events(xs, ys)


def grid_chunk():
    """Every pixel of x, y in 90..129 once, in raster order (1600 events)."""
    g = np.arange(90, 130)
    return events(np.tile(g, 40), np.repeat(g, 40))


def route_starts(n):
    """Starts the walk is aligned to: at and around the sub-step and step sizes and the chunk's end."""
    return sorted({0, 1, 63, 64, 65, 255, 256, 257, max(n - 1, 0), n, n + 1})


def _call(name, chunk, rects, start, take, cap=ROUTE_CAP):
    rects = np.asarray(rects, dtype=np.float64).reshape(-1, 4)
    return dict(name=name, chunk=chunk, rects=rects, start=np.asarray(start, dtype=np.uint32),
                take=np.asarray(take, dtype=np.uint32), cap=int(cap))


FRACTION_RECTS = (
    (100.25, 100.5, 10.5, 7.75),
    (100.75, 100.25, 7.25, 10.5),
    (100.5, 100.75, 8.0, 8.0),
    (100.0, 100.0, 8.75, 8.25),
    (99.75, 99.5, 0.5, 0.75),     # holds x = 100, y = 100 alone
    (100.25, 100.25, 0.5, 0.5),   # between the pixels: nothing
)
NOTHING_RECTS = (
    (100.0, 100.0, 0.0, 10.0),
    (100.0, 100.0, 10.0, 0.0),
    (100.0, 100.0, -5.0, 10.0),
    (100.0, 100.0, 10.0, -5.0),
    (math.nan, 100.0, 10.0, 10.0),
    (100.0, math.nan, 10.0, 10.0),
    (100.0, 100.0, math.nan, 10.0),
    (100.0, 100.0, 10.0, math.nan),
)
WHOLE_RANGE_RECT = (-16384.0, -16384.0, 32768.0, 32768.0)


def route_calls():
    """-> (chunks {key: events}, calls).  Calls that share a chunk follow each other."""
    chunks, calls = {}, []
    for n in ROUTE_LENGTHS:
        key = "dense%d" % n
        chunks[key] = dense_chunk(n)
        st = route_starts(n)
        # never filled (quota above the chunk), then filled by the start's own event
        calls.append(_call("len%d" % n, key, [DENSE_RECT] * (2 * len(st)), st + st,
                           [10 ** 6] * len(st) + [1] * len(st)))
    # the filling event at the last lane of a sub-step, of a step and the first lane of the next step; the quota
    # filled by the chunk's very last event; the quota one more than the chunk holds
    n = 1025
    st, tk = [], []
    for s in (0, 1, 63, 200):
        for q in FILLING + (n - s, n - s + 1):
            st.append(s)
            tk.append(q)
    calls.append(_call("quota", "dense1025", [DENSE_RECT] * len(st), st, tk))
    for lane in (0, 63):
        key = "sparse%d" % lane
        chunks[key] = sparse_chunk(n, lane)
        st, tk = [], []
        for s in (0, 192):
            for q in (1, 2, 3, 4, 5, 13, 14, 16, 17, 18):
                st.append(s)
                tk.append(q)
        calls.append(_call(key, key, [DENSE_RECT] * len(st), st, tk))
    # take = 0 (early and late start: next == start), cap < take, cap == take, take < cap; then cap = 1
    calls.append(_call("cap5", "dense1025", [DENSE_RECT] * 6, [0, 300, 0, 7, 64, 2000], [0, 0, 9, 5, 4, 0], cap=5))
    calls.append(_call("cap1", "dense1025", [DENSE_RECT] * 4, [0, 300, 1024, 1025], [0, 7, 1, 1], cap=1))
    # the packed range's ends: a 1 x 1 rect on each pair, a rect entirely at negative coordinates, the whole range
    chunks["coords"] = coords_chunk()
    rects = [(float(x), float(y), 1.0, 1.0) for x in COORD_ENDS for y in COORD_ENDS]
    rects += [(-16384.0, -16384.0, 16384.0, 16384.0), (-16384.0, -1.0, 16384.0, 1.0), WHOLE_RANGE_RECT,
              (0.0, 0.0, 16384.0, 16384.0), (16382.5, -16384.5, 1.0, 1.0)]
    calls.append(_call("coords", "coords", rects, [0] * len(rects), [10 ** 6] * len(rects)))
    # rect shapes on a chunk that holds every pixel once: all four borders have an event just inside and just outside
    chunks["grid"] = grid_chunk()
    rects = list(FRACTION_RECTS) + list(NOTHING_RECTS) + [WHOLE_RANGE_RECT, FRACTION_RECTS[0], FRACTION_RECTS[0]]
    calls.append(_call("shapes", "grid", rects, [0] * len(rects), [10 ** 6] * len(rects), cap=1700))
    # an empty chunk
    chunks["empty"] = events([], [])
    calls.append(_call("empty", "empty", [DENSE_RECT] * 3, [0, 1, 0], [10, 10, 0], cap=16))
    return chunks, calls


def second_call():
    """(first call, rects of the second): the second starts from the first's `next` on the same chunk."""
    takes = [1, 63, 64, 65, 255, 256, 257, 300, 1025, 2000]
    first = _call("first", "dense1025", [DENSE_RECT] * len(takes), [0] * len(takes), takes)
    moved = first["rects"] + np.array([10.75, -1.5, 0.0, 0.0])   # now holds x >= 106 only
    return first, moved


def route_select(ev, rects, start, take, cap):
    """The plain selection: the inside indices >= start, the first quota of them, next one behind the last taken."""
    x, y = ev["x"].astype(np.float64), ev["y"].astype(np.float64)
    lists, nxt = [], np.zeros(len(rects), dtype=np.uint32)
    for p, (rx, ry, rw, rh) in enumerate(np.asarray(rects, dtype=np.float64)):
        inside = np.flatnonzero((rx <= x) & (x < rx + rw) & (ry <= y) & (y < ry + rh))
        inside = inside[inside >= int(start[p])]
        quota = min(int(take[p]), int(cap))
        lists.append(inside[:quota].astype(np.uint32))
        if quota == 0:
            nxt[p] = start[p]
        elif len(inside) >= quota:
            nxt[p] = inside[quota - 1] + 1
        else:
            nxt[p] = len(ev)
    return lists, nxt


# ---- k_patch_integrate --------------------------------------------------------------------------------------------------
# one workgroup of 256 per patch, signed counts in an LDS tile of int(w) x int(h)

ERR_ARG, ERR_RANGE, ERR_UNSUPPORTED = -1, -3, -5   # include/ebo.h
GUARD = np.array([0xC0DEC0DEC0DEC0DE], dtype=np.uint64).view(np.float64)[0]  # a normal double no count can be


def span(rect):
    """x and y of the first pixel the rect holds (ceil of the corner) and its whole size."""
    return int(math.ceil(rect[0])), int(math.ceil(rect[1])), int(rect[2]), int(rect[3])


def patch_distinct(rect):
    """One event per pixel plus k extra on pixel k of the (wrapped) diagonal, sign by k's parity."""
    x0, y0, w, h = span(rect)
    xs = [x0 + i % w for i in range(w * h)]
    ys = [y0 + i // w for i in range(w * h)]
    sg = [1] * (w * h)
    for k in range(max(w, h)):
        xs += [x0 + k % w] * k
        ys += [y0 + k % h] * k
        sg += [1 if k % 2 == 0 else -1] * k
    n = len(xs)
    return events(xs, ys, 5000 - 2 * np.arange(n), sg)   # deque order: newest first


NONSQUARE = ((10.0, 20.0, 7.0, 31.0), (10.5, 20.25, 31.0, 7.0), (3.0, 4.0, 1.0, 25.0), (3.75, 4.5, 25.0, 1.0))


def patches_nonsquare():
    return [(patch_distinct(r), r) for r in NONSQUARE]


LIMIT_ADMITTED = ((5.0, 6.0, 128.0, 128.0), (5.0, -100.0, 1.0, 16384.0), (-100.0, 6.0, 16384.0, 1.0),
                  (5.5, 6.5, 127.0, 129.0))


def patches_limit():
    """Exactly 16384 pixels (and 127 x 129 = 16383): two events on the last pixel, one negative on the first, and
    one just past the last column and the last row, which the rect does not hold."""
    out = []
    for r in LIMIT_ADMITTED:
        x0, y0, w, h = span(r)
        xs = [x0 + w - 1, x0 + w - 1, x0, x0 + w, x0 + w - 1, x0 - 1]
        ys = [y0 + h - 1, y0 + h - 1, y0, y0 + h - 1, y0 + h, y0]
        out.append((events(xs, ys, 9000 - 3 * np.arange(6), [1, 1, -1, 1, 1, 1]), r))
    return out


REFUSED = (   # (rect, status): sizes the entries refuse before anything is copied or launched
    ((5.0, 6.0, 129.0, 128.0), ERR_UNSUPPORTED),
    ((5.0, 6.0, 0.0, 8.0), ERR_UNSUPPORTED),
    ((5.0, 6.0, -3.0, 8.0), ERR_UNSUPPORTED),
    ((0.0, 0.0, 7.5, 8.0), ERR_ARG),
    ((0.0, 0.0, 8.0, 7.5), ERR_ARG),
    ((0.0, 0.0, math.nan, 8.0), ERR_ARG),
    ((0.0, 0.0, 8.0, math.inf), ERR_ARG),
)

BORDER_RECTS = ((50.0, 60.0, 9.0, 7.0), (50.25, 60.75, 9.0, 7.0), (50.5, 60.5, 7.0, 9.0), (50.75, 60.25, 9.0, 7.0),
                (-3.5, 2.0, 9.0, 7.0), (2.0, -3.5, 7.0, 9.0))


def ring(x0, y0, w, h):
    """The border pixels of the w x h box at (x0, y0), clockwise from its corner."""
    pts = [(x0 + i, y0 + j) for j in range(h) for i in range(w) if i in (0, w - 1) or j in (0, h - 1)]
    return [p[0] for p in pts], [p[1] for p in pts]


def patches_border():
    """+1 on every pixel of the ring just inside the rect, -1 on every pixel of the ring just outside it."""
    out = []
    for r in BORDER_RECTS:
        x0, y0, w, h = span(r)
        xi, yi = ring(x0, y0, w, h)
        xo, yo = ring(x0 - 1, y0 - 1, w + 2, h + 2)
        n = len(xi) + len(xo)
        out.append((events(xi + xo, yi + yo, 7000 - np.arange(n), [1] * len(xi) + [-1] * len(xo)), r))
    return out


PILE_RECT = (30.0, 40.0, 25.0, 25.0)


def patches_pileup():
    """70 000 positive events on one pixel; 70 001 of alternating sign on one pixel, starting +1 and starting -1;
    257 events on 257 pixels: the 256-lane stride loop makes a second trip of one."""
    big, odd = 70000, 70001
    alt = np.where(np.arange(odd) % 2 == 0, 1, -1)
    i = np.arange(257)
    return [(events(np.full(big, 42), np.full(big, 52), 10 ** 6 - np.arange(big)), PILE_RECT),
            (events(np.full(odd, 54), np.full(odd, 64), 10 ** 6 - np.arange(odd), alt), PILE_RECT),
            (events(np.full(odd, 30), np.full(odd, 40), 10 ** 6 - np.arange(odd), -alt), PILE_RECT),
            (events(30 + i % 25, 40 + i // 25, 3000 - i, np.where(i % 3 == 0, -1, 1)), PILE_RECT)]


def patches_batch_with_empty():
    """Full, empty, full, empty (last): the empty ones own no event."""
    a = patch_distinct((10.0, 20.0, 5.0, 3.0))
    b = patch_distinct((11.5, 21.5, 3.0, 5.0))
    none = events([], [])
    return [(a, (10.0, 20.0, 5.0, 3.0)), (none, (0.0, 0.0, 4.0, 6.0)), (b, (11.5, 21.5, 3.0, 5.0)),
            (none, (7.0, 7.0, 2.0, 2.0))]


def offset_layouts(sizes):
    """nabla_offsets for images of `sizes` pixels -> {name: (offsets, buffer length)}: a gap before the first image and
    gaps between the images, in ascending and in descending order, and dense but descending."""
    out = {}
    off, pos = [], 5
    for s in sizes:
        off.append(pos)
        pos += s + 3
    out["gaps"] = (off, pos + 4)
    off, pos = [0] * len(sizes), 2
    for i in reversed(range(len(sizes))):
        off[i] = pos
        pos += sizes[i] + (7 if i % 2 else 0)   # some images touch, some do not
    out["descending"] = (off, pos + 1)
    off, pos = [0] * len(sizes), 0
    for i in reversed(range(len(sizes))):
        off[i] = pos
        pos += sizes[i]
    out["descending_dense"] = (off, pos)
    return out


# motion compensated: prelast / last = (x, y, t_us); f = (mid - t) / (last_t - prelast_t) is exact for a power of two
MC_RECT = (-4.0, 0.0, 20.0, 3.0)          # holds x = -4 .. 15
MC_PRE, MC_LAST, MC_MID = (0.0, 0.0, 1000), (1.0, 0.0, 1004), 1006   # direction (1, 0), tDif 4, half 2: passes
# (x, y, quarter steps of f) -> column it lands on (None: off the rect)
MC_TIES = (
    ((10, 0, 2), 10),    # 10.5 -> 10
    ((11, 0, 2), 12),    # 11.5 -> 12
    ((2, 0, 2), 2),      # 2.5 -> 2
    ((-1, 0, 2), 0),     # -0.5 -> -0 -> 0
    ((-2, 0, 2), -2),    # -1.5 -> -2
    ((15, 1, 1), 15),    # 15.25 -> 15: onto the last column
    ((15, 1, 2), None),  # 15.5 -> 16: just off it
    ((-5, 2, 3), -4),    # -4.25 -> -4: onto the first column
    ((-5, 2, 2), -4),    # -4.5 -> -4 (even): onto the first column
    ((-5, 2, 1), None),  # -4.75 -> -5: just off it
)


def patch_mc_ties():
    xs = [c[0][0] for c in MC_TIES]
    ys = [c[0][1] for c in MC_TIES]
    ts = [MC_MID - c[0][2] for c in MC_TIES]
    return (events(xs, ys, ts), MC_RECT, MC_PRE, MC_LAST, MC_MID)


TIME_RECT = (20.0, 30.0, 5.0, 4.0)
# (prelast t, last t, mid) -> passes R6's time test (patch.cpp:94-100)
MC_TIME_TESTS = (
    ((1000, 1010, 1015), True),    # last + half == mid
    ((1000, 1010, 1016), False),   # last + half == mid - 1
    ((1000, 1010, 1000), False),   # pre == mid
    ((1000, 1010, 1001), True),    # pre == mid - 1
    ((1000, 1003, 1004), True),    # last - pre = 3: half = 1
    ((1000, 1003, 1005), False),   # ... and not 2
    ((1003, 1000, 1004), False),   # last - pre = -3: half = -1; a negative step passes for no mid
    ((1003, 1000, 999), False),
    ((1003, 1000, 998), False),
)


def patches_mc_time():
    """One patch per time test, each with the same events (direction zero: they land where they are)."""
    ev = patch_distinct(TIME_RECT)
    return [(ev, TIME_RECT, (1.0, 2.0, t[0]), (1.0, 2.0, t[1]), t[2]) for t, _ in MC_TIME_TESTS]


MC_RANGE = ((0.0, 0.0, 0), (1.0, 0.0, 1 << 33), 5)   # a time step outside int32 microseconds


def pack_patches(patches):
    """-> (events, offsets uint64 [P + 1], rects [P][4]) of a list of patches."""
    ev = np.concatenate([p[0] for p in patches]) if patches else events([], [])
    off = np.zeros(len(patches) + 1, dtype=np.uint64)
    off[1:] = np.cumsum([len(p[0]) for p in patches])
    return ev, off, np.asarray([p[1] for p in patches], dtype=np.float64).reshape(-1, 4)


def pack_traj(patches):
    traj = np.asarray([[p[2][0], p[2][1], p[2][2], p[3][0], p[3][1], p[3][2]] for p in patches], dtype=np.float64)
    return traj, np.asarray([p[4] for p in patches], dtype=np.int64)


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def raw_patch_integrate(ebo, ctx, ev, offsets, rects, nabla_offsets, nabla, cur=None, last=None):
    """ebo_patch_integrate as include/ebo.h declares it: the caller's nabla_offsets and nabla.  -> status"""
    ev = np.ascontiguousarray(ev, dtype=ebo.EVENT_DTYPE)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    rects = np.ascontiguousarray(rects, dtype=np.float64).reshape(-1, 4)
    noff = np.ascontiguousarray(nabla_offsets, dtype=np.uint64)
    assert nabla.dtype == np.float64 and nabla.flags.c_contiguous
    return ebo.lib().ebo_patch_integrate(ctx._h, _vp(ev), _vp(offsets), len(rects), _vp(rects), _vp(noff), _vp(nabla),
                                         _vp(cur) if cur is not None else None, _vp(last) if last is not None else None)


def raw_patch_integrate_mc(ebo, ctx, ev, offsets, rects, traj, mid, nabla_offsets, nabla, updated):
    ev = np.ascontiguousarray(ev, dtype=ebo.EVENT_DTYPE)
    offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
    rects = np.ascontiguousarray(rects, dtype=np.float64).reshape(-1, 4)
    traj = np.ascontiguousarray(traj, dtype=np.float64).reshape(-1, 6)
    mid = np.ascontiguousarray(mid, dtype=np.int64)
    noff = np.ascontiguousarray(nabla_offsets, dtype=np.uint64)
    assert nabla.dtype == np.float64 and nabla.flags.c_contiguous and updated.dtype == np.int32
    return ebo.lib().ebo_patch_integrate_mc(ctx._h, _vp(ev), _vp(offsets), len(rects), _vp(rects), _vp(traj), _vp(mid),
                                            _vp(noff), _vp(nabla), _vp(updated))


def orc_patch_status(rect, mc):
    """The oracle's status for a rect it may refuse; the buffer is larger than any image it could go on to fill."""
    ev = events([int(rect[0]) if math.isfinite(rect[0]) else 0], [0])
    nabla = np.zeros(1 << 16)
    rx, ry, rw, rh = [C.c_double(float(v)) for v in rect]
    p = ev.ctypes.data_as(C.c_void_p)
    if not mc:
        return orc.lib().orc_patch_integrate(p, C.c_size_t(1), rx, ry, rw, rh, _vp(nabla), None, None)
    a, b, upd = np.zeros(2), np.ones(2), C.c_int32()
    return orc.lib().orc_patch_integrate_mc(p, C.c_size_t(1), rx, ry, rw, rh, _vp(a), C.c_int64(1000), _vp(b),
                                            C.c_int64(1004), C.c_int64(1004), _vp(nabla), C.byref(upd))


# ---- k_field_fixed / k_field_fill ---------------------------------------------------------------------------------------
# one serial walk over the patches, then one lane per pixel

FIELD_W, FIELD_H = 37, 29     # 1073 pixels = 4 * 256 + 49: the last workgroup of k_field_fill is partly idle


def seg(x, y, vx, vy, t0=2000, dt=4000):
    """Two samples: a fixed point at round(x, y) for timestamps <= t0, velocity (vx, vy) px/ms at scale 1e-3 (exact
    for the binary fractions used here)."""
    return [(x, y, t0), (x + vx * dt / 1000.0, y + vy * dt / 1000.0, t0 + dt)]


LB_TRAJ = [(5.0, 6.0, 1000), (9.0, 4.0, 5000), (10.0, 8.0, 9000)]   # fixed at sample 0 (t <= 1000) or 1 (t <= 5000)
LB_SET = [LB_TRAJ, [], [(20.0, 20.0, 5000)], [(30.0, 10.0, 5000), (31.0, 12.0, 7000)]]   # 3, 0, 1 and 2 samples
LB_TIMESTAMPS = (-5, 0, 1, 999, 1000, 1001, 4999, 5000, 5001, 8999, 9000, 9001)
# the samples the 3- and the 2-sample trajectory are fixed at (None: not fixed)
LB_EXPECT = {-5: (None, None), 0: (None, None), 1: (0, 0), 999: (0, 0), 1000: (0, 0), 1001: (1, 0), 4999: (1, 0),
             5000: (1, 0), 5001: (None, None), 8999: (None, None), 9000: (None, None), 9001: (None, None)}

ROUND_CASES = (   # (x, y) -> fixed pixel, None: rounds outside the image and is skipped
    ((2.5, 3.5), (3, 4)),
    ((0.5, 10.0), (1, 10)),
    ((-0.4, 12.0), (0, 12)),
    ((-0.5, 14.0), None),
    ((14.0, -0.5), None),
    ((FIELD_W - 0.5, 16.0), None),
    ((16.0, FIELD_H - 0.5), None),
    ((FIELD_W - 0.51, 18.0), (FIELD_W - 1, 18)),
    ((18.0, FIELD_H - 0.51), (18, FIELD_H - 1)),
    ((0.0, 0.0), (0, 0)),
    ((FIELD_W - 1.0, 0.0), (FIELD_W - 1, 0)),
    ((0.0, FIELD_H - 1.0), (0, FIELD_H - 1)),
    ((FIELD_W - 1.0, FIELD_H - 1.0), (FIELD_W - 1, FIELD_H - 1)),
)


def field_many_points(n=300):
    """300 fixed points for the length of k_field_fill's per-pixel loop (the one seeded scene)."""
    rng = np.random.RandomState(300)
    out = []
    for _ in range(n):
        x, y = rng.uniform(-0.4, FIELD_W - 0.6), rng.uniform(-0.4, FIELD_H - 0.6)
        out.append(seg(x, y, rng.randint(-64, 65) / 16.0, rng.randint(-64, 65) / 16.0))
    return out


def field_scenes():
    """-> list of (name, timestamp, trajectories)."""
    out = [("lower_bound_%d" % ts, ts, LB_SET) for ts in LB_TIMESTAMPS]
    out.append(("no_patches", 1500, []))
    out.append(("only_short", 1500, [[], [(3.0, 3.0, 2000)], []]))
    out.append(("rounding", 1500, [seg(c[0][0], c[0][1], 0.25 * (i + 1), -0.5 * (i + 1)) for i, c in enumerate(ROUND_CASES)]))
    # two patches on one pixel: the later one's velocity stands, the pixel is listed twice, the average counts both
    out.append(("same_pixel", 1500, [seg(12.2, 9.4, 1.0, 2.0), seg(30.0, 20.0, -3.0, 0.5), seg(11.8, 8.6, 4.0, -1.0)]))
    # a zero-velocity fixed point among others, alone at its end of the image; every fixed point zero
    out.append(("zero_velocity", 1500, [seg(5.0, 5.0, 0.0, 0.0), seg(30.0, 22.0, 2.0, -1.0), seg(32.0, 6.0, 0.5, 0.25)]))
    out.append(("all_zero", 1500, [seg(5.0, 5.0, 0.0, 0.0), seg(30.0, 22.0, 0.0, 0.0)]))
    # dt = 0 between the two samples: +-inf, and 0/0
    inf = [(8.0, 8.0, 2000), (9.0, 7.0, 2000)]
    nan = [(25.0, 20.0, 2000), (25.0, 21.0, 2000)]     # x: 0/0, y: inf
    out.append(("dt_zero_inf", 1500, [inf, seg(30.0, 5.0, 1.0, 1.0)]))
    out.append(("dt_zero_nan", 1500, [inf, nan, seg(30.0, 5.0, 1.0, 1.0)]))
    # nearest-fill tie: patch 0 lies to the right of patch 1, column 20 is equidistant: the first in the list wins
    out.append(("tie", 1500, [seg(30.0, 14.0, 1.0, 0.0), seg(10.0, 14.0, 0.0, 2.0)]))
    out.append(("many", 1500, field_many_points()))
    return out


def same_floats(a, b):
    """Bit equality of two float arrays; where both are NaN, sign and payload are free (x86 and the GPU differ)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape
    bits = {4: np.uint32, 8: np.uint64}[a.dtype.itemsize]
    na, nb = np.isnan(a), np.isnan(b)
    return bool(np.array_equal(na, nb) and np.array_equal(a.view(bits)[~na], b.view(bits)[~nb]))
