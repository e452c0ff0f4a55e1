"""CPU only: patch scenes that put k_eval3's bank deal (csrc/eval_deal.h) at the fit boundary of every shipped launch plan
(csrc/eval_plan.h), for tests/test_deal_fit_cases_cpu.py and tests/test_gpu_eval_deal_fit.py.

A unit is dealt when its event count is admitted (2 B <= n <= 12 B for B lanes) and  L + max(P, scratch) <= capacity,
with L = (n + 3) // 4 doubles of list at the END of the image area and P = rows x cols pixels of the largest sub-band
(cols = bw | 1).  At P + L == capacity the image's last pixel is the double in front of the list.

One scene per shape of the plan (SHAPES).  A scene is a list of at least 1024 rects for ebo_set_patches -- the rect
sizes alone select the plan's shape -- of which about a dozen hold events; the others are empty and inactive.  The
units are built by hand: with the unit's first and last event 2 x HALF_US apart the reference time is their middle, and
under the flow ((kx + 0.5) / 25, (ky + 0.5) / 25) px/ms an event HALF_US before (after) it is shifted by +(-)(k + 0.5)
pixels.  The first event sits at the high corner of the wanted box of centre taps, the last at the low corner; every
other event lies within a fraction of a millisecond of the reference time inside the box and moves by less than a pixel,
so the count is free and the box is not.  Every shift ends in .5 (or is a fraction of a pixel), far from where a last
bit could move a truncation.  unit_box restates warp_event's centres and eval_unit3's box (as
tools/ab/lds_conflict_model.py: box_base_words does) and every unit is checked against it when it is built.

Classes (UNIT["cls"]; the rule's verdict is UNIT["dealt"]):
  fit          P + L == capacity, n a multiple of 4: dealt.  One with bw even (pitch bw + 1), one with bw odd
  fit_quad     the box of the even fit with n - 3 events: the same L, dealt
  over_list    that box with n + 1 events: one double of list more, not dealt
  over_row     n of the even fit, the box one row higher: not dealt (one sub-band: cols <= L at every shipped shape)
  low_end      an exact fit with n in 2 B .. 2 B + 7, else the closest dealt unit at n = 2 B (UNIT["free"] doubles left)
  high_end     the same with n in 12 B - 7 .. 12 B, resp. n = 12 B
  below, above n = 2 B - 1 and 12 B + 1 in a small box: not admitted by the count
  clipped      an exact fit cut by the last canvas row, whose first events warp_event rejects (key 16, sorted last)
  full_canvas  30 x 22 at sigma < 1: the 90 x 66 canvas (pitch 91) always fits 6680, so the boundary is the list alone:
               n = 2696 fits exactly (fit_quad and over_list are taken from it), n = 2697 does not.  The only other exact
               fit of this shape is 90 x 65 with n = 3060 (`fit`; with a 66th row `over_row`); no odd bw has one (ODD_FIT)
  split_fit, split_over   21 x 16 with a 31-wide column only: a 91-pixel pitch leaves 2540 mod 91 = 83 doubles behind
               the largest of TWO sub-bands, so n = 332 is dealt at an exact fit and n = 333 is not.  (Nowhere else can
               a unit in two sub-bands be dealt: what a full sub-band leaves is less than a pitch, and L >= B / 2.)
"""
import numpy as np

SCALE = 1e-3          # ebo_default_params: compensateScale
HALF_US = 25_000      # first and last event of a unit lie this far from its reference time
T0_US = 1_000_000
EVENT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("sign", "<i4"), ("reserved", "<i4"), ("t_us", "<i8")])

# csrc/eval_plan.h, written out
LDS_BUDGET, LDS_STEP, MANY_SLOTS = 160 * 1024, 1280, 1024
# csrc/eval_deal.h
DEAL_MIN_ROUNDS, DEAL_MAX_ROUNDS, DEAL_KEYS = 2, 12, 17


def header_doubles(waves):
    """eight sums and four ints per wave, the ints rounded to 16 bytes"""
    return 8 * waves + (waves * 4 * 4 + 15) // 16 * 2


def plan(block, waves_per_cu):
    """(workgroups per CU, LDS bytes per workgroup, image doubles) of a many-units launch"""
    groups = waves_per_cu // (block // 64)
    lds = LDS_BUDGET // groups // LDS_STEP * LDS_STEP
    return groups, lds, (lds - header_doubles(block // 64) * 8) // 8


def _shape(rect, wide, sigma, block, image, patches):
    groups, lds, cap = plan(block, 16 if sigma is None else 12)  # k_eval3<sigma < 1> is compiled for twelve waves per CU
    return dict(rect=rect, wide=wide, sigma=sigma, block=block, image=image, patches=patches, groups=groups, lds=lds, cap=cap)


SHAPES = {
    "20x20": _shape((20, 20), None, None, 128, (240, 180), 1080),
    "21x16+31": _shape((21, 16), 31, None, 128, (346, 260), 1040),
    "30x22": _shape((30, 22), None, None, 256, (240, 180), 1088),
    "20x20 sigma<1": _shape((20, 20), None, 0.7, 128, (240, 180), 1080),
    "30x22 sigma<1": _shape((30, 22), None, 0.7, 256, (240, 180), 1088),
}
# the same as literals: (20480 - 20*8)/8, (40960 - 40*8)/8, (26880 - 20*8)/8, (53760 - 40*8)/8
CAPACITIES = {"20x20": 2540, "21x16+31": 2540, "30x22": 5080, "20x20 sigma<1": 3340, "30x22 sigma<1": 6680}
RESIDENT = {"20x20": 8, "21x16+31": 8, "30x22": 4, "20x20 sigma<1": 6, "30x22 sigma<1": 3}

CLASSES = ("fit", "fit_quad", "over_list", "over_row", "low_end", "high_end", "below", "above", "clipped")
ABSENT = {}  # shape -> {class: why the shape cannot hold it}: every shape holds every class
ODD_FIT = {name: name != "30x22 sigma<1" for name in SHAPES}  # 6680 - L is a multiple of 91 twice and of no other pitch
EXTRA = {"30x22 sigma<1": ("full_canvas",), "21x16+31": ("split_fit", "split_over")}
ORACLE_CLASSES = ("fit", "fit_quad", "low_end", "high_end", "clipped", "full_canvas", "split_fit")


def classes_of(name):
    return tuple(c for c in CLASSES if c not in ABSENT.get(name, {})) + EXTRA.get(name, ())


# ---- the rule, in plain arithmetic ----------------------------------------------------------------------------------------
def list_doubles(n):
    return (n + 3) // 4


def rule(n, block, cap, bw, rows, slip=None):
    """eval_deal.h's deal_admits && deal_fits for one row tile, as eval_unit3 calls them; `slip` names one of the
    mistakes the scenes must tell apart (the CPU test's mutation check)"""
    if block > 256 or n < DEAL_MIN_ROUNDS * block or n > DEAL_MAX_ROUNDS * block or bw == 0:
        return False
    if slip == "cap_4960":
        cap = (40 * 1024 - 160 * 8) // 8
    if slip == "header_160":
        cap = cap + header_doubles(block // 64) - 160
    cols = (bw | 1) if (bw | 1) <= cap else bw
    band = min(max(cap // cols, 1), rows) * (bw if slip == "band_bw" else cols)
    lst = n // 4 if slip == "list_floor" else list_doubles(n)
    scratch = (DEAL_KEYS * block + 1) // 2 + lst
    need = lst + max(band, scratch)
    return need < cap if slip == "less_than" else need <= cap


SLIPS = ("less_than", "band_bw", "list_floor", "cap_4960", "header_160")


def exact_fits(cap, block, rw, rh):
    """(n, bw, rows) with P + L == cap, n an admitted multiple of 4, in the canvas of an rw x rh rect"""
    out = []
    for bw in range(8, 3 * rw + 1):
        for rows in range(8, 3 * rh + 1):
            n = 4 * (cap - (bw | 1) * rows)
            if DEAL_MIN_ROUNDS * block <= n <= DEAL_MAX_ROUNDS * block:
                out.append((n, bw, rows))
    return out


def closest_fit(cap, block, rw, rh, n):
    """(free doubles, bw, rows): the largest box that leaves room for n events' list"""
    room = cap - list_doubles(n)
    best = None
    for bw in range(8, 3 * rw + 1):
        rows = min(room // (bw | 1), 3 * rh)
        if rows >= 8 and (best is None or room - (bw | 1) * rows < best[0]):
            best = (room - (bw | 1) * rows, bw, rows)
    return best


# ---- restatement of the centres and the box -------------------------------------------------------------------------------
def ref_time(t_first, t_last):
    return int(np.int32(float(int(t_first) + int(t_last)) * 0.5))


def unit_box(ev, rect, flow):
    """warp_event's centre taps and eval_unit3's box of one unit's events (time-ordered): dict with pxc, pyc (all events),
    ok (the events warp_event keeps), x0, y0, bw, rows"""
    rx, ry, rw, rh = (int(v) for v in rect)
    t = ev["t_us"].astype(np.int64)
    tau = (ref_time(t[0], t[-1]) - t).astype(np.float64) * SCALE
    pxc = np.trunc(ev["x"].astype(np.float64) + tau * flow[0]).astype(np.int64) - rx + rw
    pyc = np.trunc(ev["y"].astype(np.float64) + tau * flow[1]).astype(np.int64) - ry + rh
    ok = (pxc + 3 >= 0) & (pxc - 3 < 3 * rw) & (pyc + 3 >= 0) & (pyc - 3 < 3 * rh)
    x0, x1 = max(pxc[ok].min() - 3, 0), min(pxc[ok].max() + 3, 3 * rw - 1)
    y0, y1 = max(pyc[ok].min() - 3, 0), min(pyc[ok].max() + 3, 3 * rh - 1)
    return dict(pxc=pxc, pyc=pyc, ok=ok, x0=int(x0), y0=int(y0), bw=int(x1 - x0 + 1), rows=int(y1 - y0 + 1))


def covers_last_pixel(box):
    """events whose 7 x 7 footprint holds the box's last pixel (the image's last double where bw is odd, the one in
    front of the pad column's where it is even)"""
    x1, y1 = box["x0"] + box["bw"] - 1, box["y0"] + box["rows"] - 1
    return box["ok"] & (np.abs(box["pxc"] - x1) <= 3) & (np.abs(box["pyc"] - y1) <= 3)


# ---- building a unit ------------------------------------------------------------------------------------------------------
def _axis(lo, hi, side):
    """k, a, b with  hi = a + side + k  and  lo = b + side - k - 1: the source offsets a, b in 0 .. side - 1 of the first
    and the last event and the whole pixels k of their shift"""
    kmin = max(hi - 2 * side + 1, side - 1 - lo, 0)
    kmax = min(hi - side, 2 * side - 2 - lo)
    if kmin > kmax:
        raise ValueError("no shift puts the centres %d .. %d on a side of %d" % (lo, hi, side))
    return kmin, hi - side - kmin, lo - side + kmin + 1


def _events(x, y, t, rng):
    ev = np.zeros(len(x), dtype=EVENT_DTYPE)
    o = np.argsort(t, kind="stable")
    ev["x"], ev["y"], ev["t_us"] = np.asarray(x)[o], np.asarray(y)[o], np.asarray(t)[o]
    ev["sign"] = rng.integers(0, 2, len(x)) * 2 - 1
    return ev


def _interior(rng, count, lo, hi, side):
    """source offsets whose centre (offset + side, moved by less than a pixel) stays inside lo .. hi"""
    a, b = max(0, lo - side + 1), min(side - 1, hi - side - 1)
    if a > b:
        raise ValueError("the box of centres %d .. %d misses the rect" % (lo, hi))
    return rng.integers(a, b + 1, count)


def make_unit(rect, lo, hi, n, seed):
    """n events in `rect` = (x, y, w, h) and the flow under which their centre taps span lo = (pxc, pyc) .. hi exactly"""
    rx, ry, rw, rh = (int(v) for v in rect)
    rng = np.random.default_rng(seed)
    kx, ax, bx = _axis(lo[0], hi[0], rw)
    ky, ay, by = _axis(lo[1], hi[1], rh)
    flow = ((kx + 0.5) / (HALF_US * SCALE), (ky + 0.5) / (HALF_US * SCALE))
    dt = rng.integers(-300, 301, n - 2)
    x = np.concatenate([[ax], _interior(rng, n - 2, lo[0], hi[0], rw), [bx]]) + rx
    y = np.concatenate([[ay], _interior(rng, n - 2, lo[1], hi[1], rh), [by]]) + ry
    t = np.concatenate([[T0_US], T0_US + HALF_US - dt, [T0_US + 2 * HALF_US]])
    return _events(x, y, t, rng), flow


def box_centres(rect, bw, rows):
    """lo, hi of the centre taps of a bw x rows box centred in the canvas (not clipped: it may touch the canvas edge)"""
    rw, rh = int(rect[2]), int(rect[3])
    x0, y0 = (3 * rw - bw) // 2, (3 * rh - rows) // 2
    return (x0 + 3, y0 + 3), (x0 + bw - 4, y0 + rows - 4)


def make_clipped(rect, cap, block, seed, rejected=5, want=None):
    """An exact fit whose box ends at the last canvas row and whose first `rejected` events leave the canvas: the flow's
    row component shifts the first event (source row rh - 1, HALF_US early) by ky + 0.5 >= rh + 4.5 rows, past the three-tap
    margin, and an event of the same source row (rh + 0.5) / m1 ms early onto the last canvas row.  Searched: ky and the
    last event's source row (the rows), kx and both source columns (the width).  -> events, flow, (n, bw, rows)"""
    rx, ry, rw, rh = (int(v) for v in rect)
    for ky in range(rh + 4, 3 * rh + 3):
        m1 = (ky + 0.5) / (HALF_US * SCALE)
        d = int(round((rh + 0.5) / m1 / SCALE))
        for by in range(rh - 1, -1, -1):
            pyc_lo = by + rh - ky - 1
            if pyc_lo < -3:
                break
            rows = 3 * rh - max(pyc_lo - 3, 0)
            for bw in range(rw + 8, 3 * rw + 1):
                n = 4 * (cap - (bw | 1) * rows)
                if not DEAL_MIN_ROUNDS * block <= n <= DEAL_MAX_ROUNDS * block or (want and not want(n, bw, rows)):
                    continue
                for kx in range(2 * rw):
                    m0 = (kx + 0.5) / (HALF_US * SCALE)
                    sx = d * SCALE * m0
                    if abs(sx - round(sx)) < 0.05:
                        continue  # (keep the column shift away from a whole pixel)
                    for bx in range(min(kx, rw - 1) + 1):
                        pxc_lo = bx + rw - kx - 1
                        x0 = max(pxc_lo - 3, 0)
                        pxc_hi = x0 + bw - 4
                        ax = pxc_hi - rw - int(sx)
                        if pxc_lo < -3 or x0 + bw > 3 * rw or not 0 <= ax < rw or pxc_hi < 2 * rw:
                            continue
                        rng = np.random.default_rng(seed)
                        k = n - rejected - 2
                        dt = rng.integers(-300, 301, k)
                        x = np.concatenate([np.full(rejected, ax), [ax], _interior(rng, k, pxc_lo, pxc_hi, rw), [bx]]) + rx
                        y = np.concatenate([np.full(rejected, rh - 1), [rh - 1], _interior(rng, k, pyc_lo, 3 * rh - 1, rh), [by]]) + ry
                        t = np.concatenate([T0_US + 3 * np.arange(rejected), [T0_US + HALF_US - d], T0_US + HALF_US - dt,
                                            [T0_US + 2 * HALF_US]])
                        return _events(x, y, t, rng), (m0, m1), (n, bw, rows)
    raise ValueError("no clipped exact fit")


# ---- the scenes -----------------------------------------------------------------------------------------------------------
def lattice(name):
    """the scene's rects [patches][4]: the sensor cut into the shape's rects (the last column `wide` where the shape has
    one), repeated until there are enough; -> rects, rects per copy"""
    S = SHAPES[name]
    (W, H), (rw, rh) = S["image"], S["rect"]
    nx, ny = W // rw, H // rh
    one = [(i * rw, j * rh, S["wide"] if (S["wide"] and i == nx - 1) else rw, rh) for j in range(ny) for i in range(nx)]
    reps = -(-S["patches"] // len(one))
    return np.array((one * reps)[:S["patches"]], dtype=np.int32), len(one)


def _pick(fits, block, pred):
    """the exact fit nearest the middle of the admitted counts among those `pred` holds for"""
    cand = [f for f in fits if pred(*f)]
    return min(cand, key=lambda f: (abs(f[0] - 6 * block), f[1], f[2])) if cand else None


def _plan_units(name):
    """[(unit name, class, wide rect?, kind, arguments)] of one shape"""
    S = SHAPES[name]
    cap, B, (rw, rh) = S["cap"], S["block"], S["rect"]
    lo_n, hi_n = DEAL_MIN_ROUNDS * B, DEAL_MAX_ROUNDS * B
    units = []
    if name == "30x22 sigma<1":
        n = 4 * (cap - 91 * 66)
        full = ((2, 1), (3 * rw - 2, 3 * rh - 2))  # centres within three pixels of every canvas edge
        units += [("fit_even", "fit", False, "box", (4 * (cap - 91 * 65), 90, 65)),
                  ("over_row", "over_row", False, "box", (4 * (cap - 91 * 65), 90, 66)),
                  ("full_canvas", "full_canvas", False, "span", (*full, n)),
                  ("fit_quad", "fit_quad", False, "span", (*full, n - 3)),
                  ("over_list", "over_list", False, "span", (*full, n + 1)),
                  ("clipped", "clipped", False, "clipped", (lambda n_, bw, rows: bw == 3 * rw and rows == 3 * rh,))]
    else:
        fits = exact_fits(cap, B, rw, rh)
        inside = lambda n_, bw, rows: bw <= 3 * rw - 2 and rows <= 3 * rh - 3
        even = _pick(fits, B, lambda n_, bw, rows: bw % 2 == 0 and inside(n_, bw, rows))
        wide = S["wide"]
        odd_fits = exact_fits(cap, B, wide, rh) if wide else fits
        odd = _pick(odd_fits, B, lambda n_, bw, rows: bw % 2 == 1 and rows <= 3 * rh - 3 and bw <= 3 * (wide or rw) - 2 and bw > 3 * rw * bool(wide))
        n, bw, rows = even
        units += [("fit_even", "fit", False, "box", (n, bw, rows)),
                  ("fit_odd", "fit", bool(wide), "box", odd),
                  ("fit_quad", "fit_quad", False, "box", (n - 3, bw, rows)),
                  ("over_list", "over_list", False, "box", (n + 1, bw, rows)),
                  ("over_row", "over_row", False, "box", (n, bw, rows + 1)),
                  ("clipped", "clipped", False, "clipped", (None,))]
    for cls, n_end, quad in (("low_end", lo_n, range(lo_n, lo_n + 8)), ("high_end", hi_n, range(hi_n - 7, hi_n + 1))):
        f = None if name == "30x22 sigma<1" else _pick(fits, B, lambda n_, bw, rows: n_ in quad)
        if f is None:
            _, bw, rows = closest_fit(cap, B, rw, rh, n_end)
            f = (n_end, bw, rows)
        units.append((cls, cls, False, "box", f))
    units += [("below", "below", False, "box", (lo_n - 1, rw + 14, rh + 14)),
              ("above", "above", False, "box", (hi_n + 1, rw + 14, rh + 14))]
    if name == "21x16+31":
        # a 31-wide rect's canvas is 93 wide: pitch 91 leaves cap mod 91 doubles behind a full sub-band of cap // 91 rows
        rest = cap % 91
        units += [("split_fit", "split_fit", True, "box", (4 * rest, 91, 40)),
                  ("split_over", "split_over", True, "box", (4 * rest + 1, 91, 40))]
    return units


_scenes = {}


def units_of(name):
    """the scene's units, built once: [dict(name, cls, wide, ev, flow, n, x0, y0, bw, rows, cols, sub_bands, free, dealt,
    rejected, slot)]; slot = the index of the unit's rect in one copy of the lattice"""
    if name in _scenes:
        return _scenes[name]
    S = SHAPES[name]
    cap, B = S["cap"], S["block"]
    rects, per = lattice(name)
    nx = S["image"][0] // S["rect"][0]
    # rects at least three columns and rows inside the sensor: no warped coordinate is negative, where trunc is not floor
    regular = [i for i in range(per) if 3 <= i % nx < nx - 1 and i // nx >= 3]
    wides = [i for i in range(per) if i % nx == nx - 1 and i // nx >= 3]
    plan_ = _plan_units(name)
    out = []
    for k, (uname, cls, wide, kind, args) in enumerate(plan_):
        pool = wides if wide else regular
        slot = pool[(k * 7 + 3) % len(pool)]
        while any(u["slot"] == slot for u in out):
            slot = pool[(pool.index(slot) + 1) % len(pool)]
        rect = rects[slot]
        if kind == "clipped":
            ev, flow, (n, bw, rows) = make_clipped(rect, cap, B, seed=7000 + k, want=args[0])
        else:
            if kind == "box":
                n, bw, rows = args
                lo, hi = box_centres(rect, bw, rows)
            else:
                lo, hi, n = args
                bw, rows = min(hi[0] + 3, 3 * int(rect[2]) - 1) - max(lo[0] - 3, 0) + 1, min(hi[1] + 3, 3 * int(rect[3]) - 1) - max(lo[1] - 3, 0) + 1
            ev, flow = make_unit(rect, lo, hi, n, seed=7000 + k)
        box = unit_box(ev, rect, flow)
        assert (box["bw"], box["rows"], len(ev)) == (bw, rows, n), (name, uname, box["bw"], box["rows"], bw, rows)
        cols = bw | 1
        max_rows = max(cap // cols, 1)
        band = min(max_rows, rows) * cols
        out.append(dict(name=uname, cls=cls, wide=wide, ev=ev, flow=flow, n=n, x0=box["x0"], y0=box["y0"], bw=bw, rows=rows,
                        cols=cols, sub_bands=-(-rows // max_rows), free=cap - band - list_doubles(n), dealt=rule(n, B, cap, bw, rows),
                        rejected=int((~box["ok"]).sum()), slot=slot))
    _scenes[name] = out
    return out


def assemble(name, order="normal"):
    """(events, offsets [patches + 1], rects [patches][4], flows [patches][2], patch index per unit) of one scene.
    order: "normal" -- the units in the first copy of the lattice; "moved" -- the fit and over_list units in the same
    rects of later copies (the same coordinates, other patch indices); "reversed" -- the normal scene's patches back to
    front"""
    rects, per = lattice(name)
    units = units_of(name)
    copies = len(rects) // per
    index = []
    for k, u in enumerate(units):
        c = (1 + k % (copies - 1)) if (order == "moved" and u["cls"] in ("fit", "full_canvas", "over_list")) else 0
        index.append(u["slot"] + c * per)
    if order == "reversed":
        rects = rects[::-1].copy()
        index = [len(rects) - 1 - i for i in index]
    counts = np.zeros(len(rects), dtype=np.int64)
    flows = np.zeros((len(rects), 2))
    for u, i in zip(units, index):
        counts[i] = u["n"]
        flows[i] = u["flow"]
    by_patch = sorted(range(len(units)), key=lambda k: index[k])
    ev = np.concatenate([units[k]["ev"] for k in by_patch])
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64)
    return ev, offsets, rects, flows, index
