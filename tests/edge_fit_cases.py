"""CPU only: single units (a few dozen events each) whose edge-loss box sits at the largest size a storage form admits or
at the smallest it refuses, for tests/test_edge_fit_cases_cpu.py and tests/test_gpu_edge_fit.py.  Deterministic; a plain
module, not a conftest.  The geometry and the capacities are edge_box_ref's restatement; nothing here calls the library.

How a unit is steered.  Its first two events lie HALF_US before its reference time and its last two HALF_US after it, so
under the flow ((kx + FRAC_X) / 25, (ky + FRAC_Y) / 25) px/ms the early ones move by +(k + frac) pixels and the late ones by
-(k + frac): an early event gives the high corner of the wanted box of centre taps, a late one the low corner.  Every other
event lies within 3 ms of the reference time and is drawn (rejection sampling against the restated warp) so that its tap
falls inside that box.  Flows are never integers and no warped coordinate is within MIN_AWAY of an integer.

Regimes: a-d run on the shipped library, e-h need the A/B build's switches (Case.env).
  a   one 40x22 rect (canvas 120x66): 20 B form, limited by maxLdsPx = 7424, never by bytes
  b   52x36 sensor in 21x16 patches (a grid window): 20 B form at 80 KB - 256, the 31x20 corner unit at cap_px = 3606
  c   one 32x30 rect (canvas 96x90 > 8192): 28 B form with a slice, cap_px = 5510
  d   one 20x20 rect: nothing can spill; the full-canvas box
  e52, e40   compact form forced, budgets 52 / 40 KB, 20x20 rects; deferred units take the 20 B launch, or (EBO_EDGE_LDS_KB
      = 72) the slice; a batch of all three outcomes in both orders
  f0, f1     EBO_EDGE_LAYOUT 0 / 1 at EBO_EDGE_LDS_KB = 48, 20x20 rects
  g   claim pile-up on the compact form's 4-bit counters (PILE_CASES)
  h   device-resident solve of custom units whose box crosses the limit between start and end (SOLVE_CASES)

Case names: <regime>/<class>.  Classes:
  fit          the fitting box with the most pixels          over         its cheapest one-step neighbour that does not fit
  fit_c-1, fit_r-1   fit less a column / a row (fit)          fit_c+1, fit_r+1   fit plus a column / a row (do not fit)
  bytes_fit, bytes_over   aliased forms: the boxes with the least slack / the least excess in edge_box_fits_alias's byte
               test among those the pixel test admits
  rows_fit, rows_over     aliased forms: the same columns and box rows (so the same pixels; the box is clamped by the canvas
               on that side), rows_over with one row of taps more: iRows and qRows one more each, across the byte test.
               Of all such pairs the rect reaches (rows_pair) the one nearest the limit
  inside, outside    far from the limit on either side
  nE%8=k       compact form: the largest fitting box whose counter words end k pixels into a word
"""
import numpy as np

import edge_box_ref as ref

SCALE = 1e-3
HALF_US = 25_000
T0_US = 1_000_000
T_REF_US = T0_US + HALF_US
FRAC_X, FRAC_Y = 0.37, 0.41
MIN_AWAY = 2e-3
MIN_EVENTS = 4
N_CUS = 256
EVENT_DTYPE = np.dtype([("x", "<i4"), ("y", "<i4"), ("sign", "<i4"), ("reserved", "<i4"), ("t_us", "<i8")])


class Unit:
    def __init__(self, rect, events, flow, box):
        self.rect, self.events, self.flow, self.box = rect, events, flow, box
        self.form = None  # set by the case: what the restatement says the launch does with the unit

    def array(self):
        ev = np.zeros(len(self.events), dtype=EVENT_DTYPE)
        for i, (x, y, t) in enumerate(self.events):
            ev[i] = (x, y, 1 if i % 2 else -1, 0, t)
        return ev

    def box_at(self, flow):
        taps, _ = ref.tap_bounds(self.events, self.rect, flow, SCALE)
        return ref.Box(*taps, 3 * self.rect[2], 3 * self.rect[3])


class Case:
    def __init__(self, name, regime, units, setup, env=None, grid=None, cls=None):
        self.name, self.regime, self.units, self.setup, self.env, self.grid = name, regime, units, setup, dict(env or {}), grid
        self.cls = cls
        for u in units:
            u.form = ref.form_of(u.box, setup)

    def __repr__(self):
        return self.name

    @property
    def ab(self):
        return bool(self.env)

    def ctx_kw(self):
        kw = dict(tv_weight=0.0, min_events=MIN_EVENTS, scale=SCALE, max_events=4096)
        if self.grid:
            kw.update(image_w=self.grid[0], image_h=self.grid[1], patch_w=self.grid[2], patch_h=self.grid[3])
        return kw

    def events(self):
        """(events, offsets, rects) for ebo_set_patches; a grid case: the time-sorted window in events"""
        arrs = [u.array() for u in self.units]
        ev = np.concatenate(arrs)
        if self.grid:
            return ev[np.argsort(ev["t_us"], kind="stable")], None, None
        offs = np.concatenate([[0], np.cumsum([len(a) for a in arrs])])
        return ev, offs, [u.rect for u in self.units]

    def flows(self):
        return np.array([u.flow for u in self.units])

    def eval_flows(self, u):
        """the flows at which the unit is evaluated against the oracle"""
        return [u.flow]

    def sums(self):
        """what ebo_edge_work_stats counts over the case's units"""
        b = [u.box for u in self.units]
        return dict(units=len(b), events=sum(len(u.events) for u in self.units), box_pixels=sum(x.npx for x in b),
                    eigen_pixels=sum(x.eigen_px for x in b), nms_windows=sum(x.windows for x in b))


# ---- steering one axis ----------------------------------------------------------------------------------------------------
def _axis(r0, rlen, lo, hi, frac):
    """(k, a, b): with the shift k + frac a late event at rect offset a has its tap at canvas coordinate lo and an early one
    at offset b at hi; None where no event inside the rect reaches both"""
    def tap(off, shift):
        return int(float(r0 + off) + shift) - r0 + rlen  # warp_event's truncation, for a coordinate below zero too
    for k in range(max(0, rlen - lo - 2, hi - 2 * rlen), min(hi - rlen, 2 * rlen - lo - 1) + 2):
        s = (float(HALF_US) * SCALE) * ((k + frac) / 25.0)  # tau * m, as warp_event forms it
        for a in (lo - rlen + k + 1, lo - rlen + k):
            for b in (hi - rlen - k, hi - rlen - k + 1):
                if 0 <= a < rlen and 0 <= b < rlen and tap(a, -s) == lo and tap(b, s) == hi:
                    return k, a, b
    return None


def _axis_pairs(r0, rlen, frac):
    """every (lo, hi) of centre taps inside the canvas that events inside the rect can span"""
    L3 = 3 * rlen
    return [(lo, hi) for lo in range(L3) for hi in range(lo, L3) if _axis(r0, rlen, lo, hi, frac)]


def make_unit(rect, taps, n_events, seed):
    """a unit of n_events events in rect whose centre taps span exactly taps = (xmin, xmax, ymin, ymax)"""
    rx, ry, rw, rh = rect
    xmin, xmax, ymin, ymax = taps
    kx, ax, bx = _axis(rx, rw, xmin, xmax, FRAC_X)
    ky, ay, by = _axis(ry, rh, ymin, ymax, FRAC_Y)
    flow = ((kx + FRAC_X) / 25.0, (ky + FRAC_Y) / 25.0)
    rng = np.random.default_rng(seed)
    early = [(rx + bx, ry + by, T0_US), (rx + bx, ry + (ay + by) // 2, T0_US)]
    late = [(rx + (ax + bx) // 2, ry + ay, T0_US + 2 * HALF_US), (rx + ax, ry + ay, T0_US + 2 * HALF_US)]
    mid, tries = [], 0
    while len(mid) < n_events - 4:
        tries += 1
        assert tries < 200000, "no event falls inside the wanted box"
        d = int(rng.integers(200, 3000)) * (1 if rng.random() < 0.5 else -1)
        x, y = rx + int(rng.integers(0, rw)), ry + int(rng.integers(0, rh))
        w = ref.warp(x, y, T_REF_US + d, T_REF_US, rect, flow, SCALE)
        if w is None or not (xmin <= w[0] <= xmax and ymin <= w[1] <= ymax):
            continue
        if min(abs(w[2] - round(w[2])), abs(w[3] - round(w[3]))) < MIN_AWAY:
            continue
        mid.append((x, y, T_REF_US + d))
    mid.sort(key=lambda e: e[2])
    events = early + mid + late
    got, away = ref.tap_bounds(events, rect, flow, SCALE)
    assert got == tuple(taps) and away >= MIN_AWAY, (got, taps, away)
    return Unit(rect, events, flow, ref.Box(*taps, 3 * rw, 3 * rh))


# ---- the boxes a rect can reach, and the ones at a limit -----------------------------------------------------------------------
class Reach:
    def __init__(self, rect):
        self.rect = rect
        self.W3, self.H3 = 3 * rect[2], 3 * rect[3]
        self.xs = _axis_pairs(rect[0], rect[2], FRAC_X)
        self.ys = _axis_pairs(rect[1], rect[3], FRAC_Y)
        self.xset, self.yset = set(self.xs), set(self.ys)
        # one pair of taps per distinct geometry of an axis, the most central one
        cols, rows = {}, {}
        for lo, hi in self.xs:
            b = ref.Box(lo, hi, 3, 9, self.W3, self.H3)
            cols.setdefault(b.bc, []).append((abs(lo + hi - (self.W3 - 1)), lo, hi))
        for lo, hi in self.ys:
            b = ref.Box(3, 9, lo, hi, self.W3, self.H3)
            rows.setdefault((b.br, b.iRows, b.qRows), []).append((abs(lo + hi - (self.H3 - 1)), lo, hi))
        self.cols = {k: min(v)[1:] for k, v in cols.items()}
        self.rows = {k: min(v)[1:] for k, v in rows.items()}

    def box(self, taps):
        return ref.Box(*taps, self.W3, self.H3)

    def boxes(self):
        for xp in self.cols.values():
            for yp in self.rows.values():
                yield self.box(xp + yp)

    def step(self, taps, axis, delta):
        """the taps one column / row further (delta = +-1) along an axis; None where the rect cannot reach such a box"""
        b0 = self.box(taps)
        lo, hi = taps[2 * axis], taps[2 * axis + 1]
        pairs = self.xset if axis == 0 else self.yset
        for cand in ((lo, hi + delta), (lo - delta, hi)):
            if cand not in pairs:
                continue
            t = list(taps)
            t[2 * axis], t[2 * axis + 1] = cand
            b = self.box(t)
            if (b.bc - b0.bc, b.br - b0.br) == ((delta, 0) if axis == 0 else (0, delta)):
                return tuple(t)
        return None


def limit_taps(reach, fits, slack=None, max_px=None):
    """{class: taps} of the boxes at the limit `fits` draws among the boxes of reach.  slack(box): the aliased forms' ints
    to spare in the byte test (negative: excess) and max_px their pixel limit, for the bytes_* and rows_* classes."""
    out = {}
    boxes = list(reach.boxes())
    fit = max((b for b in boxes if fits(b)), key=lambda b: (b.npx, -abs(b.bc - b.br), b.bc))
    out["fit"] = fit.taps
    for axis, tag in ((0, "c"), (1, "r")):
        for delta in (-1, 1):
            t = reach.step(fit.taps, axis, delta)
            if t is not None:
                out["fit_%s%+d" % (tag, delta)] = t
    overs = [out[k] for k in ("fit_c+1", "fit_r+1") if k in out and not fits(reach.box(out[k]))]
    if overs:
        out["over"] = min(overs, key=lambda t: reach.box(t).npx)
    else:
        out["over"] = min((b for b in boxes if not fits(b)), key=lambda b: (b.npx, b.bc)).taps
    if slack is not None:
        near = [b for b in boxes if slack(b) >= 0 and fits(b)]
        far = [b for b in boxes if slack(b) < 0 and b.npx <= max_px]
        if near and far:
            out["bytes_fit"] = min(near, key=lambda b: (slack(b), -b.npx, b.bc)).taps
            out["bytes_over"] = min(far, key=lambda b: (-slack(b), b.npx, b.bc)).taps
        pair = rows_pair(reach, fits, slack, max_px)
        if pair:
            out["rows_fit"], out["rows_over"] = pair
    return out


def rows_pair(reach, fits, slack, max_px):
    """(taps that fit, taps that do not): the same columns, the same box rows (clamped by the canvas on that side) and so the
    same pixels, one row of taps more -- iRows and qRows one more each -- across the byte test of edge_box_fits_alias.  Over
    the rect's whole reach of rows; of all such pairs the one with the least slack, then the least excess.  None if the
    rect reaches no such pair."""
    # the row pairs first (their geometry does not depend on the columns), then every width
    rows = []
    for lo, hi in reach.ys:
        g0 = reach.box((3, 9, lo, hi))
        for cand in ((lo - 1, hi), (lo, hi + 1)):
            if cand in reach.yset:
                g1 = reach.box((3, 9) + cand)
                if (g1.br, g1.iRows, g1.qRows) == (g0.br, g0.iRows + 1, g0.qRows + 1):
                    rows.append(((lo, hi), cand))
    best = None
    for xp in reach.cols.values():
        for y0, y1 in rows:
            b0, b1 = reach.box(xp + y0), reach.box(xp + y1)
            if b0.npx > max_px or not fits(b0) or fits(b1):
                continue
            key = (slack(b0), -slack(b1), -b0.npx, b0.bc, y1)
            if best is None or key < best[0]:
                best = (key, b0.taps, b1.taps)
    return best and best[1:]


def _alias_fits(cap_px, max_px, cnt4):
    """(fits(box), slack(box) in ints, max_px) of an aliased form"""
    return ((lambda b: ref.fits_alias(b, cap_px, max_px, cnt4)),
            (lambda b: ref.alias_cap_ints(cap_px, cnt4) - b.alias_ints(cnt4)), max_px)


def _central(reach, frac):
    """taps of a box over the middle `frac` of the canvas"""
    W3, H3 = reach.W3, reach.H3
    want_x = (int(W3 * (0.5 - frac / 2)), int(W3 * (0.5 + frac / 2)))
    want_y = (int(H3 * (0.5 - frac / 2)), int(H3 * (0.5 + frac / 2)))
    x = min(reach.xs, key=lambda p: abs(p[0] - want_x[0]) + abs(p[1] - want_x[1]))
    y = min(reach.ys, key=lambda p: abs(p[0] - want_y[0]) + abs(p[1] - want_y[1]))
    return x + y


def _full(reach):
    return (0, reach.W3 - 1, 0, reach.H3 - 1)


_REACH = {}


def reach_of(rect):
    if rect not in _REACH:
        _REACH[rect] = Reach(rect)
    return _REACH[rect]


# case name -> seed of its draw, where the default draw gives a Jacobian so small that its own curvature (no tie) moves it by
# more than 1e-6 of itself over a flow step of 1e-9 (the CPU test's bar for `no coin toss`)
SEEDS = {"e52/rows_over": 3}


def _seed(name):
    return SEEDS.get(name, sum(ord(c) * (i + 1) for i, c in enumerate(name)))


def _n_events(name):
    return 24 + _seed(name) % 17  # 24 .. 40


def _single(regime, cls, rect, taps, setup, env=None):
    name = "%s/%s" % (regime, cls)
    return Case(name, regime, [make_unit(rect, taps, _n_events(name), _seed(name))], setup, env, cls=cls)


RECT_A, RECT_C, RECT_D = (100, 80, 40, 22), (90, 70, 32, 30), (110, 90, 20, 20)
GRID_B = (52, 36, 21, 16)
RECTS_B = [(0, 0, 21, 16), (21, 0, 31, 16), (0, 16, 21, 20), (21, 16, 31, 20)]
ENV_E = {"52": {"EBO_EDGE_COMPACT": "1", "EBO_EDGE_COMPACT_KB": "52"}, "40": {"EBO_EDGE_COMPACT": "1", "EBO_EDGE_COMPACT_KB": "40"}}
ENV_SLICE = {"EBO_EDGE_COMPACT": "1", "EBO_EDGE_COMPACT_KB": "52", "EBO_EDGE_LDS_KB": "72"}
ENV_F = {"0": {"EBO_EDGE_LAYOUT": "0", "EBO_EDGE_LDS_KB": "48"}, "1": {"EBO_EDGE_LAYOUT": "1", "EBO_EDGE_LDS_KB": "48"}}
RECTS_MIX = [(110, 90, 20, 20), (30, 40, 20, 20), (170, 120, 20, 20)]

# the capacities the restatement must find for the regimes (tests/test_edge_fit_cases_cpu.py)
EXPECT_SETUP = {
    "a": dict(alias=True, cap_px=7715, max_lds_px=7424, block=768, has_slice=True, compact=False),
    "b": dict(alias=True, cap_px=3606, max_lds_px=5580, block=256, has_slice=True, compact=False),
    "c": dict(alias=False, cap_px=5510, max_lds_px=7424, block=768, has_slice=True, compact=False),
    "d": dict(alias=True, cap_px=3603, max_lds_px=3600, block=256, has_slice=False, compact=False),
    "e52": dict(alias=True, cap_px=3603, block=256, compact=True, compact_cap=2912, compact_max_px=3600, compact_list_cap=964),
    "e40": dict(alias=True, cap_px=3603, block=256, compact=True, compact_cap=2192, compact_max_px=3144, compact_list_cap=850),
    "f0": dict(alias=False, cap_px=1414, block=768, has_slice=True, compact=False),
    "f1": dict(alias=True, cap_px=1980, max_lds_px=3600, block=256, has_slice=True, compact=False),
}


def _limit_cases(regime, rect, setup, env):
    """the classes of one single-rect regime"""
    reach = reach_of(rect)
    if setup.compact:
        fits, slack, max_px = _alias_fits(setup.compact_cap, setup.compact_max_px, True)
    elif setup.alias:
        fits, slack, max_px = _alias_fits(setup.cap_px, setup.cs_stride, False)
    else:
        fits, slack, max_px = (lambda b: ref.fits_28(b, setup.cap_px)), None, None
    taps = limit_taps(reach, fits, slack, max_px)
    taps["inside"] = _central(reach, 0.1)
    if not fits(reach.box(_full(reach))):
        taps["outside"] = _full(reach)
    if setup.compact:
        boxes = [b for b in reach.boxes() if fits(b)]
        for k in (0, 1, 7):
            taps["nE%%8=%d" % k] = max((b for b in boxes if b.nE % 8 == k), key=lambda b: (b.npx, b.bc)).taps
    return [_single(regime, cls, rect, t, setup, env) for cls, t in sorted(taps.items())]


def _build():
    out = []
    # a: 20 B form, limited by maxLdsPx
    S = ref.launch_setup(40, 22, 20, 20, True, n_units=1, n_cus=N_CUS)
    out += _limit_cases("a", RECT_A, S, None)
    # c: 28 B form with a slice
    S = ref.launch_setup(32, 30, 20, 20, True, n_units=1, n_cus=N_CUS)
    out += _limit_cases("c", RECT_C, S, None)
    # d: nothing can spill
    S = ref.launch_setup(20, 20, 20, 20, True, n_units=1, n_cus=N_CUS)
    reach = reach_of(RECT_D)
    out.append(_single("d", "full_canvas", RECT_D, _full(reach), S))
    out.append(_single("d", "inside", RECT_D, _central(reach, 0.1), S))
    # b: a grid window; the corner unit at the limit, the regular units far inside
    S = ref.launch_setup(31, 20, 21, 16, False, n_units=5, n_cus=N_CUS)
    corner = RECTS_B[3]
    reach = reach_of(corner)
    fits, slack, max_px = _alias_fits(S.cap_px, S.cs_stride, False)
    taps = limit_taps(reach, fits, slack, max_px)
    taps["inside"] = _central(reach, 0.1)
    taps["outside"] = _full(reach)
    for cls, t in sorted(taps.items()):
        name = "b/%s" % cls
        units = [make_unit(r, _central(reach_of(r), 0.3), 12 + i, _seed(name) + i) for i, r in enumerate(RECTS_B[:3])]
        units.append(make_unit(corner, t, _n_events(name), _seed(name)))
        out.append(Case(name, "b", units, S, None, grid=GRID_B, cls=cls))
    # e: the compact form
    for kb in ("52", "40"):
        S = ref.launch_setup(20, 20, 20, 20, True, n_units=1, n_cus=N_CUS, env=ENV_E[kb])
        out += _limit_cases("e" + kb, RECT_D, S, ENV_E[kb])
    S = ref.launch_setup(20, 20, 20, 20, True, n_units=1, n_cus=N_CUS, env=ENV_SLICE)
    reach = reach_of(RECT_D)
    out.append(_single("e52", "deferred_to_slice", RECT_D, _full(reach), S, ENV_SLICE))
    S3 = ref.launch_setup(20, 20, 20, 20, True, n_units=3, n_cus=N_CUS, env=ENV_SLICE)
    fits, _, _ = _alias_fits(S3.compact_cap, S3.compact_max_px, True)
    lim = limit_taps(reach, fits)
    mix = [("fit", lim["fit"]), ("over", lim["over"]), ("outside", _full(reach))]
    for cls, order in (("mixed", (0, 1, 2)), ("mixed_reversed", (2, 1, 0))):
        units = []
        for i in order:
            u = make_unit(RECT_D, mix[i][1], _n_events("e52/" + mix[i][0]), _seed("e52/" + mix[i][0]))
            # the same unit, moved to its own rect
            dx, dy = RECTS_MIX[i][0] - RECT_D[0], RECTS_MIX[i][1] - RECT_D[1]
            ev = [(x + dx, y + dy, t) for x, y, t in u.events]
            units.append(Unit(RECTS_MIX[i], ev, u.flow, u.box))
        out.append(Case("e52/" + cls, "e52", units, S3, ENV_SLICE, cls=cls))
    # f: both layouts under a budget a 20x20 rect can exceed
    for lay in ("0", "1"):
        S = ref.launch_setup(20, 20, 20, 20, True, n_units=1, n_cus=N_CUS, env=ENV_F[lay])
        out += _limit_cases("f" + lay, RECT_D, S, ENV_F[lay])
    return out


CASES = _build()
CASE_IDS = [c.name for c in CASES]
BY_NAME = {c.name: c for c in CASES}

# classes whose unit (the last of the case) must be on the regime's LDS form / must have left it
FIT_CLASSES = ("fit", "fit_c-1", "fit_r-1", "bytes_fit", "rows_fit", "inside", "full_canvas", "nE%8=0", "nE%8=1", "nE%8=7")
OVER_CLASSES = ("over", "fit_c+1", "fit_r+1", "bytes_over", "rows_over", "outside", "deferred_to_slice")
LDS_FORM = {"a": ref.FORM_20, "b": ref.FORM_20, "c": ref.FORM_28, "d": ref.FORM_20, "e52": ref.FORM_COMPACT,
            "e40": ref.FORM_COMPACT, "f0": ref.FORM_28, "f1": ref.FORM_20}


# ---- g: claim pile-up on the compact form's 4-bit counters --------------------------------------------------------------------
# One isolated cluster of 16 events (taps within a few pixels): the brightest eigenvalue pixel lies at even canvas coordinates
# and is the argmax of all nine 5x5 windows that hold it (centres are even: three per axis), so its 4-bit field counts to 9.
# Placed so that the field is the last (p & 7 == 7) or the first (p & 7 == 0) of its counter word.  No window can claim the
# pixel next to it in its row (every window that holds x + 1 or x - 1 also holds x, which is brighter): the nearest claimed
# pixels, the flank of the same blob, lie two and four columns away in the same word.  (tests/test_edge_fit_cases_cpu.py finds
# the pixel and the claims with edge_box_ref.eigen_image / window_claims on the oracle's image.)
PILE_SPECS = [("g/p&7=7", (30, 32, 26, 27), 0, 7), ("g/p&7=0", (27, 29, 26, 28), 2, 0)]


def _pile_cases():
    S = ref.launch_setup(20, 20, 20, 20, True, n_units=1, n_cus=N_CUS, env=ENV_E["52"])
    out = []
    for name, taps, seed, field in PILE_SPECS:
        c = Case(name, "g", [make_unit(RECT_D, taps, 16, seed)], S, ENV_E["52"], cls="pile")
        c.field = field
        out.append(c)
    return out


PILE_CASES = _pile_cases()


# ---- h: the device-resident solve across the limit ----------------------------------------------------------------------------
# Eight dots drift through a 20x20 rect at SOLVE_V px/ms; an event wherever a dot, sampled every 5 ms, is inside the rect.  At
# zero flow (where every solve starts) the box is the rect's extent plus 22: 42 x 42.  The per-patch LM, started with a small
# trust region (initial_radius 1e-6: the first step is a fraction of a pixel per millisecond, not thousands), ends near the
# drift, where the early and late events have moved by up to 7 pixels and the box has grown to 48 x 46.  EBO_EDGE_LDS_KB puts
# the capacity between the two on either layout.
SOLVE_V = (-0.25, 0.15)
SOLVE_RECT = (0, 0, 20, 20)
SOLVE_OPTS = dict(max_num_iterations=8, initial_radius=1e-6)
SOLVE_END = (-0.28483776, 0.14038276)  # the oracle's solution (orc.compensate_events_contrast, SOLVE_OPTS), to 1e-8
ENV_H = {"0": {"EBO_EDGE_LAYOUT": "0", "EBO_EDGE_LDS_KB": "64"}, "1": {"EBO_EDGE_LAYOUT": "1", "EBO_EDGE_LDS_KB": "40"}}


def solve_events():
    rng = np.random.default_rng(0)
    rx, ry, rw, rh = SOLVE_RECT
    ev = []
    for _ in range(8):
        p = (rng.uniform(rx - 6, rx + rw + 6), rng.uniform(ry - 4, ry + rh + 4))
        t = -25.0 + rng.uniform(0, 5.0)
        while t <= 25.0:
            x, y = p[0] + SOLVE_V[0] * t, p[1] + SOLVE_V[1] * t
            if rx <= x < rx + rw and ry <= y < ry + rh:
                ev.append((int(x), int(y), T_REF_US + int(round(t * 1000))))
            t += 5.0
    ev.sort(key=lambda e: e[2])
    # the first and the last event pin the reference time
    return [(ev[0][0], ev[0][1], T0_US)] + ev[1:-1] + [(ev[-1][0], ev[-1][1], T0_US + 2 * HALF_US)]


def _solve_cases():
    out = []
    for lay in ("0", "1"):
        S = ref.launch_setup(20, 20, 20, 20, True, n_units=1, for_solve=True, n_cus=N_CUS, env=ENV_H[lay])
        u = Unit(SOLVE_RECT, solve_events(), SOLVE_END, None)
        u.box = u.box_at(SOLVE_END)
        u.box_start = u.box_at((0.0, 0.0))
        c = Case("h/layout" + lay, "h", [u], S, ENV_H[lay], cls="solve")
        c.form_start = ref.form_of(u.box_start, S)
        out.append(c)
    return out


SOLVE_CASES = _solve_cases()
