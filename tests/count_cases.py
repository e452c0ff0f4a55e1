"""The inputs of the count-image edge tests (tests/test_gpu_count_edges.py), shared with the CPU test that makes their
teeth a checked condition (tests/test_count_cases_cpu.py): events laddered around rounding ties, events that land on the
seams of tiles and bands, pile-ups at the limits of the packed 16-bit counters, and k_count_tiles's safe16 rule at its
edge.  Two numpy restatements go with them: `positions`, the reference's f64 position and round-half-away pixel, and
`pretest`, the float32 pre-test of count_target / count_hit_uniform (csrc/ebo_kernels.hip, csrc/ebo_count.inc) with its
three constants as parameters.  Every expected image of the tests comes from the oracle, never from here.  All
deterministic.  A plain module, not a conftest."""
import functools

import numpy as np

from orc import EVENT_DTYPE

SCALE = 1e-3
# the shipped constants of the float pre-test (kSureBase, and the two error terms of count_target)
SURE_BASE, C_DISP, C_POS = 0.499999, 4e-7, 6e-8
# weakened variants of the pre-test: which of them the cases catch is measured by the CPU test
VARIANTS = {
    "shipped": (SURE_BASE, C_DISP, C_POS),
    "no displacement term": (SURE_BASE, 0.0, C_POS),
    "no position term": (SURE_BASE, C_DISP, 0.0),
    "no terms": (SURE_BASE, 0.0, 0.0),
    "base 0.5": (0.5, C_DISP, C_POS),
    "displacement term halved": (SURE_BASE, C_DISP / 2, C_POS),
    "position term halved": (SURE_BASE, C_DISP, C_POS / 2),
    "slack halved": (0.4999995, C_DISP, C_POS),
}

# the ladder: distance of the f64 position from a half-integer ("ulp": the neighbouring double of the tie)
RUNGS = ["ulp", 1e-12, 1e-9, 1e-8, 1e-7, 4e-7, 1e-6, 2e-6, 1e-5, 1e-4]
# displacement classes by |displacement| in pixels; the last two need a sensor 16383 pixels long on that axis
CLASSES = {"0.5": (0.4, 1.6), "3": (2.0, 5.0), "40": (30.0, 60.0), "1000": (800.0, 1500.0), "4000+": (4000.0, 1e9)}
_CLASS_N = {"0.5": (0, 0), "3": (2, 4), "40": (30, 59), "1000": (800, 1499), "4000+": (4000, 16300)}
# t_ref - t in us: small, a typical window, and beyond 2^24 where float(dtw) is inexact (odd values), both signs
DTW_FLAVOURS = [37, -211, 20011, -33333, (1 << 24) + 4321, -((1 << 24) + 1235)]
HALF_SPAN = (1 << 24) + 200000  # the anchors' distance from the reference time

# Shapes of the store-form tests: W, H, patch, EBO_COUNT_LDS_KB per implementation -> the plan pinned in
# tests/cpp/count_plan_test.cpp.  W * H is odd (a second window starts at an odd pixel offset: 8 mod 16 bytes); with
# these LDS sizes the bands have an odd pixel count and an aligned start (band 0, even bands) or an odd start (odd bands).
STORE_SHAPE = dict(w=61, h=43, pw=20, ph=21)
STORE_LDS_KB = {1: 3, 2: 3, 3: 3, 4: 2}  # bands of 25, 21, 25 and 15 rows of 61 pixels


def make_events(x, y, t_us):
    ev = np.zeros(len(x), dtype=EVENT_DTYPE)
    ev["x"], ev["y"], ev["t_us"], ev["sign"] = x, y, t_us, 1
    return ev


def ref_time(t_first, t_last):
    """The window's reference time (feature_detector.cpp:305-306): the mean of the first and last stamp through a
    double and an int32."""
    return int(np.int32(int(float(int(t_first) + int(t_last)) * 0.5)))


def grid(w, h, pw, ph):
    return w // pw, h // ph


def patch_of(x, y, geom):
    """Index of the grid patch of the final loop (:436-441): C division, clamped into the grid on both sides."""
    w, h, pw, ph = geom
    npx, npy = grid(*geom)
    bx = np.clip(np.trunc(np.asarray(x) / pw).astype(np.int64), 0, npx - 1)
    by = np.clip(np.trunc(np.asarray(y) / ph).astype(np.int64), 0, npy - 1)
    return by * npx + bx


def round_half_away(f):
    """std::round on doubles below 2^52: f - trunc(f) is exact."""
    t = np.trunc(f)
    return t + np.where(np.abs(f - t) >= 0.5, np.sign(f), 0.0)


def positions(ev, t_ref, scale, geom, flows=None, field=None):
    """The reference's f64 position x + (dtw * scale) * m, in that operation order, of every event of one window, and its
    round-half-away-from-zero pixel.  flows [P][2] f64 (the warped image), field [h][w][2] float32 (the field image), or
    neither (the un-warped image).  -> fx, fy, nx, ny (float64), live (the event is counted by the reference at all:
    inside the sensor in field mode, position convertible to int)."""
    w, h, pw, ph = geom
    x, y = ev["x"].astype(np.int64), ev["y"].astype(np.int64)
    live = np.ones(len(ev), dtype=bool)
    m0 = m1 = np.zeros(len(ev))
    if flows is not None:
        fl = np.asarray(flows, dtype=np.float64).reshape(-1, 2)
        p = patch_of(x, y, geom)
        m0, m1 = fl[p, 0], fl[p, 1]
    elif field is not None:
        live = (x >= 0) & (x < w) & (y >= 0) & (y < h)
        f = np.asarray(field, dtype=np.float32).reshape(h, w, 2)
        xc, yc = np.clip(x, 0, w - 1), np.clip(y, 0, h - 1)
        m0, m1 = f[yc, xc, 0].astype(np.float64), f[yc, xc, 1].astype(np.float64)
    a = (t_ref - ev["t_us"]).astype(np.float64) * scale
    with np.errstate(invalid="ignore", over="ignore"):
        fx, fy = x + a * m0, y + a * m1
        live = live & (np.abs(fx) < 1073741824.0) & (np.abs(fy) < 1073741824.0)
    return fx, fy, round_half_away(fx), round_half_away(fy), live


def image_of(nx, ny, live, w, h):
    """The count image of rounded positions: one count per event inside the image."""
    inside = live & (nx >= 0) & (nx < w) & (ny >= 0) & (ny < h)
    at = (ny[inside] * w + nx[inside]).astype(np.int64)
    return np.bincount(at, minlength=w * h).astype(np.float64).reshape(h, w)


def case_image(case, k):
    """`positions` + `image_of` on window k of a case: the restatement's image, to be compared with the oracle's."""
    ev = window_events(case, k)
    geom = (case["w"], case["h"], case["pw"], case["ph"])
    flows = case["flows"][k] if case.get("flows") is not None else None
    field = case["field"][k] if case.get("field") is not None else None
    if len(ev) == 0:
        return np.zeros((case["h"], case["w"]))
    t_ref = ref_time(ev["t_us"][0], ev["t_us"][-1])
    fx, fy, nx, ny, live = positions(ev, t_ref, case["scale"], geom, flows, field)
    return image_of(nx, ny, live, case["w"], case["h"])


def window_events(case, k):
    return case["ev"][int(case["offsets"][k]):int(case["offsets"][k + 1])]


def float_position(c, dtw, m, scale):
    """The float32 position of one axis and its displacement, operation by operation as count_target computes them."""
    f = np.float32
    dtw = np.asarray(dtw, dtype=np.int64).astype(np.int32)
    with np.errstate(invalid="ignore", over="ignore"):
        prod = dtw.astype(f) * f(scale)
        p = prod * np.asarray(m, dtype=np.float64).astype(f)
        return np.asarray(c).astype(f) + p, p


def pretest(c, dtw, m, scale, base=SURE_BASE, c_disp=C_DISP, c_pos=C_POS, unit=None):
    """The float32 pre-test of one axis, as the kernels compute it (the file is built with -ffp-contract=off: every
    float operation rounds once, as numpy's do).  c: integer coordinate, dtw: t_ref - t (int32), m: the f64 flow (a float32
    field value converts exactly).  unit=None: count_target's per-event test; unit=(max_dt, extent):
    count_hit_uniform's test against count_unit_tolerance(max_dt, scale, m, extent).
    -> (the float pixel rintf gives, sure)."""
    f = np.float32
    m = np.asarray(m, dtype=np.float64)
    v, p = float_position(c, dtw, m, scale)
    with np.errstate(invalid="ignore", over="ignore"):
        r = np.rint(v)
        if unit is None:
            thr = (f(base) - f(c_disp) * np.abs(p)) - f(c_pos) * np.abs(v)
        else:
            max_dt, extent = unit
            reach = (np.asarray(max_dt, dtype=np.float64) * abs(scale) * np.abs(m)).astype(f) * f(1.000001)
            thr = (f(base) - f(c_disp) * reach) - f(c_pos) * ((f(extent) + reach) + f(1.0))
        sure = np.abs(v - r) < thr
    return r.astype(np.float64), sure


def misrounds(case, consts, per_unit=False):
    """Events of a case that the pre-test with these constants calls sure on both axes and rounds to another pixel than
    the reference.  per_unit: k_count_tiles's form (warped cases only) -> (misrounded, sure, not sure)."""
    geom = (case["w"], case["h"], case["pw"], case["ph"])
    bad = n_sure = n_not = 0
    for k in range(len(case["offsets"]) - 1):
        ev = window_events(case, k)
        t_ref = ref_time(ev["t_us"][0], ev["t_us"][-1])
        flows = case["flows"][k] if case.get("flows") is not None else None
        field = case["field"][k] if case.get("field") is not None else None
        fx, fy, nx, ny, live = positions(ev, t_ref, case["scale"], geom, flows, field)
        dtw = t_ref - ev["t_us"]
        if flows is not None:
            p = patch_of(ev["x"], ev["y"], geom)
            m0, m1 = flows[p, 0], flows[p, 1]
        else:
            f = field.reshape(case["h"], case["w"], 2)
            xc, yc = np.clip(ev["x"], 0, case["w"] - 1), np.clip(ev["y"], 0, case["h"] - 1)
            m0, m1 = f[yc, xc, 0].astype(np.float64), f[yc, xc, 1].astype(np.float64)
        ux = uy = None
        if per_unit:
            p = patch_of(ev["x"], ev["y"], geom)
            max_dt = np.zeros(p.max() + 1, dtype=np.int64)
            np.maximum.at(max_dt, p, np.abs(dtw))
            ux, uy = (max_dt[p], case["w"]), (max_dt[p], case["h"])
        rx, sx = pretest(ev["x"], dtw, m0, case["scale"], *consts, unit=ux)
        ry, sy = pretest(ev["y"], dtw, m1, case["scale"], *consts, unit=uy)
        sure = sx & sy & live
        bad += int((sure & ((rx != nx) | (ry != ny))).sum())
        n_sure += int(sure.sum())
        n_not += int((live & ~sure).sum())
    return bad, n_sure, n_not


def tie_distance(f):
    """Signed distance of a position from its nearest half-integer, and that half-integer."""
    tie = np.floor(f) + 0.5
    return f - tie, tie


def ladder_coverage(case):
    """The (axis, displacement class, rung, side) combinations a tie case really holds after the f64 evaluation, and
    the signs of the positions of its exact ties per axis.  rung: "exact", "ulp" or a distance d met within [d/2, 2d]."""
    geom = (case["w"], case["h"], case["pw"], case["ph"])
    got, exact_signs = set(), set()
    for k in range(len(case["offsets"]) - 1):
        ev = window_events(case, k)
        t_ref = ref_time(ev["t_us"][0], ev["t_us"][-1])
        flows = case["flows"][k] if case.get("flows") is not None else None
        field = case["field"][k] if case.get("field") is not None else None
        fx, fy, _, _, live = positions(ev, t_ref, case["scale"], geom, flows, field)
        for axis, f, c in (("x", fx, ev["x"]), ("y", fy, ev["y"])):
            disp = np.abs(f - c)
            dist, tie = tie_distance(f)
            near = live & (np.abs(dist) <= 2e-4) & (disp > 0)
            for cls, (lo, hi) in CLASSES.items():
                sel = near & (disp >= lo) & (disp < hi)
                if not sel.any():
                    continue
                d, t, ff = dist[sel], tie[sel], f[sel]
                for s in np.unique(np.sign(t[d == 0])):
                    got.add((axis, cls, "exact", 0))
                    exact_signs.add((axis, int(s)))
                for side in (-1, 1):
                    if (ff == np.nextafter(t, side * np.inf)).any():
                        got.add((axis, cls, "ulp", side))
                    for rung in RUNGS[1:]:
                        if ((d * side >= rung / 2) & (d * side <= rung * 2)).any():
                            got.add((axis, cls, rung, side))
    return got, exact_signs


# ---- ties ------------------------------------------------------------------------------------------------------------
def _solve_m(c, a, target, tie, side, f32=False):
    """A flow m whose f64 evaluation fl(c + fl(a * m)) lies on `side` of the tie (0: on it) and as close to the target as
    stepping m by ulps allows.  -> (m, position) or None."""
    m0 = (target - c) / a
    if f32:
        cand = [np.float32(m0)]
        for _ in range(3):
            cand = [np.nextafter(cand[0], np.float32(-np.inf))] + cand + [np.nextafter(cand[-1], np.float32(np.inf))]
        cand = np.array(cand, dtype=np.float32).astype(np.float64)
    else:
        cand = (np.array([m0]).view(np.int64) + np.arange(-48, 49)).view(np.float64)
    pos = c + a * cand
    ok = (pos == tie) if side == 0 else ((pos - tie) * side > 0)
    if not ok.any():
        return None
    err = np.where(ok, np.abs(pos - target), np.inf)
    i = int(np.argmin(err))
    return float(cand[i]), float(pos[i])


def _signed_rungs():
    out = [(0, 0.0)]
    for r in RUNGS:
        out += [(-1, r), (1, r)]
    return out


def _tie_specs(axes, classes, repeat=1):
    """One spec per rung x side x axis x class x placement.  Placements: the event moves up or down the axis and stays
    inside the image ("up", "down"), lands at -0.5 ("low": half-away drops it, rintf would keep it at pixel 0), or at
    extent - 0.5 ("high")."""
    specs = []
    for _ in range(repeat):
        for places in (("low", "high"), ("up", "down")):  # the placements that need a particular patch first
            for axis in axes:
                for cls in classes:
                    for place in places:
                        for side, rung in _signed_rungs():
                            specs.append(dict(axis=axis, cls=cls, place=place, side=side, rung=rung))
    return specs


def _place(spec, lo, hi, extent, k):
    """The designated coordinate c, the integer part n of the displacement and its sign for a spec in a patch [lo, hi]
    of the axis, whose events lie on c, c + 1 ... c + span (c - 1 ... for "high"); None if the spec does not fit there.
    k varies n inside the class."""
    n_lo, n_hi = _CLASS_N[spec["cls"]]
    n_hi = min(n_hi, extent - 8)
    span = min(3, hi - lo)
    if n_hi < n_lo:
        return None
    n = n_lo + k % (n_hi - n_lo + 1)
    place = spec["place"]
    if place == "up":
        return (lo, n, 1) if lo + span + n + 1 <= extent - 1 else None
    if place == "down":
        return (lo, n, -1) if lo - n - 1 >= 0 else None
    if place == "low":
        c = max(lo, n_lo)
        return (c, c, -1) if c <= min(hi - span, n_hi) else None
    c = min(hi, extent - 1 - n_lo)
    return (c, extent - 1 - c, 1) if c >= max(lo + span, extent - 1 - n_hi) else None


def _target(c, n, s, side, rung):
    tie = c + s * (n + 0.5)
    if side == 0:
        return tie, tie
    if rung == "ulp":
        return tie, float(np.nextafter(tie, side * np.inf))
    return tie, tie + side * rung


def _window_times(k):
    base = 1_000_000 + 1000 * k
    return base, base + 2 * HALF_SPAN  # first and last stamp: t_ref = base + HALF_SPAN


def _ranges(extent, pitch):
    n = extent // pitch
    return [(i * pitch, (i + 1) * pitch - 1 if i < n - 1 else extent - 1) for i in range(n)]


def _build_ties(w, h, pw, ph, axes, classes, n_windows, field, name, repeat=1):
    geom = (w, h, pw, ph)
    npx, npy = grid(*geom)
    P = npx * npy
    xr, yr = _ranges(w, pw), _ranges(h, ph)
    anchor_patch = P - 1
    free = np.ones((n_windows, P), dtype=bool)
    free[:, anchor_patch] = False
    used_px = [set() for _ in range(n_windows)]
    flows = np.zeros((n_windows, P, 2))
    fld = np.zeros((n_windows, h, w, 2), dtype=np.float32) if field else None
    evs = [[] for _ in range(n_windows)]
    dropped = 0
    for idx, spec in enumerate(_tie_specs(axes, classes, repeat)):
        ax = 0 if spec["axis"] == "x" else 1
        main, cross = (xr, yr) if ax == 0 else (yr, xr)
        extent = w if ax == 0 else h
        fits = []
        for bi, (lo, hi) in enumerate(main):
            got = _place(spec, lo, hi, extent, idx + bi)
            if got is not None:
                fits.append((bi, got))
        slot = None
        for kw in range(n_windows):
            k = (kw + idx) % n_windows
            for j in range(len(fits)):
                bi, got = fits[(j + idx) % len(fits)]
                for ci0 in range(len(cross)):
                    ci = (ci0 + idx) % len(cross)
                    p = (ci * npx + bi) if ax == 0 else (bi * npx + ci)
                    if free[k, p]:
                        slot = (k, p, ci, bi, got)
                        break
                if slot:
                    break
            if slot:
                break
        if slot is None:
            dropped += 1
            continue
        k, p, ci, bi, (c, n, s) = slot
        free[k, p] = False
        t_ref = _window_times(k)[0] + HALF_SPAN
        step = -1 if spec["place"] == "high" else 1
        n_ev = 1 + min(3, main[bi][1] - main[bi][0])
        clo, chi = cross[ci]
        cc = clo + idx % (chi - clo + 1)
        dtw = DTW_FLAVOURS[idx % len(DTW_FLAVOURS)]
        tie, target = _target(c, n, s, spec["side"], spec["rung"])
        want_exact = spec["side"] == 0 or spec["rung"] == "ulp"
        if not field:
            best = None
            # From 1e-7 up, on the long axes: of 256 neighbouring times, the one whose FLOAT position errs farthest
            # towards the other side of the tie -- a pre-test that trusts the float too far then rounds it wrongly.
            hostile = not want_exact and spec["rung"] >= 1e-7 and spec["cls"] in ("1000", "4000+")
            worst = -np.inf
            for _ in range(256 if hostile else 64):
                got = _solve_m(c, dtw * SCALE, target, tie, spec["side"])
                if hostile:
                    if got is not None:
                        err = float(float_position(c, dtw, got[0], SCALE)[0]) - got[1]
                        if -spec["side"] * err > worst:
                            worst, best = -spec["side"] * err, (dtw, got)
                else:
                    if got is not None and (best is None or abs(got[1] - target) < abs(best[1][1] - target)):
                        best = (dtw, got)
                    if best is not None and (not want_exact or best[1][1] == target):
                        break
                dtw += 2 if dtw > 0 else -2
            assert best is not None, spec
            dtw, (m, _) = best
            flows[k, p, ax] = m
            for j in range(n_ev):
                xy = (c + j * step, cc) if ax == 0 else (cc, c + j * step)
                evs[k].append((xy[0], xy[1], t_ref - dtw))
        else:
            # a float32 flow: one event per pixel, each with a time of its own chosen so that the product meets the target
            for j in range(n_ev):
                cj = c + j * step
                xy = (cj, cc) if ax == 0 else (cc, cj)
                if xy in used_px[k]:
                    continue
                tie_j = tie + j * step
                target_j = target + j * step if spec["rung"] != "ulp" else float(np.nextafter(tie_j, spec["side"] * np.inf))
                if spec["side"] == 0:
                    # an exact tie: dtw = 1000 * 2^e us, so that dtw * scale is a power of two and m a short float
                    e = [0, 3, 14][idx % 3]
                    d = (1000 << e) * (1 if dtw > 0 else -1)
                    assert d * SCALE == float(np.sign(d)) * (1 << e)
                    got = _solve_m(cj, d * SCALE, target_j, tie_j, 0, f32=True)
                else:
                    # (the wide search for the spec's first event only: the others land where the same search, cut
                    # short, leaves them)
                    span = 1 << (16 if j == 0 and (spec["rung"] == "ulp" or spec["rung"] < 1e-7) else 11)
                    ds = dtw + np.arange(span) * (1 if dtw > 0 else -1)
                    a = ds * SCALE
                    got, d = None, 0
                    m32 = ((target_j - cj) / a).astype(np.float32)
                    for mm in (m32, np.nextafter(m32, np.float32(np.inf)), np.nextafter(m32, np.float32(-np.inf))):
                        pos = cj + a * mm.astype(np.float64)
                        err = np.where((pos - tie_j) * spec["side"] > 0, np.abs(pos - target_j), np.inf)
                        i = int(np.argmin(err))
                        if np.isfinite(err[i]) and (got is None or err[i] < abs(got[1] - target_j)):
                            got, d = (float(mm[i]), float(pos[i])), int(ds[i])
                if got is None:
                    continue
                used_px[k].add(xy)
                fld[k, xy[1], xy[0], ax] = got[0]
                evs[k].append((xy[0], xy[1], t_ref - d))
    # the anchors: first and last stamp of every window, in a patch of their own whose flow is zero
    ev_all, offsets = [], [0]
    ax0, ay0 = xr[anchor_patch % npx][0], yr[anchor_patch // npx][0]
    for k in range(n_windows):
        t0, t1 = _window_times(k)
        rows = sorted(evs[k], key=lambda r: r[2])
        rows = [(ax0, ay0, t0)] + rows + [(ax0 + 1, ay0, t1)]
        a = np.array(rows, dtype=np.int64)
        ev_all.append(make_events(a[:, 0], a[:, 1], a[:, 2]))
        offsets.append(offsets[-1] + len(rows))
    return dict(name=name, w=w, h=h, pw=pw, ph=ph, scale=SCALE, ev=np.concatenate(ev_all),
                offsets=np.array(offsets, dtype=np.uint64), flows=None if field else flows, field=fld, axes=axes,
                classes=classes, dropped=dropped)


# sensors of the tie cases: `small` has odd sides (extent - 0.5 is a tie rintf rounds DOWN into the image), `wide` and
# `tall` the 16383-pixel axis the large displacements need, `c2` BASELINE's 240 x 180 in 30 x 22 patches for the batches
# the shipped library plans by itself (tiles from 22 windows, the whole-window LDS image in field mode from 64), `fine`
# the same sensor in 3 x 3 patches (4800 unit headers do not fit a tile workgroup: unit waves from 32 windows)
_TIE_SENSORS = {
    "small": dict(w=241, h=181, pw=8, ph=6, axes=("x", "y"), classes=("0.5", "3", "40"), n_windows=3),
    "wide": dict(w=16383, h=8, pw=32, ph=4, axes=("x",), classes=("1000", "4000+"), n_windows=2),
    "tall": dict(w=8, h=16383, pw=4, ph=32, axes=("y",), classes=("1000", "4000+"), n_windows=2),
    "c2": dict(w=240, h=180, pw=30, ph=22, axes=("x", "y"), classes=("0.5", "3", "40"), n_windows=24, repeat=2),
    "c2x64": dict(w=240, h=180, pw=30, ph=22, axes=("x", "y"), classes=("0.5", "3", "40"), n_windows=64, repeat=2),
    "fine": dict(w=240, h=180, pw=3, ph=3, axes=("x", "y"), classes=("0.5", "3", "40"), n_windows=32, repeat=2),
}
TIE_SENSORS = tuple(_TIE_SENSORS)


@functools.lru_cache(maxsize=None)
def ties_warped(sensor):
    """Per-patch flows whose f64 evaluation puts the events of the patch at k + 0.5 + delta: every rung of the ladder on
    both sides, both axes, every displacement class the sensor admits, positions from -0.5 to extent - 0.5."""
    return _build_ties(field=False, name="ties_warped " + sensor, **_TIE_SENSORS[sensor])


@functools.lru_cache(maxsize=None)
def ties_field(sensor):
    """The same ladder with a float32 field: every event's own pixel carries its flow, and its own time brings the
    product to the target below the float32 grid of the flow."""
    return _build_ties(field=True, name="ties_field " + sensor, **_TIE_SENSORS[sensor])


def field_rung_reachable(cls, rung):
    """What a float32 flow times an integer time in us can meet.  Exact ties are constructed (a power-of-two time, a short
    flow).  Otherwise the product moves in steps of |displacement| x 6e-8 with the flow, and only the choice of the time
    fills the gaps: of the 65536 times the builder tries, about 65536 x 1.5 d / (|displacement| x 6e-8) land within
    [d / 2, 2 d] of the target -- several at d = 1e-9 up to 1500 pixels, at 1e-8 up to 16000; a handful of chances in a
    thousand at 1e-12 or at the neighbouring double."""
    if rung == "ulp":
        return False
    return rung >= (1e-8 if cls == "4000+" else 1e-9)


# ---- seams -----------------------------------------------------------------------------------------------------------
SEAM_DELTA = 1e-9


@functools.lru_cache(maxsize=None)
def seams(tile_w, tile_h, n_windows=0, w=240, h=180, pw=30, ph=22):
    """Events on the corners of their patches, at the unit's largest |dt|, whose flows land them exactly on the last
    column (row) before and the first after every seam of a tile pitch tile_w x tile_h (tile_w = 0: full-width bands), from
    patches at least one and at least two tiles away, on both sides -- and at the seam's tie (seam - 0.5) exactly and
    SEAM_DELTA on either side of it.  Two interior events per patch carry smaller |dt|.  The case has as many windows as
    the specs need at one x and one y spec per patch; n_windows asks for more (the first ones again, with the other sign
    of dt), for a plan that depends on the batch size."""
    geom = (w, h, pw, ph)
    npx, npy = grid(*geom)
    P = npx * npy
    xr, yr = _ranges(w, pw), _ranges(h, ph)
    anchor_patch = P - 1

    def axis_specs(extent, pitch, ranges):
        out = []
        if not pitch:
            return out
        for j in range(1, (extent + pitch - 1) // pitch):
            b = j * pitch  # first column of tile j; the seam's tie is b - 0.5
            for what in ("last", "first", "tie-", "tie", "tie+"):
                for direction in (1, -1):
                    for hops in (1, 2):
                        # the source corner: the far end of a patch that lies `hops` tile pitches (or more) before the
                        # seam; the nearest patch on that side where the image has none that far
                        if direction == 1:
                            srcs = [hi for lo, hi in ranges if hi < b - hops * pitch] or [hi for lo, hi in ranges if hi < b - 1]
                            src = max(srcs) if srcs else None
                        else:
                            srcs = [lo for lo, hi in ranges if lo >= b + hops * pitch] or [lo for lo, hi in ranges if lo > b]
                            src = min(srcs) if srcs else None
                        if src is not None:
                            out.append((b, what, src))
        return out

    def target_of(b, what):
        tie = b - 0.5
        return {"last": (b - 1.0, None, 0), "first": (float(b), None, 0), "tie": (tie, tie, 0),
                "tie-": (tie - SEAM_DELTA, tie, -1), "tie+": (tie + SEAM_DELTA, tie, 1)}[what]

    xs, ys = axis_specs(w, tile_w, xr), axis_specs(h, tile_h, yr)
    # a patch hosts one x spec (its column of patches fixes the source corner) and one y spec
    windows = []  # per window: {patch: [xspec or None, yspec or None]}

    def host(spec, ax):
        b, what, src = spec
        ranges = xr if ax == 0 else yr
        bi = [i for i, (lo, hi) in enumerate(ranges) if src in (lo, hi)][0]
        n_cross = npy if ax == 0 else npx
        for win in windows + [None]:
            if win is None:
                win = {}
                windows.append(win)
            for ci in range(n_cross):
                p = ci * npx + bi if ax == 0 else bi * npx + ci
                if p == anchor_patch:
                    continue
                cell = win.setdefault(p, [None, None])
                if cell[ax] is None:
                    cell[ax] = spec
                    return

    for s in xs:
        host(s, 0)
    for s in ys:
        host(s, 1)
    for k in range(len(windows), n_windows):
        windows.append(windows[k % len(windows)] if (k // len(windows)) % 2 == 0 else windows[-1 - k % len(windows)])
    n_windows = len(windows)
    flows = np.zeros((n_windows, P, 2))
    ev_all, offsets = [], [0]
    for k, win in enumerate(windows):
        t0, t1 = 1_000_000 + 1000 * k, 1_000_000 + 1000 * k + 60000
        t_ref = ref_time(t0, t1)
        rows = []
        for p, cell in sorted(win.items()):
            (xlo, xhi), (ylo, yhi) = xr[p % npx], yr[p // npx]
            dtw = (20011 + 2 * (p % 7)) * (1 if (p + k) % 2 else -1)  # the corners' dt: the unit's largest
            for ax, spec in enumerate(cell):
                if spec is None:
                    continue
                b, what, src = spec
                target, tie, side = target_of(b, what)
                got = None
                for _ in range(64):
                    if tie is None:  # an integer position: the "tie" to meet exactly is the pixel itself
                        got = _solve_m(src, dtw * SCALE, target, target, 0)
                    else:
                        got = _solve_m(src, dtw * SCALE, target, tie, side)
                    if got is not None:
                        break
                    dtw += 2 if dtw > 0 else -2
                assert got is not None, spec
                flows[k, p, ax] = got[0]
            for cx in (xlo, xhi):
                for cy in (ylo, yhi):
                    rows.append((cx, cy, t_ref - dtw))
            rows.append((xlo + 1, ylo + 1, t_ref - dtw // 2))
            rows.append((xhi - 1, yhi - 1, t_ref + dtw // 3))
        rows.sort(key=lambda r: r[2])
        ax0, ay0 = xr[anchor_patch % npx][0], yr[anchor_patch // npx][0]
        rows = [(ax0, ay0, t0)] + rows + [(ax0 + 1, ay0, t1)]
        a = np.array(rows, dtype=np.int64)
        ev_all.append(make_events(a[:, 0], a[:, 1], a[:, 2]))
        offsets.append(offsets[-1] + len(rows))
    return dict(name="seams %dx%d" % (tile_w, tile_h), w=w, h=h, pw=pw, ph=ph, scale=SCALE, ev=np.concatenate(ev_all),
                offsets=np.array(offsets, dtype=np.uint64), flows=flows, field=None, tile_w=tile_w, tile_h=tile_h)


def seam_lines(extent, pitch):
    """The last column (row) before and the first after every seam of a pitch."""
    out = []
    for j in range(1, (extent + pitch - 1) // pitch if pitch else 0):
        out += [j * pitch - 1, j * pitch]
    return out


# ---- pile-ups --------------------------------------------------------------------------------------------------------
PILE = dict(w=64, h=48, pw=16, ph=12, src=(5, 3), dst=(37, 29))
PILE_VARIANTS = [(65535, 0, 0), (65535, 0, 5), (65535, 1, 0), (65536, 0, 0), (65536, 1, 3), (70000, 1, 0)]


@functools.lru_cache(maxsize=None)
def pileup(mode, n, parity, extra=0):
    """One window whose n events (the two anchors that fix t_ref included) land on ONE pixel, whose x has the given
    parity (the low or the high half of a packed dword: the sensor's width is even), and `extra` events on the other half
    of that dword.  mode 1 / 2: all but the anchors start at PILE["src"], in another patch, band and tile, and are
    carried over by the patch's flow / the field at their pixel; mode 0: they lie on the pixel.
    -> case, the pixel, the expected counts (pixel, neighbour)."""
    g = PILE
    w, h, pw, ph = g["w"], g["h"], g["pw"], g["ph"]
    geom = (w, h, pw, ph)
    npx, npy = grid(*geom)
    X, Y = g["dst"][0] - (g["dst"][0] & 1) + parity, g["dst"][1]
    sx, sy = g["src"][0] - (g["src"][0] & 1) + parity, g["src"][1]
    t0, t1 = 1_000_000, 1_060_000
    t_ref = ref_time(t0, t1)
    m_x, m_y = (X - sx) / 20.0, (Y - sy) / 20.0  # 20000 us x 1e-3: the displacement at the middle of the times
    k = np.arange(n - 2 + extra)
    dtw = 20000 + (k * 7) % 201 - 100  # +-100 us: +-0.16 px around the pixel's centre
    t = t_ref - dtw
    x = np.where(k < n - 2, sx, sx ^ 1)
    y = np.full(len(k), sy)
    if mode == 0:
        x, y = np.where(k < n - 2, X, X ^ 1), np.full(len(k), Y)
    order = np.argsort(t, kind="stable")
    ev = make_events(np.concatenate([[X], x[order], [X]]), np.concatenate([[Y], y[order], [Y]]),
                     np.concatenate([[t0], t[order], [t1]]))
    flows = field = None
    if mode == 1:
        flows = np.zeros((1, npx * npy, 2))
        flows[0, patch_of(sx, sy, geom)] = (m_x, m_y)
    elif mode == 2:
        field = np.zeros((1, h, w, 2), dtype=np.float32)
        field[0, sy, sx] = field[0, sy, sx ^ 1] = (m_x, m_y)
    case = dict(name="pileup m%d n%d p%d e%d" % (mode, n, parity, extra), w=w, h=h, pw=pw, ph=ph, scale=SCALE, ev=ev,
                offsets=np.array([0, len(ev)], dtype=np.uint64), flows=flows, field=field)
    return case, (X, Y), (n, extra)


# ---- the 16-bit rule of the tiles ---------------------------------------------------------------------------------
TILE_LIMIT = dict(w=64, h=48, pw=16, ph=12, dst=(24, 18))
TILE_LIMIT_VARIANTS = ("max16", "over16", "wide_reach")


@functools.lru_cache(maxsize=None)
def tile_limit(variant):
    """k_count_tiles's safe16 rule (nx * ny * maxEvents < 65536) at its edge: the 3 x 3 patches around TILE_LIMIT["dst"]
    send all their events to it, each displaced by at most 9 pixels at the patch's largest |dt| (reach <= 12 with the + 1:
    nx = ny = 3).  max16: 7281 events per patch, 9 x 7281 = 65529, the 16-bit counters at their largest; over16: 7282,
    65538, the 32-bit slices; wide_reach: 7281 and one far unit of 3 events whose reach of 21 pixels makes nx = ny = 5 without
    putting an event on the pixel.  The anchors lie in a patch of their own.  -> case, the pixel, its expected count."""
    g = TILE_LIMIT
    w, h, pw, ph = g["w"], g["h"], g["pw"], g["ph"]
    geom = (w, h, pw, ph)
    npx, npy = grid(*geom)
    X, Y = g["dst"]
    per = 7282 if variant == "over16" else 7281
    t0, t1 = 1_000_000, 1_060_000
    t_ref = ref_time(t0, t1)
    flows = np.zeros((1, npx * npy, 2))
    xs, ys, ts = [], [], []
    for by in range(3):
        for bx in range(3):
            # the pixel of the patch nearest the target
            sx = min(max(X, bx * pw), bx * pw + pw - 1)
            sy = min(max(Y, by * ph), by * ph + ph - 1)
            k = np.arange(per)
            sign = 1 if (bx + by) % 2 else -1
            dtw = sign * (19900 + (k * 7) % 101)  # |dt| <= 20000 us: the displacement grows by at most 0.5 %
            flows[0, by * npx + bx] = ((X - sx) / (sign * 19.95), (Y - sy) / (sign * 19.95))
            xs.append(np.full(per, sx))
            ys.append(np.full(per, sy))
            ts.append(t_ref - dtw)
    if variant == "wide_reach":
        p = patch_of(60, 44, geom)
        flows[0, p] = (-1.0, -1.0)  # 20 pixels at 20000 us towards the pixel: reach 21, it lands 8 pixels short of it
        xs.append(np.array([60, 61, 62]))
        ys.append(np.array([44, 45, 46]))
        ts.append(t_ref - np.array([20000, 15000, -20000]))
    x, y, t = np.concatenate(xs), np.concatenate(ys), np.concatenate(ts)
    order = np.argsort(t, kind="stable")
    ax, ay = 49, 1  # patch (3, 0): flow zero
    ev = make_events(np.concatenate([[ax], x[order], [ax + 1]]), np.concatenate([[ay], y[order], [ay]]),
                     np.concatenate([[t0], t[order], [t1]]))
    case = dict(name="tile_limit " + variant, w=w, h=h, pw=pw, ph=ph, scale=SCALE, ev=ev,
                offsets=np.array([0, len(ev)], dtype=np.uint64), flows=flows, field=None)
    return case, (X, Y), 9 * per


# ---- store forms -----------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def store_pattern(mode, n_windows=3):
    """STORE_SHAPE in n_windows windows with a distinct pattern per window: pixel i of window k holds
    (i * (k + 2) + k) % 5 events, the last pixel of every row (so of every band, whatever its height) at least k + 1.
    mode 1 / 2: the events start one pixel to the left, 10000 us before the reference time, and a flow / field of
    (0.1, 0) carries them over; the first column is then fed from outside the sensor (the stray unit) in mode 1 and stays
    empty in mode 2.  The two anchors, 20000 us either side of the reference time, are events of the image like the
    others."""
    g = STORE_SHAPE
    w, h, pw, ph = g["w"], g["h"], g["pw"], g["ph"]
    npx, npy = grid(w, h, pw, ph)
    ev_all, offsets = [], [0]
    for k in range(n_windows):
        cnt = ((np.arange(w * h) * (k + 2) + k) % 5).reshape(h, w)
        cnt[:, w - 1] = np.maximum(cnt[:, w - 1], k + 1)
        ys, xs = np.nonzero(cnt)
        rep = cnt[ys, xs]
        x, y = np.repeat(xs, rep), np.repeat(ys, rep)
        t0 = 1_000_000 + 1000 * k
        t1 = t0 + 40000
        t_ref = ref_time(t0, t1)
        ev = make_events(x - (1 if mode else 0), y, np.full(len(x), t_ref - 10000))
        ev_all += [make_events([10], [0], [t0]), ev, make_events([10], [1], [t1])]
        offsets.append(offsets[-1] + len(ev) + 2)
    flows = field = None
    if mode == 1:
        flows = np.zeros((n_windows, npx * npy, 2))
        flows[:, :, 0] = 0.1
    elif mode == 2:
        field = np.zeros((n_windows, h, w, 2), dtype=np.float32)
        field[..., 0] = 0.1
    return dict(name="store m%d" % mode, w=w, h=h, pw=pw, ph=ph, scale=SCALE, ev=np.concatenate(ev_all),
                offsets=np.array(offsets, dtype=np.uint64), flows=flows, field=field)
