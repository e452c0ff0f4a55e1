"""CPU only: every case of tests/edge_fit_cases.py sits where its name says (the restatement of tests/edge_box_ref.py puts
the largest fitting box on the regime's LDS form and its neighbour off it, one row / column / the least excess apart), is
evaluated outside the penalty branch, and is no coin toss for the oracle (an argmax tie would move the Jacobian by far
more than a flow step of 1e-9 can)."""
import numpy as np
import pytest

import edge_box_ref as ref
import edge_fit_cases as fc

LOSS_EDGE = 0  # include/ebo.h: EBO_LOSS_EDGE

EXPECTED_NAMES = """
a/fit a/fit_c+1 a/fit_c-1 a/fit_r+1 a/fit_r-1 a/inside a/outside a/over
c/fit c/fit_c+1 c/fit_c-1 c/fit_r+1 c/fit_r-1 c/inside c/outside c/over
d/full_canvas d/inside
b/bytes_fit b/bytes_over b/fit b/fit_r+1 b/fit_r-1 b/inside b/outside b/over b/rows_fit b/rows_over
e52/bytes_fit e52/bytes_over e52/fit e52/fit_c+1 e52/fit_c-1 e52/fit_r+1 e52/fit_r-1 e52/inside
e52/nE%8=0 e52/nE%8=1 e52/nE%8=7 e52/outside e52/over e52/rows_fit e52/rows_over
e40/bytes_fit e40/bytes_over e40/fit e40/fit_c+1 e40/fit_c-1 e40/fit_r+1 e40/fit_r-1 e40/inside
e40/nE%8=0 e40/nE%8=1 e40/nE%8=7 e40/outside e40/over e40/rows_fit e40/rows_over
e52/deferred_to_slice e52/mixed e52/mixed_reversed
f0/fit f0/fit_c+1 f0/fit_c-1 f0/fit_r+1 f0/fit_r-1 f0/inside f0/outside f0/over
f1/bytes_fit f1/bytes_over f1/fit f1/fit_c+1 f1/fit_c-1 f1/fit_r+1 f1/fit_r-1 f1/inside f1/outside f1/over f1/rows_fit f1/rows_over
""".split()


def test_no_case_is_missing():
    assert fc.CASE_IDS == EXPECTED_NAMES
    assert [c.name for c in fc.PILE_CASES] == ["g/p&7=7", "g/p&7=0"]
    assert [c.name for c in fc.SOLVE_CASES] == ["h/layout0", "h/layout1"]


def test_launch_setup_restates_the_documented_capacities():
    """DESIGN.md's figures, from the restated edge_launch_setup: the shipped regimes and the A/B ones"""
    for regime, want in fc.EXPECT_SETUP.items():
        S = next(c for c in fc.CASES if c.regime == regime).setup
        assert {k: getattr(S, k) for k in want} == want, regime
    # the shipped library takes the compact form by itself from more than eight units per CU on, never in a solve
    many = ref.launch_setup(20, 20, 20, 20, False, n_units=8 * 256 + 1, n_cus=256)
    assert many.compact and (many.compact_cap, many.compact_max_px, many.compact_list_cap) == (2912, 3600, 964)
    assert many.compact_cap % 8 == 0 and many.compact_bytes == 53248
    assert not ref.launch_setup(20, 20, 20, 20, False, n_units=8 * 256, n_cus=256).compact
    assert not ref.launch_setup(20, 20, 20, 20, False, n_units=1 << 20, n_cus=256, for_solve=True).compact
    # the argmax list of an LDS-resident box ends in front of k_solve_edge's state: a window per four pixels and the slack
    assert 7424 // 4 + ref.LIST_SLACK == ref.LIST_CAP - ref.LM_INTS
    # C4's canvas is limited by the list, not by bytes; the reference default can never spill
    a = next(c for c in fc.CASES if c.regime == "a").setup
    assert a.max_lds_px < a.cap_px < a.canvas_px
    d = next(c for c in fc.CASES if c.regime == "d").setup
    assert d.cap_px >= d.canvas_px == d.max_lds_px


@pytest.mark.parametrize("case", fc.CASES, ids=fc.CASE_IDS)
def test_case_sits_at_its_limit(case):
    S = case.setup
    lds = fc.LDS_FORM[case.regime]
    for u in case.units:
        # the unit's events give the box the case was built for, no warped coordinate near a truncation edge
        taps, away = ref.tap_bounds(u.events, u.rect, u.flow, fc.SCALE)
        assert taps == u.box.taps and away >= fc.MIN_AWAY
        assert 8 <= len(u.events) <= 40 and len(u.events) > fc.MIN_EVENTS
        assert all(abs(m - round(m)) > 1e-3 for m in u.flow)
        assert u.form == ref.form_of(u.box, S)
    u = case.units[-1]
    if case.cls in fc.FIT_CLASSES:
        assert u.form == lds
    elif case.cls in fc.OVER_CLASSES:
        # the compact launch defers to the 20 B launch, which holds every 20x20 box unless EBO_EDGE_LDS_KB trims it
        off = ref.FORM_20 if lds == ref.FORM_COMPACT and "EBO_EDGE_LDS_KB" not in case.env else ref.FORM_SLICE
        assert u.form == off
    else:
        assert case.cls in ("mixed", "mixed_reversed")
        assert sorted(x.form for x in case.units) == sorted([ref.FORM_COMPACT, ref.FORM_20, ref.FORM_SLICE])
    if case.regime == "b":
        # the regular units: far inside (less than half of the bytes)
        assert [x.form for x in case.units[:3]] == [ref.FORM_20] * 3
        assert all(2 * x.box.alias_ints(False) < ref.alias_cap_ints(S.cap_px, False) for x in case.units[:3])


def _fit_of(regime):
    return fc.BY_NAME[regime + "/fit"].units[-1].box


@pytest.mark.parametrize("regime", ["a", "b", "c", "e52", "e40", "f0", "f1"])
def test_the_limit_is_one_step_wide(regime):
    """`over` is `fit` plus one column or one row; the stepped cases differ from `fit` by exactly that; the bytes_* pair lies
    on either side of edge_box_fits_alias's byte test with nothing reachable between them"""
    fit = _fit_of(regime)
    S = fc.BY_NAME[regime + "/fit"].setup
    over = fc.BY_NAME[regime + "/over"].units[-1].box
    assert (over.bc - fit.bc, over.br - fit.br) in ((1, 0), (0, 1))
    for cls, d in (("fit_c-1", (-1, 0)), ("fit_c+1", (1, 0)), ("fit_r-1", (0, -1)), ("fit_r+1", (0, 1))):
        c = fc.BY_NAME.get("%s/%s" % (regime, cls))
        if c is None:
            # (the corner unit's fitting box spans the canvas's width: a column more or less is not reachable)
            assert regime == "b" and cls.startswith("fit_c") and fit.bc == fit.W3
            continue
        b = c.units[-1].box
        assert (b.bc - fit.bc, b.br - fit.br) == d
    if regime == "a":
        # 7424 = 116 x 64 is reachable; the next count above it that a 120x66 canvas holds is 118 x 63
        assert fit.npx == 7424 == S.max_lds_px
        reach = fc.reach_of(fc.RECT_A)
        assert min(b.npx for b in reach.boxes() if b.npx > 7424) == 7434
        # the byte test never refuses what the pixel test admits here, and admits boxes the pixel test refuses
        assert all(b.alias_ints(False) <= ref.alias_cap_ints(S.cap_px, False) for b in reach.boxes() if b.npx <= 7424)
        assert over.alias_ints(False) <= ref.alias_cap_ints(S.cap_px, False) and over.npx > S.max_lds_px
    if regime == "c":
        assert fit.npx == S.cap_px == 5510
    if regime in ("b", "e52", "e40", "f1"):
        cnt4 = S.compact
        cap = ref.alias_cap_ints(S.compact_cap if cnt4 else S.cap_px, cnt4)
        bf = fc.BY_NAME[regime + "/bytes_fit"].units[-1].box
        bo = fc.BY_NAME[regime + "/bytes_over"].units[-1].box
        assert bf.alias_ints(cnt4) <= cap < bo.alias_ints(cnt4)
        rect = fc.RECTS_B[3] if regime == "b" else fc.RECT_D
        max_px = S.compact_max_px if cnt4 else S.cs_stride
        ints = sorted({b.alias_ints(cnt4) for b in fc.reach_of(rect).boxes() if b.npx <= max_px})
        assert max(i for i in ints if i <= cap) == bf.alias_ints(cnt4) and min(i for i in ints if i > cap) == bo.alias_ints(cnt4)
        # the rows-only step across the byte test: the same columns, box rows and pixels, one stored row of I and of E / A /
        # counters more (the layout E = I + bc * iRows, cnt = E + bc * qRows at its last byte); no such pair of the rect's
        # whole reach lies nearer the limit
        rf = fc.BY_NAME[regime + "/rows_fit"].units[-1].box
        ro = fc.BY_NAME[regime + "/rows_over"].units[-1].box
        assert (ro.bc, ro.br, ro.npx) == (rf.bc, rf.br, rf.npx) and rf.npx <= max_px
        assert (ro.iRows, ro.qRows) == (rf.iRows + 1, rf.qRows + 1)
        assert rf.taps[:2] == ro.taps[:2] and sorted((ro.taps[2] - rf.taps[2], ro.taps[3] - rf.taps[3])) in ([-1, 0], [0, 1])
        assert rf.alias_ints(cnt4) <= cap < ro.alias_ints(cnt4)
        reach = fc.reach_of(rect)
        for xp in reach.cols.values():
            for lo, hi in reach.ys:
                b0 = reach.box(xp + (lo, hi))
                if b0.npx > max_px or not cap - rf.alias_ints(cnt4) > cap - b0.alias_ints(cnt4) >= 0:
                    continue
                for cand in ((lo - 1, hi), (lo, hi + 1)):
                    if cand in reach.yset:
                        b1 = reach.box(xp + cand)
                        same = (b1.br, b1.iRows, b1.qRows) == (b0.br, b0.iRows + 1, b0.qRows + 1)
                        assert not (same and b1.alias_ints(cnt4) > cap), (b0, b1)
    if regime in ("e52", "e40"):
        for k in (0, 1, 7):
            assert fc.BY_NAME["%s/nE%%8=%d" % (regime, k)].units[-1].box.nE % 8 == k


def test_full_canvas_box_hits_every_clamp():
    b = fc.BY_NAME["d/full_canvas"].units[-1].box
    assert b.taps == (0, 59, 0, 59)
    assert (b.x0, b.x1, b.y0, b.y1, b.bx0, b.by0, b.bc, b.br) == (0, 59, 0, 59, 0, 0, 60, 60)
    assert (b.iRows, b.qRows, b.ew, b.eh) == (60, 60, 59, 59)


def _all_units():
    seen = []
    for c in fc.CASES + fc.PILE_CASES + fc.SOLVE_CASES:
        for i, u in enumerate(c.units):
            seen.append(pytest.param(c, u, id="%s[%d]" % (c.name, i)))
    return seen


@pytest.mark.parametrize("case,u", _all_units())
def test_unit_is_evaluated_and_is_no_coin_toss(orc, case, u):
    ev = u.array()
    for flow in case.eval_flows(u):
        r, J = orc.contrast_eval(ev, u.rect, flow, LOSS_EDGE, scale=fc.SCALE)
        assert r < orc.default_consts().max_possible_residual  # the penalty branch gives max_res (1 + |m|^2)
        assert np.isfinite(J).all() and np.abs(J).min() > 0
        for d in ((1e-9, 0.0), (-1e-9, 0.0), (0.0, 1e-9), (0.0, -1e-9)):
            _, Jd = orc.contrast_eval(ev, u.rect, (flow[0] + d[0], flow[1] + d[1]), LOSS_EDGE, scale=fc.SCALE)
            assert np.abs(Jd - J).max() <= 1e-6 * np.abs(J).max()


@pytest.mark.parametrize("case", fc.PILE_CASES, ids=[c.name for c in fc.PILE_CASES])
def test_pile_up_reaches_the_first_and_the_last_field_of_a_counter_word(orc, case):
    u = case.units[0]
    assert u.form == ref.FORM_COMPACT
    I = orc.contrast_image(u.array(), u.rect, u.flow, channels=1, scale=fc.SCALE)[0]
    E = ref.eigen_image(I, orc.default_consts().sigma_st)
    claims = ref.window_claims(E, u.box)
    y, x = (int(v) for v in np.unravel_index(np.argmax(E), E.shape))
    # the brightest pixel: even coordinates, the argmax of all nine windows that hold it
    assert x % 2 == 0 and y % 2 == 0 and claims[(x, y)] == 9 == max(claims.values())
    runner_up = max(v for k, v in claims.items() if k != (x, y))
    assert E[y, x] > 1.001 * max(E[k[1], k[0]] for k in claims if k != (x, y)) and runner_up < 9
    p = ref.counter_index(u.box, x, y)
    assert 0 <= p < u.box.nE and p & 7 == case.field
    # no window can claim its neighbours in the row; the flank of the blob is claimed two columns on, in the same word
    assert (x - 1, y) not in claims and (x + 1, y) not in claims
    near = (x - 2, y) if case.field == 7 else (x + 2, y)
    assert near in claims and ref.counter_index(u.box, *near) >> 3 == p >> 3


@pytest.mark.parametrize("case", fc.SOLVE_CASES, ids=[c.name for c in fc.SOLVE_CASES])
def test_solve_case_crosses_the_limit_between_start_and_end(orc, case):
    u, S = case.units[0], case.setup
    assert S.block == (512 if case.name.endswith("0") else 256) and S.has_slice and not S.compact
    prm = orc.default_params(image_w=20, image_h=20, patch_w=20, patch_h=20, tv_weight=0.0, min_events=fc.MIN_EVENTS)
    flows, _, summ = orc.compensate_events_contrast(u.array(), prm, orc.default_solver(mode=1, **fc.SOLVE_OPTS), want_image=False)
    np.testing.assert_allclose(flows[0], fc.SOLVE_END, rtol=0, atol=1e-7)
    assert summ.num_evals_jac >= 5  # steps were accepted: the iterates moved
    # at the start the box is the events' extent plus 22 and fits; at the end it has grown past the capacity
    assert (u.box_start.bc, u.box_start.br) == (42, 42) and case.form_start == (ref.FORM_28 if case.name.endswith("0") else ref.FORM_20)
    assert (u.box.bc, u.box.br) == (48, 46) and u.form == ref.FORM_SLICE
    # ... and stays the same box for every end within 1e-5 of the oracle's (the bar the solves are compared at)
    for dx in (-1e-5, 1e-5):
        for dy in (-1e-5, 1e-5):
            assert u.box_at((fc.SOLVE_END[0] + dx, fc.SOLVE_END[1] + dy)).key() == u.box.key()


def _ints(name, cnt4=False):
    b = fc.BY_NAME[name].units[-1].box
    return (b.bc, b.br, b.alias_ints(cnt4))


def test_documented_limits():
    """the figures of DESIGN.md's table"""
    assert _ints("b/bytes_fit") == (67, 59, 18023) and _ints("b/bytes_over") == (73, 54, 18031) and _ints("b/fit")[:2] == (93, 48)
    assert _ints("e52/bytes_fit", True)[2] == 12011 and _ints("e52/bytes_over", True)[2] == 12013 and _ints("e52/fit")[:2] == (59, 59)
    assert _ints("e40/bytes_fit", True)[2] == 9039 and _ints("e40/bytes_over", True)[2] == 9045
    assert _ints("f0/fit")[:2] == (47, 30) and _ints("f0/over")[:2] == (48, 30)
    assert _ints("f1/bytes_fit")[2] == 9900 and _ints("f1/bytes_over")[2] == 9905
    assert _ints("b/rows_fit") == (66, 60, 18018) and _ints("b/rows_over") == (66, 60, 18348)
    assert _ints("e52/rows_fit", True) == (51, 60, 12005) and _ints("e52/rows_over", True) == (51, 60, 12215)
    assert _ints("e40/rows_fit", True) == (47, 57, 9036) and _ints("e40/rows_over", True) == (47, 57, 9230)
    assert _ints("f1/rows_fit") == (36, 60, 9900) and _ints("f1/rows_over") == (36, 60, 10080)
    assert _ints("c/fit")[:2] == (95, 58) and _ints("a/fit")[:2] == (116, 64) and _ints("d/full_canvas")[2] == 18000


# Mistakes in the fit tests and in the capacities, applied to the RESTATEMENT: each must move at least one case's unit to
# another storage form than the restatement gives it, i.e. the cases lie close enough to the limits to be sensitive to it.
# This says nothing about the kernel: the GPU test does not observe the form a unit took (tests/test_gpu_edge_fit.py).
def _slipped_form(box, S, slip):
    cap_px, max_px = S.cap_px, S.cs_stride
    ccap, cmax = S.compact_cap, S.compact_max_px
    if slip == "compact_cap_not_rounded" and S.compact:
        budget = int(S.env["EBO_EDGE_COMPACT_KB"]) * 1024
        ccap = min((budget - (168 + S.compact_list_cap // 2) * 8) * 2 // 33, cmax)
    if slip == "max_lds_px_without_solver_state":
        max_px = min(S.canvas_px, 4 * (ref.LIST_CAP - ref.LIST_SLACK)) if S.alias else max_px

    def alias(b, cap, mx, cnt4):
        need, have = b.alias_ints(cnt4), ref.alias_cap_ints(cap, cnt4)
        if slip == "counter_words_floor" and cnt4:
            need = 2 * (b.nI + b.nE) + (b.nE >> 3)
        if slip == "bytes_by_npx":
            need = 2 * (b.npx + b.npx) + ((b.npx + 7) >> 3 if cnt4 else b.npx)
        ok_bytes = need < have if slip == "less_than" else need <= have
        ok_px = b.npx < mx if slip == "less_than" else b.npx <= mx
        return ok_bytes and ok_px
    if S.compact and alias(box, ccap, cmax, True):
        return ref.FORM_COMPACT
    if S.alias:
        return ref.FORM_20 if alias(box, cap_px, max_px, False) else ref.FORM_SLICE
    return ref.FORM_28 if (box.npx < cap_px if slip == "less_than" else box.npx <= cap_px) else ref.FORM_SLICE


@pytest.mark.parametrize("slip", ["less_than", "counter_words_floor", "bytes_by_npx", "compact_cap_not_rounded",
                                  "max_lds_px_without_solver_state"])
def test_cases_tell_a_slipped_fit_test_apart(slip):
    moved = []
    for c in fc.CASES:
        for u in c.units:
            if _slipped_form(u.box, c.setup, slip) != u.form:
                moved.append(c.name)
    assert moved, slip
    print(slip, sorted(set(moved)))
