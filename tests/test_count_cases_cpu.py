"""CPU: the cases of tests/count_cases.py have the teeth tests/test_gpu_count_edges.py relies on.  The numpy restatement
`positions` gives the oracle's image on every case; the tie ladders hold every rung on both sides, both axes and every
displacement class after the f64 evaluation; the float pre-test restated in float32 (`pretest`) runs both of its branches
on them, misrounds nothing with the shipped constants and misrounds events once its displacement term is dropped; the
pile-ups and the tile-limit cases put exactly the stated counts on their pixel; the seam cases touch every seam line.
The misround counts of the weakened variants are printed (pytest -s) and recorded in DESIGN.md 4.4."""
import numpy as np
import pytest

import count_cases as cc

WARPED = ("small", "wide", "tall", "c2", "fine")
FIELD = ("small", "wide", "tall", "c2x64")
SEAM_PITCHES = [(0, 25, 0), (0, 23, 0), (30, 23, 8), (8, 8, 0), (30, 22, 0)]


def _prm(orc, c):
    return orc.default_params(image_w=c["w"], image_h=c["h"], patch_w=c["pw"], patch_h=c["ph"], scale=c["scale"], loss=1)


def oracle_image(orc, c, k):
    ev = cc.window_events(c, k)
    if c["flows"] is not None:
        return orc.final_count_image(ev, _prm(orc, c), c["flows"][k])
    if c["field"] is not None:
        return orc.compensate_events_field(ev, c["w"], c["h"], c["field"][k], scale=c["scale"])
    return orc.integrate_events(ev, c["w"], c["h"])


def _all_cases():
    for s in WARPED:
        yield cc.ties_warped(s)
    for s in FIELD:
        yield cc.ties_field(s)
    for p in SEAM_PITCHES:
        yield cc.seams(*p)
    for mode in (0, 1, 2):
        for n, parity, extra in cc.PILE_VARIANTS:
            yield cc.pileup(mode, n, parity, extra)[0]
        yield cc.store_pattern(mode)
    for v in cc.TILE_LIMIT_VARIANTS:
        yield cc.tile_limit(v)[0]


def test_positions_give_the_oracles_image_on_every_case(orc):
    n = 0
    for c in _all_cases():
        for k in range(len(c["offsets"]) - 1):
            assert np.array_equal(cc.case_image(c, k), oracle_image(orc, c, k)), (c["name"], k)
            n += 1
    assert n > 150


def _required(c, field):
    need = set()
    for ax in c["axes"]:
        for cls in c["classes"]:
            need.add((ax, cls, "exact", 0))
            for rung in cc.RUNGS:
                if not field or cc.field_rung_reachable(cls, rung):
                    need |= {(ax, cls, rung, -1), (ax, cls, rung, 1)}
    return need


@pytest.mark.parametrize("sensor", WARPED)
def test_warped_ladder_holds_every_rung_side_axis_and_class(sensor):
    c = cc.ties_warped(sensor)
    assert c["dropped"] == 0
    got, exact_signs = cc.ladder_coverage(c)
    assert not _required(c, False) - got
    if sensor in ("small", "wide", "tall"):
        assert {(ax, s) for ax in c["axes"] for s in (-1, 1)} <= exact_signs  # exact ties at -0.5 and inside the image
    # the two ties where half-away and rintf differ at the image's border: -0.5 and extent - 0.5 (odd extent)
    geom = (c["w"], c["h"], c["pw"], c["ph"])
    at_low, at_high = set(), set()
    for k in range(len(c["offsets"]) - 1):
        ev = cc.window_events(c, k)
        fx, fy, _, _, _ = cc.positions(ev, cc.ref_time(ev["t_us"][0], ev["t_us"][-1]), c["scale"], geom, c["flows"][k])
        for ax, f, extent in (("x", fx, c["w"]), ("y", fy, c["h"])):
            if (f == -0.5).any():
                at_low.add(ax)
            if (f == extent - 0.5).any():
                at_high.add(ax)
    assert at_low == set(c["axes"]) and at_high == set(c["axes"])


@pytest.mark.parametrize("sensor", FIELD)
def test_field_ladder_holds_every_rung_a_float_flow_can_meet(sensor):
    """A float32 flow times an integer time cannot be steered to the neighbouring double of a tie, nor (for large
    displacements) within 1e-9 of it: count_cases.field_rung_reachable says which rungs the field ladder owes; the warped
    ladder, whose flows are doubles, owes all of them."""
    c = cc.ties_field(sensor)
    got, exact_signs = cc.ladder_coverage(c)
    assert not _required(c, True) - got
    assert {(ax, 1) for ax in c["axes"]} <= exact_signs


def test_pretest_runs_both_branches_and_only_the_shipped_constants_round_right(capsys):
    """Events within 1e-4 of a tie: the shipped pre-test is sure of >= 100 and unsure of >= 100 (both branches run), and
    misrounds none -- in count_target's per-event form on the warped and field ladders, and in count_hit_uniform's per-unit
    form on the warped ones.  Without the displacement term, and without both terms, events are misrounded."""
    cases = [(cc.ties_warped(s), False) for s in WARPED] + [(cc.ties_warped(s), True) for s in WARPED] + \
            [(cc.ties_field(s), False) for s in FIELD]
    table = {}
    for name, consts in cc.VARIANTS.items():
        ev = [0, 0]
        un = [0, 0]
        for c, per_unit in cases:
            bad, n_sure, n_not = cc.misrounds(c, consts, per_unit=per_unit)
            tgt = un if per_unit else ev
            tgt[0] += bad
            tgt[1] += n_sure + n_not
        table[name] = (ev[0], un[0], ev[1], un[1])
    with capsys.disabled():
        print("\nmisrounded events of %d (per-event form) / %d (per-unit form):" % table["shipped"][2:])
        for name, (a, b, _, _) in table.items():
            print("  %-26s per-event %4d   per-unit %4d" % (name, a, b))
    # both branches, on events near a tie only
    for c, per_unit in cases:
        if c["name"].split()[1] in ("wide", "tall"):
            continue  # at thousands of pixels of displacement the tolerance leaves (rightly) next to nothing sure
        bad, n_sure, n_not = cc.misrounds(c, cc.VARIANTS["shipped"], per_unit=per_unit)
        assert n_sure >= 100 and n_not >= 100, (c["name"], per_unit, n_sure, n_not)
    assert table["shipped"][:2] == (0, 0)
    assert table["no displacement term"][0] >= 1 and table["no displacement term"][1] >= 1
    assert table["no terms"][0] >= 1 and table["no terms"][1] >= 1


@pytest.mark.parametrize("mode", [0, 1, 2])
def test_pileups_put_the_stated_counts_on_one_dword(orc, mode):
    for n, parity, extra in cc.PILE_VARIANTS:
        c, (x, y), (a, b) = cc.pileup(mode, n, parity, extra)
        img = oracle_image(orc, c, 0)
        assert (x & 1) == parity and len(c["ev"]) == n + extra
        assert img[y, x] == n and img[y, x ^ 1] == extra and img.sum() == n + extra
        if mode:  # the pile comes from another patch and another 8-row band
            src = c["ev"][1]
            geom = (c["w"], c["h"], c["pw"], c["ph"])
            assert cc.patch_of(src["x"], src["y"], geom) != cc.patch_of(x, y, geom) and src["y"] // 8 != y // 8


def test_tile_limit_variants_sit_on_both_sides_of_the_16_bit_rule(orc):
    """nx * ny * maxEvents as k_count_tiles computes it from the largest reach (ceil, + 1 included) and the largest unit:
    9 x 7281 < 65536 <= 9 x 7282, and 25 x 7281 with the far unit's reach."""
    want = {"max16": (65529, 3, True), "over16": (65538, 3, False), "wide_reach": (65529, 5, False)}
    for v in cc.TILE_LIMIT_VARIANTS:
        c, (x, y), n = cc.tile_limit(v)
        img = oracle_image(orc, c, 0)
        assert img[y, x] == n == want[v][0] and len(c["ev"]) <= 70000
        geom = (c["w"], c["h"], c["pw"], c["ph"])
        ev = c["ev"]
        t_ref = cc.ref_time(ev["t_us"][0], ev["t_us"][-1])
        p = cc.patch_of(ev["x"], ev["y"], geom)
        reach, most = 0.0, 0
        for u in np.unique(p):
            sel = p == u
            max_dt = float(np.abs(t_ref - ev["t_us"][sel]).max())
            t = max_dt * abs(c["scale"])
            reach = max(reach, t * abs(c["flows"][0, u, 0]) + 1.0, t * abs(c["flows"][0, u, 1]) + 1.0)
            most = max(most, int(sel.sum()))
        r = int(np.ceil(reach))
        nx, ny = 1 + 2 * ((r + c["pw"] - 1) // c["pw"]), 1 + 2 * ((r + c["ph"] - 1) // c["ph"])
        assert (nx, ny) == (want[v][1], want[v][1]) and r <= (12 if v != "wide_reach" else 32)
        assert (nx * ny * most < 65536) == want[v][2]


@pytest.mark.parametrize("pitch", SEAM_PITCHES)
def test_seams_touch_every_seam_row_and_column(orc, pitch):
    c = cc.seams(*pitch)
    img = sum(oracle_image(orc, c, k) for k in range(len(c["offsets"]) - 1))
    cols, rows = img.sum(axis=0), img.sum(axis=1)
    assert all(cols[x] > 0 for x in cc.seam_lines(c["w"], pitch[0]))
    assert all(rows[y] > 0 for y in cc.seam_lines(c["h"], pitch[1]))
    # the corners carry the largest |dt| of their unit: the reach the kernels derive from it is the corners' own
    geom = (c["w"], c["h"], c["pw"], c["ph"])
    ev = cc.window_events(c, 0)[1:-1]
    t_ref = cc.ref_time(*cc.window_events(c, 0)["t_us"][[0, -1]])
    p = cc.patch_of(ev["x"], ev["y"], geom)
    for u in np.unique(p):
        e = ev[p == u]
        dt = np.abs(t_ref - e["t_us"])
        corner = np.isin(e["x"], (e["x"].min(), e["x"].max())) & np.isin(e["y"], (e["y"].min(), e["y"].max()))
        assert corner.sum() == 4 and (dt[corner] == dt.max()).all() and (dt[~corner] < dt.max()).all()
    # and events sit exactly on the seams' ties and SEAM_DELTA either side of them
    dists = set()
    for k in range(len(c["offsets"]) - 1):
        w = cc.window_events(c, k)
        fx, fy, _, _, _ = cc.positions(w, cc.ref_time(w["t_us"][0], w["t_us"][-1]), c["scale"], geom, c["flows"][k])
        for f, pit in ((fx, pitch[0]), (fy, pitch[1])):
            if pit:
                d, tie = cc.tie_distance(f)
                on_seam = ((tie + 0.5) % pit == 0) & (np.abs(d) < 1e-8)
                dists |= set(np.sign(d[on_seam]).astype(int).tolist())
    assert dists == {-1, 0, 1}


def test_store_pattern_differs_per_window_and_feeds_every_rows_last_pixel(orc):
    for mode in (0, 1, 2):
        c = cc.store_pattern(mode)
        imgs = [oracle_image(orc, c, k) for k in range(3)]
        assert (c["w"] * c["h"]) % 2 == 1
        assert not np.array_equal(imgs[0], imgs[1]) and not np.array_equal(imgs[1], imgs[2])
        for k, img in enumerate(imgs):
            assert (img[:, -1] > 0).all() and img.max() < 65536


def test_the_restatements_own_teeth(orc):
    """What a reviewer can check without a GPU, checked: counts taken modulo 65536 in the restatement's image miss the
    pile-ups and the tile limit; the oracle does not wrap."""
    for c, (x, y), n in [cc.pileup(1, 65536, 0, 0)[:2] + (65536,), cc.pileup(0, 70000, 1, 0)[:2] + (70000,),
                         cc.tile_limit("over16")]:
        wrapped = np.mod(cc.case_image(c, 0), 65536)
        assert not np.array_equal(wrapped, oracle_image(orc, c, 0))
        assert oracle_image(orc, c, 0)[y, x] == n
