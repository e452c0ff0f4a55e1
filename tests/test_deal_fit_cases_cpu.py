"""CPU: the scenes of tests/deal_fit_cases.py do sit on the fit boundary of k_eval3's bank deal, at every shipped shape.

  * the capacities written out in the scenes are csrc/eval_plan.h's own (a small program prints plan_eval), and each scene's
    rects select its shape;
  * every class is present in every shape and classified as intended by two independent statements of the rule -- the
    arithmetic P + L against the capacity written here, and tools/ab/lds_conflict_model.py's deal_admitted / dealt_list on the
    unit's packed records -- and by csrc/eval_deal.h's deal_admits && deal_fits on the same (n, block, capacity, band) tuples;
  * the scenes tell the slips apart that the boundary is there to catch: each of `<` for `<=`, the band taken with bw for the
    pitch, L = n // 4, the capacity of the plan below 1024 slots and the 160-double header changes the verdict of at least one
    class (restated rule only: no altered kernel exists)."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

import deal_fit_cases as cases

HERE = os.path.dirname(os.path.abspath(__file__))
CSRC = os.path.join(os.path.dirname(HERE), "event-based-odomety_amd", "csrc")
NAMES = list(cases.SHAPES)
NOT_DEALT = ("over_list", "over_row", "below", "above", "split_over")


def _model():
    path = os.path.join(os.path.dirname(CSRC), "tools", "ab", "lds_conflict_model.py")
    spec = importlib.util.spec_from_file_location("lds_conflict_model", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def _records(m, u):
    """the unit's packed records in the canonical order, as a load leaves them on the device"""
    ev = u["ev"]
    x, y, t = ev["x"].astype(np.int64), ev["y"].astype(np.int64), ev["t_us"].astype(np.int64)
    dt = cases.ref_time(t[0], t[-1]) - t
    lo = (x & 0x7FFF) | ((ev["sign"] > 0).astype(np.int64) << 15) | ((y & 0x7FFF) << 16)
    rec = (lo | ((dt & 0xFFFFFFFF) << 32)).astype(np.uint64)
    return rec[m.canonical(x, y, ev["sign"], dt)]


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    """a filter around the headers themselves: `plan rw rh max_rw slots waves` -> block, workgroups, bytes, header, capacity;
    `deal n block cap band` -> deal_admits(n, block, 1) && deal_fits(n, block, cap, band)"""
    d = tmp_path_factory.mktemp("deal_fit")
    src = d / "rule.cpp"
    src.write_text('#include "%s"\n#include "%s"\n#include <cstdio>\n#include <cstring>\n'
                   'int main() { char op[16]; long a, b, c, d, e;\n'
                   '  while (std::scanf("%%15s %%ld %%ld %%ld %%ld %%ld", op, &a, &b, &c, &d, &e) == 6) {\n'
                   '    if (!std::strcmp(op, "plan")) { ebo::EvalShape S; S.reg_rw = a; S.reg_rh = b; S.max_rw = c; S.flow_slots = d;\n'
                   '      S.lds_budget = 160 * 1024; S.waves_per_cu = e; const ebo::EvalPlan p = ebo::plan_eval(S);\n'
                   '      std::printf("%%d %%d %%zu %%d %%d\\n", p.block, p.workgroups_per_cu, p.lds_bytes, p.header_doubles, p.cap_doubles); }\n'
                   '    else std::printf("%%d\\n", ebo::deal_admits(a, b, 1) && ebo::deal_fits(a, b, c, d) ? 1 : 0); }\n'
                   '  return 0; }\n' % (os.path.join(CSRC, "eval_plan.h"), os.path.join(CSRC, "eval_deal.h")))
    exe = str(d / "rule")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", exe, str(src)])

    def ask(lines):
        out = subprocess.run([exe], input="".join(l + "\n" for l in lines), capture_output=True, text=True, timeout=60)
        assert out.returncode == 0, out.stderr
        return [[int(v) for v in l.split()] for l in out.stdout.splitlines()]
    return ask


@pytest.mark.parametrize("name", NAMES)
def test_the_capacity_is_the_plans_and_the_rects_select_the_shape(native, name):
    S = cases.SHAPES[name]
    assert S["cap"] == cases.CAPACITIES[name] and S["groups"] == cases.RESIDENT[name]
    rects, _ = cases.lattice(name)
    assert len(rects) >= cases.MANY_SLOTS and len(rects) <= 1100
    rw, rh, max_rw = int(rects[:, 2].min()), int(rects[:, 3].min()), int(rects[:, 2].max())
    assert (rw, rh) == S["rect"] and max_rw == (S["wide"] or rw) and int(rects[:, 3].max()) == rh
    waves = 16 if S["sigma"] is None else 12
    block, groups, lds, header, cap = native(["plan %d %d %d %d %d" % (rw, rh, max_rw, len(rects), waves)])[0]
    assert (block, groups, lds, cap) == (S["block"], S["groups"], S["lds"], S["cap"])
    assert header == cases.header_doubles(block // 64)
    # one row tile (eval_launch_shape: sub-bands of the widest canvas / 6, at least 1)
    assert -(-9 * max_rw * rh // cap) // 6 <= 1
    # the scene: the units' patches hold their events, every other patch is empty
    ev, offsets, rects, flows, index = cases.assemble(name)
    counts = np.diff(offsets.astype(np.int64))
    units = cases.units_of(name)
    assert (counts > 0).sum() == len(units) <= 14 and max(u["n"] for u in units) <= 3073
    for u, i in zip(units, index):
        assert counts[i] == u["n"] and np.array_equal(ev[int(offsets[i]):int(offsets[i + 1])], u["ev"])
        x, y, w, h = rects[i]
        assert ((u["ev"]["x"] >= x) & (u["ev"]["x"] < x + w) & (u["ev"]["y"] >= y) & (u["ev"]["y"] < y + h)).all()
        assert (w == S["wide"]) if u["wide"] else (w == rw)


@pytest.mark.parametrize("name", NAMES)
def test_every_class_is_present_and_classified(native, name):
    S = cases.SHAPES[name]
    cap, B = S["cap"], S["block"]
    m = _model()
    rects, _ = cases.lattice(name)
    units = cases.units_of(name)
    assert {u["cls"] for u in units} == set(cases.classes_of(name))
    assert set(cases.classes_of(name)) | set(cases.ABSENT.get(name, {})) >= set(cases.CLASSES)
    verdicts = native(["deal %d %d %d %d 0" % (u["n"], B, cap, min(max(cap // u["cols"], 1), u["rows"]) * u["cols"]) for u in units])
    for u, (verdict,) in zip(units, verdicts):
        n, bw, rows, cols = u["n"], u["bw"], u["rows"], u["cols"]
        rect = rects[u["slot"]]
        P, L = rows * cols, (n + 3) // 4
        assert cols == bw | 1
        # the arithmetic, per class
        cls = u["cls"]
        if cls in ("fit", "full_canvas", "clipped"):
            assert P + L == cap and n % 4 == 0 and 2 * B <= n <= 12 * B
        elif cls == "fit_quad":
            assert P + L == cap and n % 4 == 1
        elif cls == "over_list":
            assert P + L == cap + 1 and n % 4 == 1
        elif cls == "over_row":
            assert P - cols + L == cap and P <= cap  # one row too many, still one sub-band
        elif cls in ("low_end", "high_end"):
            assert (2 * B <= n <= 2 * B + 7) if cls == "low_end" else (12 * B - 7 <= n <= 12 * B)
            assert P + L == cap - u["free"] and u["free"] >= 0
            if u["free"]:  # no exact fit at this end: nothing fits closer
                assert u["free"] == cases.closest_fit(cap, B, *S["rect"], n)[0]
                assert not [f for f in cases.exact_fits(cap, B, *S["rect"]) if abs(f[0] - n) < 8 and (f[0] + 3) // 4 == L]
        elif cls == "below":
            assert n == 2 * B - 1 and P + L < cap
        elif cls == "above":
            assert n == 12 * B + 1 and P + L < cap
        elif cls in ("split_fit", "split_over"):
            band = (cap // cols) * cols
            assert rows > cap // cols and band + L == cap + (cls == "split_over")
        dealt = cls not in NOT_DEALT
        assert u["sub_bands"] == (2 if cls.startswith("split") else 1)
        # three statements of the rule
        assert u["dealt"] == dealt and cases.rule(n, B, cap, bw, rows) == dealt, (name, u["name"])
        assert m.deal_admitted(n, B, 1, cap, cols, rows) == dealt, (name, u["name"])
        assert bool(verdict) == dealt, (name, u["name"])
        # the model's box of the packed records is the scene's, and its list a permutation exactly where dealt
        rec = _records(m, u)
        base, mcols, mrows = m.box_base_words(*m.unpack_records(rec), rect, u["flow"], cap)
        assert (mcols, mrows) == (cols, rows) and int((base == m.REJECT).sum()) == u["rejected"]
        lst = m.dealt_list(rec, rect, u["flow"], B, cap)
        assert len(lst) == (n if dealt else 0)
        if dealt:
            assert np.array_equal(np.sort(lst), np.arange(n))
        box = cases.unit_box(u["ev"], rect, u["flow"])
        if cls in ("fit", "full_canvas", "clipped", "fit_quad", "low_end", "high_end"):
            assert cases.covers_last_pixel(box).any(), (name, u["name"])  # a footprint reaches the image's last pixel
        if cls == "clipped":
            assert u["rejected"] > 0 and box["y0"] + rows == 3 * int(rect[3])  # cut by the last canvas row
            order = m.dealt_order(base, B, 16)[np.argsort(m.deal_positions(n, B, 16))]  # the sorted order
            assert (base[order[-u["rejected"]:]] == m.REJECT).all()  # key 16 sorts last
        elif cls not in ("full_canvas", "fit_quad", "over_list") and name != "30x22 sigma<1":
            assert u["rejected"] == 0 and 0 <= box["x0"] and box["x0"] + bw <= 3 * int(rect[2])
    fits = [u for u in units if u["cls"] == "fit"]
    assert sorted(u["bw"] % 2 for u in fits) == ([0, 1] if cases.ODD_FIT[name] else [0])
    if name != "30x22 sigma<1":
        assert len(cases.exact_fits(cap, B, *S["rect"])) >= 55
        if S["wide"]:
            assert any(u["wide"] and u["bw"] > 3 * S["rect"][0] for u in fits)  # a box only the wide canvas holds
    else:
        assert [u["n"] for u in units if u["cls"] == "full_canvas"] == [2696]
        assert cases.exact_fits(cap, B, *S["rect"]) == [(3060, 90, 65), (2696, 90, 66)]


def test_exact_fits_at_the_ends_of_the_admitted_counts():
    """n = 260 in 45 x 55 and n = 1536 in 49 x 44 at 2540; n = 3072 in 77 x 56 at 5080; none at the sigma < 1 capacities"""
    free = {name: {u["cls"]: u["free"] for u in cases.units_of(name) if u["cls"] in ("low_end", "high_end")} for name in NAMES}
    assert free["20x20"] == {"low_end": 0, "high_end": 0} and free["21x16+31"] == {"low_end": 0, "high_end": 0}
    assert free["30x22"]["high_end"] == 0 and free["30x22"]["low_end"] > 0
    assert min(free["20x20 sigma<1"].values()) > 0 and min(free["30x22 sigma<1"].values()) > 0
    by = {(name, u["cls"]): (u["n"], u["cols"], u["rows"]) for name in NAMES for u in cases.units_of(name)}
    assert by[("20x20", "low_end")] == (260, 45, 55) and by[("20x20", "high_end")] == (1536, 49, 44)
    assert by[("30x22", "high_end")] == (3072, 77, 56)


def test_the_scenes_tell_the_slips_apart():
    """each slip changes the restated verdict of at least one class in EVERY shape (so whichever plan a launch takes)"""
    caught = {}
    for name in NAMES:
        S = cases.SHAPES[name]
        for slip in cases.SLIPS:
            hit = sorted({u["cls"] for u in cases.units_of(name)
                          if cases.rule(u["n"], S["block"], S["cap"], u["bw"], u["rows"], slip) != u["dealt"]})
            caught[(name, slip)] = hit
            assert hit, (name, slip)
    print({k: v for k, v in caught.items()})
    for name in NAMES:
        assert "fit" in caught[(name, "less_than")] and "fit" in caught[(name, "header_160")]
        assert "over_list" in caught[(name, "band_bw")] and "over_list" in caught[(name, "list_floor")]
        # 4960 doubles are more than two of the shipped capacities and less than the other three
        wrong = {"over_list", "over_row"} if cases.SHAPES[name]["cap"] < 4960 else {"fit", "fit_quad", "clipped"}
        assert wrong <= set(caught[(name, "cap_4960")])


@pytest.mark.parametrize("name", NAMES)
def test_moved_and_reversed_scenes_hold_the_same_units(name):
    units = cases.units_of(name)
    _, _, rects0, _, index0 = cases.assemble(name)
    moved = 0
    for order in ("moved", "reversed"):
        ev, offsets, rects, flows, index = cases.assemble(name, order)
        assert len(set(index)) == len(units) and (np.diff(offsets.astype(np.int64)) > 0).sum() == len(units)
        for u, i, i0 in zip(units, index, index0):
            assert np.array_equal(rects[i], rects0[i0]) and tuple(flows[i]) == tuple(u["flow"])
            assert np.array_equal(ev[int(offsets[i]):int(offsets[i + 1])], u["ev"])
            moved += order == "moved" and i != i0
    assert moved >= 2
