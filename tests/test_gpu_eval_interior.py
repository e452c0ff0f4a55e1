"""GPU: k_eval3's all-interior path (csrc/eval_interior.h).

A unit whose box came from the extents table, is not cut by the canvas and fits one sub-band of one row tile runs its three
event passes without the per-event reject, row and clip tests.  The A/B library switches the path off
(EBO_EVAL_INTERIOR=0) and counts the units that took it (ebo_interior_path_counts).  Scenes: 20 x 20 patches of a 100 x 80
image, a few hundred events per unit, built by hand (tests/deal_fit_cases.py: make_unit puts a unit's first event on the
high corner of its box, so its footprint ends on the box's last column and last row, and its last event on the low corner):

  * boxes whose xmin is exactly 3 / 2, whose xmax is 3 rw - 4 / 3 rw - 3, the same on both y sides, and the box that
    fills the canvas but for the margin (admitted / not, one unit loaded at a time so that the counter names the unit);
  * rowsAll == maxRows (admitted) and maxRows + 1 (not), forced with EBO_LDS_KB; a launch with row tiles (none admitted);
  * a unit with one event outside its rect and a rect wider than 64 (no table, not admitted); an inactive unit; a unit
    below two rounds of 128 lanes (not dealt, admitted); the stray bucket and inactive patches of the window path;
  * value only and with Jacobian, central differences, a lock-step solve, sigma < 1, workgroups of 128, 256 and 512 lanes.
Asserted: EBO_EVAL_INTERIOR=0 against the default, r and J bit for bit; the counter equals the numpy restatement of the
rule (test_gpu_box_extents._rule for table and box, tools/ab/lds_conflict_model.py: box_base_words for pitch and rows);
the shipped library has the A/B library's bits and holds against the oracle at the parity bounds of the neighbouring
k_eval3 tests (r: rtol 1e-9, atol 1e-12; J: jac_check.assert_jac_close), at 512 lanes and, in 1040 patches, at 128."""
import importlib.util
import os

import numpy as np
import pytest

import deal_fit_cases as cases
import test_gpu_box_extents as bx
from jac_check import assert_jac_close

pytestmark = pytest.mark.gpu

IMAGE, PATCH = (100, 80), (20, 20)
SCALE = cases.SCALE
MIN_EVENTS = 100


def _cap(slots, max_rw=PATCH[0], lds_kb=0):
    """csrc/eval_plan.h written out for 20 x 20 regular patches: the image capacity of one workgroup, whatever the forced block
    below 1024 slots; at least 24 rows of the WIDEST rect's canvas"""
    many = slots >= 1024
    header = cases.header_doubles(2) if many else 160
    lds = max(lds_kb, 4) * 1024 if lds_kb else (cases.plan(128, 16)[1] if many else 40 * 1024)
    lds = min(max(lds, 24 * 3 * max_rw * 8 + header * 8), cases.LDS_BUDGET)
    return (lds - header * 8) // 8


CAP_512 = _cap(60)               # 4960 pixels
CAP_WIDE = _cap(61, 70)          # 5040: the 70-wide rect raises the floor
CAP_FLOOR = _cap(60, lds_kb=4)   # EBO_LDS_KB=4: the floor of 24 rows of the 60-pixel canvas, 1440
CAP_MANY = _cap(1040)            # from 1024 slots: 2540
assert (CAP_512, CAP_WIDE, CAP_FLOOR, CAP_MANY) == (4960, 5040, 1440, cases.CAPACITIES["20x20"])
SWITCHES = ("EBO_EVAL_INTERIOR", "EBO_EVAL_BLOCK", "EBO_LDS_KB", "EBO_EVAL_TILES")

GRID = [(20 * i, 20 * j, 20, 20) for j in range(4) for i in range(5)]
USABLE = [k for k, r in enumerate(GRID) if r[0] >= 40 and r[1] >= 40]  # no warped coordinate below 0, where trunc is not floor
WIDE_RECT = (20, 40, 70, 20)

# name: (lo, hi of the centre taps, events, admitted at CAP_512 / CAP_FLOOR / CAP_MANY)
BOXES = {
    "xmin3": ((3, 22), (45, 34), 300, (True, True, True)),
    "xmin2": ((2, 22), (45, 34), 300, (False, False, False)),
    "xmax56": ((14, 22), (56, 34), 300, (True, True, True)),
    "xmax57": ((14, 22), (57, 34), 300, (False, False, False)),
    "ymin3": ((22, 3), (34, 45), 300, (True, True, True)),
    "ymin2": ((22, 2), (34, 45), 300, (False, False, False)),
    "ymax56": ((22, 14), (34, 56), 300, (True, True, True)),
    "ymax57": ((22, 14), (34, 57), 300, (False, False, False)),
    "full": ((3, 3), (56, 56), 400, (True, False, False)),        # 61 x 60 pixels: two sub-bands below 3660
    "rows_eq": ((10, 12), (43, 40), 300, (True, True, True)),     # pitch 41, 35 rows = 1440 // 41
    "rows_over": ((10, 12), (43, 41), 300, (True, False, True)),  # 36 rows
    "few": ((15, 15), (44, 44), 150, (True, True, True)),         # below two rounds of 128 lanes: not dealt
}
NO_TABLE = ("outside", "wide")
_cache = {}


def _model():
    if "model" not in _cache:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "event-based-odomety_amd", "tools", "ab",
                            "lds_conflict_model.py")
        spec = importlib.util.spec_from_file_location("lds_conflict_model", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _cache["model"] = mod
    return _cache["model"]


def _scene(copies=3, wide=True):
    """rects (the grid `copies` times, then the 70-wide rect), and per unit name: rect index, events, flow"""
    key = ("scene", copies, wide)
    if key in _cache:
        return _cache[key]
    rects = GRID * copies + ([WIDE_RECT] if wide else [])
    units = {}
    slots = [u + 20 * c for c in range(copies) for u in USABLE]
    names = list(BOXES) + ["outside", "inactive", "plain"]
    assert len(names) <= len(slots)
    for k, name in enumerate(names):
        i = slots[k]
        if name in BOXES:
            lo, hi, n, _ = BOXES[name]
            ev, flow = cases.make_unit(rects[i], lo, hi, n, seed=8100 + k)
            box = cases.unit_box(ev, rects[i], flow)
            assert box["ok"].all() and (box["pxc"].min(), box["pyc"].min()) == lo and (box["pxc"].max(), box["pyc"].max()) == hi
            # the first event's footprint ends on the box's last column and last row, the last event's begins on its first
            # (where the canvas does not cut the box)
            assert not BOXES[name][3][0] or ((box["pxc"][0] + 3, box["pyc"][0] + 3) == (box["x0"] + box["bw"] - 1, box["y0"] + box["rows"] - 1)
                                             and (box["pxc"][-1] - 3, box["pyc"][-1] - 3) == (box["x0"], box["y0"]))
        else:
            ev, flow = cases.make_unit(rects[i], (15, 15), (44, 44), 50 if name == "inactive" else 300, seed=8100 + k)
            if name == "outside":
                ev["x"][len(ev) // 2] = rects[i][0] - 1  # one event outside its rect, next to the reference time
        units[name] = (i, ev, flow)
    if wide:
        rng = np.random.default_rng(8200)
        ev = np.zeros(300, dtype=cases.EVENT_DTYPE)
        ev["x"], ev["y"] = WIDE_RECT[0] + rng.integers(0, 70, 300), WIDE_RECT[1] + rng.integers(0, 20, 300)
        ev["sign"], ev["t_us"] = 1, cases.T0_US + np.sort(rng.integers(0, 50_000, 300))
        units["wide"] = (len(rects) - 1, ev, (0.3, -0.2))
    _cache[key] = (np.array(rects, dtype=np.int32), units)
    return _cache[key]


def _assemble(rects, units, only=None):
    """events, offsets and flows of the scene with the units `only` (all by default) in their rects, the others empty"""
    held = {i: (ev, flow) for name, (i, ev, flow) in units.items() if only is None or name in only}
    counts = np.array([len(held[i][0]) if i in held else 0 for i in range(len(rects))], dtype=np.int64)
    flows = np.zeros((len(rects), 2))
    for i, (_, flow) in held.items():
        flows[i] = flow
    ev = np.concatenate([held[i][0] for i in sorted(held)])
    return ev, np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), flows


def _ctx(lib, n_events, n_rects, **kw):
    sigma = kw.pop("sigma", None)
    args = dict(image_w=IMAGE[0], image_h=IMAGE[1], patch_w=PATCH[0], patch_h=PATCH[1], loss=lib.LOSS_VARIANCE, tv_weight=0.0,
                scale=SCALE, min_events=MIN_EVENTS, max_events=int(n_events), max_windows=-(-n_rects // len(GRID)))
    args.update(kw)
    p = lib.default_params(**args)
    if sigma is not None:
        p.k.sigma_compensate = sigma
    return lib.Context(p)


def _rule(c, rects, flows, cap, tiles):
    """the numpy restatement of unit_all_interior per unit of a set_patches load (inactive units: False)"""
    m = _model()
    table = c.unit_extents()
    out = np.zeros(len(rects), dtype=bool)
    for i, rect in enumerate(rects):
        if not c.patch_info(i, 0)[1]:
            continue
        ok, box = bx._rule(table[i], tuple(int(v) for v in rect), flows[i][0], flows[i][1])
        if not ok or box is None:
            continue
        _, cols, rows = m.box_base_words(*m.unpack_records(c.unit_records(0, i)), rect, flows[i], cap, SCALE)
        rw, rh = int(rect[2]), int(rect[3])
        out[i] = (tiles == 1 and box[0] >= 3 and box[1] <= 3 * rw - 4 and box[2] >= 3 and box[3] <= 3 * rh - 4
                  and rows <= max(cap // cols, 1))
    return out


class _env:
    def __init__(self, **kv):
        self.kv = kv

    def __enter__(self):
        self.saved = {k: os.environ.get(k) for k in SWITCHES}
        for k in SWITCHES:
            os.environ.pop(k, None)
        os.environ.update(self.kv)

    def __exit__(self, *a):
        for k, v in self.saved.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


def _eval_on_off(lib, rects, ev, offsets, flows, env, cap, **kw):
    """(r, J, r value-only) with the path on, the counters after each of its two launches, the restated rule; asserted:
    the same bits and no unit counted with the path off"""
    res = {}
    for sw in ("on", "off"):
        with _env(**env, **({"EBO_EVAL_INTERIOR": "0"} if sw == "off" else {})):
            with _ctx(lib, len(ev), len(rects), **kw) as c:
                c.set_patches(ev, offsets, rects)
                tiles = c.eval_launch_shape(True)[0]
                r, J = c.eval(flows[None])
                n_jac = c.interior_path_counts()
                rv = c.eval(flows[None], want_jac=False)[0]
                n_val = c.interior_path_counts()
                want = _rule(c, rects, flows, cap, tiles)
                res[sw] = (r[0], J[0], rv[0], n_jac, n_val, want, c.eval_launch_shape(True))
    on, off = res["on"], res["off"]
    for a, b in zip(on[:3], off[:3]):
        assert a.shape == b.shape and a.tobytes() == b.tobytes()
    assert (off[3], off[4]) == (0, 0)
    assert on[3] == on[4] == int(on[5].sum()), (on[3], on[4], int(on[5].sum()))
    return on


@pytest.mark.parametrize("block", [128, 256, 512])
def test_on_against_off_and_the_counter_is_the_rule(ebo_ab, block):
    rects, units = _scene()
    ev, offsets, flows = _assemble(rects, units)
    r, J, rv, n, _, want, shape = _eval_on_off(ebo_ab, rects, ev, offsets, flows, {"EBO_EVAL_BLOCK": str(block)}, CAP_WIDE)
    assert shape[:2] == (1, block)
    for name, (i, _, _) in units.items():
        expect = BOXES[name][3][0] if name in BOXES else name == "plain"
        assert want[i] == expect, name
        assert (r[i] != 0) == (name != "inactive") and ((J[i] != 0).any() == (name != "inactive")), name
    assert n == sum(b[3][0] for b in BOXES.values()) + 1
    assert np.array_equal(r, rv) and (r[[i for i in range(len(rects)) if i not in {u[0] for u in units.values()}]] == 0).all()


def test_one_unit_at_a_time(ebo_ab):
    """the counter of a load that holds ONE unit is that unit's verdict: the edges of the rule on the device, at 128 lanes
    (units of 256 events and more are dealt, `few` is not) and, forced with EBO_LDS_KB, at rowsAll == maxRows and one over"""
    rects, units = _scene(copies=3, wide=False)
    total = sum(len(u[1]) for u in units.values())
    for col, (env, cap) in enumerate((({"EBO_EVAL_BLOCK": "128"}, CAP_512), ({"EBO_EVAL_BLOCK": "128", "EBO_LDS_KB": "4"}, CAP_FLOOR))):
        with _env(**env), _ctx(ebo_ab, total, len(rects)) as c:
            for name in BOXES if col == 0 else ("rows_eq", "rows_over", "xmin3", "xmin2", "full", "few"):
                ev, offsets, flows = _assemble(rects, units, only=(name,))
                c.set_patches(ev, offsets, rects)
                assert c.eval_launch_shape(True)[:2] == (1, 128)
                r, J = c.eval(flows[None])
                got = c.interior_path_counts()
                assert got == int(BOXES[name][3][col]) == int(_rule(c, rects, flows, cap, 1).sum()), (name, env, got)
                i = units[name][0]
                assert r[0][i] != 0 and np.count_nonzero(r[0]) == 1
    rects, units = _scene()
    with _env(EBO_EVAL_BLOCK="128"), _ctx(ebo_ab, total + 300, len(rects)) as c:
        for name in NO_TABLE + ("inactive", "plain"):
            ev, offsets, flows = _assemble(rects, units, only=(name,))
            c.set_patches(ev, offsets, rects)
            c.eval(flows[None])
            assert c.interior_path_counts() == int(name == "plain"), name
            assert c.box_path_counts() == {"plain": (0, 1), "inactive": (0, 0)}.get(name, (1, 0)), name


def test_sub_bands_and_row_tiles(ebo_ab):
    rects, units = _scene(copies=3, wide=False)
    ev, offsets, flows = _assemble(rects, units)
    _, _, _, n, _, want, shape = _eval_on_off(ebo_ab, rects, ev, offsets, flows, {"EBO_EVAL_BLOCK": "128", "EBO_LDS_KB": "4"}, CAP_FLOOR)
    for name, (i, _, _) in units.items():
        assert want[i] == (BOXES[name][3][1] if name in BOXES else name == "plain"), name
    assert shape[0] == 1 and 0 < n < sum(b[3][0] for b in BOXES.values())
    _, _, _, n, _, want, shape = _eval_on_off(ebo_ab, rects, ev, offsets, flows, {"EBO_EVAL_TILES": "2"}, CAP_512)
    assert shape[0] == 2 and n == 0 and not want.any()  # a launch with row tiles: nobody is admitted


@pytest.mark.parametrize("variant", ["central", "sigma<1", "sigma<1 block 128"])
def test_central_differences_and_sigma_below_one(ebo_ab, variant):
    rects, units = _scene()
    ev, offsets, flows = _assemble(rects, units)
    kw = {"grad": ebo_ab.GRAD_CENTRAL} if variant == "central" else {"sigma": 0.7}
    env = {"EBO_EVAL_BLOCK": "128"} if variant.endswith("128") else {}
    r, J, _, n, _, _, shape = _eval_on_off(ebo_ab, rects, ev, offsets, flows, env, CAP_WIDE, **kw)
    assert shape[2] == (5 if variant == "central" else 1) and n > 0  # (five flow sets; the first one is counted)
    assert (J != 0).any()


def _windows():
    """two windows over the grid: a few hundred events per patch, two patches below min_events, strays outside the image"""
    if "windows" not in _cache:
        rng = np.random.default_rng(8300)
        evs = []
        for w in range(2):
            parts = []
            for p, (x0, y0, rw, rh) in enumerate(GRID):
                n = 40 if p in (3 + w, 11) else int(rng.integers(260, 420))
                parts.append((x0 + rng.integers(0, rw, n), y0 + rng.integers(0, rh, n), rng.integers(0, 40_001, n)))
            parts.append((np.full(5, IMAGE[0] + 7), rng.integers(0, IMAGE[1], 5), rng.integers(0, 40_001, 5)))
            x, y, t = (np.concatenate(a) for a in zip(*parts))
            t[0], t[-6] = 0, 40_000  # (the window's time range is that of its patch events: the strays are the last five)
            o = np.argsort(t, kind="stable")
            ev = np.zeros(len(x), dtype=cases.EVENT_DTYPE)
            ev["x"], ev["y"], ev["t_us"], ev["sign"] = x[o], y[o], t[o] + cases.T0_US + w * 80_000, 1
            evs.append(ev)
        flows = rng.uniform(-0.9, 0.9, (2, len(GRID), 2))
        flows[0, :4] *= 2.0  # boxes that reach the canvas's edge
        flows[0, 0] = (1.7, -1.6)  # 34 pixels at the window's ends: events leave the canvas, the box comes from the event pass
        _cache["windows"] = (evs, np.concatenate([[0], np.cumsum([len(e) for e in evs])]).astype(np.uint64), flows)
    return _cache["windows"]


@pytest.mark.parametrize("block", [128, 512])
def test_windows_with_strays_and_inactive_patches(ebo, ebo_ab, orc, block):
    evs, offsets, flows = _windows()
    P = len(GRID)
    res = {}
    for sw in ("on", "off"):
        with _env(EBO_EVAL_BLOCK=str(block), **({"EBO_EVAL_INTERIOR": "0"} if sw == "off" else {})):
            with _ctx(ebo_ab, offsets[-1], 2 * P) as c:
                c.set_windows(np.concatenate(evs), offsets)
                res[sw] = c.eval(flows) + (c.interior_path_counts(), c.box_path_counts())
                if sw == "on":
                    table, m, want = c.unit_extents(), _model(), 0
                    active = np.array([[c.patch_info(p, w)[1] for p in range(P)] for w in range(2)], dtype=bool)
                    for w in range(2):
                        for p in np.flatnonzero(active[w]):
                            ok, box = bx._rule(table[w * (P + 1) + p], GRID[p], *flows[w, p])
                            if ok and box is not None:
                                _, cols, rows = m.box_base_words(*m.unpack_records(c.unit_records(w, p)), GRID[p], flows[w, p], CAP_512, SCALE)
                                want += bool(box[0] >= 3 and box[1] <= 56 and box[2] >= 3 and box[3] <= 56 and rows <= CAP_512 // cols)
    (r, J, n, paths), (r0, J0, n0, paths0) = res["on"], res["off"]
    assert r.tobytes() == r0.tobytes() and J.tobytes() == J0.tobytes()
    assert n0 == 0 and n == want and 0 < n < active.sum() and paths == paths0 and paths[0] > 0
    assert (~active).sum() == 4 and (r[~active] == 0).all() and (J[~active] == 0).all() and (r[active] != 0).all()
    if block == 512:  # the shipped library's shape for 40 slots: its bits, and the oracle's value and Jacobian
        with _ctx(ebo, offsets[-1], 2 * P) as c:
            c.set_windows(np.concatenate(evs), offsets)
            assert c.eval_launch_shape(True)[:2] == (1, 512)
            rs, Js = c.eval(flows)
        assert rs.tobytes() == r.tobytes() and Js.tobytes() == J.tobytes()
        prm = orc.default_params(image_w=IMAGE[0], image_h=IMAGE[1], patch_w=PATCH[0], patch_h=PATCH[1], loss=1, tv_weight=0.0)
        ro, Jo, act, _ = orc.window_eval(evs[0][evs[0]["x"] < IMAGE[0]], prm, flows[0])  # (without the strays)
        assert np.array_equal(np.asarray(act, dtype=bool), active[0])
        np.testing.assert_allclose(rs[0], ro, rtol=1e-9, atol=1e-12)
        assert_jac_close(Js[0], Jo)


def test_lock_step_solve(ebo_ab):
    """a lock-step solve (rounds with per-slot modes 0 / 1 / 2): the same flows and statistics with the path off"""
    evs, offsets, _ = _windows()
    res = {}
    for sw in ("on", "off"):
        with _env(**({"EBO_EVAL_INTERIOR": "0"} if sw == "off" else {})):
            with _ctx(ebo_ab, offsets[-1], 2 * len(GRID), tv_weight=1e3) as c:
                c.set_windows(np.concatenate(evs), offsets)
                opts = ebo_ab.default_solver()
                opts.max_num_iterations = 6
                flows, summ = c.solve(opts)
                res[sw] = (flows.copy(), [(s.iterations, s.final_cost, s.termination, s.num_evals_cost, s.num_evals_jac) for s in summ])
    assert res["on"][0].tobytes() == res["off"][0].tobytes() and res["on"][1] == res["off"][1]
    assert (res["on"][0] != 0).any()


@pytest.mark.parametrize("copies,block,col", [(3, 512, 0), (52, 128, 2)], ids=["61 rects", "1040 rects"])
def test_shipped_library_against_the_oracle(ebo, ebo_ab, orc, copies, block, col):
    """the shipped plan: 512 lanes and 4960 pixels below 1024 slots, 128 lanes and 2540 pixels from there (units of 256
    events and more are dealt there); every hand-made unit against the oracle's contrastFunctor, and the A/B library's bits"""
    rects, units = _scene(copies=copies, wide=col == 0)  # (the 70-wide rect would raise the capacity of the 128-lane plan)
    ev, offsets, flows = _assemble(rects, units)
    with _env(), _ctx(ebo, len(ev), len(rects)) as c:
        c.set_patches(ev, offsets, rects)
        assert c.eval_launch_shape(True)[:2] == (1, block)
        r, J = c.eval(flows[None])
        rv = c.eval(flows[None], want_jac=False)[0]
        with pytest.raises(ebo.EboError):
            c.interior_path_counts()
    ra, Ja, rva, n, _, want, _ = _eval_on_off(ebo_ab, rects, ev, offsets, flows, {}, CAP_MANY if col == 2 else CAP_WIDE)
    assert r[0].tobytes() == ra.tobytes() and J[0].tobytes() == Ja.tobytes() and rv[0].tobytes() == rva.tobytes()
    assert n == sum(b[3][col] for b in BOXES.values()) + 1
    for name, (i, uev, flow) in units.items():
        if name == "inactive":
            assert r[0][i] == 0
            continue
        ro, Jo = orc.contrast_eval(uev, rects[i], flow, 1, scale=SCALE)
        np.testing.assert_allclose(r[0][i], ro, rtol=1e-9, atol=1e-12, err_msg=name)
        assert_jac_close(J[0][i], Jo)
        assert ro != 0.0 and np.abs(Jo).max() > 0.0
