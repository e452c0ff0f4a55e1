"""GPU: k_eval3's bank deal (csrc/eval_deal.h) at the fit boundary of every shipped launch plan (csrc/eval_plan.h).

A unit is dealt when the list of its events' 16-bit indices fits behind the largest sub-band's image: L + P <= capacity.  At
P + L == capacity the image's last pixel is the double in front of the list, so a pitch, a row count, a capacity or a header
that differs between the rule, the plan and the kernel by one lets the zeroing or a tap overwrite indices the gather pass
addresses the events with.  tests/deal_fit_cases.py builds, per shape of the plan (20 x 20, 21 x 16 with a 31-wide column,
30 x 22, and the first and the last at sigma < 1), a scene of 1040 .. 1088 patches of which a dozen hold hand-built units
exactly at, one double of list over, one row over and far from that boundary, at both ends of the admitted counts, with a
box cut by the canvas and rejected events, and -- in a 31-wide rect -- in two sub-bands; tests/test_deal_fit_cases_cpu.py
holds the scenes against the rule.  No launch here forces a block or an LDS size: the plan is the shipped one.  Per shape:

  * the launch is the plan's (1 tile, 128 or 256 lanes, 8 / 4 / 6 / 3 workgroups per CU planned and resident);
  * the list read back (A/B library) is tools/ab/lds_conflict_model.py's dealt_list of the unit's records at the capacity
    written out from eval_plan.h, a permutation where the scene says dealt and empty where not, with and without Jacobian;
  * against EBO_EVAL_DEAL=0: r bit for bit, J bit for bit where not dealt and within jac_check's bounds (and not equal
    everywhere) where dealt; the same evaluation twice: the same bits;
  * r and J of every unit against the oracle's contrastFunctor on the same events, rect and flow, at the suite's parity
    bounds (r: rtol 1e-9, atol 1e-12; J: jac_check.assert_jac_close);
  * the shipped library has the A/B library's bits; EBO_EVAL_BOX=events has the default's lists and bits, and the default
    took the table for every unit without rejected events; the fit units in other patches, the patches back to front and
    EBO_EVAL_ORDER=index leave every unit's list and bits alone.

Window path: ten windows of the reference geometry (1080 slots) with 36 000 events each, about 330 per patch, so that the
placed units hold the 256 events the deal needs.  With L >= 64 and a pitch of at most 61 a unit here is never dealt at capacity // pitch rows (a
full sub-band leaves less than a pitch), so the boundary is rows == (capacity - L) // pitch: in window 3 flows are
searched on the host (tools/ab/box_sizes.py) for units at that row count (dealt), one row over (not dealt), in two
sub-bands (not dealt) and clipped by the canvas; lists against the restatement, the window against the oracle and against
its bits in a batch of ten copies."""
import importlib.util
import os
import time

import numpy as np
import pytest

import deal_fit_cases as cases
from jac_check import assert_jac_close

pytestmark = pytest.mark.gpu

NAMES = list(cases.SHAPES)
_cache = {}


def _tool(name):
    if name not in _cache:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "event-based-odomety_amd", "tools", "ab",
                            name + ".py")
        spec = importlib.util.spec_from_file_location(name, path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _cache[name] = mod
    return _cache[name]


def _ctx(lib, name, n_events):
    S = cases.SHAPES[name]
    (W, H), (rw, rh) = S["image"], S["rect"]
    grid = (W // rw) * (H // rh)
    p = lib.default_params(image_w=W, image_h=H, patch_w=rw, patch_h=rh, loss=lib.LOSS_VARIANCE, tv_weight=0.0, scale=cases.SCALE,
                           max_events=int(n_events), max_windows=-(-S["patches"] // grid))
    if S["sigma"] is not None:
        p.k.sigma_compensate = S["sigma"]
    return lib.Context(p)


def _run(lib, which, name, order="normal", env=None):
    """One evaluation set of one scene, computed once: r, J (twice), the value-only r, the launch's shape and residency;
    from the A/B library (which == "ab") also every unit's list with and without Jacobian, its records, the box path counts
    and the [patches][3] output of the last list launch.  env: A/B switches set for the load and the launches."""
    key = (which, name, order, tuple(sorted((env or {}).items())))
    if key in _cache:
        return _cache[key]
    ev, offsets, rects, flows, index = cases.assemble(name, order)
    saved = {k: os.environ.get(k) for k in (env or {})}
    t0 = time.perf_counter()
    try:
        os.environ.update(env or {})
        with _ctx(lib, name, len(ev)) as c:
            c.set_patches(ev, offsets, rects)
            out = dict(index=index, rects=rects, flows=flows, shape=(c.eval_launch_shape(True), c.eval_launch_shape(False)),
                       resident=(c.eval_resident_workgroups(True), c.eval_resident_workgroups(False)))
            (r, J), (r2, J2) = c.eval(flows[None]), c.eval(flows[None])
            out.update(r=r[0], J=J[0], r2=r2[0], J2=J2[0])
            if which == "ab":
                out["paths"] = c.box_path_counts()
            out["r_val"] = c.eval(flows[None], want_jac=False)[0][0]
            if which == "ab":
                import torch
                d_flows = torch.from_numpy(flows).to("cuda")
                d_out = torch.zeros((len(rects), 3), dtype=torch.float64, device="cuda")
                d_val = torch.zeros((len(rects), 3), dtype=torch.float64, device="cuda")
                out["lists"] = [c.unit_deal(i, d_flows.data_ptr(), 1, d_out.data_ptr()) for i in index]
                out["lists_val"] = [c.unit_deal(i, d_flows.data_ptr(), 0, d_val.data_ptr()) for i in index]
                out["records"] = [c.unit_records(0, i) for i in index]
                out["device"] = d_out.cpu().numpy().copy()
    finally:
        for k, v in saved.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v
    for a in out.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    print("%s, %s, %s, %s: %.2f s" % (name, which, order, env or {}, time.perf_counter() - t0))
    _cache[key] = out
    return out


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("name", NAMES)
def test_the_plan_is_the_shipped_one(ebo, ebo_ab, name):
    S = cases.SHAPES[name]
    for lib, which in ((ebo, "shipped"), (ebo_ab, "ab")):
        got = _run(lib, which, name)
        assert len(got["rects"]) >= 1024
        for shape, resident in zip(got["shape"], got["resident"]):
            assert shape[:2] == (1, S["block"]), (which, shape)
            assert resident == (cases.RESIDENT[name], cases.RESIDENT[name]), (which, resident)


@pytest.mark.parametrize("name", NAMES)
def test_the_lists_are_the_restatement(ebo_ab, name):
    S = cases.SHAPES[name]
    m = _tool("lds_conflict_model")
    got = _run(ebo_ab, "ab", name)
    units = cases.units_of(name)
    for k, u in enumerate(units):
        i = got["index"][k]
        assert len(got["records"][k]) == u["n"]
        want = m.dealt_list(got["records"][k], got["rects"][i], u["flow"], S["block"], S["cap"], scale=cases.SCALE)
        assert len(want) == (u["n"] if u["dealt"] else 0), (u["name"], len(want))
        for lst in (got["lists"][k], got["lists_val"][k]):
            assert np.array_equal(lst, want), (u["name"], len(lst), len(want))
        if u["dealt"]:
            assert np.array_equal(np.sort(got["lists"][k]), np.arange(u["n"]))
    print("%s: " % name + ", ".join("%s n=%d %dx%d %s" % (u["name"], u["n"], u["bw"], u["rows"], "dealt" if u["dealt"] else "not")
                                    for u in units))
    # the launch that read the last list back computed what ebo_eval computes
    assert _same(got["device"][:, 0], got["r"]) and _same(got["device"][:, 1:], got["J"])


@pytest.mark.parametrize("name", NAMES)
def test_deal_on_against_deal_off_and_twice(ebo_ab, name):
    on = _run(ebo_ab, "ab", name)
    off = _run(ebo_ab, "ab", name, env={"EBO_EVAL_DEAL": "0"})
    units = cases.units_of(name)
    assert all(len(l) == 0 for l in off["lists"] + off["lists_val"])
    assert _same(on["r"], on["r2"]) and _same(on["J"], on["J2"])  # the same launch twice
    assert _same(on["r"], off["r"]) and _same(on["r_val"], off["r"]) and _same(off["r_val"], off["r"])
    dealt = np.zeros(len(on["r"]), dtype=bool)
    dealt[[i for u, i in zip(units, on["index"]) if u["dealt"]]] = True
    assert _same(on["J"][~dealt], off["J"][~dealt])
    assert_jac_close(on["J"][dealt], off["J"][dealt])
    moved = (on["J"][dealt] != off["J"][dealt]).any(axis=1)
    print("%s: J of %d of %d dealt units differs from the canonical order's" % (name, int(moved.sum()), int(dealt.sum())))
    assert moved.any()
    active = np.zeros(len(on["r"]), dtype=bool)
    active[on["index"]] = True
    assert (on["r"][active] != 0).all() and (on["r"][~active] == 0).all() and (on["J"][~active] == 0).all()


@pytest.mark.parametrize("name", NAMES)
def test_against_the_oracle(ebo, orc, name):
    S = cases.SHAPES[name]
    got = _run(ebo, "shipped", name)
    k_ = orc.default_consts()
    if S["sigma"] is not None:
        k_.sigma_compensate = S["sigma"]
    units = cases.units_of(name)
    assert {u["cls"] for u in units} >= set(cases.ORACLE_CLASSES) & set(cases.classes_of(name))
    for u, i in zip(units, got["index"]):
        if u["n"] > 3072:
            continue
        ro, Jo = orc.contrast_eval(u["ev"], got["rects"][i], u["flow"], 1, scale=cases.SCALE, consts=k_)
        print("%s %s: r %.17g oracle %.17g; J %r oracle %r" % (name, u["name"], got["r"][i], ro, got["J"][i], Jo))
        np.testing.assert_allclose(got["r"][i], ro, rtol=1e-9, atol=1e-12, err_msg=u["name"])
        assert_jac_close(got["J"][i], Jo)
        assert ro != 0.0 and np.abs(Jo).max() > 0.0


@pytest.mark.parametrize("name", NAMES)
def test_the_shipped_library_has_the_ab_librarys_bits(ebo, ebo_ab, name):
    a, b = _run(ebo, "shipped", name), _run(ebo_ab, "ab", name)
    for key in ("r", "J", "r_val"):
        assert _same(a[key], b[key]), key
    assert _same(a["r"], a["r2"]) and _same(a["J"], a["J2"])


@pytest.mark.parametrize("name", NAMES)
def test_both_box_paths(ebo_ab, name):
    """the table gives a unit's box where warp_event rejects none of its events (csrc/box_extents.h): every unit here
    but the clipped one, so the fit units' boxes came from the table in the default run, and from the event pass under
    EBO_EVAL_BOX=events -- the same box, so the same lists and bits"""
    table = _run(ebo_ab, "ab", name)
    events = _run(ebo_ab, "ab", name, env={"EBO_EVAL_BOX": "events"})
    units = cases.units_of(name)
    rejecting = sum(u["rejected"] > 0 for u in units)
    assert rejecting == 1 and all(u["rejected"] == 0 for u in units if u["cls"] in ("fit", "full_canvas"))
    assert table["paths"] == (rejecting, len(units) - rejecting)
    assert events["paths"] == (len(units), 0)
    for key in ("r", "J", "r_val"):
        assert _same(table[key], events[key]), key
    for k, u in enumerate(units):
        assert np.array_equal(table["lists"][k], events["lists"][k]), u["name"]
        assert np.array_equal(table["lists_val"][k], events["lists_val"][k]), u["name"]


@pytest.mark.parametrize("variant", ["moved", "reversed", "index-order"])
@pytest.mark.parametrize("name", NAMES)
def test_placement_does_not_matter(ebo_ab, name, variant):
    base = _run(ebo_ab, "ab", name)
    if variant == "index-order":
        other = _run(ebo_ab, "ab", name, env={"EBO_EVAL_ORDER": "index"})
    else:
        other = _run(ebo_ab, "ab", name, order=variant)
    units = cases.units_of(name)
    if variant != "index-order":
        assert sum(i != j for i, j in zip(base["index"], other["index"])) >= 2
    for k, u in enumerate(units):
        i, j = base["index"][k], other["index"][k]
        assert np.array_equal(base["rects"][i], other["rects"][j])
        assert np.array_equal(base["lists"][k], other["lists"][k]), u["name"]
        assert np.array_equal(base["lists_val"][k], other["lists_val"][k]), u["name"]
        for key in ("r", "J", "r_val"):
            assert _same(base[key][i], other[key][j]), (u["name"], key)
    active = np.zeros(len(other["r"]), dtype=bool)
    active[other["index"]] = True
    assert (other["r"][~active] == 0).all() and (other["J"][~active] == 0).all()


# ---- the window path --------------------------------------------------------------------------------------------------------
CONFIG, WINDOWS, N_EVENTS, W_PLACED = 0, 10, 36_000, 3
CAP, BLOCK = cases.CAPACITIES["20x20"], 128
WINDOW_CLASSES = ("fit", "over", "split", "clipped")


def _extent(bs, ev, rect, axis, m):
    """rows or columns of the box at flow component m (the other component zero: the axes do not mix while no event leaves)"""
    c = bs.unit_centres(ev, rect, (m, 0.0) if axis == 0 else (0.0, m))[axis]
    size = 3 * int(rect[2 + axis])
    return min(c.max() + 3, size - 1) - max(c.min() - 3, 0) + 1


def _search(bs, ev, rect, cls, L):
    if cls == "clipped":
        return (1.45, -1.45)
    grid = np.arange(0.30, 1.60, 0.01)
    for m0 in grid[::4]:
        cols = int(_extent(bs, ev, rect, 0, m0)) | 1
        if cols < 41 or cols >= 57:
            continue
        last = (CAP - L) // cols  # the last row count that leaves room for the list
        want = {"fit": last, "over": last + 1, "split": CAP // cols + 2}[cls]
        if want >= 3 * int(rect[3]):
            continue
        for m1 in grid:
            if _extent(bs, ev, rect, 1, m1) == want:
                return (m0, m1)
    return None


def _window_setup(synth):
    """events per window, offsets, flows [W][P][2], rects, and per class the patches of window W_PLACED the restatement puts
    there, with the rule's verdict per patch of that window"""
    if "windows" in _cache:
        return _cache["windows"]
    bs, m = _tool("box_sizes"), _tool("lds_conflict_model")
    cfg = synth.CONFIGS[CONFIG]
    _, _, rects = synth.grid_rects(cfg["image"], cfg["patch"])
    evs, flows = [], []
    for w in range(WINDOWS):
        ev, gt = synth.make_window(CONFIG, window=w, n_events=N_EVENTS)
        f = gt * 0.5
        if w == W_PLACED:
            for k, p in enumerate(range(1, len(rects), 3)):
                n = bs.unit_centres(ev, rects[p], (0.0, 0.0))[2]
                if n < 2 * BLOCK:
                    continue  # (a patch the edges' events have left: too few for the deal whatever its box)
                found = _search(bs, ev, rects[p], WINDOW_CLASSES[k % len(WINDOW_CLASSES)], (n + 3) // 4)
                if found is not None:
                    f[p] = found
        evs.append(ev)
        flows.append(f)
    ev, f = evs[W_PLACED], flows[W_PLACED]
    units = {c: [] for c in WINDOW_CLASSES}
    verdict = np.zeros(len(rects), dtype=bool)
    counts = np.zeros(len(rects), dtype=np.int64)
    for p, (active, x0, y0, bw, rows) in enumerate(bs.unit_boxes(ev, rects, f)):
        counts[p] = bs.unit_centres(ev, rects[p], f[p])[2]
        if not active or bw == 0:
            continue
        cols, L = bs.pitch(int(bw), CAP), (counts[p] + 3) // 4
        verdict[p] = m.deal_admitted(int(counts[p]), BLOCK, 1, CAP, cols, int(rows))
        bands = bs.sub_bands(int(bw), int(rows), CAP)
        if verdict[p] and rows == (CAP - L) // cols:
            units["fit"].append(p)
        admitted = 2 * BLOCK <= counts[p] <= 12 * BLOCK  # not dealt for the box's sake, not for the count's
        if admitted and not verdict[p] and bands == 1 and rows == (CAP - L) // cols + 1:
            units["over"].append(p)
        if admitted and not verdict[p] and bands == 2:
            units["split"].append(p)
        if verdict[p] and (x0 == 0 or y0 == 0 or x0 + bw == 3 * rects[p][2] or y0 + rows == 3 * rects[p][3]):
            units["clipped"].append(p)
    offsets = np.concatenate([[0], np.cumsum([len(e) for e in evs])]).astype(np.uint64)
    _cache["windows"] = (evs, offsets, np.stack(flows), rects, units, verdict, counts)
    return _cache["windows"]


def _window_ctx(lib, synth, n_events):
    cfg = synth.CONFIGS[CONFIG]
    return lib.Context(lib.default_params(image_w=cfg["image"][0], image_h=cfg["image"][1], patch_w=cfg["patch"][0],
                                          patch_h=cfg["patch"][1], loss=lib.LOSS_VARIANCE, tv_weight=0.0, max_events=int(n_events),
                                          max_windows=WINDOWS))


def _window_device(lib, synth):
    if "window device" not in _cache:
        evs, offsets, flows, _, _, _, _ = _window_setup(synth)
        with _window_ctx(lib, synth, offsets[-1]) as c:
            c.set_windows(np.concatenate(evs), offsets)
            assert WINDOWS * c.P >= 1024 and c.eval_launch_shape(True)[:2] == (1, BLOCK)
            assert c.eval_resident_workgroups(True) == (8, 8)
            r, J = c.eval(flows)
        r.setflags(write=False)
        J.setflags(write=False)
        _cache["window device"] = (r, J)
    return _cache["window device"]


def test_window_every_class_of_box_is_there(synth):
    """host arithmetic only: the searched flows put units of window 3 on either side of the list's boundary"""
    _, _, _, rects, units, verdict, counts = _window_setup(synth)
    for cls in WINDOW_CLASSES:
        assert len(units[cls]) > 0, {k: len(v) for k, v in units.items()}
        assert all(2 * BLOCK <= counts[p] <= 12 * BLOCK for p in units[cls])
    print("window %d: %d units dealt, %d not; %s" % (W_PLACED, int(verdict.sum()), int((~verdict).sum()),
                                                      {k: len(v) for k, v in units.items()}))
    assert verdict.sum() > 10 and (~verdict).sum() > 10


def test_window_lists_are_the_restatement(ebo, ebo_ab, synth):
    import torch
    evs, offsets, flows, rects, units, verdict, counts = _window_setup(synth)
    m = _tool("lds_conflict_model")
    r, J = _window_device(ebo, synth)
    placed = sorted({p for cls in WINDOW_CLASSES for p in units[cls][:3]})
    with _window_ctx(ebo_ab, synth, offsets[-1]) as c:
        c.set_windows(np.concatenate(evs), offsets)
        d_flows = torch.from_numpy(flows.reshape(-1, 2)).to("cuda")
        d_out = torch.zeros((WINDOWS * c.P, 3), dtype=torch.float64, device="cuda")
        for p in placed:
            got = c.unit_deal(W_PLACED * (c.P + 1) + p, d_flows.data_ptr(), 1, d_out.data_ptr())
            rec = c.unit_records(W_PLACED, p)
            want = m.dealt_list(rec, rects[p], flows[W_PLACED][p], BLOCK, CAP)
            assert len(rec) == counts[p] and len(want) == (counts[p] if verdict[p] else 0), p
            assert np.array_equal(got, want), (p, len(got), len(want))
        res = d_out.cpu().numpy().reshape(WINDOWS, c.P, 3)
    assert _same(res[..., 0], r) and _same(res[..., 1:], J)  # the A/B library's bits are the shipped library's


def test_window_against_the_oracle_and_alone_against_in_a_batch(ebo, orc, synth):
    evs, offsets, flows, rects, units, verdict, _ = _window_setup(synth)
    r, J = _window_device(ebo, synth)
    w = W_PLACED
    prm = orc.default_params(image_w=240, image_h=180, patch_w=20, patch_h=20, loss=1, tv_weight=0.0)
    ro, Jo, active, _ = orc.window_eval(evs[w], prm, flows[w])
    assert active.all()
    np.testing.assert_allclose(r[w], ro, rtol=1e-9, atol=1e-12)
    assert_jac_close(J[w], Jo)
    offs1 = np.arange(WINDOWS + 1, dtype=np.uint64) * np.uint64(len(evs[w]))
    with _window_ctx(ebo, synth, offs1[-1]) as c:
        c.set_windows(np.concatenate([evs[w]] * WINDOWS), offs1)
        assert c.eval_launch_shape(True)[:2] == (1, BLOCK)
        rb, Jb = c.eval(np.stack([flows[w]] * WINDOWS))
    for k in (0, WINDOWS - 1):
        assert _same(rb[k], r[w]) and _same(Jb[k], J[w])
