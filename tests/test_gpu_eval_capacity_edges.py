"""GPU: the variance evaluation at the edges of its image capacity (csrc/eval_plan.h).

With 1024 flow slots or more on a small canvas a workgroup owns 20 480 B of LDS: a 20-double header and an image of 2540
pixels (2656 before the plan).  A box that does not fit is walked in sequential sub-bands of capacity // pitch rows.
The smallest shape that takes this branch: ten windows of the reference's geometry (240 x 180, 20 x 20 patches: 1080
slots), 4000 events per window, units active from ten events.  The flows of chosen units are searched on the host, with
the numpy restatement of warp_event and of the box rule (tools/ab/box_sizes.py), so that among the units there are

  fit       boxes of exactly capacity // pitch rows (the last row count that fits one sub-band)
  over      boxes one row over: two sub-bands, the second one row high, with footprints that straddle the cut
  far       boxes five rows over: events centred on either side of the cut straddle it
  between   boxes of more than 2540 and at most 2656 pixels (one sub-band before, two now)
  clipped   boxes clipped by the canvas

and every other unit sits at 0.5 x its ground truth.  Value and Jacobian against the oracle -- r at test_gpu_parity.py's
rtol 1e-9 / atol 1e-12, J at jac_check.assert_jac_close's bounds -- and one window in a batch of its own (ten copies: 1080
slots) against its bits inside the ten.  One oracle evaluation per window.  These units hold about 37 events, below the two
full rounds the bank deal needs, so none of them is dealt: the dealt counterpart, boxes that leave exactly enough room for
the list, lives in tests/test_gpu_eval_deal_fit.py."""
import importlib.util
import os

import numpy as np
import pytest

from jac_check import assert_jac_close

pytestmark = pytest.mark.gpu

CONFIG = 0
WINDOWS = 10
N_EVENTS = 4000
MIN_EVENTS = 10
CAP_NEW = (20480 - 20 * 8) // 8   # 2540
CAP_OLD = (22 * 1024 - 160 * 8) // 8  # 2656
CLASSES = ("fit", "over", "far", "between", "clipped")

_cache = {}


def _box_sizes():
    if "mod" not in _cache:
        path = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "event-based-odomety_amd", "tools", "ab",
                            "box_sizes.py")
        spec = importlib.util.spec_from_file_location("box_sizes", path)
        mod = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(mod)
        _cache["mod"] = mod
    return _cache["mod"]


def _extent(bs, ev, rect, axis, m):
    """box extent (lo, n) along one axis at flow component m (the other axis does not move: its flow is zero)"""
    flow = (m, 0.0) if axis == 0 else (0.0, m)
    c = bs.unit_centres(ev, rect, flow)[axis]
    size = 3 * int(rect[2 + axis])
    lo, hi = max(c.min() - 3, 0), min(c.max() + 3, size - 1)
    return lo, hi - lo + 1


def _search(bs, ev, rect, cls):
    """a flow that puts the unit's box into class `cls`, or None.  Columns follow m0 alone and rows m1 alone (as long
    as no event leaves the canvas), so the two are searched one after the other."""
    grid = np.arange(0.30, 1.60, 0.01)
    if cls == "clipped":
        return (1.45, -1.45)
    for m0 in grid[::4]:
        _, bw = _extent(bs, ev, rect, 0, m0)
        cols = bw | 1
        if cols < 45 or cols >= 57:
            continue
        fit = CAP_NEW // cols
        want = {"fit": [fit], "over": [fit + 1], "far": [fit + 5],
                "between": [r for r in range(fit + 1, fit + 4) if CAP_NEW < cols * r <= CAP_OLD]}[cls]
        for m1 in grid:
            _, rows = _extent(bs, ev, rect, 1, m1)
            if rows in want and rows < 3 * int(rect[3]):
                return (m0, m1)
    return None


def _setup(synth):
    """events, offsets, flows [W][P][2] and per class the (window, patch) units the restatement puts there"""
    if "setup" in _cache:
        return _cache["setup"]
    bs = _box_sizes()
    cfg = synth.CONFIGS[CONFIG]
    _, _, rects = synth.grid_rects(cfg["image"], cfg["patch"])
    evs, flows = [], []
    for w in range(WINDOWS):
        ev, gt = synth.make_window(CONFIG, window=w, n_events=N_EVENTS)
        f = gt * 0.5
        # every fifth patch of the window is placed, the classes in turn
        for k, p in enumerate(range(w % 5, len(rects), 5)):
            if bs.unit_centres(ev, rects[p], (0.0, 0.0))[2] <= MIN_EVENTS:
                continue
            found = _search(bs, ev, rects[p], CLASSES[(k + w) % len(CLASSES)])
            if found is not None:
                f[p] = found
        evs.append(ev)
        flows.append(f)
    # classify by the restatement at the flows actually used
    units = {c: [] for c in CLASSES}
    for w in range(WINDOWS):
        boxes = bs.unit_boxes(evs[w], rects, flows[w], min_events=MIN_EVENTS)
        for p, (active, x0, y0, bw, rows) in enumerate(boxes):
            if not active or bw == 0:
                continue
            rw, rh = int(rects[p][2]), int(rects[p][3])
            cols = bs.pitch(int(bw), CAP_NEW)
            fit = CAP_NEW // cols
            pyc = bs.unit_centres(evs[w], rects[p], flows[w][p])[1]
            cut = y0 + fit  # first row of the second sub-band
            straddle = (pyc - 3 < cut) & (cut <= pyc + 3)
            if rows == fit:
                units["fit"].append((w, p))
            if rows == fit + 1 and straddle.any():
                units["over"].append((w, p))
            if rows >= fit + 4 and bs.sub_bands(int(bw), int(rows), CAP_NEW) == 2 and (straddle & (pyc < cut)).any() and (straddle & (pyc >= cut)).any():
                units["far"].append((w, p))
            if bs.sub_bands(int(bw), int(rows), CAP_NEW) == 2 and bs.sub_bands(int(bw), int(rows), CAP_OLD) == 1:
                units["between"].append((w, p))
            if x0 == 0 or y0 == 0 or x0 + bw == 3 * rw or y0 + rows == 3 * rh:
                units["clipped"].append((w, p))
    offsets = np.zeros(WINDOWS + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(e) for e in evs])
    _cache["setup"] = (evs, offsets, np.stack(flows), units, rects)
    return _cache["setup"]


def _ctx(lib, synth, n_events):
    cfg = synth.CONFIGS[CONFIG]
    p = lib.default_params(image_w=cfg["image"][0], image_h=cfg["image"][1], patch_w=cfg["patch"][0], patch_h=cfg["patch"][1],
                           loss=lib.LOSS_VARIANCE, min_events=MIN_EVENTS, max_events=int(n_events), max_windows=WINDOWS)
    return lib.Context(p)


def _device(lib, synth):
    """(r, J) of the ten windows in one batch, computed once"""
    if "device" not in _cache:
        evs, offsets, flows, _, _ = _setup(synth)
        with _ctx(lib, synth, offsets[-1]) as c:
            c.set_windows(np.concatenate(evs), offsets)
            assert WINDOWS * c.P >= 1024 and c.eval_launch_shape(True)[:2] == (1, 128)
            assert c.eval_resident_workgroups(True)[0] == 8
            # the restatement's buckets and reference times are the library's
            bs, rects = _box_sizes(), _setup(synth)[4]
            for p in (0, 53, 107):
                n, _, t_ref = c.patch_info(p, 3)
                x, y, w, h = rects[p]
                e = evs[3]
                t = e["t_us"][(e["x"] >= x) & (e["x"] < x + w) & (e["y"] >= y) & (e["y"] < y + h)]
                assert len(t) == n and bs.ref_time(int(t[0]), int(t[-1])) == t_ref
            r, J = c.eval(flows)
            r1, _ = c.eval(flows, want_jac=False)
        assert np.array_equal(r1, r)  # the value does not know whether the scatter formed D1 beside it
        r.setflags(write=False)
        J.setflags(write=False)
        _cache["device"] = (r, J)
    return _cache["device"]


def test_every_class_of_box_is_there(synth):
    _, _, _, units, _ = _setup(synth)
    for cls in CLASSES:
        assert len(units[cls]) > 0, (cls, {k: len(v) for k, v in units.items()})


def test_value_and_jacobian_against_the_oracle(ebo, orc, synth):
    evs, _, flows, units, _ = _setup(synth)
    r, J = _device(ebo, synth)
    prm = orc.default_params(image_w=240, image_h=180, patch_w=20, patch_h=20, loss=1, tv_weight=0.0, min_events=MIN_EVENTS)
    placed = {u for cls in CLASSES for u in units[cls]}
    for w in range(WINDOWS):
        ro, Jo, active, _ = orc.window_eval(evs[w], prm, flows[w])
        assert active.sum() > 50
        assert all(active[p] for (ww, p) in placed if ww == w)
        np.testing.assert_allclose(r[w], ro, rtol=1e-9, atol=1e-12)
        assert_jac_close(J[w], Jo)
    assert np.abs(J).max() > 0.0


def test_a_window_in_a_batch_of_its_own_has_the_same_bits(ebo, synth):
    """window 3, ten times over: the same side of 1024 slots, so the same shape, so the same bits"""
    evs, _, flows, units, _ = _setup(synth)
    r, J = _device(ebo, synth)
    w = 3
    assert any(ww == w for cls in ("over", "between") for (ww, _) in units[cls])
    offsets = np.arange(WINDOWS + 1, dtype=np.uint64) * np.uint64(len(evs[w]))
    with _ctx(ebo, synth, offsets[-1]) as c:
        c.set_windows(np.concatenate([evs[w]] * WINDOWS), offsets)
        assert WINDOWS * c.P >= 1024
        rb, Jb = c.eval(np.stack([flows[w]] * WINDOWS))
    for k in (0, WINDOWS - 1):
        assert np.array_equal(rb[k], r[w])
        assert np.array_equal(Jb[k], J[w])
