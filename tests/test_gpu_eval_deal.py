"""GPU: k_eval3's bank deal (csrc/eval_deal.h).

Once per evaluation a workgroup sorts its unit's events by the bank pair of their first tap (a counting sort with private
counters, order unique) and walks them in the dealt order in both tap passes.  The A/B library reads one unit's dealt list
back (ebo_unit_deal) and switches the deal off (EBO_EVAL_DEAL=0).  Here:

  * the list read back equals the numpy restatement of keys, sort and layout (tools/ab/lds_conflict_model.py: dealt_list,
    written from eval_deal.h's header comment) on 20 x 20 patches of a 240 x 180 sensor, for workgroups of 128, 256 and 512
    lanes (EBO_EVAL_BLOCK = B; at 512 no unit is dealt): units of 101, 128, 129 and about 800 events; of 2B - 1, 2B,
    2B + 1 (the lower admission bound), 12B and 12B + 1 (the upper one); a unit whose events all warp onto one pixel (a single key); a unit with events
    rejected over the canvas edge; the sigma < 1 instantiation; and units forced into two sub-bands (EBO_LDS_KB), which
    leave no room for the list and are not dealt;
  * deal on against deal off: r bit for bit (the image is an integer sum and keeps its place, pitch and sub-bands), J within
    jac_check.assert_jac_close's bounds; the same launch twice gives the same bits;
  * shipped library: a window alone and repeated in a batch on the same side of 1024 slots gives the same bits (ten
    windows: 128-lane workgroups; below 1024 slots the workgroups have 512 lanes and are not dealt), and value and
    Jacobian hold against the oracle at the existing parity bounds.
One oracle evaluation per scene; every evaluation is a few hundred thousand events at the most."""
import importlib.util
import os

import numpy as np
import pytest

from jac_check import assert_jac_close

pytestmark = pytest.mark.gpu

IMAGE, PATCH = (240, 180), (20, 20)
SCALE = 1e-3
CAP_512 = (40 * 1024 - 160 * 8) // 8      # image capacity below 1024 flow slots (eval_plan.h): 4960 pixels
CAP_FLOOR = 24 * 3 * 20                   # EBO_LDS_KB below the floor: 24 rows of the 60-pixel canvas

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


def _sizes(block):
    return [101, 128, 129, 800, 2 * block - 1, 2 * block, 2 * block + 1, 12 * block, 12 * block + 1, 3 * block, 3 * block + 7,
            4 * block + 5]


ONE_PIXEL, REJECTED, WIDE = 9, 10, 11  # indices into _sizes: the special units


def _patch_scene(ebo, block):
    """twelve patches of the grid, one per size; time-ordered events uniform over each patch over 50 ms"""
    key = ("scene", block)
    if key not in _cache:
        rng = np.random.default_rng(1900 + block)
        sizes = _sizes(block)
        rects = np.array([(20 * (p % 12), 20 * (p // 12 + 2), 20, 20) for p in range(len(sizes))], dtype=np.int32)
        parts = []
        for p, n in enumerate(sizes):
            ev = np.zeros(n, dtype=ebo.EVENT_DTYPE)
            ev["x"] = rects[p][0] + (7 if p == ONE_PIXEL else rng.integers(0, 20, n))
            ev["y"] = rects[p][1] + (11 if p == ONE_PIXEL else rng.integers(0, 20, n))
            ev["sign"] = rng.integers(0, 2, n) * 2 - 1
            ev["t_us"] = 1_000_000 + np.sort(rng.integers(0, 50_000, n))
            parts.append(ev)
        offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.uint64)
        flows = rng.uniform(-0.6, 0.6, (len(sizes), 2))
        flows[ONE_PIXEL] = 0.0           # every event on its own pixel: one key
        flows[REJECTED] = (1.45, -1.45)  # 36 px in 25 ms: the earliest and latest events leave the 60 x 60 canvas
        flows[WIDE] = (1.2, 1.2)         # a box of about 50 x 50: two sub-bands in CAP_FLOOR
        _cache[key] = (np.concatenate(parts), offsets, rects, flows)
    return _cache[key]


def _ctx(lib, n_events, sigma=None, windows=1, min_events=100):
    p = lib.default_params(image_w=IMAGE[0], image_h=IMAGE[1], patch_w=PATCH[0], patch_h=PATCH[1], loss=lib.LOSS_VARIANCE,
                           tv_weight=0.0, scale=SCALE, min_events=min_events, max_events=int(n_events), max_windows=windows)
    if sigma is not None:
        p.k.sigma_compensate = sigma
    return lib.Context(p)


def _lists(lib, block, cap, sigma=None, want_jac=True):
    """per unit of the patch scene: (list read back, restated list), and (r, J) of the evaluation that dealt"""
    import torch
    ev, offsets, rects, flows = _patch_scene(lib, block)
    m = _model()
    out = []
    with _ctx(lib, len(ev), sigma) as c:
        c.set_patches(ev, offsets, rects)
        assert c.eval_launch_shape(want_jac)[:2] == (1, block)
        d_flows = torch.from_numpy(flows).to("cuda")
        d_out = torch.zeros((len(rects), 3), dtype=torch.float64, device="cuda")
        for u in range(len(rects)):
            got = c.unit_deal(u, d_flows.data_ptr(), want_jac, d_out.data_ptr())
            want = m.dealt_list(c.unit_records(0, u), rects[u], flows[u], block, cap, scale=SCALE)
            out.append((got, want))
        res = d_out.cpu().numpy().copy()
    return out, res


def _check_lists(pairs, block, expect_dealt):
    sizes = _sizes(block)
    for u, (got, want) in enumerate(pairs):
        assert (len(want) > 0) == expect_dealt(u, sizes[u]), (u, sizes[u], len(want))
        assert np.array_equal(got, want), (u, sizes[u], len(got), len(want))
        if len(got):
            assert np.array_equal(np.sort(got), np.arange(sizes[u]))  # a permutation of the unit's events


@pytest.mark.parametrize("block", [128, 256, 512])
def test_the_list_read_back_is_the_restatement(ebo_ab, monkeypatch, block):
    monkeypatch.setenv("EBO_EVAL_BLOCK", str(block))
    try:
        pairs, _ = _lists(ebo_ab, block, CAP_512)
        pairs_val, _ = _lists(ebo_ab, block, CAP_512, want_jac=False)
    finally:
        monkeypatch.delenv("EBO_EVAL_BLOCK", raising=False)
    dealt = lambda u, n: block <= 256 and 2 * block <= n <= 12 * block  # (512-lane workgroups are not dealt)
    _check_lists(pairs, block, dealt)
    _check_lists(pairs_val, block, dealt)  # the value-only evaluation deals alike
    m = _model()
    # the rejected unit does hold rejected events (they sort last)
    ev, offsets, rects, flows = _patch_scene(ebo_ab, block)
    with _ctx(ebo_ab, len(ev)) as c:
        c.set_patches(ev, offsets, rects)
        rec = c.unit_records(0, REJECTED)
    base = m.box_base_words(*m.unpack_records(rec), rects[REJECTED], flows[REJECTED], CAP_512, SCALE)[0]
    assert 0 < (base == m.REJECT).sum() < len(base)


def test_the_sigma_below_one_instantiation_deals_alike(ebo_ab, monkeypatch):
    monkeypatch.setenv("EBO_EVAL_BLOCK", "128")
    try:
        pairs, _ = _lists(ebo_ab, 128, CAP_512, sigma=0.7)
    finally:
        monkeypatch.delenv("EBO_EVAL_BLOCK", raising=False)
    _check_lists(pairs, 128, lambda u, n: 256 <= n <= 1536)


def test_units_in_two_sub_bands_are_not_dealt(ebo_ab, monkeypatch):
    """EBO_LDS_KB=4 leaves the floor of 24 canvas rows: the wide unit's box needs two sub-bands, whose first fills the
    capacity, so there is no room for its list; it is evaluated in the canonical order, with the bits of deal off"""
    res = {}
    try:
        monkeypatch.setenv("EBO_EVAL_BLOCK", "128")
        monkeypatch.setenv("EBO_LDS_KB", "4")
        pairs, res["on"] = _lists(ebo_ab, 128, CAP_FLOOR)
        monkeypatch.setenv("EBO_EVAL_DEAL", "0")
        off, res["off"] = _lists(ebo_ab, 128, CAP_FLOOR)
    finally:
        for k in ("EBO_EVAL_BLOCK", "EBO_LDS_KB", "EBO_EVAL_DEAL"):
            monkeypatch.delenv(k, raising=False)
    m = _model()
    ev, offsets, rects, flows = _patch_scene(ebo_ab, 128)
    for u, (got, want) in enumerate(pairs):
        assert np.array_equal(got, want), u
    assert len(pairs[WIDE][0]) == 0 and any(len(g) for g, _ in pairs)
    assert all(len(g) == 0 for g, _ in off)
    assert np.array_equal(res["on"][:, 0], res["off"][:, 0])
    assert np.array_equal(res["on"][WIDE], res["off"][WIDE])


@pytest.mark.parametrize("block", [128, 256])
def test_deal_on_against_deal_off_and_twice(ebo_ab, monkeypatch, block):
    ev, offsets, rects, flows = _patch_scene(ebo_ab, block)
    res = {}
    try:
        monkeypatch.setenv("EBO_EVAL_BLOCK", str(block))
        for name in ("on", "off", "again"):
            if name == "off":
                monkeypatch.setenv("EBO_EVAL_DEAL", "0")
            else:
                monkeypatch.delenv("EBO_EVAL_DEAL", raising=False)
            with _ctx(ebo_ab, len(ev)) as c:
                c.set_patches(ev, offsets, rects)
                res[name] = c.eval(flows[None])
                res[name + "_val"] = c.eval(flows[None], want_jac=False)[0]
    finally:
        for k in ("EBO_EVAL_BLOCK", "EBO_EVAL_DEAL"):
            monkeypatch.delenv(k, raising=False)
    (r, J), (r0, J0), (r2, J2) = res["on"], res["off"], res["again"]
    assert np.array_equal(r, r0) and np.array_equal(res["on_val"], r0) and np.array_equal(res["off_val"], r0)
    assert np.array_equal(r, r2) and np.array_equal(J, J2)
    scale = np.abs(J0).reshape(-1, 2).max(axis=1, keepdims=True)
    print("deal on - off, block %d: max |dJ| / max |J of the patch| = %.2e; patches whose J moved: %d of %d"
          % (block, (np.abs(J - J0).reshape(-1, 2) / scale).max(), int((J != J0).any(axis=-1).sum()), J0.shape[1]))
    assert (J != J0).any()  # the dealt units sum in another order
    assert_jac_close(J, J0)


def _window_scene(synth, windows, n_events):
    key = ("windows", windows, n_events)
    if key not in _cache:
        made = [synth.make_window(0, window=w, n_events=n_events) for w in range(windows)]
        _cache[key] = ([e for e, _ in made], np.stack([g for _, g in made]) * 0.5)
    return _cache[key]


@pytest.mark.parametrize("windows,n_events,block", [(10, 40_000, 128)])
def test_shipped_against_the_oracle_and_alone_against_in_a_batch(ebo, ebo_ab, orc, synth, windows, n_events, block):
    """ten windows are 1080 slots: 128-lane workgroups, units of about 370 events, dealt from 256 (below 1024 slots the
    workgroups have 512 lanes and are not dealt: the other tests' ground); window 3 alone in a batch of ten copies has
    the bits it has among the others, and the oracle's value and Jacobian"""
    import torch
    evs, flows = _window_scene(synth, windows, n_events)
    w = 3
    offsets = np.concatenate([[0], np.cumsum([len(e) for e in evs])]).astype(np.uint64)
    with _ctx(ebo, offsets[-1], windows=windows) as c:
        c.set_windows(np.concatenate(evs), offsets)
        assert c.eval_launch_shape(True)[:2] == (1, block)
        r, J = c.eval(flows)
        r2, J2 = c.eval(flows)
        counts = np.array([c.patch_info(p, w)[0] for p in range(c.P)])
    assert np.array_equal(r, r2) and np.array_equal(J, J2)
    dealt = (counts >= 2 * block) & (counts <= 12 * block)
    assert dealt.sum() > 10 and (~dealt).sum() > 0, (dealt.sum(), counts.min(), counts.max())
    # the A/B library deals these units (and says so), and has the shipped library's bits
    with _ctx(ebo_ab, offsets[-1], windows=windows) as c:
        c.set_windows(np.concatenate(evs), offsets)
        d_flows = torch.from_numpy(flows).to("cuda")
        d_out = torch.zeros((windows * c.P, 3), dtype=torch.float64, device="cuda")
        p = int(np.flatnonzero(dealt)[0])
        assert len(c.unit_deal(w * (c.P + 1) + p, d_flows.data_ptr(), 1, d_out.data_ptr())) == counts[p]
        res = d_out.cpu().numpy().reshape(windows, c.P, 3)
    assert np.array_equal(res[..., 0], r) and np.array_equal(res[..., 1:], J)
    copies = windows
    offs1 = np.arange(copies + 1, dtype=np.uint64) * np.uint64(len(evs[w]))
    with _ctx(ebo, offs1[-1], windows=copies) as c:
        c.set_windows(np.concatenate([evs[w]] * copies), offs1)
        assert c.eval_launch_shape(True)[:2] == (1, block)
        rb, Jb = c.eval(np.stack([flows[w]] * copies))
    for k in (0, copies - 1):
        assert np.array_equal(rb[k], r[w]) and np.array_equal(Jb[k], J[w])
    prm = orc.default_params(image_w=IMAGE[0], image_h=IMAGE[1], patch_w=PATCH[0], patch_h=PATCH[1], loss=1, tv_weight=0.0)
    ro, Jo, active, _ = orc.window_eval(evs[w], prm, flows[w])
    assert active[dealt].all()
    np.testing.assert_allclose(r[w], ro, rtol=1e-9, atol=1e-12)
    assert_jac_close(J[w], Jo)
