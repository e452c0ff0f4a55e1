"""GPU: k_eval3's division of the Jacobian between its two tap passes against the oracle.

The image-free sums D1k are formed in the SCATTER pass (on weights that carry the fixed-point prefactors, where the
launch wants a Jacobian), the image sums D2k in the gather from a table of the seven x-derivative weights, and the
sigma >= 1 exponentials come from csrc/exp_taps.h.  Each case is a place where that split can go wrong: clipped
footprints (both passes must mask the same taps), negative fractional parts (the paired exponential's other half),
sequential sub-bands and row tiles (a tap's D1 counted exactly once), other block shapes, the sigma < 1 instantiation
(unscaled weights, library exp), central differences (value-only sets: no D1 at all), and two bit-for-bit invariants.

Bounds: tests/test_gpu_parity.py's -- r at rtol 1e-9 / atol 1e-12, J at atol 1e-10 -- on its shape, config 0 windows
of 15 000 events.  One oracle evaluation per (window, flow) is shared by every case that uses it.
"""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

CONFIG = 0
N_EVENTS = 15000
RTOL = 1e-9

_cache = {}


def _ctx(lib, synth, sigma=None, **kw):
    cfg = synth.CONFIGS[CONFIG]
    p = lib.default_params(image_w=cfg["image"][0], image_h=cfg["image"][1], patch_w=cfg["patch"][0],
                           patch_h=cfg["patch"][1], loss=lib.LOSS_VARIANCE, **kw)
    if sigma is not None:
        p.k.sigma_compensate = sigma
    return lib.Context(p)


def _oparams(orc, p):
    prm = orc.default_params(image_w=p.image_w, image_h=p.image_h, patch_w=p.patch_w, patch_h=p.patch_h,
                             tv_weight=p.tv_weight, tv_huber=p.tv_huber, scale=p.scale, min_events=p.min_events,
                             loss=p.loss)
    prm.k.sigma_compensate = p.k.sigma_compensate
    return prm


def _window(synth):
    if "window" not in _cache:
        _cache["window"] = synth.make_window(CONFIG, n_events=N_EVENTS)
    return _cache["window"]


def _corner_window(synth):
    """The window's events folded onto x, y < 3: with a negative flow the warped coordinates of the events before the
    reference time are negative, truncate towards zero and leave fractional parts in (-1, 0]."""
    if "corner" not in _cache:
        ev, _ = _window(synth)
        ev = ev.copy()
        ev["x"] %= 3
        ev["y"] %= 3
        _cache["corner"] = ev
    return _cache["corner"]


def _flows(synth, name, P):
    _, gt = _window(synth)
    return {"zero": np.zeros((P, 2)), "half": gt * 0.5, "plus2": np.full((P, 2), 2.0), "minus2": np.full((P, 2), -2.0),
            "corner": np.tile(np.array([[-0.7, -0.45]]), (P, 1))}[name]


def _oracle(orc, synth, c, name, sigma=1.0):
    """(r, J, active) of the oracle for the named flow (and its window), computed once."""
    key = (name, sigma)
    if key not in _cache:
        ev = _corner_window(synth) if name == "corner" else _window(synth)[0]
        ro, Jo, active, _ = orc.window_eval(ev, _oparams(orc, c.params), _flows(synth, name, c.P))
        ro.setflags(write=False)
        Jo.setflags(write=False)
        _cache[key] = (ro, Jo, active)
    return _cache[key]


def _boxes(c, ev, flows):
    """Per active patch: (columns, rows) of the bounding box of its warped events' footprints inside the canvas, as
    eval_unit3 forms it, and the smallest warped coordinate of an event whose centre pixel lies on the canvas."""
    out = []
    for p in range(c.P):
        n, active, t_ref = c.patch_info(p)
        if not active:
            continue
        x, y, w, h = c.patch_rect(p % c.npx, p // c.npx)
        m = (ev["x"] >= x) & (ev["x"] < x + w) & (ev["y"] >= y) & (ev["y"] < y + h)
        tau = (t_ref - ev["t_us"][m]).astype(np.float64) * c.params.scale
        wx, wy = ev["x"][m] + tau * flows[p, 0], ev["y"][m] + tau * flows[p, 1]
        cx, cy = np.trunc(wx).astype(int) - x + w, np.trunc(wy).astype(int) - y + h
        ok = (cx >= -3) & (cx < 3 * w + 3) & (cy >= -3) & (cy < 3 * h + 3)
        if not ok.any():
            continue
        cols = (min(cx[ok].max() + 3, 3 * w - 1) - max(cx[ok].min() - 3, 0) + 1) | 1
        rows = min(cy[ok].max() + 3, 3 * h - 1) - max(cy[ok].min() - 3, 0) + 1
        out.append((cols, rows, min(wx[ok].min(), wy[ok].min())))
    return out


def _check(lib, orc, synth, name, sigma=None, shape=None):
    ev = _corner_window(synth) if name == "corner" else _window(synth)[0]
    with _ctx(lib, synth, sigma) as c:
        c.set_window(ev)
        flows = _flows(synth, name, c.P)
        if shape is not None:
            shape(c, _boxes(c, ev, flows))
        r, J = c.eval(flows)
        r1, _ = c.eval(flows, want_jac=False)
        ro, Jo, active = _oracle(orc, synth, c, name, 1.0 if sigma is None else sigma)
    assert active.sum() > 0
    np.testing.assert_allclose(r[0], ro, rtol=RTOL, atol=1e-12)
    np.testing.assert_allclose(J[0], Jo, rtol=RTOL, atol=1e-10)
    # the value does not know whether the scatter formed D1 beside it
    assert np.array_equal(r1[0], r[0])
    return r[0], J[0]


@pytest.mark.parametrize("name", ["zero", "half", "plus2", "minus2"])
def test_flows_interior_and_clipped(ebo, orc, synth, name):
    """+-2 px per time unit push the footprints over the canvas edge: both passes take the clipped path."""
    _, J = _check(ebo, orc, synth, name)
    assert np.abs(J).max() > 0.0


def test_negative_fractional_parts(ebo, orc, synth):
    def shape(c, boxes):
        assert min(b[2] for b in boxes) < 0.0  # some warped coordinate on the canvas is negative

    r, J = _check(ebo, orc, synth, "corner", shape=shape)
    assert np.abs(J).max() > 0.0


@pytest.mark.parametrize("env", [{"EBO_LDS_KB": "4"}, {"EBO_EVAL_TILES": "2"}, {"EBO_LDS_KB": "4", "EBO_EVAL_TILES": "2"}],
                         ids=["lds4", "tiles2", "lds4-tiles2"])
@pytest.mark.parametrize("name", ["half", "minus2"])
def test_sub_bands_and_row_tiles_count_d1_once(ebo_ab, orc, synth, monkeypatch, env, name):
    """Sequential sub-bands (a small LDS), row tiles (k_combine_variance) and both: an event whose footprint straddles
    two bands takes the clipped path in each, and every tap's D1 share must land in exactly one."""
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    tiles = int(env.get("EBO_EVAL_TILES", "1"))

    def shape(c, boxes):
        if "EBO_EVAL_TILES" in env:
            assert c.eval_launch_shape()[0] == tiles
        if "EBO_LDS_KB" in env and name == "minus2":
            # 4 KB hold 1440 pixels of a 20 x 20 patch's canvas (image_capacity): a workgroup of some patch walks
            # at least two sub-bands (at +-2 the box spans the canvas; at 0.5 x gt it may fit one band)
            t = c.eval_launch_shape()[0]
            assert any(-(-rows // t) > 1440 // cols for cols, rows, _ in boxes)

    _check(ebo_ab, orc, synth, name, shape=shape)


@pytest.mark.parametrize("block", ["64", "128", "512"])
def test_block_shapes(ebo_ab, orc, synth, monkeypatch, block):
    monkeypatch.setenv("EBO_EVAL_BLOCK", block)
    _check(ebo_ab, orc, synth, "half")


@pytest.mark.parametrize("name", ["half", "minus2"])
def test_sigma_below_one(ebo, orc, synth, name):
    """sigma = 0.5 takes k_eval3<false>: biased taps, so unscaled weights in the scatter's D1, and the library exp."""
    _check(ebo, orc, synth, name, sigma=0.5)


def test_central_differences_form_no_d1(ebo, orc, synth):
    """GRAD_CENTRAL evaluates five value-only sets; the bounds are test_gpu_parity.py's for this mode."""
    ev, gt = _window(synth)
    h = 1e-6
    flows = gt * 0.5
    with _ctx(ebo, synth, grad=ebo.GRAD_CENTRAL, fd_step=h) as c:
        c.set_window(ev)
        r, J = c.eval(flows)
        ro, _, active = _oracle(orc, synth, c, "half")
        prm = _oparams(orc, c.params)
    np.testing.assert_allclose(r[0], ro, rtol=RTOL, atol=1e-12)
    num = np.zeros((len(ro), 2))
    for k in range(2):
        d = np.zeros_like(flows)
        d[:, k] = h
        rp, _, _, _ = orc.window_eval(ev, prm, flows + d, want_jac=False)
        rm, _, _, _ = orc.window_eval(ev, prm, flows - d, want_jac=False)
        num[:, k] = (rp - rm) / (2 * h)
    np.testing.assert_allclose(J[0], num, rtol=0, atol=2e-6)


def test_one_window_alone_and_in_a_batch_of_eight(ebo, synth):
    """A unit's (r, J) does not depend on the launch it is part of (both launches below 1024 units)."""
    evs, gts = [], []
    for w in range(8):
        e, g = synth.make_window(CONFIG, window=w, n_events=N_EVENTS)
        evs.append(e)
        gts.append(g * 0.5)
    offsets = np.zeros(9, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(e) for e in evs])
    with _ctx(ebo, synth, max_events=int(offsets[-1]), max_windows=8) as c:
        assert 8 * c.P < 1024
        c.set_windows(np.concatenate(evs), offsets)
        rb, Jb = c.eval(np.stack(gts))
        for w in (0, 5):
            c.set_window(evs[w])
            r, J = c.eval(gts[w])
            assert np.abs(J[0]).max() > 0.0
            assert np.array_equal(r[0], rb[w])
            assert np.array_equal(J[0], Jb[w])
