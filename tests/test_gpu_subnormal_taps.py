"""k_eval3's value taps as subnormal products (csrc/fix_form.h) give the bits of the biased
fma + subtract form.  The shipped library (one form) is compared with libebo_hip_ab.so under EBO_FIX_FORM=bias, which
runs the biased form in the same kernels: every (r, J) with np.array_equal, value-only and with the Jacobian, and the
flows and statistics of the device-resident solve.  Patches are 20 x 20 (canvas 60 x 60), times in [0, 20000] us at
scale 1e-3: the reference time is 10000 us and tau lies in [-10, 10]."""
import math

import numpy as np
import pytest

import eval_cases as EC

pytestmark = pytest.mark.gpu

T_END = 20000
RECT = (40, 40, 20, 20)
BIAS = {"EBO_FIX_FORM": "bias"}


def _params(lib, sigma=1.0):
    p = lib.default_params(image_w=128, image_h=128, patch_w=20, patch_h=20, scale=1e-3, tv_weight=0.0,
                           loss=lib.LOSS_VARIANCE, min_events=0, max_events=1 << 17, max_windows=1)
    p.k.sigma_compensate = sigma
    return p


def _eval(lib, units, rects, flows, sigma=1.0):
    """(r, J, r of the value-only call) of the units (one event array each) at `flows` [n][2]."""
    offs = np.concatenate([[0], np.cumsum([len(u) for u in units])])
    with lib.Context(_params(lib, sigma)) as c:
        c.set_patches(np.concatenate(units), offs, rects)
        r, J = c.eval(flows)
        r1, _ = c.eval(flows, want_jac=False)
    return r, J, r1


def _same(ebo, ebo_ab, monkeypatch, units, rects, flows, sigma=1.0, env=None, both_ab=False):
    """The subnormal form (the shipped library; both_ab: the A/B library, which alone reads `env`) against the biased
    form.  Returns the subnormal side's (r, J)."""
    flows = np.asarray(flows, dtype=np.float64).reshape(len(units), 2)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    a = _eval(ebo_ab if both_ab else ebo, units, rects, flows, sigma)
    for k, v in BIAS.items():
        monkeypatch.setenv(k, v)
    try:
        b = _eval(ebo_ab, units, rects, flows, sigma)
    finally:
        for k in list(BIAS) + list(env or {}):
            monkeypatch.delenv(k, raising=False)
    assert np.isfinite(a[0]).all() and np.isfinite(a[1]).all()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and np.array_equal(a[2], b[2])
    assert np.array_equal(a[0], a[2])  # (value-only and with the Jacobian: the same image)
    return a[0], a[1]


def _unit(ebo, x, y, t):
    """Events of one unit; the first at t = 0 and the last at T_END pin the reference time."""
    o = np.argsort(t, kind="stable")
    return ebo.make_events(np.asarray(x)[o], np.asarray(y)[o], np.asarray(t)[o])


def _random_unit(ebo, rng, n, rect=RECT):
    x = rng.integers(rect[0], rect[0] + rect[2], n)
    y = rng.integers(rect[1], rect[1] + rect[3], n)
    t = rng.integers(0, T_END + 1, n)
    if n >= 2:
        t[0], t[1] = 0, T_END
    return _unit(ebo, x, y, t)


def test_one_event_at_integer_coordinates(ebo, ebo_ab, monkeypatch):
    """fx = fy = 0: the centre tap is norm itself, the axis weights are the bare constants."""
    u = ebo.make_events([47], [52], [1234])
    _same(ebo, ebo_ab, monkeypatch, [u], [RECT], [[0.0, 0.0]])


def test_fractions_within_1e_12_of_one(ebo, ebo_ab, monkeypatch):
    """tau = +-10: the flow (1 - 1e-12) / 10 warps one event to a fraction within 1e-12 of 1 and the other to 1e-12."""
    u = _unit(ebo, [47, 50], [52, 49], [0, T_END])
    m = (1.0 - 1e-12) / 10.0
    for flow in ([m, m], [-m, -m], [m, -m]):
        _same(ebo, ebo_ab, monkeypatch, [u], [RECT], [flow])


def test_footprints_clipped_by_edges_and_corners(ebo, ebo_ab, monkeypatch):
    """64 events whose 7 x 7 footprints leave the 60 x 60 canvas over its four edges and four corners: the clipped path."""
    lo = [-3, -2, -1, 0, 1, 2, 0, 1]        # canvas coordinates of the centre tap near the low edge ...
    hi = [57, 58, 59, 60, 61, 62, 58, 59]   # ... and near the high one (62: one column left inside)
    mid = [9, 17, 25, 30, 36, 44, 50, 28]
    cx, cy = [], []
    for ax, ay in ((lo, mid), (hi, mid), (mid, lo), (mid, hi), (lo, lo), (lo, hi), (hi, lo), (hi, hi)):
        cx += ax
        cy += ay
    assert len(cx) == 64
    # canvas column = x - rx + rw
    x = np.asarray(cx) + RECT[0] - RECT[2]
    y = np.asarray(cy) + RECT[1] - RECT[3]
    t = np.full(64, T_END // 2)
    t[0], t[-1] = 0, T_END
    u = ebo.make_events(x, y, t)
    for flow in ([0.0, 0.0], [0.013, -0.021]):
        _same(ebo, ebo_ab, monkeypatch, [u], [RECT], [flow])


@pytest.mark.parametrize("env", [{"EBO_LDS_KB": "4"}, {"EBO_LDS_KB": "4", "EBO_EVAL_TILES": "2"}, {"EBO_EVAL_TILES": "2"}],
                         ids=["sub-bands", "sub-bands-tiles2", "tiles2"])
def test_row_bands_and_sub_bands(ebo, ebo_ab, monkeypatch, env):
    """A flow of 2 spreads the unit over the whole canvas (60 rows of pitch 61).  With EBO_LDS_KB=4 a workgroup holds
    24 rows of the widest canvas (image_capacity: 1440 pixels), so the image takes three sub-bands; tiles = 2 halves
    the rows between two workgroups.  Every event is tested against the rows of each band before its taps."""
    rng = np.random.default_rng(4)
    u = _random_unit(ebo, rng, 400)
    tau = (T_END // 2 - u["t_us"]) * 1e-3
    cx = np.floor(u["x"] + tau * 2.0).astype(int) - RECT[0] + RECT[2]
    cy = np.floor(u["y"] + tau * 2.0).astype(int) - RECT[1] + RECT[3]
    ok = (cx >= -3) & (cx < 63) & (cy >= -3) & (cy < 63)
    cols = (min(cx[ok].max() + 3, 59) - max(cx[ok].min() - 3, 0) + 1) | 1
    rows = min(cy[ok].max() + 3, 59) - max(cy[ok].min() - 3, 0) + 1
    tiles = int(env.get("EBO_EVAL_TILES", "1"))
    if "EBO_LDS_KB" in env:
        assert -(-rows // tiles) > 1440 // cols  # >= 2 sub-bands per workgroup
    assert rows >= 48
    _same(ebo, ebo_ab, monkeypatch, [u], [RECT], [[2.0, 2.0]], env=env, both_ab=True)


@pytest.mark.parametrize("raises", [1, 2])
def test_pile_up_raises_the_grid(ebo, ebo_ab, monkeypatch, raises):
    """Enough events on one pixel that unit_fix_grid raises make_consts' k once / twice (n_ev norm >= 2^(11 + k)): preY is
    halved with every doubling of the bias."""
    k0 = EC.fixed_exponent(1.0)
    n = int(math.ceil(math.ldexp(1.0, 11 + k0 + raises - 1) / EC.norm_of(1.0))) + 1
    assert EC.unit_exponent(1.0, n) == k0 + raises and EC.unit_exponent(1.0, n - 2) == k0 + raises - 1
    rng = np.random.default_rng(5)
    t = np.sort(rng.integers(0, T_END + 1, n))
    t[0], t[-1] = 0, T_END
    u = ebo.make_events(np.full(n, 50), np.full(n, 49), t)
    _same(ebo, ebo_ab, monkeypatch, [u], [RECT], [[0.004, -0.003]])


def test_random_units(ebo, ebo_ab, monkeypatch):
    """Units of 1, 63, 64, 65 and 781 events (around one wave's lanes and the 512-lane workgroup) at 0, 0.5 and 1.0 x a
    synthetic ground truth."""
    rng = np.random.default_rng(6)
    sizes = [1, 63, 64, 65, 781]
    rects = [(20 * i + 20, 40, 20, 20) for i in range(len(sizes))]
    units = [_random_unit(ebo, rng, n, rect) for n, rect in zip(sizes, rects)]
    gt = rng.uniform(-0.9, 0.9, (len(sizes), 2))
    for s in (0.0, 0.5, 1.0):
        _same(ebo, ebo_ab, monkeypatch, units, rects, gt * s)


def test_sigma_below_one_and_the_host_guard(ebo, ebo_ab, monkeypatch):
    """sigma = 0.5 runs the <false> instantiation, which keeps the biased form: unchanged against the A/B form.  A
    context that trips the host rule (EBO_FIX_GUARD_EXP=1 in the A/B build: norm = 0.159 < 2^-1) takes that instantiation
    at sigma = 1 as well: the same bits with and without the switch, and the objective of the unguarded context to the
    suite's bars (value relative 1e-9, Jacobian absolute 1e-10 more: library exp against exp_small, 4e-16 each)."""
    rng = np.random.default_rng(7)
    units = [_random_unit(ebo, rng, n) for n in (65, 300)]
    rects = [RECT, RECT]
    flows = [[0.31, -0.27], [-0.62, 0.44]]
    _same(ebo, ebo_ab, monkeypatch, units, rects, flows, sigma=0.5)
    r, J = _same(ebo, ebo_ab, monkeypatch, units, rects, flows)
    rg, Jg = _same(ebo, ebo_ab, monkeypatch, units, rects, flows, env={"EBO_FIX_GUARD_EXP": "1"}, both_ab=True)
    np.testing.assert_allclose(rg, r, rtol=1e-9, atol=1e-12)
    np.testing.assert_allclose(Jg, J, rtol=1e-9, atol=1e-10)


def test_solve_device_independent(ebo, ebo_ab, monkeypatch):
    """k_solve_independent on 8 patches: flows and statistics of the two forms, bit for bit."""
    import torch
    rng = np.random.default_rng(8)
    rects = [(20 * (i % 4) + 20, 20 * (i // 4) + 40, 20, 20) for i in range(8)]
    units = []
    for i, rect in enumerate(rects):
        # a moving edge: events on a line that travels with a flow of its own
        n = 200 + 37 * i
        t = np.sort(rng.integers(0, T_END + 1, n))
        t[0], t[-1] = 0, T_END
        vx, vy = rng.uniform(-0.4, 0.4, 2)
        s = rng.uniform(0, 20, n)
        x = rect[0] + np.clip(6 + 0.4 * s + vx * (t - T_END / 2) * 1e-3, 0, 19).astype(int)
        y = rect[1] + np.clip(s - vy * (t - T_END / 2) * 1e-3, 0, 19).astype(int)
        units.append(ebo.make_events(x, y, t))
    offs = np.concatenate([[0], np.cumsum([len(u) for u in units])])
    out = []
    for lib, env in ((ebo, {}), (ebo_ab, BIAS)):
        for k, v in env.items():
            monkeypatch.setenv(k, v)
        try:
            with lib.Context(_params(lib)) as c:
                c.set_patches(np.concatenate(units), offs, rects)
                opts = lib.default_solver(mode=lib.SOLVE_INDEPENDENT, max_num_iterations=12)
                d_sol = torch.zeros((8, 2), dtype=torch.float64, device="cuda")
                d_stats = torch.zeros((8, 4), dtype=torch.int32, device="cuda")
                torch.cuda.synchronize()
                c.solve_device(opts, d_sol.data_ptr(), d_stats.data_ptr())
                c.synchronize()
                out.append((d_sol.cpu().numpy().copy(), d_stats.cpu().numpy().copy()))
        finally:
            for k in env:
                monkeypatch.delenv(k, raising=False)
    assert (np.abs(out[0][0]).max(axis=1) > 0).sum() >= 6  # the solves moved
    assert np.array_equal(out[0][0], out[1][0]) and np.array_equal(out[0][1], out[1][1])
