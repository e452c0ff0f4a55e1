"""GPU: the Jacobian sums of an interior event from tap moments (csrc/tap_moments.h).

eval_unit3 forms D1 and the gather's D2 of an event whose footprint lies inside the image from first moments of the tap
weights; an event cut by the image keeps the per-tap statements.  The value sums are not touched, so r keeps its bits;
J moves in its last bits against the per-tap form and must hold against the oracle at the bounds of the neighbouring
k_eval3 tests (r: rtol 1e-9, atol 1e-12; J: jac_check.assert_jac_close).

Scenes: 20 x 20 patches of a 100 x 80 image, the hand-made units and windows of tests/test_gpu_eval_interior.py:
  * all-interior dealt units (300 events at 128 lanes) and one below two rounds (`few`); boxes cut by the canvas on each
    of its four sides (`xmin2`, `xmax57`, `ymin2`, `ymax57`: the clipped branch); two sub-bands (EBO_LDS_KB=4) and row
    tiles (EBO_EVAL_TILES=2) in the A/B library; sigma 0.7; workgroups of 128, 256 and 512 lanes;
  * windows whose patches at the image's low edges warp below 0, where truncation leaves NEGATIVE fractional parts;
  * value only, central differences, a lock-step solve and solve_device.
Asserted: (r, J) against the oracle; r bit-equal with and without the Jacobian; a window alone against inside a batch of
eight, bit for bit; EBO_EVAL_INTERIOR=0 against 1, bit for bit; EBO_EVAL_DEAL=0 against 1, r bit-equal and J within 1e-15
of its largest entry (the deal changes the order in which the events' sums are added, nothing else); the shipped library
at the A/B library's bits."""
import os

import numpy as np
import pytest

import test_gpu_eval_interior as ti
from jac_check import assert_jac_close

pytestmark = pytest.mark.gpu

cases = ti.cases
SCALE = ti.SCALE
SWITCHES = ti.SWITCHES + ("EBO_EVAL_DEAL",)
CLIPPED = ("xmin2", "xmax57", "ymin2", "ymax57")
_cache = {}


class _env:
    """the A/B switches as given and no others, put back on exit"""

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


def _oracle_units(orc, copies, wide, sigma=None):
    """(r, J) of every hand-made unit from the oracle's contrastFunctor, computed once per scene"""
    key = ("oracle", copies, wide, sigma)
    if key not in _cache:
        rects, units = ti._scene(copies=copies, wide=wide)
        consts = None
        if sigma is not None:
            consts = orc.default_consts()
            consts.sigma_compensate = sigma
        out = {}
        for name, (i, uev, flow) in units.items():
            if name != "inactive":
                out[name] = orc.contrast_eval(uev, rects[i], flow, 1, scale=SCALE, consts=consts)
                assert out[name][0] != 0.0 and np.abs(out[name][1]).max() > 0.0
        _cache[key] = out
    return _cache[key]


def _assert_units_at_the_oracle(orc, units, r, J, copies, wide, sigma=None):
    ref = _oracle_units(orc, copies, wide, sigma)
    for name, (i, _, _) in units.items():
        if name == "inactive":
            assert r[i] == 0 and (J[i] == 0).all()
            continue
        ro, Jo = ref[name]
        np.testing.assert_allclose(r[i], ro, rtol=1e-9, atol=1e-12, err_msg=name)
        assert_jac_close(J[i], Jo)


def _eval(lib, rects, ev, offsets, flows, env, **kw):
    """(r, J, r value-only, launch shape) of one load under the switches `env`"""
    with _env(**env), ti._ctx(lib, len(ev), len(rects), **kw) as c:
        c.set_patches(ev, offsets, rects)
        r, J = c.eval(flows[None])
        rv = c.eval(flows[None], want_jac=False)[0]
        return r[0], J[0], rv[0], c.eval_launch_shape(True)


def _same(a, b):
    return a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("block", [128, 256, 512])
def test_hand_made_units_oracle_interior_and_deal_switches(ebo_ab, orc, block):
    """every hand-made unit -- all-interior dealt, below two rounds, cut by the canvas on each side, no table -- against the
    oracle, with the all-interior path and the deal switched off and on"""
    rects, units = ti._scene()
    ev, offsets, flows = ti._assemble(rects, units)
    env = {"EBO_EVAL_BLOCK": str(block)}
    r, J, rv, shape = _eval(ebo_ab, rects, ev, offsets, flows, env)
    assert shape[:2] == (1, block)
    assert _same(r, rv)  # the value sums do not know whether the Jacobian is wanted
    _assert_units_at_the_oracle(orc, units, r, J, 3, True)
    r0, J0, rv0, _ = _eval(ebo_ab, rects, ev, offsets, flows, dict(env, EBO_EVAL_INTERIOR="0"))
    assert _same(r, r0) and _same(J, J0) and _same(rv, rv0)
    r1, J1, rv1, _ = _eval(ebo_ab, rects, ev, offsets, flows, dict(env, EBO_EVAL_DEAL="0"))
    assert _same(r, r1) and _same(rv, rv1)
    top = np.abs(J1).max()
    print("block %d: deal off against on, max |dJ| / max |J| = %.3e" % (block, np.abs(J - J1).max() / top))
    assert np.abs(J - J1).max() <= 1e-15 * top
    if block == 128:  # units of two rounds and more (300 events at 128 lanes) are dealt: another order of the same sums
        assert (J != J1).any()
    else:
        assert _same(J, J1)
    for name in CLIPPED:  # the clipped branch was run: these boxes touch the canvas's edge
        assert not ti.BOXES[name][3][0]


@pytest.mark.parametrize("env,copies", [({"EBO_EVAL_BLOCK": "128", "EBO_LDS_KB": "4"}, 3), ({"EBO_EVAL_TILES": "2"}, 3)],
                         ids=["two sub-bands", "row tiles"])
def test_sub_bands_and_row_tiles(ebo_ab, orc, env, copies):
    rects, units = ti._scene(copies=copies, wide=False)
    ev, offsets, flows = ti._assemble(rects, units)
    r, J, rv, shape = _eval(ebo_ab, rects, ev, offsets, flows, env)
    assert shape[0] == (2 if "EBO_EVAL_TILES" in env else 1)
    if "EBO_LDS_KB" in env:
        # 1440 pixels: the box that fills the canvas (61 x 60) walks three sub-bands, `rows_over` two
        lo, hi = ti.BOXES["full"][0], ti.BOXES["full"][1]
        assert (hi[1] - lo[1] + 7) * ((hi[0] - lo[0] + 7) | 1) > 2 * ti.CAP_FLOOR
    assert _same(r, rv)
    _assert_units_at_the_oracle(orc, units, r, J, copies, False)
    r0, J0, rv0, _ = _eval(ebo_ab, rects, ev, offsets, flows, dict(env, EBO_EVAL_INTERIOR="0"))
    assert _same(r, r0) and _same(J, J0) and _same(rv, rv0)
    # one band of one tile holds the same image: r has its bits, J the same sums in another grouping
    r1, J1, _, _ = _eval(ebo_ab, rects, ev, offsets, flows, {"EBO_EVAL_BLOCK": "128"} if "EBO_LDS_KB" in env else {})
    np.testing.assert_allclose(r, r1, rtol=1e-12)
    assert_jac_close(J, J1)


@pytest.mark.parametrize("block", [128, 512])
def test_sigma_below_one(ebo_ab, orc, block):
    """the library-exp instantiation shares the moment forms (the quarter-argument exponentials are not its)"""
    rects, units = ti._scene()
    ev, offsets, flows = ti._assemble(rects, units)
    env = {"EBO_EVAL_BLOCK": str(block)}
    r, J, rv, _ = _eval(ebo_ab, rects, ev, offsets, flows, env, sigma=0.7)
    assert _same(r, rv)
    _assert_units_at_the_oracle(orc, units, r, J, 3, True, sigma=0.7)
    r0, J0, _, _ = _eval(ebo_ab, rects, ev, offsets, flows, dict(env, EBO_EVAL_INTERIOR="0"), sigma=0.7)
    assert _same(r, r0) and _same(J, J0)


def test_central_differences(ebo_ab):
    """five value-only flow sets (no Jacobian sum is formed): the interior path on against off bit for bit, the centre set's
    r the analytic run's, and the analytic J (moment forms) within the noise of the difference quotients of r.

    The bound, from the number format and the step h = 1e-6 (the default fd_step): r = max_possible_residual - var with r
    near 1e3, so each of the quotient's two r values is rounded to ulp(r) = 1.1e-13 by that subtraction (half an ulp each),
    and var itself is a combination of three sums over at most NPIX = 61 x 60 pixels, each within NPIX eps of its terms,
    which are a few var: 8 NPIX eps var for the two values together.  Over 2 h that is a few 1e-7 absolute, about 1e-5 of
    this scene's largest |J| (a wrong sign, a dropped term or a wrong factor in the moment forms is of order 1); the
    truncation term, h^2 / 6 times a third derivative, is nine orders below.  The analytic J's own parity bound, 1e-8 of
    the largest entry (jac_check), comes on top."""
    rects, units = ti._scene()
    ev, offsets, flows = ti._assemble(rects, units)
    rc, Jc, _, shape = _eval(ebo_ab, rects, ev, offsets, flows, {}, grad=ebo_ab.GRAD_CENTRAL)
    assert shape[2] == 5
    r0, J0, _, _ = _eval(ebo_ab, rects, ev, offsets, flows, {"EBO_EVAL_INTERIOR": "0"}, grad=ebo_ab.GRAD_CENTRAL)
    assert _same(rc, r0) and _same(Jc, J0)
    r, J, _, _ = _eval(ebo_ab, rects, ev, offsets, flows, {})
    assert _same(r, rc)
    h, max_res, npix = 1e-6, 1e3, 61 * 60
    top = np.abs(J).max()
    var = np.abs(max_res - r[r != 0]).max()
    noise = (np.spacing(np.abs(r).max()) + 8 * npix * np.finfo(np.float64).eps * var) / (2 * h)
    bound = noise + 1e-8 * top
    print("central differences against the analytic J: max |dJ| = %.3e (%.3e of max |J|), bound %.3e (var up to %.3e)"
          % (np.abs(Jc - J).max(), np.abs(Jc - J).max() / top, bound, var))
    assert (Jc != 0).any() and np.isfinite(Jc).all()
    assert np.abs(Jc - J).max() <= bound


def _negative_fractions(c, flows, w):
    """per patch of window w: the number of events whose warped coordinate lies below 0 off the pixel grid (truncation
    toward zero leaves them a negative fractional part), from the device's own records"""
    m = ti._model()
    out = []
    for p in range(len(ti.GRID)):
        n = 0
        if c.patch_info(p, w)[1]:
            x, y, dt = m.unpack_records(c.unit_records(w, p))
            tau = dt.astype(np.float64) * SCALE
            cx, cy = x + tau * flows[w, p, 0], y + tau * flows[w, p, 1]
            n = int((((cx < 0) & (cx != np.trunc(cx))) | ((cy < 0) & (cy != np.trunc(cy)))).sum())
        out.append(n)
    return np.array(out)


@pytest.mark.parametrize("lib_name,block", [("ebo", 512), ("ebo_ab", 128)])
def test_window_alone_against_in_a_batch_of_eight(request, orc, lib_name, block):
    """window 0 (patches at the image's low edges warp below 0: negative fractional parts; boxes that reach the canvas's
    edge; a box from the event pass) alone, and as the sixth of eight windows: the same bits, and the oracle's (r, J)"""
    lib = request.getfixturevalue(lib_name)
    evs, _, flows = ti._windows()
    P = len(ti.GRID)
    env = {"EBO_EVAL_BLOCK": "128"} if lib_name == "ebo_ab" else {}
    with _env(**env), ti._ctx(lib, len(evs[0]), P) as c:
        c.set_windows(evs[0], np.array([0, len(evs[0])], dtype=np.uint64))
        assert c.eval_launch_shape(True)[:2] == (1, block)
        r, J = c.eval(flows[:1])
        rv = c.eval(flows[:1], want_jac=False)[0]
        neg = _negative_fractions(c, flows, 0)
        active = np.array([c.patch_info(p, 0)[1] for p in range(P)], dtype=bool)
    assert _same(r, rv)
    assert (neg >= 50).sum() >= 3, neg  # whole units' worth of events with negative fractional parts
    order = [1, 1, 1, 1, 1, 0, 1, 1]
    batch = [evs[k] for k in order]
    offsets = np.concatenate([[0], np.cumsum([len(e) for e in batch])]).astype(np.uint64)
    with _env(**env), ti._ctx(lib, offsets[-1], 8 * P) as c:
        c.set_windows(np.concatenate(batch), offsets)
        assert c.eval_launch_shape(True)[:2] == (1, block)
        rb, Jb = c.eval(np.stack([flows[k] for k in order]))
    assert _same(rb[5], r[0]) and _same(Jb[5], J[0])
    assert _same(rb[0], rb[7]) and _same(Jb[0], Jb[7]) and not _same(rb[0], rb[5])
    prm = orc.default_params(image_w=ti.IMAGE[0], image_h=ti.IMAGE[1], patch_w=ti.PATCH[0], patch_h=ti.PATCH[1], loss=1, tv_weight=0.0)
    if "window0" not in _cache:
        _cache["window0"] = orc.window_eval(evs[0][evs[0]["x"] < ti.IMAGE[0]], prm, flows[0])  # (without the strays)
    ro, Jo, act, _ = _cache["window0"]
    assert np.array_equal(np.asarray(act, dtype=bool), active)
    np.testing.assert_allclose(r[0], ro, rtol=1e-9, atol=1e-12)
    assert_jac_close(J[0], Jo)


def _lock_step(lib, env):
    evs, offsets, _ = ti._windows()
    with _env(**env), ti._ctx(lib, offsets[-1], 2 * len(ti.GRID), tv_weight=1e3) as c:
        c.set_windows(np.concatenate(evs), offsets)
        opts = lib.default_solver()
        opts.max_num_iterations = 6
        flows, summ = c.solve(opts)
        return flows.copy(), [(s.iterations, s.final_cost, s.termination, s.num_evals_cost, s.num_evals_jac) for s in summ]


def test_lock_step_solve(ebo, ebo_ab):
    """rounds with per-slot modes 0 / 1 / 2: the shipped library, the A/B library and the A/B library with the all-interior
    path off take the same steps to the same flows"""
    a = _lock_step(ebo, {})
    b = _lock_step(ebo_ab, {})
    c = _lock_step(ebo_ab, {"EBO_EVAL_INTERIOR": "0"})
    assert a[0].tobytes() == b[0].tobytes() == c[0].tobytes() and a[1] == b[1] == c[1]
    assert (a[0] != 0).any() and all(s[4] > 0 for s in a[1])


def _solve_device(lib):
    import torch
    evs, offsets, _ = ti._windows()
    P = len(ti.GRID)
    with _env(), ti._ctx(lib, offsets[-1], 2 * P) as c:
        c.set_windows(np.concatenate(evs), offsets)
        opts = lib.default_solver(mode=lib.SOLVE_INDEPENDENT, max_num_iterations=8)
        d_sol = torch.full((2 * P, 2), -5.0, dtype=torch.float64, device="cuda")
        d_stats = torch.full((2 * P, 4), -5, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        c.solve_device(opts, d_sol.data_ptr(), d_stats.data_ptr())
        c.synchronize()
        sol, stats = d_sol.cpu().numpy().reshape(2, P, 2).copy(), d_stats.cpu().numpy().reshape(2, P, 4).copy()
        active = np.array([[c.patch_info(p, w)[1] for p in range(P)] for w in range(2)], dtype=bool)
        r_start = c.eval(np.zeros((2, P, 2)), want_jac=False)[0]
        r_end = c.eval(sol, want_jac=False)[0]
    return sol, stats, active, r_start, r_end


def test_solve_device(ebo, ebo_ab):
    """the per-patch solve forms D1 in the gather (an accepted step's Jacobian evaluation runs no scatter) from the same
    moment statements: the shipped and the A/B library agree bit for bit, every active slot is written, and no active patch
    ends above the residual it started from at zero flow (an LM step is accepted only if the cost falls; on these windows
    of uniform noise a patch may well end where it started)"""
    sol, stats, active, r_start, r_end = _solve_device(ebo)
    sol_ab, stats_ab, _, _, _ = _solve_device(ebo_ab)
    assert sol.tobytes() == sol_ab.tobytes() and stats.tobytes() == stats_ab.tobytes()
    assert (sol[active] != -5.0).all() and (stats[active] != -5).all()
    assert (r_end[active] <= r_start[active]).all()


@pytest.mark.parametrize("copies,block,wide", [(3, 512, True), (52, 128, False)], ids=["61 rects", "1040 rects"])
def test_shipped_library_at_the_ab_librarys_bits(ebo, ebo_ab, orc, copies, block, wide):
    """the shipped plan: 512 lanes below 1024 slots, 128 lanes from there (units of 256 events and more are dealt)"""
    rects, units = ti._scene(copies=copies, wide=wide)
    ev, offsets, flows = ti._assemble(rects, units)
    r, J, rv, shape = _eval(ebo, rects, ev, offsets, flows, {})
    assert shape[:2] == (1, block)
    ra, Ja, rva, _ = _eval(ebo_ab, rects, ev, offsets, flows, {})
    assert _same(r, ra) and _same(J, Ja) and _same(rv, rva) and _same(r, rv)
    _assert_units_at_the_oracle(orc, units, r, J, copies, wide)
