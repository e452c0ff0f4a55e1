"""GPU: the edge loss where a unit's box meets the limits of its storage forms (tests/edge_fit_cases.py: single units of a few
dozen events, each built and checked at its limit on the CPU by tests/test_edge_fit_cases_cpu.py).  For every case the
device's own work counters (ebo_edge_work_stats) must equal the restated box's -- the case sits at its limit on the device
too -- and value and Jacobian must equal the oracle's at the bars of the other edge tests (value: check_rj's rtol 1e-9 of
tests/test_gpu_edge.py; Jacobian: jac_check.assert_jac_close as tests/test_gpu_random.py uses it), the same bits from the
value-only launch and from a second run, and the same bits wherever the code promises them (compact against the single
launch, the classify kernel on and off, the direction table on and off, a unit alone against the unit in a batch).

What this does not observe: the counters pin a unit's box, not the storage form the kernel chose for it.  The form is
inferred from the restatement.  A slip in the device's fit test that sends a fitting box to the slice changes no result;
one that admits a box too large shows only if it corrupts the value or the Jacobian past the oracle's bars."""
import numpy as np
import pytest

import edge_box_ref as ref
import edge_fit_cases as fc
from jac_check import assert_jac_close

pytestmark = pytest.mark.gpu

COUNTED = ("units", "events", "box_pixels", "eigen_pixels", "nms_windows")


def _oparams(orc, case):
    kw = dict(tv_weight=0.0, min_events=fc.MIN_EVENTS, scale=fc.SCALE, loss=0)
    if case.grid:
        kw.update(image_w=case.grid[0], image_h=case.grid[1], patch_w=case.grid[2], patch_h=case.grid[3])
    return orc.default_params(**kw)


def _oracle(orc, case):
    if case.grid:
        ev, _, _ = case.events()
        ro, Jo, active, _ = orc.window_eval(ev, _oparams(orc, case), case.flows())
        assert active.all()
        return ro, Jo
    got = [orc.contrast_eval(u.array(), u.rect, u.flow, 0, scale=fc.SCALE) for u in case.units]
    return np.array([g[0] for g in got]), np.array([g[1] for g in got])


def _load(lib, case):
    c = lib.Context(loss=lib.LOSS_EDGE, **case.ctx_kw())
    ev, offs, rects = case.events()
    if case.grid:
        c.set_window(ev)
    else:
        c.set_patches(ev, offs, rects)
    return c


def _check_against_oracle(r, J, ro, Jo):
    np.testing.assert_allclose(r, ro, rtol=1e-9, atol=1e-12)
    assert_jac_close(J, Jo, rtol=1e-8)
    assert np.isfinite(J).all() and (r < 1e3).all()


def _run_case(lib, orc, case, monkeypatch):
    """counters, oracle, value-only bits, run-to-run bits, the direction table on and off -> (r, J) of the case"""
    import torch
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    flows = case.flows()
    with _load(lib, case) as c:
        r, J = c.eval(flows)
        d_flows = torch.from_numpy(np.ascontiguousarray(flows)).to("cuda")
        want = case.sums()
        for want_jac in (True, False):
            st = c.edge_work_stats(d_flows.data_ptr(), want_jac)
            print(case.name, "jac" if want_jac else "value", st, "restated", want)
            assert {k: st[k] for k in COUNTED} == want
            assert (st["argmax_entries"] > 0) == want_jac
        v, _ = c.eval(flows, want_jac=False)
        r2, J2 = c.eval(flows)
        monkeypatch.setenv("EBO_EDGE_CS_MB", "0")  # (the shipped library reads this one too) no direction table
        r3, J3 = c.eval(flows)
        monkeypatch.delenv("EBO_EDGE_CS_MB")
    ro, Jo = _oracle(orc, case)
    print(case.name, "r - oracle", r[0] - ro, "J", J[0], "oracle", Jo)
    _check_against_oracle(r[0], J[0], ro, Jo)
    assert np.array_equal(v, r) and np.array_equal(r2, r) and np.array_equal(J2, J)
    assert np.array_equal(r3, r)
    assert np.abs(J3 - J).max() <= 1e-11 * np.abs(J).max()
    return r, J


SHIPPED = [c for c in fc.CASES if not c.ab]
AB = [c for c in fc.CASES if c.ab] + fc.PILE_CASES


def test_every_case_runs():
    assert len(SHIPPED) + len(AB) == len(fc.CASES) + len(fc.PILE_CASES) and {c.regime for c in SHIPPED} == {"a", "b", "c", "d"}


@pytest.mark.parametrize("case", SHIPPED, ids=[c.name for c in SHIPPED])
def test_shipped_library_at_the_limit(ebo, orc, monkeypatch, case):
    _run_case(ebo, orc, case, monkeypatch)


@pytest.mark.parametrize("case", AB, ids=[c.name for c in AB])
def test_ab_build_at_the_limit(ebo_ab, orc, monkeypatch, case):
    r, J = _run_case(ebo_ab, orc, case, monkeypatch)
    flows = case.flows()
    if case.setup.compact:
        # the two-launch compact path against the single launch on the 20 B form, and with the boxes and the second launch's
        # list made inside the compact launch instead of by k_edge_classify: bit for bit
        with _load(ebo_ab, case) as c:
            monkeypatch.setenv("EBO_EDGE_CLASSIFY", "0")
            r1, J1 = c.eval(flows)
            v1, _ = c.eval(flows, want_jac=False)
            monkeypatch.delenv("EBO_EDGE_CLASSIFY")
            monkeypatch.setenv("EBO_EDGE_COMPACT", "0")
            r0, J0 = c.eval(flows)
            v0, _ = c.eval(flows, want_jac=False)
        for rr, JJ, vv in ((r1, J1, v1), (r0, J0, v0)):
            assert np.array_equal(rr, r) and np.array_equal(JJ, J) and np.array_equal(vv, r)
    if case.cls in ("mixed", "mixed_reversed"):
        # each unit of the batch against the same unit alone (in its own context, under the same switches)
        monkeypatch.setenv("EBO_EDGE_COMPACT", "1")
        for i, u in enumerate(case.units):
            alone = fc.Case(case.name + "[%d]" % i, case.regime, [u], case.setup, case.env)
            with _load(ebo_ab, alone) as c:
                ra, Ja = c.eval(alone.flows())
            assert ra[0, 0] == r[0, i] and np.array_equal(Ja[0, 0], J[0, i]), i


def test_mixed_batch_in_both_orders_gives_the_same_bits(ebo_ab, monkeypatch):
    got = {}
    for name in ("e52/mixed", "e52/mixed_reversed"):
        case = fc.BY_NAME[name]
        for k, v in case.env.items():
            monkeypatch.setenv(k, v)
        with _load(ebo_ab, case) as c:
            got[name] = c.eval(case.flows())
    (ra, Ja), (rb, Jb) = got["e52/mixed"], got["e52/mixed_reversed"]
    assert np.array_equal(ra[0], rb[0][::-1]) and np.array_equal(Ja[0], Jb[0][::-1])


@pytest.mark.parametrize("case", fc.SOLVE_CASES, ids=[c.name for c in fc.SOLVE_CASES])
def test_device_solve_across_the_limit(ebo_ab, monkeypatch, case):
    """k_solve_edge on a unit whose box fits at the start and has outgrown the capacity at the end (the record of a value-only
    evaluation is dropped whenever a point lands on the slice): the lock-step solve's flows to 1e-9 and its counts, as
    test_edge_device_solve_equals_the_lockstep_solve asks; the same bits without the record; run to run the same bits"""
    ebo = ebo_ab
    for k, v in case.env.items():
        monkeypatch.setenv(k, v)
    u = case.units[0]
    with _load(ebo, case) as c:
        opts = ebo.default_solver(mode=ebo.SOLVE_INDEPENDENT, **fc.SOLVE_OPTS)
        dev, sd = c.solve(opts)
        dev2, _ = c.solve(opts)
        monkeypatch.setenv("EBO_SOLVE_NO_REUSE", "1")
        plain, sp = c.solve(opts)
        monkeypatch.delenv("EBO_SOLVE_NO_REUSE")
        monkeypatch.setenv("EBO_SOLVE_EDGE", "lockstep")
        lock, sl = c.solve(opts)
    print(case.name, "device", dev[0, 0], "lockstep", lock[0, 0], "iterations", sd[0].iterations, sl[0].iterations)
    assert np.array_equal(dev, dev2) and np.array_equal(dev, plain)
    np.testing.assert_allclose(dev, lock, rtol=0, atol=1e-9)
    for s in (sd[0], sp[0]):
        assert (s.iterations, s.num_evals_cost, s.num_evals_jac) == (sl[0].iterations, sl[0].num_evals_cost, sl[0].num_evals_jac)
    # the restatement at the start and at the device's end: on the LDS form, then on the slice
    assert ref.form_of(u.box_at((0.0, 0.0)), case.setup) == case.form_start != ref.FORM_SLICE
    assert ref.form_of(u.box_at(tuple(dev[0, 0])), case.setup) == ref.FORM_SLICE
