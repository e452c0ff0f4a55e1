"""The objective kernels over the functor constants ebo_create admits and over pixel pile-ups, against the oracle
given the SAME constants: k_eval3 (both exp paths), the edge kernels, the device-resident per-patch solve and the
contrast image.  The cases are tests/eval_cases.py's; tests/test_eval_consts_cpu.py checks the oracle itself at
those constants against a second restatement.  Bars as tests/test_gpu_parity.py: value relative 1e-9, variance
Jacobian as test_eval_value_and_jacobian, edge Jacobian by jac_check, solved flows 1e-5."""
import ctypes as C
import json
import os

import numpy as np
import pytest

import eval_cases as EC
from jac_check import assert_jac_close

pytestmark = pytest.mark.gpu

RTOL = 1e-9
# below the TV-free solve's chaos horizon (tests/test_gpu_parity.py), which is shorter for the edge loss
# (tests/test_gpu_edge.py): its derivative jumps when a window's argmax moves.  Measured on the case
# max_possible_residual = 1: device and oracle take the same steps (equal evaluation counts at every cap) while
# their flows part by ~100x per iteration from 1e-13 after the first -- 1.6e-7 after 3, 1.6e-4 after 4, 4.9 after 8.
# On the sigma 0.25 pile-up (a unit on a grid 4x coarser, unit_fix_grid) they part from 7e-10 after the first to
# 1.6e-7 after the second; in the third one side accepts a 979-pixel step the other rejects (9 against 8 evaluations)
SOLVE_ITERS = {"variance": 8, "edge": 2}
_RECORD = os.environ.get("EBO_SWEEP_RECORD")  # diagnostics: the largest error / bar per case, as JSON lines


def _record(case, loss, what, ratio):
    if _RECORD:
        with open(_RECORD, "a") as f:
            f.write(json.dumps(dict(case=case.name, loss=loss, what=what, ratio=float(ratio))) + "\n")


def check_value(case, loss, r, ro):
    """Relative 1e-9; the absolute floor scales with max_possible_residual (1e-12 at the reference's 1e3)."""
    r, ro = np.asarray(r), np.asarray(ro)
    atol = 1e-12 * case.max_res / 1e3
    bar = RTOL * np.abs(ro) + atol
    _record(case, loss, "value", np.nanmax(np.abs(r - ro) / bar) if r.size else 0.0)
    np.testing.assert_allclose(r, ro, rtol=RTOL, atol=atol)


def check_jac(case, loss, J, Jo, n_ev=0, retie=None):
    """Variance: as test_eval_value_and_jacobian (the absolute floor scaled with max_possible_residual).  Edge:
    jac_check's bound on every patch whose oracle Jacobian is finite (the reference's Jet arithmetic gives NaN / inf
    where an eigenvalue difference is 0 or denormal); a patch outside it must be an argmax tie: retie(q) re-evaluates
    it the reference's way (test_gpu_random.py's protocol) and must then agree."""
    J, Jo = np.asarray(J, dtype=np.float64).reshape(-1, 2), np.asarray(Jo, dtype=np.float64).reshape(-1, 2)
    if loss == "variance":
        # a unit whose events could fill a pixel stores its image on a coarser grid (unit_fix_grid): the bar grows
        # with the grid step
        g = 2.0 ** (EC.unit_exponent(case.sigma, n_ev) - EC.fixed_exponent(case.sigma))
        atol = g * 1e-10 * case.max_res / 1e3
        bar = g * RTOL * np.abs(Jo) + atol
        _record(case, loss, "jacobian", np.nanmax(np.abs(J - Jo) / bar) if J.size else 0.0)
        np.testing.assert_allclose(J, Jo, rtol=g * RTOL, atol=atol)
        return
    fin = np.isfinite(Jo).all(axis=1)
    scale = np.abs(Jo).max(axis=1, keepdims=True)
    out = ((np.abs(J - Jo) > 1e-8 * np.abs(Jo) + 1e-8 * scale + 1e-13) | ~np.isfinite(J)).any(axis=1) & fin
    _record(case, loss, "edge_jacobian_ties", out.sum())
    assert_jac_close(J[fin & ~out], Jo[fin & ~out])
    for q in np.flatnonzero(out):
        assert retie is not None, "edge Jacobian of patch %d: %r, oracle %r" % (q, J[q], Jo[q])
        rq, Jq = retie(q)
        assert_jac_close(Jq, Jo[q], rtol=1e-8, patch_rel=1e-5, floor=5e-8)  # a tie patch in reference-order mode


REFERENCE_ORDER = {"EBO_KEEP_ORDER": "1", "EBO_EDGE_ABLATE": "64", "EBO_EDGE_SEPARABLE": "0"}


def reference_order_eval(ebo_ab, monkeypatch, case, ev, rect, flow):
    """One edge-loss patch by the A/B build's reference-order diagnostic (as tests/test_gpu_random.py), with the
    case's constants.  ev: the patch's events in list order.  -> (r, J[2])"""
    for k, v in REFERENCE_ORDER.items():
        monkeypatch.setenv(k, v)
    try:
        p = case.params(ebo_ab, ebo_ab.LOSS_EDGE)
        p.max_events = max(len(ev), 1)
        with ebo_ab.Context(p) as c1:
            c1.set_patches(ev, [0, len(ev)], [rect])
            r1, J1 = c1.eval(np.asarray(flow, dtype=np.float64).reshape(1, 2))
    finally:
        for k in REFERENCE_ORDER:
            monkeypatch.delenv(k, raising=False)
    return r1[0][0], J1[0][0]


def _in_rect(ev, rect):
    x, y, w, h = rect
    return ev[(ev["x"] >= x) & (ev["x"] < x + w) & (ev["y"] >= y) & (ev["y"] < y + h)]


def _losses(ebo):
    return [("variance", ebo.LOSS_VARIANCE), ("edge", ebo.LOSS_EDGE)]


def _variance_case(case, orc, values):
    """sigma cases: the variance loss with max_possible_residual = twice the largest variance term of the case
    (values: the oracle's variance terms), so that the value bar is relative to the variance itself -- at the
    reference's 1e3 the term vanishes in r = 1e3 - var for sigma >= 30."""
    if not case.name.startswith("sigma="):
        return case
    v = np.asarray(values, dtype=np.float64)
    return case.with_max_res(max(2.0 * float(v[np.isfinite(v)].max()), 1e-300))


def _var_terms_window(case, orc, ev, sets):
    prm = case.with_max_res(1e-300).oparams(orc, 1)
    return np.concatenate([-orc.window_eval(ev, prm, f, want_jac=False)[0] for f in sets])


def _ctx(ebo, case, loss):
    return ebo.Context(case.params(ebo, loss))


def _fd_jacobian(orc, ev, prm, flows, h):
    """EBO_GRAD_CENTRAL's formula on the oracle's values."""
    num = np.zeros_like(flows)
    for k in range(2):
        d = np.zeros_like(flows)
        d[:, k] = h
        rp = orc.window_eval(ev, prm, flows + d, want_jac=False)[0]
        rm = orc.window_eval(ev, prm, flows - d, want_jac=False)[0]
        num[:, k] = (rp - rm) / (2 * h)
    return num


@pytest.mark.parametrize("case", EC.CASES, ids=EC.CASE_IDS)
def test_window_eval_against_the_oracle(ebo, ebo_ab, monkeypatch, orc, case):
    """ebo_set_window + ebo_eval (value with Jacobian, value only) and ebo_eval_device, both losses."""
    ev = EC.window(case, orc)
    hip = C.CDLL("libamdhip64.so")
    rects = EC.grid_rects()
    for lname, loss in _losses(ebo):
        sets = EC.flow_sets(case, len(rects))
        if case.pile and lname == "variance":
            sets.append(np.zeros((len(rects), 2)))  # zero fraction: every pile-up event adds the full central tap
        cs = _variance_case(case, orc, _var_terms_window(case, orc, ev, sets)) if lname == "variance" else case
        prm = cs.oparams(orc, loss)
        with _ctx(ebo, cs, loss) as c:
            c.set_window(ev)
            for flows in sets:
                retie = lambda q: reference_order_eval(ebo_ab, monkeypatch, cs, _in_rect(ev, rects[q]), rects[q],
                                                       flows[q])
                r, J = c.eval(flows)
                ro, Jo, active, counts = orc.window_eval(ev, prm, flows)
                assert [c.patch_info(p)[0] for p in range(c.P)] == list(counts)
                check_value(cs, lname, r[0], ro)
                if case.fd_step is None:
                    check_jac(cs, lname, J[0], Jo, max(counts), retie)
                else:
                    h = case.fd_step
                    num = _fd_jacobian(orc, ev, prm, flows, h)
                    # the same formula on both sides, limited by the cancellation in (r+ - r-)
                    atol = 2e-15 * np.abs(ro).max() / h
                    np.testing.assert_allclose(J[0], num, rtol=0, atol=atol)
                r1, _ = c.eval(flows, want_jac=False)
                check_value(cs, lname, r1[0], ro)
            # ebo_eval_device: the same numbers as ebo_eval
            flows = np.ascontiguousarray(sets[0])
            n = c.P
            d_flows, d_out = C.c_void_p(), C.c_void_p()
            assert hip.hipMalloc(C.byref(d_flows), C.c_size_t(n * 16)) == 0
            assert hip.hipMalloc(C.byref(d_out), C.c_size_t(n * 24)) == 0
            try:
                assert hip.hipMemcpy(d_flows, flows.ctypes.data_as(C.c_void_p), C.c_size_t(n * 16), 1) == 0
                c.eval_device(d_flows.value, 1, d_out.value)
                c.synchronize()
                got = np.zeros((n, 3))
                assert hip.hipMemcpy(got.ctypes.data_as(C.c_void_p), d_out, C.c_size_t(n * 24), 2) == 0
            finally:
                hip.hipFree(d_flows)
                hip.hipFree(d_out)
            r, J = c.eval(flows)
            if lname == "variance":
                assert np.array_equal(got[:, 0], r[0]) and np.array_equal(got[:, 1:], J[0])
            else:  # f64 LDS atomics of the edge reverse pass: not bit-reproducible
                ro, Jo, _, _ = orc.window_eval(ev, prm, flows)
                check_value(cs, lname, got[:, 0], ro)
                if case.fd_step is None:
                    check_jac(cs, lname, got[:, 1:], Jo, len(ev),
                              lambda q: reference_order_eval(ebo_ab, monkeypatch, cs, _in_rect(ev, rects[q]), rects[q],
                                                             flows[q]))


@pytest.mark.parametrize("case", EC.CASES, ids=EC.CASE_IDS)
def test_patches_eval_and_contrast_image_against_the_oracle(ebo, ebo_ab, monkeypatch, orc, case):
    """ebo_set_patches (1x1, 1xN, regular and odd-sized rects) + ebo_eval, both losses; and the three channels of
    ebo_contrast_image (its own float64 splat: it checks the warp, the taps and their derivatives, not the
    fixed-point image of the objective)."""
    evs, offs, rects = EC.patch_lists(case, orc)
    ev = np.concatenate(evs)
    for lname, loss in _losses(ebo):
        sets = EC.flow_sets(case, len(rects))
        cs = case
        if lname == "variance":
            k0 = case.with_max_res(1e-300).consts(orc)
            cs = _variance_case(case, orc, [-orc.contrast_eval(evs[q], rects[q], f[q], loss, want_jac=False,
                                                                scale=case.scale, consts=k0)[0]
                                            for f in sets for q in range(len(rects))])
        k = cs.consts(orc)
        with _ctx(ebo, cs, loss) as c:
            c.set_patches(ev, offs, rects)
            for flows in sets:
                r, J = c.eval(flows)
                r1, _ = c.eval(flows, want_jac=False)
                out = [orc.contrast_eval(evs[q], rects[q], flows[q], loss, scale=case.scale, consts=k)
                       for q in range(len(rects))]
                ro = np.array([o[0] for o in out])
                check_value(cs, lname, r[0], ro)
                check_value(cs, lname, r1[0], ro)
                if case.fd_step is None:
                    check_jac(cs, lname, J[0], np.array([o[1] for o in out]), max(len(e) for e in evs),
                              lambda q: reference_order_eval(ebo_ab, monkeypatch, cs, evs[q], rects[q], flows[q]))
        if lname == "edge":
            continue
        with _ctx(ebo, cs, loss) as c:
            c.set_patches(ev, offs, rects)
            flows = sets[1]
            for q in range(len(rects)):
                img = c.contrast_image(q, flows[q], 3)
                ref = orc.contrast_image(evs[q], rects[q], flows[q], 3, scale=case.scale, consts=k)
                np.testing.assert_allclose(img, ref, rtol=1e-11, atol=1e-13 * max(1.0, np.abs(ref).max()))


# the per-patch device solve: every case but the central-difference ones, both losses
SOLVE_CASES = [c for c in EC.CASES if c.fd_step is None]


@pytest.mark.parametrize("case", SOLVE_CASES, ids=[c.name for c in SOLVE_CASES])
def test_solve_independent_against_the_oracle(ebo, orc, case):
    ev = EC.window(case, orc)
    for lname, loss in _losses(ebo):
        with _ctx(ebo, case, loss) as c:
            c.set_window(ev)
            flows, summ = c.solve(mode=ebo.SOLVE_INDEPENDENT, max_num_iterations=SOLVE_ITERS[lname])
        fo, _, so = orc.compensate_events_contrast(
            ev, case.oparams(orc, loss), orc.default_solver(mode=1, max_num_iterations=SOLVE_ITERS[lname]),
            want_image=False)
        err = np.abs(flows[0] - fo).max()
        _record(case, lname, "solve", err / 1e-5)
        assert err <= 1e-5, "%s: max |flow_gpu - flow_oracle| = %.3e" % (lname, err)
        assert summ[0].num_evals_jac == so.num_evals_jac and summ[0].iterations == so.iterations
