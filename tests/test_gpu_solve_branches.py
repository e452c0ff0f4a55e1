"""The per-patch device LM (LmUnit: k_solve_independent<SMALL> for the variance loss, k_solve_edge for the edge loss)
and its host copy (HostLm, driven by lockstep.h) on the scenes of tests/lm2_scenes.py, against the plain restatement
tests/lm2_ref.py: per patch the iteration, evaluation and termination statistics EXACTLY, the flows within 1e-5 (the
project's bar for a solved parameter).  tests/test_lm2_cpu.py admits the scenes on the CPU: the restatement agrees with
the oracle's own solver on them, each takes the branch it is named for, and none changes a decision under evaluation
errors ten times those measured between device and oracle.

Replay (test_replay_*): the restatement driven in lock step by the device's OWN standalone evaluations has no chaos
limit -- it sees the numbers the kernel sees, if the in-kernel evaluation gives the bits of the standalone kernels.
REPLAY_BIT_EQUAL records per loss what the first run on an MI355X found ("Per-patch LM: the branch
scenes")."""
import numpy as np
import pytest

import eval_cases as EC
import lm2_ref as R
import lm2_scenes as S

pytestmark = pytest.mark.gpu

SENTINEL = -5
P = len(EC.grid_rects())
# Per loss: did every option set replay bit for bit at the full 50 iterations on the first run (2026-10-20, MI355X)?
#   edge:     yes, 22 of 22 option sets: statistics equal and flows the same bits.  k_solve_edge's in-kernel evaluation
#             gives the bits of the standalone k_eval_edge, so the replay is asserted with np.array_equal from now on.
#   variance: no.  33 of 40 option sets ended with equal statistics, 16 with the same flow bits; the first difference is
#             at the rounding level after one accepted step (1.8e-16 on param_tol-var1) and grows to 7.4e-2 on cap_n-var1
#             by iteration 50: k_solve_independent's evaluation rounds differently from the standalone k_eval3
#             (eval_unit's comment: the same statements, another schedule).  Full-length variance runs keep to invariants.
REPLAY_BIT_EQUAL = {"variance": False, "edge": True}
FULL_LENGTH = 50

_ref_cache, _dev_cache = {}, {}


def reference(scene, orc):
    """The restatement on the oracle's objective, once per scene."""
    if scene.name not in _ref_cache:
        _ref_cache[scene.name] = S.solve_scene(scene, orc)
    return _ref_cache[scene.name]


def load(c, evs):
    if len(evs) == 1:
        c.set_window(evs[0])
    else:
        offs = np.concatenate([[0], np.cumsum([len(e) for e in evs])]).astype(np.uint64)
        c.set_windows(np.concatenate(evs), offs)


def context(lib, scene, n_windows=1, **kw):
    return lib.Context(scene.objective.params(lib, max_windows=n_windows, **kw))


def device_solve(lib, scene, evs, opts):
    """One ebo_solve_device launch into sentinel-filled torch tensors, then ebo_solve on the same context.
    -> (flows [n][2], stats [n][4], ebo_solve's flows [n][2], ebo_solve's summaries)"""
    import torch
    n = len(evs) * P
    o = R.to_struct(lib, opts)
    with context(lib, scene, len(evs)) as c:
        load(c, evs)
        d_sol = torch.full((n, 2), float(SENTINEL), dtype=torch.float64, device="cuda")
        d_stats = torch.full((n, 4), SENTINEL, dtype=torch.int32, device="cuda")
        torch.cuda.synchronize()
        c.solve_device(o, d_sol.data_ptr(), d_stats.data_ptr())
        c.synchronize()
        flows, stats = d_sol.cpu().numpy().copy(), d_stats.cpu().numpy().copy()
        flows2, summ = c.solve(o)
    return flows, stats, flows2.reshape(n, 2), [(s.iterations, s.num_evals_cost, s.num_evals_jac, s.termination,
                                                 s.initial_cost, s.final_cost) for s in summ]


def device(ebo, scene, orc):
    if scene.name not in _dev_cache:
        _dev_cache[scene.name] = device_solve(ebo, scene, S.windows(scene.window, orc), scene.options(ebo))
    return _dev_cache[scene.name]


def assert_matches(ref, flows, stats, what):
    """Every active patch: statistics equal, flows within the bar.  Every other slot: zeros.  Nothing skipped."""
    assert len(ref) == len(flows) == len(stats)
    worst = 0.0
    for k, r in enumerate(ref):
        if r is None:
            assert (stats[k] == 0).all() and (flows[k] == 0.0).all(), (what, k, stats[k], flows[k])
            continue
        assert tuple(int(v) for v in stats[k]) == r.counts, (what, k, tuple(stats[k]), r.counts, r.kinds)
        worst = max(worst, float(np.abs(flows[k] - np.array(r.best)).max()))
    print("%s: max |flow - restatement| = %.3e" % (what, worst))
    assert worst <= S.FLOW_BAR, (what, worst)


@pytest.mark.parametrize("scene", S.SCENES, ids=S.SCENE_IDS)
def test_device_solve_against_the_restatement(ebo, orc, scene):
    """ebo_solve_device: per patch (iterations, value evaluations, Jacobian evaluations, termination) equal the
    restatement's, flows within 1e-5; inactive patches all zero; every slot written (the stray unit has none)."""
    flows, stats, _, _ = device(ebo, scene, orc)
    assert (stats != SENTINEL).all() and (flows != float(SENTINEL)).all()
    assert_matches(reference(scene, orc), flows, stats, scene.name)


@pytest.mark.parametrize("scene", S.SCENES, ids=S.SCENE_IDS)
def test_ebo_solve_is_the_fold_of_the_device_statistics(ebo, orc, scene):
    """ebo_solve (device-resident path) on the same scenes: the flows of ebo_solve_device bit for bit, the summary
    exactly the fold of the per-patch statistics (max of iterations and termination, sums of the evaluation counts),
    initial_cost and final_cost 0 (include/ebo.h: only the lock-step path reports them in independent mode)."""
    flows, stats, flows2, summ = device(ebo, scene, orc)
    assert np.array_equal(flows, flows2)
    for w in range(len(summ)):
        assert summ[w][:4] == R.fold_counts(stats[w * P:(w + 1) * P]), (w, summ[w])
        assert summ[w][4] == 0.0 and summ[w][5] == 0.0


# ---- lock-step HostLm ----------------------------------------------------------------------------------------------
def lockstep_patches(lib, scene, orc, monkeypatch, **ctx_kw):
    """Every patch of the scene as its own ebo_set_patches list through the host path (HostLm + lockstep.h), so that
    ebo_solve's summary is per patch.  -> list of (flow [2], summary tuple) or None where inactive"""
    out = []
    o = R.to_struct(lib, scene.options(lib))
    with context(lib, scene, 1, **ctx_kw) as c:
        for (w, p, rect, ev, active) in S.patch_events(scene.window, orc):
            if not active:
                out.append(None)
                continue
            c.set_patches(ev, [0, len(ev)], [rect])
            f, s = c.solve(o)
            s = s[0]
            out.append((f.reshape(2).copy(), (s.iterations, s.num_evals_cost, s.num_evals_jac, s.termination,
                                              s.initial_cost, s.final_cost)))
    return out


def assert_lockstep(ref, got, what):
    worst = 0.0
    for k, r in enumerate(ref):
        if r is None:
            assert got[k] is None
            continue
        flow, summ = got[k]
        assert summ[:4] == r.counts, (what, k, summ, r.counts, r.kinds)
        assert summ[4] == pytest.approx(r.stats[4], rel=1e-9), (what, k)
        assert summ[5] == pytest.approx(r.stats[5], rel=1e-9), (what, k)
        worst = max(worst, float(np.abs(flow - np.array(r.best)).max()))
    print("%s: max |flow - restatement| = %.3e" % (what, worst))
    assert worst <= S.FLOW_BAR, (what, worst)


EDGE_SCENES = [s for s in S.SCENES if s.objective.loss == "edge"]


@pytest.mark.parametrize("scene", EDGE_SCENES, ids=[s.name for s in EDGE_SCENES])
def test_lockstep_host_lm_edge(ebo_ab, orc, monkeypatch, scene):
    """EBO_SOLVE_EDGE=lockstep (the A/B build): HostLm per patch over batched evaluations, the same option table.
    Statistics equal, flows within 1e-5, initial_cost and final_cost (reported on this path) within 1e-9 relative."""
    monkeypatch.setenv("EBO_SOLVE_EDGE", "lockstep")
    got = lockstep_patches(ebo_ab, scene, orc, monkeypatch)
    assert_lockstep(reference(scene, orc), got, scene.name)


CENTRAL_SCENES = [s for s in S.SCENES if s.name in S.CENTRAL_SCENES]


@pytest.mark.parametrize("scene", CENTRAL_SCENES, ids=[s.name for s in CENTRAL_SCENES])
def test_lockstep_host_lm_variance_central(ebo, orc, monkeypatch, scene):
    """grad = EBO_GRAD_CENTRAL sends the variance loss through HostLm too.  The restatement's objective is then the
    oracle's central-difference formula (as _fd_jacobian in tests/test_gpu_eval_sweep.py)."""
    ref = S.solve_scene(scene, orc, central=S.CENTRAL_STEP)
    got = lockstep_patches(ebo, scene, orc, monkeypatch, grad=ebo.GRAD_CENTRAL, fd_step=S.CENTRAL_STEP)
    assert_lockstep(ref, got, scene.name)


# ---- batch ---------------------------------------------------------------------------------------------------------
BATCH_SCENES = [s for s in S.SCENES if len(S.WINDOWS_COUNT[s.window]) > 1]


@pytest.mark.parametrize("scene", BATCH_SCENES, ids=[s.name for s in BATCH_SCENES])
def test_batch_equals_each_window_alone(ebo, orc, scene):
    """The 2-window batch: per-patch statistics and flows are those of each window solved alone, bit for bit."""
    flows, stats, _, _ = device(ebo, scene, orc)
    for w, ev in enumerate(S.windows(scene.window, orc)):
        f1, s1, _, _ = device_solve(ebo, scene, [ev], scene.options(ebo))
        assert np.array_equal(f1, flows[w * P:(w + 1) * P]) and np.array_equal(s1, stats[w * P:(w + 1) * P]), w


# ---- replay --------------------------------------------------------------------------------------------------------
def replay(lib, scene, evs, opts):
    """tests/lm2_ref.py's lock-step helper driven by the device's own standalone evaluations (ebo_eval): per round
    one launch with Jacobians for the patches that want them and one without for the others."""
    n = len(evs) * P
    with context(lib, scene, len(evs)) as c:
        load(c, evs)
        active = np.array([c.patch_info(k % P, k // P)[1] for k in range(n)])

        def batched(points, jac, live):
            r = np.zeros(n)
            J = np.zeros((n, 2))
            if (live & jac).any():
                rj, Jj = c.eval(points)
                sel = live & jac
                r[sel], J[sel] = rj.reshape(n)[sel], Jj.reshape(n, 2)[sel]
            if (live & ~jac).any():
                rv, _ = c.eval(points, want_jac=False)
                sel = live & ~jac
                r[sel] = rv.reshape(n)[sel]
            return r, J
        return R.solve_lockstep(batched, n, opts, active)


def full_length(scene, lib):
    o = scene.options(lib)
    if "max_num_iterations" not in scene.opts or scene.opts["max_num_iterations"] > 0:
        o["max_num_iterations"] = FULL_LENGTH
    return o


OPTION_SETS = {}
for _s in S.SCENES:
    OPTION_SETS.setdefault((_s.objective.name, _s.window, tuple(sorted((k, v) for k, v in _s.opts.items()
                                                                          if k != "max_num_iterations"))), _s)
REPLAY_SCENES = list(OPTION_SETS.values())


@pytest.mark.parametrize("scene", REPLAY_SCENES, ids=[s.name for s in REPLAY_SCENES])
def test_replay_with_the_devices_own_evaluations(ebo, orc, scene):
    """Every option set at the full 50 iterations.  On the admitted (capped) scene: statistics equal, flows within
    1e-5.  At full length: bit equality of flows and statistics where REPLAY_BIT_EQUAL says the first run found it for
    the loss, otherwise the invariants (termination in {0, 1, 2}, iterations <= cap, the oracle's cost at the returned
    flow <= its cost at zero flow on every active patch)."""
    evs = S.windows(scene.window, orc)
    loss = scene.objective.loss
    # the admitted scene
    flows, stats, _, _ = device(ebo, scene, orc)
    assert_matches(replay(ebo, scene, evs, scene.options(ebo)), flows, stats, scene.name + " (replay)")
    # full length
    o = full_length(scene, ebo)
    ref = replay(ebo, scene, evs, o)
    flows, stats, _, _ = device_solve(ebo, scene, evs, o)
    act = [k for k, r in enumerate(ref) if r is not None]
    same_stats = all(tuple(int(v) for v in stats[k]) == ref[k].counts for k in act)
    dflow = max([float(np.abs(flows[k] - np.array(ref[k].best)).max()) for k in act] or [0.0])
    print("REPLAY %s loss=%s full length: stats %s, max |dflow| = %.3e" % (scene.name, loss,
                                                                         "equal" if same_stats else "DIFFER", dflow))
    if REPLAY_BIT_EQUAL[loss]:
        want_flows = np.array([r.best if r is not None else (0.0, 0.0) for r in ref])
        want_stats = np.array([r.counts if r is not None else (0, 0, 0, 0) for r in ref], dtype=np.int32)
        assert np.array_equal(flows, want_flows) and np.array_equal(stats, want_stats)
        return
    prm = scene.objective.oparams(orc)
    for w, ev in enumerate(evs):
        f = flows[w * P:(w + 1) * P]
        r1 = orc.window_eval(ev, prm, f, want_jac=False)[0]
        r0 = orc.window_eval(ev, prm, np.zeros((P, 2)), want_jac=False)[0]
        for p in range(P):
            k = w * P + p
            if ref[k] is None:
                assert (stats[k] == 0).all()
                continue
            assert stats[k][3] in (0, 1, 2) and 0 <= stats[k][0] <= o["max_num_iterations"]
            assert 0.5 * r1[p] ** 2 <= 0.5 * r0[p] ** 2, (scene.name, k)
