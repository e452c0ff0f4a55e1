"""The scenes of tests/lm2_scenes.py are sound (CPU only): the admission gate of tests/test_gpu_solve_branches.py, so
that the GPU tests cannot hide behind chaos.

  * the restatement tests/lm2_ref.py (objective: the oracle's contrastFunctor, one call per patch) against the
    oracle's own C++ solver (compensate_events_contrast, mode 1, the same options): evaluation counts, iterations and
    termination folded the way ebo_solve folds them are equal, flows agree within 1e-5;
  * every scene takes the branch it is named for, read from the traces, and differs from its base (the option put
    back);
  * no edge-loss window has a tie patch at zero flow, where every solve starts (tests/edge_ties.py);
  * every scene keeps every patch's decisions, and its flows to 1e-6, under eight seeded perturbations of the
    objective of the size lm2_scenes.E_V / E_J (ten times the measured device-to-oracle differences)."""
import numpy as np
import pytest

import lm2_ref as R
import lm2_scenes as S

_cache = {}


def results(scene, orc):
    if scene.name not in _cache:
        base = None if scene.base is None else S.solve_scene(scene, orc, scene.base_options(orc))
        _cache[scene.name] = (S.solve_scene(scene, orc), base)
    return _cache[scene.name]


@pytest.mark.parametrize("scene", S.SCENES, ids=S.SCENE_IDS)
def test_restatement_against_the_oracle_solver(orc, scene):
    res, _ = results(scene, orc)
    n = len(res) // len(S.windows(scene.window, orc))
    for w, ev in enumerate(S.windows(scene.window, orc)):
        fo, _, so = orc.compensate_events_contrast(ev, scene.objective.oparams(orc),
                                                   R.to_struct(orc, scene.options(orc)), want_image=False)
        mine = res[w * n:(w + 1) * n]
        fold = R.fold(mine)
        assert fold[:4] == (so.iterations, so.num_evals_cost, so.num_evals_jac, so.termination)
        assert fold[4] == pytest.approx(so.initial_cost, rel=1e-12) and fold[5] == pytest.approx(so.final_cost, rel=1e-9)
        flows = np.array([r.best if r is not None else (0.0, 0.0) for r in mine])
        assert np.abs(flows - fo).max() <= S.FLOW_BAR
        assert [r is not None for r in mine] == [bool(a) for a in orc.window_eval(ev, scene.objective.oparams(orc),
                                                                                  np.zeros((n, 2)))[2]]


@pytest.mark.parametrize("scene", S.SCENES, ids=["%s[%s]" % (s.name, s.branch) for s in S.SCENES])
def test_scene_takes_its_branch(orc, scene):
    res, base = results(scene, orc)
    hit = S.branch_patches(scene, orc, res, base)
    print(scene.name, scene.branch, "patches", hit)
    assert hit, [r.kinds for r in res if r is not None]
    if base is not None:  # the option put back gives another trace: the scene tests the option
        assert any(r is not None and r.trace != b.trace for r, b in zip(res, base))


def test_wild_candidates_of_the_edge_scene(orc):
    """The edge scene whose first accepted step follows rejected wild candidates: which of them take the objective's
    penalty branch (a value above max_possible_residual) and which are wild without it (the outer events move by more
    than a patch width)."""
    scene = next(s for s in S.SCENES if s.name == "wild_then_accept-edge")
    res, _ = results(scene, orc)
    for k, r in enumerate(res):
        pen, far = S.wild_candidates(scene, r)
        print("patch %d: penalty candidates %s, wild without penalty %s, first accepted at %d" % (k, pen, far, len(pen) + len(far) + 1))
        assert pen[:6] == [0, 1, 2, 3, 4, 5] and pen == list(range(len(pen)))  # the first divisors leave the step wild
    assert any(S.wild_candidates(scene, r)[1] for r in res)


EDGE_WINDOWS = sorted({s.window for s in S.SCENES if s.objective.loss == "edge"})


@pytest.mark.parametrize("window", EDGE_WINDOWS)
def test_no_tie_patches_at_zero_flow(orc, window):
    """Every active patch's oracle Jacobian at zero flow is unchanged to 1e-8 relative under reversal of its event list
    and three seeded shuffles: no argmax tie, so the order of the sums decides nothing.  Cap: zero tie patches.  (A
    shuffle keeps the list's first and last event in place: the functor takes its reference time from them.)"""
    edge = S.OBJECTIVES["edge"]
    ties = []
    for k, (w, p, rect, ev, active) in enumerate(S.patch_events(window, orc)):
        if not active:
            continue
        J0 = edge.patch_f(orc, ev, rect)((0.0, 0.0), True)[1]
        orders = [np.arange(len(ev))[::-1]]
        for s in range(3):
            inner = 1 + np.random.default_rng([77, s]).permutation(len(ev) - 2)
            orders.append(np.concatenate([[0], inner, [len(ev) - 1]]))
        for o in orders:
            J = edge.patch_f(orc, ev[o], rect)((0.0, 0.0), True)[1]
            if not (np.abs(J - J0) <= 1e-8 * np.abs(J0)).all():
                ties.append(k)
    assert ties == []


@pytest.mark.parametrize("scene", S.SCENES, ids=S.SCENE_IDS)
def test_scene_is_stable(orc, scene):
    res, _ = results(scene, orc)
    changed, move = S.stability(scene, orc, res)
    print("%s: flows move by %.2e under the perturbations" % (scene.name, move))
    assert changed == [] and move <= S.STABILITY_FLOW


CENTRAL = [s for s in S.SCENES if s.name in S.CENTRAL_SCENES]


@pytest.mark.parametrize("scene", CENTRAL, ids=[s.name for s in CENTRAL])
def test_central_difference_scene_is_stable(orc, scene):
    """The scenes run through HostLm with EBO_GRAD_CENTRAL: the same bar with the Jacobian a central difference of
    values perturbed one by one."""
    assert len(CENTRAL) == len(S.CENTRAL_SCENES)
    res = S.solve_scene(scene, orc, central=S.CENTRAL_STEP)
    changed, move = S.stability(scene, orc, res, central=S.CENTRAL_STEP)
    assert changed == [] and move <= S.STABILITY_FLOW
    assert S.branch_patches(scene, orc, res, None if scene.base is None else
                            S.solve_scene(scene, orc, scene.base_options(orc), central=S.CENTRAL_STEP))


@pytest.mark.parametrize("branch", sorted(S.UNREACHABLE), ids=["unreachable: " + b for b in sorted(S.UNREACHABLE)])
def test_unreachable_branch_is_named_with_its_reason(orc, branch):
    assert len(S.UNREACHABLE[branch]) > 40
    f = S.OBJECTIVES["var1"].patch_f(orc, *[S.patch_events("w0", orc)[0][i] for i in (3, 2)])
    if branch.startswith("non-finite"):
        assert np.isfinite(f((0.0, 0.0), False)[0]) and np.isfinite(f((1e70, -1e70), False)[0])
    else:
        # the undamped step: invalid on the exact evaluations, and not on every perturbed one
        scene = S.Scene("undamped", "w0", "var1", dict(initial_radius=float("inf")), "invalid_n")
        res = S.solve_scene(scene, orc)
        assert all(r.kinds == [R.INVALID] * 5 for r in res)
        assert S.stability(scene, orc, res)[0] != []


def test_lockstep_helper_is_the_single_solve(orc):
    """solve_lockstep (one batched call per round) walks every patch through the trace of solve()."""
    scene = next(s for s in S.SCENES if s.name == "sparse-var1")
    res, _ = results(scene, orc)
    patches = S.patch_events(scene.window, orc)
    fs = [scene.objective.patch_f(orc, ev, rect) for (_, _, rect, ev, _) in patches]
    calls = []

    def batched(points, jac, live):
        calls.append((jac & live).sum())
        r, J = np.zeros(len(fs)), np.zeros((len(fs), 2))
        for k in np.flatnonzero(live):
            r[k], J[k] = fs[k](points[k], bool(jac[k]))
        return r, J
    out = R.solve_lockstep(batched, len(fs), scene.options(orc), [p[4] for p in patches])
    assert [o is None for o in out] == [r is None for r in res] and any(o is None for o in out)
    assert all(o.trace == r.trace and o.best == r.best and o.stats == r.stats for o, r in zip(out, res) if r is not None)
    assert len(calls) == max(r.stats[1] + r.stats[2] for r in res if r is not None)
