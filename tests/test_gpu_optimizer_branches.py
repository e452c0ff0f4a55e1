"""The tracker's LM (k_optimizer_solve, csrc/ebo_optimizer.inc: the third copy of the trust-region state machine)
under option variants, per patch against the oracle's own solver (oracle/optimizer_oracle.cpp) given the same options:
each exit, min_relative_decrease, the non-monotonic steps, Jacobi scaling, the diagonal clips, max_radius, invalid
steps and a small initial radius.  On tests/test_optimizer.py's _batch(orc, 6) at caps <= 10, the horizon that file
documents.  A CPU test first shows that each variant changes the oracle's per-patch summary against the default on at
least one patch (max_consecutive_nonmonotonic: against the variant it is added to): otherwise the variant would test
nothing."""
import numpy as np
import pytest

from test_optimizer import _batch, _ctx

N = 6
TINY = dict(initial_radius=1e-320, min_radius=0.0)  # diagonal / radius overflows: every step is invalid
VARIANTS = {
    "cap 0": dict(max_num_iterations=0),
    "cap 3": dict(max_num_iterations=3),
    "gradient tolerance at iteration 0": dict(gradient_tolerance=1e3),
    "gradient tolerance after accepted steps": dict(gradient_tolerance=1e-3),
    "minimum radius": dict(min_radius=1e3),
    "minimum radius at iteration 0": dict(min_radius=1e5),
    "parameter tolerance alone": dict(parameter_tolerance=1e-2, function_tolerance=0.0),
    "function tolerance alone": dict(function_tolerance=1e-3, parameter_tolerance=0.0),
    "min_relative_decrease 0.5": dict(min_relative_decrease=0.5),
    "use_nonmonotonic off": dict(use_nonmonotonic=0),
    # at the default options no patch of the batch takes three cost-raising steps in a row within 10 iterations; with
    # the diagonal held at 1 one does, so this variant is compared with that one (BASES)
    "max_consecutive_nonmonotonic 2": dict(min_lm_diagonal=1.0, max_lm_diagonal=1.0, max_consecutive_nonmonotonic=2),
    "jacobi_scaling off": dict(jacobi_scaling=0),
    "both diagonal clips": dict(min_lm_diagonal=1.0, max_lm_diagonal=1.0),
    "lower diagonal clip": dict(min_lm_diagonal=1e-2),
    "upper diagonal clip": dict(max_lm_diagonal=1e-2),
    "max_radius": dict(max_radius=1e2),
    "five invalid steps": dict(TINY),
    "max_consecutive_invalid 1": dict(TINY, max_consecutive_invalid=1),
    "small initial radius": dict(initial_radius=1e-3),
}
# Not a variant: function_tolerance = parameter_tolerance = 0.  A converged patch then ends only when a cost change is
# EXACTLY zero, a comparison at the rounding level of the objective: the oracle's own summary of patch 4 changes when
# its input moves by 1e-12 relative (test_variant_is_stable_on_the_oracle would refuse it), and the device, whose
# residuals agree with the oracle's to 1e-12 (test_device_functor_matches_oracle), took 9 Jacobian evaluations there
# against the oracle's 10 with iterations and termination equal.
BASES = {"max_consecutive_nonmonotonic 2": "both diagonal clips"}  # every other variant: against the default options
IDS = list(VARIANTS)

_cache = {}


def oracle_solves(orc, name):
    """-> list over the patches of (pose, flow direction, summary tuple)"""
    if name not in _cache:
        grad, items = _batch(orc, N)
        o = orc.optimizer_default_solver(**VARIANTS.get(name, {}))
        out = []
        for it in items:
            p, f, s = orc.optimizer_solve(grad, it["rect"], it["nabla"], it["start"][0], it["start"][1], opts=o)
            out.append((p, f, (s.iterations, s.termination, s.num_evals_cost, s.num_evals_jac, s.initial_cost, s.final_cost)))
        _cache[name] = out
    return _cache[name]


@pytest.mark.parametrize("name", IDS)
def test_variant_changes_the_oracle_summary(orc, name):
    base, got = oracle_solves(orc, BASES.get(name, "default")), oracle_solves(orc, name)
    differ = [i for i in range(N) if got[i][2] != base[i][2]]
    print(name, "differs from", BASES.get(name, "default"), "on patches", differ, [g[2][:4] for g in got])
    assert differ


@pytest.mark.parametrize("name", IDS)
def test_variant_is_stable_on_the_oracle(orc, name):
    """The admission gate of the GPU test: the oracle's own per-patch summary stands when the integrated nabla moves by
    1e-12 relative (the bar between the device's and the oracle's residuals), eight seeded times."""
    grad, items = _batch(orc, N)
    o = orc.optimizer_default_solver(**VARIANTS[name])
    want = [s[2][:4] for s in oracle_solves(orc, name)]
    for seed in range(8):
        for k, it in enumerate(items):
            nabla = it["nabla"] * (1.0 + 1e-12 * np.random.default_rng([seed, k]).uniform(-1.0, 1.0, it["nabla"].shape))
            _, _, s = orc.optimizer_solve(grad, it["rect"], nabla, it["start"][0], it["start"][1], opts=o)
            assert (s.iterations, s.termination, s.num_evals_cost, s.num_evals_jac) == want[k], (seed, k)


@pytest.mark.gpu
@pytest.mark.parametrize("name", IDS)
def test_device_solve_matches_oracle_under_the_variant(ebo, orc, name):
    grad, items = _batch(orc, N)
    opts = ebo.optimizer_default_solver(**VARIANTS[name])
    c = _ctx(ebo)
    try:
        c.optimizer_set_grad(grad[..., 0], grad[..., 1])
        poses, fds, sums = c.optimizer_solve([it["rect"] for it in items], [it["nabla"] for it in items],
                                             [it["start"][0] for it in items], [it["start"][1] for it in items],
                                             opts=opts)
    finally:
        c.close()
    for i, (po, fo, so) in enumerate(oracle_solves(orc, name)):
        s = sums[i]
        assert (s.iterations, s.termination, s.num_evals_cost, s.num_evals_jac) == so[:4], (i, so)
        assert s.initial_cost == pytest.approx(so[4], rel=1e-11)
        assert s.final_cost == pytest.approx(so[5], rel=1e-7, abs=1e-13)
        d = max(np.abs(poses[i] - po).max(), abs(fds[i] - fo))
        assert d < 1e-5, (i, d)  # the bar for a solved parameter vector
