"""A plain restatement of the per-patch trust-region Levenberg-Marquardt: 2 parameters, 1 residual, float64 scalars.

The rules are those of LmUnit (csrc/ebo_kernels.hip), in its operation order; HostLm (csrc/host_lm.cpp, driven by
lockstep.h) and the oracle's minimize() (oracle/oracle.cpp, mode 1) state the same rules for n parameters.  Every
comparison the solver makes is kept with the two numbers compared, so that a test can read a decision's margin.

The objective is a callable f(m, want_jac) -> (r, J): m the point (2 floats), r the residual, J its two derivatives
(ignored when want_jac is false).  The options are a dict in ebo_solver_opts order (default_opts).

Rules, numbered as the comments below:
  R0  iteration zero: f, J at x = 0.  A non-finite cost ends with termination 2 and all-zero statistics but the one
      Jacobian evaluation.  Jacobi scaling 1 / (1 + sqrt(J^2)) is fixed here for the whole solve.
  R1  loop top: the best point is updated after a successful step; then the exits in this order: iteration cap
      (termination 1), gradient tolerance after a successful step (0), minimum radius (0).
  R2  step: diagonal = clip(j^2, min_lm_diagonal, max_lm_diagonal) unless reused, l = sqrt(d / radius), the 2x2
      Cholesky of j'j + l^2 with its h00 > 0, dd > 0 and finite tests, step = -solution.
  R3  modelCostChange = -mr (f + mr / 2) with mr = j . step; a step is invalid unless it is > 0.
  R4  invalid step: the counter rises, termination 2 at max_consecutive_invalid, else radius halves.
  R5  candidate = x + step * scale; its cost 0.5 r^2, DBL_MAX when not finite.
  R6  parameter tolerance (termination 0), THEN function tolerance (0), both BEFORE the step's quality.
  R7  quality = max(relDec, histDec); accepted when quality > min_relative_decrease.
  R8  accepted: f, J at the candidate; radius / max(1/3, 1 - (2q - 1)^3) clipped to max_radius; the step
      evaluator's bookkeeping (use_nonmonotonic off = max_consecutive_nonmonotonic 0).
  R9  rejected: radius / divisor, the divisor doubles (2, 4, 8, ...), the diagonal is reused."""
import numpy as np

DBL_MAX = float(np.finfo(np.float64).max)

OPT_ORDER = ("max_num_iterations", "use_nonmonotonic", "function_tolerance", "gradient_tolerance",
             "parameter_tolerance", "initial_radius", "max_radius", "min_radius", "min_relative_decrease",
             "min_lm_diagonal", "max_lm_diagonal", "max_consecutive_nonmonotonic", "max_consecutive_invalid",
             "jacobi_scaling")

# trace kinds
ACCEPTED, REJECTED, INVALID, EXIT_STEP_NORM, EXIT_COST_CHANGE = "accepted", "rejected", "invalid", "exit-step-norm", \
    "exit-cost-change"

F = np.float64


def default_opts(lib, **kw):
    """The library's (or the oracle's) default solver options as a dict in ebo_solver_opts order."""
    o = lib.default_solver()
    d = {k: getattr(o, k) for k in OPT_ORDER}
    for k, v in kw.items():
        assert k in d, k
        d[k] = v
    return d


def to_struct(lib, opts, mode=1):
    """The dict as the library's (or the oracle's) ebo_solver_opts, independent mode."""
    return lib.default_solver(mode=mode, **opts)


class Result:
    """best: the returned point; stats: (iterations, evals_cost, evals_jac, termination, initial_cost, final_cost);
    last: the last iterate; trace: one (kind, cost, radius, quality) row per iteration; checks: (step norm, its
    bound, |cost change|, its bound) per candidate; exit_checks: (what, value, bound) per loop-top test;
    qualities: (quality, min_relative_decrease, relDec, histDec) per step that reached R7; candidates: (point,
    residual) of every value-only evaluation; diagonals: (j0^2, j1^2, d0, d1) of every diagonal R2 forms afresh."""

    def __init__(self):
        self.best = (0.0, 0.0)
        self.last = (0.0, 0.0)
        self.stats = (0, 0, 0, 1, 0.0, 0.0)
        self.trace, self.checks, self.exit_checks, self.qualities, self.candidates = [], [], [], [], []
        self.diagonals = []

    @property
    def kinds(self):
        return [t[0] for t in self.trace]

    @property
    def counts(self):
        """(iterations, value evaluations, Jacobian evaluations, termination): what the device reports per patch."""
        return tuple(int(v) for v in self.stats[:4])


def lm(opts):
    """The solver as a generator: yields (m0, m1, want_jac), is sent (r, J0, J1), returns a Result."""
    o = opts
    out = Result()
    max_nonmono = o["max_consecutive_nonmonotonic"] if o["use_nonmonotonic"] else 0
    iteration = evals_cost = evals_jac = 0
    with np.errstate(all="ignore"):
        # R0
        x0 = x1 = F(0.0)
        r, a, b = yield (0.0, 0.0, True)
        f, J0, J1 = F(r), F(a), F(b)
        evals_jac += 1
        x_cost = F(0.5) * f * f
        if not np.isfinite(x_cost):
            out.stats = (0, 0, evals_jac, 2, 0.0, 0.0)
            return out
        initial_cost = x_cost
        g0, g1 = J0 * f, J1 * f
        sc0 = sc1 = F(1.0)
        if o["jacobi_scaling"]:
            sc0 = F(1.0) / (F(1.0) + np.sqrt(J0 * J0))
            sc1 = F(1.0) / (F(1.0) + np.sqrt(J1 * J1))
        j0, j1 = J0 * sc0, J1 * sc1
        x_norm = np.sqrt(x0 * x0 + x1 * x1)
        grad_max = np.fmax(np.abs(g0), np.abs(g1))
        minimum_cost = x_cost
        best0, best1 = x0, x1
        se_min = se_cur = se_ref = se_cand = x_cost
        se_acc_ref = se_acc_cand = F(0.0)
        se_nonmono = 0
        radius = F(o["initial_radius"])
        decrease = F(2.0)
        reuse_diagonal = False
        last_successful = True
        d0 = d1 = F(0.0)
        num_invalid = 0
        termination = 1
        while True:
            # R1
            if last_successful and x_cost < minimum_cost:
                minimum_cost = x_cost
                best0, best1 = x0, x1
            out.exit_checks.append(("iterations", iteration, o["max_num_iterations"]))
            if iteration >= o["max_num_iterations"]:
                termination = 1
                break
            if last_successful:
                out.exit_checks.append(("gradient", float(grad_max), o["gradient_tolerance"]))
                if grad_max <= o["gradient_tolerance"]:
                    termination = 0
                    break
            out.exit_checks.append(("radius", float(radius), o["min_radius"]))
            if radius < o["min_radius"]:
                termination = 0
                break
            iteration += 1
            last_successful = False
            # R2
            if not reuse_diagonal:
                d0 = np.fmin(np.fmax(j0 * j0, F(o["min_lm_diagonal"])), F(o["max_lm_diagonal"]))
                d1 = np.fmin(np.fmax(j1 * j1, F(o["min_lm_diagonal"])), F(o["max_lm_diagonal"]))
                out.diagonals.append((float(j0 * j0), float(j1 * j1), float(d0), float(d1)))
            l0 = np.sqrt(d0 / radius)
            l1 = np.sqrt(d1 / radius)
            reuse_diagonal = True
            h00 = j0 * j0 + l0 * l0
            h10 = j1 * j0
            h11 = j1 * j1 + l1 * l1
            valid = bool(h00 > 0.0) and bool(np.isfinite(h00))
            s0 = s1 = F(0.0)
            if valid:
                L00 = np.sqrt(h00)
                L10 = h10 / L00
                dd = h11 - L10 * L10
                valid = bool(dd > 0.0) and bool(np.isfinite(dd))
                if valid:
                    L11 = np.sqrt(dd)
                    b0 = (j0 * f) / L00
                    b1 = ((j1 * f) - L10 * b0) / L11
                    b1 = b1 / L11
                    b0 = (b0 - L10 * b1) / L00
                    valid = bool(np.isfinite(b0)) and bool(np.isfinite(b1))
                    s0, s1 = -b0, -b1
            # R3
            model_cost_change = F(0.0)
            if valid:
                mr = j0 * s0 + j1 * s1
                model_cost_change = F(0.0) - mr * (f + mr / F(2.0))
                valid = bool(model_cost_change > 0.0)
            if not valid:
                # R4
                num_invalid += 1
                if num_invalid >= o["max_consecutive_invalid"]:
                    out.trace.append((INVALID, float(x_cost), float(radius), 0.0))
                    termination = 2
                    break
                radius = radius * F(0.5)
                reuse_diagonal = True
                out.trace.append((INVALID, float(x_cost), float(radius), 0.0))
                continue
            num_invalid = 0
            # R5
            c0 = x0 + s0 * sc0
            c1 = x1 + s1 * sc1
            r, _, _ = yield (float(c0), float(c1), False)
            evals_cost += 1
            out.candidates.append(((float(c0), float(c1)), float(r)))
            cand_cost = F(0.5) * F(r) * F(r)
            if not np.isfinite(cand_cost):
                cand_cost = F(DBL_MAX)
            # R6
            e0, e1 = x0 - c0, x1 - c1
            step_norm = np.sqrt(e0 * e0 + e1 * e1)
            step_bound = F(o["parameter_tolerance"]) * (x_norm + F(o["parameter_tolerance"]))
            cost_change = x_cost - cand_cost
            cost_bound = F(o["function_tolerance"]) * x_cost
            out.checks.append((float(step_norm), float(step_bound), float(np.abs(cost_change)), float(cost_bound)))
            if step_norm <= step_bound:
                out.trace.append((EXIT_STEP_NORM, float(cand_cost), float(radius), 0.0))
                termination = 0
                break
            if np.abs(cost_change) <= cost_bound:
                out.trace.append((EXIT_COST_CHANGE, float(cand_cost), float(radius), 0.0))
                termination = 0
                break
            # R7
            rel_dec = (se_cur - cand_cost) / model_cost_change
            hist_dec = (se_ref - cand_cost) / (se_acc_ref + model_cost_change)
            quality = np.fmax(rel_dec, hist_dec)
            out.qualities.append((float(quality), o["min_relative_decrease"], float(rel_dec), float(hist_dec)))
            if not (quality > o["min_relative_decrease"]):
                # R9
                radius = radius / decrease
                decrease = decrease * F(2.0)
                reuse_diagonal = True
                out.trace.append((REJECTED, float(cand_cost), float(radius), float(quality)))
                continue
            # R8
            x0, x1 = c0, c1
            x_norm = np.sqrt(x0 * x0 + x1 * x1)
            r, a, b = yield (float(x0), float(x1), True)
            f, J0, J1 = F(r), F(a), F(b)
            evals_jac += 1
            x_cost = F(0.5) * f * f
            if not np.isfinite(x_cost):
                out.trace.append((ACCEPTED, float(x_cost), float(radius), float(quality)))
                termination = 2
                break
            g0, g1 = J0 * f, J1 * f
            j0, j1 = J0 * sc0, J1 * sc1
            grad_max = np.fmax(np.abs(g0), np.abs(g1))
            last_successful = True
            q = F(2.0) * quality - F(1.0)
            radius = radius / np.fmax(F(1.0) / F(3.0), F(1.0) - q * q * q)
            radius = np.fmin(F(o["max_radius"]), radius)
            decrease = F(2.0)
            reuse_diagonal = False
            se_cur = cand_cost
            se_acc_cand = se_acc_cand + model_cost_change
            se_acc_ref = se_acc_ref + model_cost_change
            if se_cur < se_min:
                se_min = se_cur
                se_nonmono = 0
                se_cand = se_cur
                se_acc_cand = F(0.0)
            else:
                se_nonmono += 1
                if se_cur > se_cand:
                    se_cand = se_cur
                    se_acc_cand = F(0.0)
            if se_nonmono == max_nonmono:
                se_ref = se_cand
                se_acc_ref = se_acc_cand
            out.trace.append((ACCEPTED, float(x_cost), float(radius), float(quality)))
        out.best = (float(best0), float(best1))
        out.last = (float(x0), float(x1))
        out.stats = (iteration, evals_cost, evals_jac, termination, float(initial_cost), float(minimum_cost))
        return out


def solve(f, opts):
    """One problem: f(m, want_jac) -> (r, J).  -> Result"""
    g = lm(opts)
    try:
        q = next(g)
        while True:
            r, J = f((q[0], q[1]), q[2])
            q = g.send((r, J[0], J[1]) if q[2] else (r, 0.0, 0.0))
    except StopIteration as e:
        return e.value


def solve_lockstep(batched, n, opts, active=None):
    """n problems advanced in lock step, as lockstep.h drives the host LMs: every round is ONE call
    batched(points [n][2], want_jac [n] bool, live [n] bool) -> (r [n], J [n][2]); a problem that is finished (or
    not active) keeps its last point and is not live.  -> list of Result (None where not active)"""
    active = np.ones(n, bool) if active is None else np.asarray(active, bool)
    gens = [lm(opts) if active[p] else None for p in range(n)]
    out = [None] * n
    want = [None] * n
    points = np.zeros((n, 2))
    for p in range(n):
        if gens[p] is not None:
            want[p] = next(gens[p])
    while any(w is not None for w in want):
        live = np.array([w is not None for w in want])
        jac = np.array([bool(w[2]) if w is not None else False for w in want])
        for p in np.flatnonzero(live):
            points[p] = want[p][:2]
        r, J = batched(points.copy(), jac, live)
        for p in np.flatnonzero(live):
            try:
                want[p] = gens[p].send((float(r[p]), float(J[p][0]), float(J[p][1])) if jac[p]
                                       else (float(r[p]), 0.0, 0.0))
            except StopIteration as e:
                out[p] = e.value
                want[p] = None
    return out


def fold(results):
    """A window's per-patch statistics folded the way ebo_solve and the oracle fold them: max of iterations and
    termination, sums of the evaluation counts and of the costs.  -> (iterations, evals_cost, evals_jac,
    termination, initial_cost, final_cost)"""
    rs = [r for r in results if r is not None]
    if not rs:
        return (0, 0, 0, 0, 0.0, 0.0)
    return (max(r.stats[0] for r in rs), sum(r.stats[1] for r in rs), sum(r.stats[2] for r in rs),
            max(r.stats[3] for r in rs), sum(r.stats[4] for r in rs), sum(r.stats[5] for r in rs))


def fold_counts(stats):
    """The same fold of an [n][4] table of device statistics (inactive rows all zero)."""
    s = np.asarray(stats).reshape(-1, 4)
    return (int(s[:, 0].max()), int(s[:, 1].sum()), int(s[:, 2].sum()), int(s[:, 3].max()))
