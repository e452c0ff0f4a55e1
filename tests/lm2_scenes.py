"""Named scenes for the per-patch LM (LmUnit in csrc/ebo_kernels.hip, HostLm, lockstep.h), each there for one branch
of the state machine.  tests/test_lm2_cpu.py admits them on the CPU (restatement against the oracle's own solver,
the branch read from the trace, no tie patches, stable decisions under perturbed evaluations);
tests/test_gpu_solve_branches.py runs the device on them.  A plain module, not a conftest.

A scene is (window, objective, options, branch, base): `base` names the options the scene's option is put back to,
so that a test can show the option changes the trace.  The windows are eval_cases.py's 61 x 43 geometry (3 x 2
patches with remainder column, row and corner, about 1.5 k events): the smallest shape at which the state machine and
its LDS placement can go wrong."""
import numpy as np

import eval_cases as EC
import lm2_ref as R

# ---- stability amplitudes ------------------------------------------------------------------------------------------
# The largest relative device-to-oracle difference of value and Jacobian that tests/test_gpu_eval_sweep.py's
# test_window_eval_against_the_oracle records (EBO_SWEEP_RECORD: ratio x bar, non-pile cases) on these windows, and 10x
# that, floored at 1e-13: the amplitudes under which every scene must keep its decisions (test_lm2_cpu.py).
# Measured 2026-10-20 on an MI355X at commit 71e5355 (ratio x the relative bar of 1e-9, the largest over the 20 non-pile
# cases): variance value 9.75e-3 x 1e-9 (case sigma=1000.0), variance Jacobian 6.02e-4 x 1e-9 (sigma=1000.0), edge
# value 3.87e-6 x 1e-9 (fd_step=1e-08).  The sweep records no ratio for the edge Jacobian (it counts tie patches: 0 on
# every case), so that figure was measured the same day on the windows of the edge scenes below, at zero flow and at
# each scene's returned and last flows: 3.41e-11 of a patch's larger component (tests/test_gpu_edge_ties.py documents
# 1e-11 on its 100 windows).  On the scene windows themselves the variance differences are far smaller (value 0,
# Jacobian 7.7e-14 at sigma 1, 3.3e-14 at sigma 0.5); the sweep's figures are taken as the rule says.
MEASURED_ON = "2026-10-20, commit 71e5355"
MEASURED_VALUE_REL = {"variance": 9.75e-12, "edge": 3.87e-15}
MEASURED_JACOBIAN_REL = {"variance": 6.02e-13, "edge": 3.41e-11}
E_V = {k: max(10.0 * v, 1e-13) for k, v in MEASURED_VALUE_REL.items()}
E_J = {k: max(10.0 * v, 1e-13) for k, v in MEASURED_JACOBIAN_REL.items()}
STABILITY_SEEDS = tuple(range(8))
STABILITY_FLOW = 1e-6   # a tenth of the 1e-5 bar of a solved parameter
FLOW_BAR = 1e-5

LOSS_ID = {"edge": 0, "variance": 1}  # EBO_LOSS_EDGE, EBO_LOSS_VARIANCE
MIN_EVENTS = 100                      # ebo_default_params: a patch is active with MORE than this many events


# ---- windows -------------------------------------------------------------------------------------------------------
def _case(sigma, seed):
    return EC.Case("lm2", sigma=sigma, seed=seed)


def _single(seed):
    return lambda orc: [EC.window(_case(1.0, seed), orc)]


def _sparse(seed, patch=4, keep=60, strays=5):
    """The window of `seed` with `patch` thinned to `keep` events (below min_events: inactive) and `strays` events
    outside the sensor."""
    def make(orc):
        ev = EC.window(_case(1.0, seed), orc)
        x, y, w, h = EC.grid_rects()[patch]
        inside = np.flatnonzero((ev["x"] >= x) & (ev["x"] < x + w) & (ev["y"] >= y) & (ev["y"] < y + h))
        drop = inside[1:-1][keep - 2:]
        ev = np.delete(ev, drop)
        s = orc.make_events([EC.IMAGE_W + 9] * strays, list(range(strays)), [3000 + 1000 * i for i in range(strays)])
        ev = np.concatenate([ev, s])
        return [ev[np.argsort(ev["t_us"], kind="stable")]]
    return make


WINDOWS = {
    **{"w%d" % i: _single(i) for i in range(16)},
    "pair": lambda orc: [EC.window(_case(1.0, 0), orc), EC.window(_case(1.0, 1), orc)],
    "sparse": _sparse(2),
}
_cache = {}


def windows(name, orc):
    """The list of event arrays (one per window) of a named window set."""
    if name not in _cache:
        _cache[name] = WINDOWS[name](orc)
    return _cache[name]


def in_rect(ev, rect):
    x, y, w, h = rect
    return ev[(ev["x"] >= x) & (ev["x"] < x + w) & (ev["y"] >= y) & (ev["y"] < y + h)]


def patch_events(name, orc):
    """[(window, patch, rect, events of the patch in list order, active)] over every grid patch of the set."""
    out = []
    for w, ev in enumerate(windows(name, orc)):
        for p, rect in enumerate(EC.grid_rects()):
            e = in_rect(ev, rect)
            out.append((w, p, rect, e, len(e) > MIN_EVENTS))
    return out


# ---- objectives ----------------------------------------------------------------------------------------------------
class Objective:
    """A loss and its sigma_compensate: 'variance' at sigma 1.0 and 0.5 are the two k_solve_independent
    instantiations (exp_taps.h's polynomials / the library exp), 'edge' is k_solve_edge."""

    def __init__(self, name, loss, sigma):
        self.name, self.loss, self.sigma = name, loss, sigma
        self.case = _case(sigma, 0)

    def __repr__(self):
        return self.name

    def params(self, lib, **kw):
        p = self.case.params(lib, LOSS_ID[self.loss])
        for k, v in kw.items():
            setattr(p, k, v)
        return p

    def oparams(self, orc):
        return self.case.oparams(orc, LOSS_ID[self.loss])

    def patch_f(self, orc, events, rect, perturb=None, central=None):
        """f(m, want_jac) -> (r, J) of one patch by the oracle's contrastFunctor.  perturb = (rng, e_v, e_J):
        r (1 + e_v u), J (1 + e_J u) with u uniform in [-1, 1] per evaluation.  central = h: the Jacobian is
        EBO_GRAD_CENTRAL's formula (r(m + h e_k) - r(m - h e_k)) / 2h on the oracle's values (each of them perturbed
        on its own), as _fd_jacobian in tests/test_gpu_eval_sweep.py."""
        consts = self.case.consts(orc)
        loss, scale = LOSS_ID[self.loss], self.case.scale

        def value(m):
            r = orc.contrast_eval(events, rect, m, loss, False, scale, consts)[0]
            return r * (1.0 + perturb[1] * perturb[0].uniform(-1.0, 1.0)) if perturb is not None else r

        def f(m, want_jac):
            if central is not None:
                r = value(m)
                if not want_jac:
                    return r, (0.0, 0.0)
                J = np.zeros(2)
                for k in range(2):
                    d = np.zeros(2)
                    d[k] = central
                    J[k] = (value(np.asarray(m) + d) - value(np.asarray(m) - d)) / (2 * central)
                return r, J
            r, J = orc.contrast_eval(events, rect, m, loss, want_jac, scale, consts)
            if perturb is not None:
                rng, e_v, e_j = perturb
                r = r * (1.0 + e_v * rng.uniform(-1.0, 1.0))
                if want_jac:
                    J = J * (1.0 + e_j * rng.uniform(-1.0, 1.0, 2))
            return r, (J if want_jac else (0.0, 0.0))
        return f


OBJECTIVES = {"var1": Objective("var1", "variance", 1.0), "var05": Objective("var05", "variance", 0.5),
              "edge": Objective("edge", "edge", 1.0)}


class Scene:
    def __init__(self, name, window, objective, opts, branch, base=None, where=None, note=""):
        self.name, self.window, self.objective, self.opts = name, window, OBJECTIVES[objective], dict(opts)
        self.branch, self.base, self.where, self.note = branch, (None if base is None else dict(base)), where, note

    def __repr__(self):
        return self.name

    def options(self, lib):
        return R.default_opts(lib, **self.opts)

    def base_options(self, lib):
        return None if self.base is None else R.default_opts(lib, **self.base)


def solve_scene(scene, orc, opts=None, perturb_seed=None, central=None):
    """The restatement on every patch of the scene's windows.  -> list over (window, patch) of Result or None"""
    o = scene.options(orc) if opts is None else opts
    out = []
    for k, (w, p, rect, ev, active) in enumerate(patch_events(scene.window, orc)):
        if not active:
            out.append(None)
            continue
        perturb = None
        if perturb_seed is not None:
            loss = scene.objective.loss
            perturb = (np.random.default_rng([perturb_seed, k]), E_V[loss], E_J[loss])
        out.append(R.solve(scene.objective.patch_f(orc, ev, rect, perturb, central), o))
    return out


def stability(scene, orc, results=None, opts=None, central=None):
    """Re-runs the scene under the seeded perturbations of the objective.  -> (patches whose decision sequence
    (trace kinds and counts) changed under some seed, the largest move of a returned flow)"""
    results = solve_scene(scene, orc, opts, central=central) if results is None else results
    changed, move = set(), 0.0
    for seed in STABILITY_SEEDS:
        again = solve_scene(scene, orc, opts, perturb_seed=seed, central=central)
        for k, (a, b) in enumerate(zip(results, again)):
            if a is None:
                continue
            if a.kinds != b.kinds or a.counts != b.counts:
                changed.add(k)
            move = max(move, abs(a.best[0] - b.best[0]), abs(a.best[1] - b.best[1]))
    return sorted(changed), move


# ---- branch assertions, read from the traces -----------------------------------------------------------------------
# Each takes (scene options, results of the scene, results of its base or None) and returns the (window, patch) slots
# where the branch is taken; a scene is sound when that list is not empty (or is the whole list where noted).
def _rises(r):
    """Indices of the trace rows that are accepted steps whose cost is above the cost before them."""
    out, cur = [], r.stats[4]
    for i, t in enumerate(r.trace):
        if t[0] == R.ACCEPTED:
            if t[1] > cur:
                out.append(i)
            cur = t[1]
    return out


def _first_difference(a, b):
    """First trace row at which two solves differ (kind), or None when one is a prefix of the other."""
    for i, (s, t) in enumerate(zip(a.kinds, b.kinds)):
        if s != t:
            return i
    return None


def _all(results, pred):
    act = [k for k, r in enumerate(results) if r is not None]
    hit = [k for k in act if pred(results[k])]
    return hit if hit == act else []


def _some(results, pred):
    return [k for k, r in enumerate(results) if r is not None and pred(r)]


def _last_exit(r, what):
    e = r.exit_checks[-1]
    return e[0] == what and (e[1] < e[2] if what == "radius" else e[1] <= e[2])


def b_cap0(o, res, base):
    return _all(res, lambda r: r.counts == (0, 0, 1, 1) and r.trace == [] and r.best == (0.0, 0.0))


def b_cap_n(o, res, base):
    n = o["max_num_iterations"]
    hit = _all(res, lambda r: r.counts[0] == n and r.counts[3] == 1 and len(r.trace) == n)
    return hit if any(R.ACCEPTED in res[k].kinds for k in hit) else []


def b_grad0(o, res, base):
    return _all(res, lambda r: r.counts == (0, 0, 1, 0) and _last_exit(r, "gradient"))


def b_grad_after_accept(o, res, base):
    return _some(res, lambda r: r.counts[3] == 0 and r.kinds and r.kinds[-1] == R.ACCEPTED and _last_exit(r, "gradient"))


def b_min_radius(o, res, base):
    return _some(res, lambda r: r.counts[3] == 0 and r.kinds and r.kinds[-1] == R.REJECTED and _last_exit(r, "radius"))


def b_param_tol(o, res, base):
    assert o["function_tolerance"] == 0.0
    return _some(res, lambda r: r.counts[3] == 0 and r.kinds[-1] == R.EXIT_STEP_NORM and r.checks[-1][0] <= r.checks[-1][1])


def b_param_tol_earlier(o, res, base):
    """The larger parameter tolerance ends a patch earlier than the base's smaller one does (and none later)."""
    hit = b_param_tol(o, res, base)
    if any(res[k].counts[0] > base[k].counts[0] for k in hit):
        return []
    return [k for k in hit if res[k].counts[0] < base[k].counts[0] and base[k].kinds[-1] == R.EXIT_STEP_NORM]


def b_func_tol(o, res, base):
    assert o["parameter_tolerance"] == 0.0
    return _some(res, lambda r: r.counts[3] == 0 and r.kinds[-1] == R.EXIT_COST_CHANGE and
                 r.checks[-1][0] > r.checks[-1][1] and r.checks[-1][2] <= r.checks[-1][3])


def b_invalid_n(o, res, base):
    n = o["max_consecutive_invalid"]
    return _all(res, lambda r: r.counts == (n, 0, 1, 2) and r.kinds == [R.INVALID] * n and r.best == (0.0, 0.0))


def b_accept_first(o, res, base):
    return _some(res, lambda r: r.kinds[:1] == [R.ACCEPTED])


def _reject_run(r):
    n = 0
    while n < len(r.kinds) and r.kinds[n] == R.REJECTED:
        n += 1
    return n


def b_reject3_accept(o, res, base):
    """Three or more rejections in a row, the radius divided by 2, 4, 8, ... (exact: powers of two), then an accepted
    step; a rejection after it divides by 2 again (the divisor was reset)."""
    def pred(r):
        n = _reject_run(r)
        if n < 3 or n >= len(r.kinds) or r.kinds[n] != R.ACCEPTED:
            return False
        radius = o["initial_radius"]
        for i in range(n):
            radius /= 2.0 ** (i + 1)
            if r.trace[i][2] != radius:
                return False
        later = [i for i in range(n + 1, len(r.kinds)) if r.kinds[i] == R.REJECTED and r.kinds[i - 1] == R.ACCEPTED]
        return all(r.trace[i][2] == r.trace[i - 1][2] / 2.0 for i in later) and len(r.diagonals) >= 2
    return _some(res, pred)


def wild_candidates(scene, r):
    """Of a solve's rejected candidates before its first accepted step: (those whose residual is above
    max_possible_residual: the penalty branch of the objective; those that are wild without it: a flow that carries
    the window's outer events, half of T_END from the reference time, farther than a patch is wide, so that their box
    is not the patch's any more)."""
    n = _reject_run(r)
    mx = scene.objective.case.max_res
    pen = [i for i in range(n) if r.candidates[i][1] > mx]
    reach = EC.PATCH / (0.5 * EC.T_END * scene.objective.case.scale)
    far = [i for i in range(n) if i not in pen and max(abs(r.candidates[i][0][0]), abs(r.candidates[i][0][1])) > reach]
    return pen, far


def b_wild_then_accept(o, res, base):
    mx = 1e3

    def pred(r):
        n = _reject_run(r)
        return 0 < n < len(r.kinds) and r.kinds[n] == R.ACCEPTED and r.candidates[0][1] > mx and \
            max(abs(r.candidates[0][0][0]), abs(r.candidates[0][0][1])) > EC.IMAGE_W
    return _some(res, pred)


def b_max_radius(o, res, base):
    cap = o["max_radius"]
    hit = _some(res, lambda r: any(t[0] == R.ACCEPTED and t[2] == cap for t in r.trace) and
                all(t[2] <= cap for t in r.trace))
    return [k for k in hit if any(t[2] > cap for t in base[k].trace)]


def b_min_relative_decrease(o, res, base):
    """A decision flips: at the first row where the two solves differ, the base accepts a step of quality in
    (its bar, the scene's bar] that the scene rejects."""
    def flipped(k):
        i = _first_difference(res[k], base[k])
        if i is None or res[k].kinds[i] != R.REJECTED or base[k].kinds[i] != R.ACCEPTED:
            return False
        q = res[k].trace[i][3]
        return q == base[k].trace[i][3] and 0.001 < q <= o["min_relative_decrease"]
    return [k for k, r in enumerate(res) if r is not None and flipped(k)]


def b_nonmonotonic_off(o, res, base):
    """use_nonmonotonic = 0 rejects a cost-raising step that the base (1) accepts, after identical rows."""
    assert o["use_nonmonotonic"] == 0

    def flipped(k):
        i = _first_difference(res[k], base[k])
        return i is not None and res[k].kinds[i] == R.REJECTED and i in _rises(base[k]) and \
            res[k].trace[:i] == base[k].trace[:i] and not _rises(res[k])
    return [k for k, r in enumerate(res) if r is not None and flipped(k)]


def b_nonmonotonic_on(o, res, base):
    """use_nonmonotonic = 1 accepts a step whose cost rises; the base (0) rejects the same step."""
    assert o["use_nonmonotonic"] == 1
    return b_nonmonotonic_off(dict(o, use_nonmonotonic=0), base, res)


def b_parts_from_base(o, res, base):
    """The decision sequences of scene and base part on these patches."""
    return [k for k, r in enumerate(res) if r is not None and _first_difference(r, base[k]) is not None]


def b_moves_from_base(o, res, base):
    """Same decisions or not, the traces (costs, radii) of scene and base differ on these patches."""
    return [k for k, r in enumerate(res) if r is not None and r.trace != base[k].trace]


def b_cut_after_rise(o, res, base):
    """The cap falls right after a cost-raising accepted step: the returned point is the minimum, not the last."""
    def pred(r):
        return r.counts[3] == 1 and r.kinds[-1] == R.ACCEPTED and (len(r.trace) - 1) in _rises(r) and \
            r.best != r.last and r.stats[5] < r.trace[-1][1] and r.stats[5] == min(
                [r.stats[4]] + [t[1] for t in r.trace if t[0] == R.ACCEPTED])
    return _some(res, pred)


def b_diagonal_clips(o, res, base):
    """min_lm_diagonal = max_lm_diagonal: a diagonal raised to the value and one lowered to it, and a trace that
    differs from the base's."""
    v = o["min_lm_diagonal"]
    assert v == o["max_lm_diagonal"]
    ds = [d for r in res if r is not None for d in r.diagonals]
    if not (all(d[2] == v and d[3] == v for d in ds) and any(min(d[:2]) < v for d in ds) and any(max(d[:2]) > v for d in ds)):
        return []
    return b_moves_from_base(o, res, base)


BRANCHES = {f.__name__[2:]: f for f in (
    b_cap0, b_cap_n, b_grad0, b_grad_after_accept, b_min_radius, b_param_tol, b_param_tol_earlier, b_func_tol, b_invalid_n,
    b_accept_first, b_reject3_accept, b_wild_then_accept, b_max_radius, b_min_relative_decrease, b_nonmonotonic_off,
    b_nonmonotonic_on, b_parts_from_base, b_moves_from_base, b_cut_after_rise, b_diagonal_clips)}


def branch_patches(scene, orc, results, base_results):
    return BRANCHES[scene.branch](scene.options(orc), results, base_results)


# ---- the scenes ----------------------------------------------------------------------------------------------------
# Windows and caps were chosen by tests/test_lm2_cpu.py's admission (another seed or a smaller max_num_iterations until
# every patch keeps its decisions under the perturbed evaluations and moves its flows by <= STABILITY_FLOW).  The
# variance loss at sigma 1 admits few accepted steps: its residual is max_possible_residual - variance with the
# variance four orders below the residual, so E_V relative to the residual is 1e-6 of what the solver works with.
WINDOWS["pair_e"] = lambda orc: [EC.window(_case(1.0, 0), orc), EC.window(_case(1.0, 2), orc)]
WINDOWS["pair_v"] = lambda orc: [EC.window(_case(1.0, 1), orc), EC.window(_case(1.0, 4), orc)]
WINDOWS_COUNT = {k: ([0, 1] if k.startswith("pair") else [0]) for k in WINDOWS}

SMALL = dict(initial_radius=1e-6)  # accepted steps from iteration 1 on: at the default 1e4 the first eight steps are wild
TINY = dict(initial_radius=1e-320, min_radius=0.0)  # d / radius overflows: the Cholesky's finite test fails


def _scenes():
    out = []

    def add(name, window, objective, opts, branch, base=None, note=""):
        out.append(Scene("%s-%s" % (name, objective), window, objective, opts, branch, base, note=note))

    for obj in ("var1", "var05", "edge"):
        # exits
        add("cap0", "w0", obj, dict(max_num_iterations=0), "cap0", {})
        add("grad0", "w0", obj, dict(gradient_tolerance=1e9), "grad0", {})
        add("min_radius", "w0", obj, dict(min_radius=1.0), "min_radius", {})
        add("param_tol", "w0", obj, dict(parameter_tolerance=0.3, function_tolerance=0.0), "param_tol",
            dict(function_tolerance=0.0))
        add("param_tol_larger", "w0", obj, dict(parameter_tolerance=3.0, function_tolerance=0.0), "param_tol_earlier",
            dict(parameter_tolerance=0.3, function_tolerance=0.0))
        add("func_tol", "w0", obj, dict(SMALL, function_tolerance=1e-6, parameter_tolerance=0.0), "func_tol",
            dict(SMALL, parameter_tolerance=0.0))
        add("func_tol_wild", "w0", obj, dict(function_tolerance=1e-3, parameter_tolerance=0.0), "func_tol",
            dict(parameter_tolerance=0.0), note="ends on a wild candidate below the penalty branch")
        add("invalid5", "w0", obj, dict(TINY), "invalid_n", dict(min_radius=0.0))
        add("invalid1", "w0", obj, dict(TINY, max_consecutive_invalid=1), "invalid_n", dict(TINY))

    def capped(name, window, obj, cap, opts, branch, base=None, note=""):
        """A scene cut at `cap` iterations; its base is cut there too (but keeps a cap of its own)."""
        add(name, window, obj, dict(opts, max_num_iterations=cap), branch,
            None if base is None else dict(dict(max_num_iterations=cap), **base), note)

    at_zero = dict(SMALL, max_num_iterations=0)  # base of the scenes about the cap n itself: the cheapest other cap
    for obj, window, cap in (("var1", "w2", 4), ("var05", "w1", 7), ("edge", "w0", 7)):
        capped("cap_n", window, obj, cap, SMALL, "cap_n", at_zero)
    for obj, window, cap, g in (("var1", "w0", 5, 15.0), ("var05", "w0", 5, 60.0), ("edge", "w6", 5, 3.5)):
        capped("grad_after_accept", window, obj, cap, dict(SMALL, gradient_tolerance=g), "grad_after_accept", SMALL)
    for obj, window, cap in (("var1", "w2", 4), ("edge", "w6", 6)):
        capped("accept_first", window, obj, cap, SMALL, "accept_first", {})
    for obj, window in (("var1", "w1"), ("var05", "w6"), ("edge", "w11")):
        capped("reject3_accept", window, obj, 11, {}, "reject3_accept", SMALL)
    for obj, window in (("var1", "w4"), ("var05", "w0"), ("edge", "w0")):
        capped("wild_then_accept", window, obj, 11, {}, "wild_then_accept", SMALL,
               note="the rejected wild candidates are what invalidates the kernels' image-reuse record")
    for obj, window, cap in (("var1", "w8", 6), ("var05", "w4", 7), ("edge", "w7", 5)):
        capped("max_radius", window, obj, cap, dict(SMALL, max_radius=1e-6), "max_radius", SMALL)
    for obj, window, cap in (("var1", "w3", 6), ("var05", "w0", 7), ("edge", "w0", 7)):
        capped("min_relative_decrease", window, obj, cap, dict(SMALL, min_relative_decrease=0.5),
               "min_relative_decrease", SMALL)
    for obj, window, cap in (("var05", "w9", 7), ("edge", "w10", 7)):
        capped("nonmonotonic_off", window, obj, cap, dict(SMALL, use_nonmonotonic=0), "nonmonotonic_off", SMALL)
    for obj, window, cap in (("var05", "w9", 7), ("edge", "w0", 7)):
        capped("nonmonotonic_on", window, obj, cap, SMALL, "nonmonotonic_on", dict(SMALL, use_nonmonotonic=0))
    capped("nonmonotonic_2", "w0", "edge", 8, dict(SMALL, max_consecutive_nonmonotonic=2), "parts_from_base", SMALL)
    for obj, window, cap in (("var1", "w2", 6), ("var05", "w4", 8), ("edge", "w11", 8)):
        capped("nonmonotonic_1", window, obj, cap, dict(SMALL, max_consecutive_nonmonotonic=1), "parts_from_base", SMALL)
    for obj, window, cap in (("var1", "w2", 4), ("var05", "w4", 7), ("edge", "w0", 6)):
        capped("cut_after_rise", window, obj, cap, SMALL, "cut_after_rise", None)
    for obj, window, cap in (("var1", "w2", 6), ("var05", "w1", 7), ("edge", "w0", 7)):
        capped("jacobi_scaling_off", window, obj, cap, dict(SMALL, jacobi_scaling=0), "moves_from_base", SMALL)
    for obj, window, cap, v in (("var1", "w11", 3, 3e-4), ("var05", "w2", 7, 3e-4), ("edge", "w0", 7, 1e-4)):
        capped("diagonal_clips", window, obj, cap, dict(SMALL, min_lm_diagonal=v, max_lm_diagonal=v), "diagonal_clips", SMALL)
    # the 2-window batches and the window with a patch below min_events and stray events
    capped("batch", "pair_e", "edge", 7, SMALL, "cap_n", at_zero)
    capped("batch", "pair_v", "var05", 7, SMALL, "cap_n", at_zero)
    capped("sparse", "sparse", "var1", 4, SMALL, "cap_n", at_zero)
    capped("sparse", "sparse", "edge", 7, SMALL, "cap_n", at_zero)
    return out


SCENES = _scenes()
SCENE_IDS = [s.name for s in SCENES]
assert len(set(SCENE_IDS)) == len(SCENE_IDS)

# The variance scenes that the host path takes with grad = EBO_GRAD_CENTRAL (tests/test_gpu_solve_branches.py): those
# whose decisions also stand when the Jacobian is a central difference of perturbed values (admitted by
# tests/test_lm2_cpu.py).  A Jacobian from values that carry E_V is good to E_V |r| / (h |J|), about 1e-3 at
# h = CENTRAL_STEP: no scene with an accepted step keeps its decisions under it.
CENTRAL_STEP = 1e-3
CENTRAL_SCENES = tuple("%s-%s" % (n, o) for o in ("var1", "var05") for n in (
    "cap0", "grad0", "min_radius", "param_tol_larger", "func_tol_wild", "invalid5", "invalid1"))

# Branches that no scene reaches, with the reason (DESIGN.md repeats them)
UNREACHABLE = {
    "non-finite initial cost": "every solve starts at zero flow, where the objective is finite for any event list",
    "non-finite candidate cost": "the penalty branch grows as |flow|^2, so 0.5 r^2 overflows only for a step beyond "
                                 "1e77; steps grow with the radius, and from a radius of 2^53 on the damping d / radius "
                                 "is lost against j^2 in rounding: the noise regime of the next entry",
    "recovery after an invalid step": "a step is invalid here only when d / radius overflows (every halving makes it "
                                      "worse) or when the damping vanishes (initial_radius = inf, min_lm_diagonal = "
                                      "max_lm_diagonal = 0): then dd = j1^2 - L10^2 is pure rounding noise and a "
                                      "perturbation of 1e-11 turns an invalid step into a valid one and back, so no such "
                                      "scene keeps its decisions (inadmissible by the stability rule)",
}
