"""numpy restatement of the relative-pose refinement rules of include/ebo.h (R1-R8), on top of twoview_ref.py, and the
scenes the tests solve.

One float64 operation per numpy operation, in the association the rules state; vectorised only across the listed
inliers, never inside a stated sum.  A quantity with a derivative slot is a Dual; every operation on Duals is one of the
formulas of R4, one statement per rounding.  `reverse_sums=True` takes every stated sum in descending order: the
(inlier, row) products of R6 and R8 are reversed before they are dealt to the 64 partials and each partial adds from
its last entry; the folds of the tree, the factorisation and the two triangular solves are the algorithm, not a sum's
order, and stay; so do dot and the five-term mr_k.
"""
import numpy as np

import twoview_ref as T

LANES = 64
MIN_INLIERS = 5
DBL_MAX = 1.7976931348623157e308


def default_opts(**over):
    """ebo_default_ba_opts."""
    o = dict(max_num_iterations=50, use_nonmonotonic=0, function_tolerance=1e-6, gradient_tolerance=1e-10,
             parameter_tolerance=1e-8, initial_radius=1e4, max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3,
             min_lm_diagonal=1e-6, max_lm_diagonal=1e32, max_consecutive_nonmonotonic=5, max_consecutive_invalid=5,
             jacobi_scaling=1)
    o.update(over)
    return o


OPT_ORDER = ("max_num_iterations", "use_nonmonotonic", "function_tolerance", "gradient_tolerance", "parameter_tolerance",
             "initial_radius", "max_radius", "min_radius", "min_relative_decrease", "min_lm_diagonal", "max_lm_diagonal",
             "max_consecutive_nonmonotonic", "max_consecutive_invalid", "jacobi_scaling")


def finite(v):
    return bool(v >= -DBL_MAX and v <= DBL_MAX)


# ---- R4: a value and one derivative slot ---------------------------------------------------------------------------
class Dual:
    __slots__ = ("v", "d")

    def __init__(self, v, d):
        self.v = v
        self.d = d


def add(x, y):
    return Dual(x.v + y.v, x.d + y.d)


def sub(x, y):
    return Dual(x.v - y.v, x.d - y.d)


def neg(x):
    return Dual(-x.v, -x.d)


def mul(x, y):
    v = x.v * y.v
    a = x.v * y.d
    b = y.v * x.d
    return Dual(v, a + b)


def mulc(c, x):
    return Dual(c * x.v, c * x.d)


def div(x, y):
    c = x.v / y.v
    a = c * y.d
    b = x.d - a
    return Dual(c, b / y.v)


def divc(x, c):
    return Dual(x.v / c, x.d / c)


def root(x):
    s = np.sqrt(x.v)
    t = 2.0 * s
    return Dual(s, x.d / t)


def dot(a, b):
    return add(add(mul(a[0], b[0]), mul(a[1], b[1])), mul(a[2], b[2]))


def dotc(a, c):
    return add(add(mulc(c[0], a[0]), mulc(c[1], a[1])), mulc(c[2], a[2]))


def chords(M, dM, f1, f2):
    """R3 and one slot of R4: M, dM (12,) model and seed (complex allowed), f1 f2 (m, 3) -> c (m, 6), c.d (m, 6)."""
    z = np.zeros(len(f1), dtype=np.result_type(M.dtype, dM.dtype))
    R = [[Dual(M[4 * i + j] + z, dM[4 * i + j] + z) for j in range(3)] for i in range(3)]
    t = [Dual(M[4 * i + 3] + z, dM[4 * i + 3] + z) for i in range(3)]
    f1 = [f1[:, 0], f1[:, 1], f1[:, 2]]
    f2 = [f2[:, 0], f2[:, 1], f2[:, 2]]
    with np.errstate(all="ignore"):
        g = [dotc(R[i], f2) for i in range(3)]
        b0 = dotc(t, f1)
        b1 = dot(t, g)
        a00 = (f1[0] * f1[0] + f1[1] * f1[1]) + f1[2] * f1[2]
        fg = dotc(g, f1)
        a01 = neg(fg)
        a10 = fg
        a11 = neg(dot(g, g))
        det = sub(mulc(a00, a11), mul(a01, a10))
        l0 = div(sub(mul(a11, b0), mul(a01, b1)), det)
        l1 = div(sub(mulc(a00, b1), mul(a10, b0)), det)
        p = []
        for i in range(3):
            x = mulc(f1[i], l0)
            y = mul(l1, g[i])
            w = add(x, add(t[i], y))
            p.append(divc(w, 2.0))
        n1 = root(dot(p, p))
        d = [sub(p[i], t[i]) for i in range(3)]
        q = [add(add(mul(R[0][j], d[0]), mul(R[1][j], d[1])), mul(R[2][j], d[2])) for j in range(3)]
        n2 = root(dot(q, q))
        c, dc = [], []
        for i in range(3):
            r1 = div(p[i], n1)
            c.append(f1[i] - r1.v)
            dc.append(-r1.d)
        for i in range(3):
            r2 = div(q[i], n2)
            c.append(f2[i] - r2.v)
            dc.append(-r2.d)
    return np.stack(c, axis=1), np.stack(dc, axis=1)


def basis(M):
    """R2 at the model M (12,)."""
    t = np.array([M[3], M[7], M[11]])
    k, least = 0, abs(t[0])
    if abs(t[1]) < least:
        k, least = 1, abs(t[1])
    if abs(t[2]) < least:
        k = 2
    w = [np.array([0.0, t[2], -t[1]]), np.array([-t[2], 0.0, t[0]]), np.array([t[1], -t[0], 0.0])][k]
    n = np.sqrt((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2])
    e1 = w / n
    e2 = np.array([t[1] * e1[2] - t[2] * e1[1], t[2] * e1[0] - t[0] * e1[2], t[0] * e1[1] - t[1] * e1[0]])
    return e1, e2


def seed(M, e1, e2, s):
    """R4: the seed of variable s."""
    dM = np.zeros(12, dtype=M.dtype)
    for i in range(3):
        r0, r1, r2 = M[4 * i], M[4 * i + 1], M[4 * i + 2]
        if s == 0:
            dM[4 * i + 3] = e1[i]
        elif s == 1:
            dM[4 * i + 3] = e2[i]
        elif s == 2:
            dM[4 * i + 1], dM[4 * i + 2] = r2, -r1
        elif s == 3:
            dM[4 * i], dM[4 * i + 2] = -r2, r0
        else:
            dM[4 * i], dM[4 * i + 1] = r1, -r0
    return dM


def retract(M, e1, e2, s):
    """R5: s the step already multiplied by the scales (complex allowed)."""
    a, b = s[0], s[1]
    nt = np.sqrt(1.0 + (a * a + b * b))
    hx, hy, hz = s[2] * 0.5, s[3] * 0.5, s[4] * 0.5
    n = np.sqrt(1.0 + ((hx * hx + hy * hy) + hz * hz))
    x, y, z, w = hx / n, hy / n, hz / n, 1.0 / n
    x2, y2, z2 = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = x2 * w, y2 * w, z2 * w
    txx, txy, txz = x2 * x, y2 * x, z2 * x
    tyy, tyz, tzz = y2 * y, z2 * y, z2 * z
    C = [[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx],
         [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]
    out = np.zeros(12, dtype=np.result_type(M.dtype, np.asarray(s).dtype))
    for i in range(3):
        for j in range(3):
            out[4 * i + j] = (M[4 * i] * C[0][j] + M[4 * i + 1] * C[1][j]) + M[4 * i + 2] * C[2][j]
        out[4 * i + 3] = (M[4 * i + 3] + (a * e1[i] + b * e2[i])) / nt
    return out


def tree64(v, rev=False):
    """R6: v (m, rows): the products of inlier i's rows, dealt to partial i mod 64, rows in order."""
    v = np.asarray(v, dtype=np.float64)
    m, rows = v.shape
    chunks = max((m + LANES - 1) // LANES, 1)
    pad = np.zeros((chunks * LANES, rows))
    pad[:m] = v[::-1] if rev else v
    pad = pad.reshape(chunks, LANES, rows)
    acc = np.zeros(LANES)
    with np.errstate(all="ignore"):
        for r in (range(chunks - 1, -1, -1) if rev else range(chunks)):
            for k in (range(rows - 1, -1, -1) if rev else range(rows)):
                acc = acc + pad[r, :, k]
        s = LANES // 2
        while s:
            acc[:s] = acc[:s] + acc[s:2 * s]
            s //= 2
    return acc[0]


def norm12(a, b=None, rev=False):
    d = a if b is None else a - b
    with np.errstate(all="ignore"):
        return np.sqrt(tree64((d * d).reshape(12, 1), rev))


class Solver:
    """One pair: model (3, 4), f1 f2 (n, 3), idx the listed inliers."""

    def __init__(self, model, f1, f2, idx, opts=None, reverse_sums=False):
        self.o = opts or default_opts()
        self.rev = bool(reverse_sums)
        self.model0 = np.array(model, np.float64).reshape(12)
        self.f1 = np.asarray(f1, np.float64).reshape(-1, 3)
        self.f2 = np.asarray(f2, np.float64).reshape(-1, 3)
        self.idx = np.asarray(idx, np.int64).reshape(-1)
        self.scale = np.ones(5)
        # what the guard of tests/test_relpose_refine_cpu.py looks at
        self.qualities, self.checks, self.exit_checks, self.failed_pivots = [], [], [], []

    def eval_jac(self, M):
        a1, a2 = self.f1[self.idx], self.f2[self.idx]
        self.e1, self.e2 = basis(M)
        J = np.zeros((len(self.idx), 6, 5))
        for s in range(5):
            c, dc = chords(M, seed(M, self.e1, self.e2, s), a1, a2)
            with np.errstate(all="ignore"):
                J[:, :, s] = dc * self.scale[s]
        self.J, self.c = J, c
        with np.errstate(all="ignore"):
            self.H = np.zeros((5, 5))
            for a in range(5):
                for b in range(a + 1):
                    self.H[a, b] = self.H[b, a] = tree64(J[:, :, a] * J[:, :, b], self.rev)
            self.g = np.array([tree64(J[:, :, a] * c, self.rev) for a in range(5)])
            return 0.5 * tree64(c * c, self.rev)

    def cost_at(self, M):
        c, _ = chords(M, np.zeros(12), self.f1[self.idx], self.f2[self.idx])
        with np.errstate(all="ignore"):
            return 0.5 * tree64(c * c, self.rev)

    def grad_max(self):
        gm = 0.0
        with np.errstate(all="ignore"):
            for a in range(5):
                v = abs(self.g[a] / self.scale[a])
                gm = v if v > gm else gm
        return gm

    def damp(self, d, radius):
        o = self.o
        d = d if d > o["min_lm_diagonal"] else o["min_lm_diagonal"]
        d = d if d < o["max_lm_diagonal"] else o["max_lm_diagonal"]
        l = np.sqrt(np.float64(d) / radius)
        return l * l

    def damped(self, radius):
        S = self.H.copy()
        for a in range(5):
            S[a, a] = S[a, a] + self.damp(S[a, a], radius)
        return S

    def compute_step(self, radius):
        """R7; None for an invalid step."""
        with np.errstate(all="ignore"):
            L = self.damped(radius)
            for k in range(5):
                d = L[k, k]
                if not (d > 0.0 and finite(d)):
                    self.failed_pivots.append(float(d))
                    return None
                L[k, k] = np.sqrt(d)
                L[k + 1:, k] = L[k + 1:, k] / L[k, k]
                L[k + 1:, k + 1:] = L[k + 1:, k + 1:] - L[k + 1:, k, None] * L[None, k + 1:, k]
            vec = self.g.copy()
            sol = np.zeros(5)
            for k in range(5):
                y = vec[k] / L[k, k]
                vec[k + 1:] = vec[k + 1:] - L[k + 1:, k] * y
                sol[k] = y
            x = np.zeros(5)
            for k in range(4, -1, -1):
                xk = sol[k] / L[k, k]
                sol[:k] = sol[:k] - L[k, :k] * xk
                x[k] = xk
            step = -x
        return step if np.isfinite(step).all() else None

    def model_cost_change(self, step):
        J = self.J
        with np.errstate(all="ignore"):
            mr = J[:, :, 0] * step[0] + J[:, :, 1] * step[1]
            mr = mr + J[:, :, 2] * step[2]
            mr = mr + J[:, :, 3] * step[3]
            mr = mr + J[:, :, 4] * step[4]
            return -tree64(mr * (self.c + mr / 2.0), self.rev)

    def solve(self):
        o = self.o
        max_it = o["max_num_iterations"]
        trace = np.zeros((max_it + 1, 4))
        st = dict(iterations=0, num_evals_cost=0, num_evals_jac=0, termination=1, initial_cost=0.0, final_cost=0.0)
        state = dict(best=self.model0.copy(), last=self.model0.copy())

        def done(term):
            st["termination"] = term
            return dict(model=state["best"].reshape(3, 4), summary=st, trace=trace, last_model=state["last"].reshape(3, 4))

        # R1
        if len(self.idx) < MIN_INLIERS:
            return done(1)
        with np.errstate(all="ignore"):
            tn = np.sqrt((self.model0[3] * self.model0[3] + self.model0[7] * self.model0[7]) + self.model0[11] * self.model0[11])
        ok = np.isfinite(self.model0).all() and np.isfinite(self.f1).all() and np.isfinite(self.f2).all()
        ok = ok and bool(((self.idx >= 0) & (self.idx < len(self.f1))).all()) and tn > 0.0 and finite(tn)
        if not ok:
            return done(2)
        x = self.model0.copy()
        x[3], x[7], x[11] = x[3] / tn, x[7] / tn, x[11] / tn
        state["last"] = x
        radius, decrease = o["initial_radius"], 2.0
        max_nonmono = o["max_consecutive_nonmonotonic"] if o["use_nonmonotonic"] else 0
        x_cost = self.eval_jac(x)
        st["num_evals_jac"] = 1
        st["initial_cost"] = st["final_cost"] = min_cost = x_cost
        trace[0] = (x_cost, radius, 0.0, 1.0)
        if not finite(x_cost):
            return done(2)
        state["best"] = x.copy()
        if o["jacobi_scaling"]:
            with np.errstate(all="ignore"):
                self.scale = 1.0 / (1.0 + np.sqrt(np.diag(self.H).copy()))
            x_cost = self.eval_jac(x)
        grad_max = self.grad_max()
        x_norm = norm12(x, None, self.rev)
        se_min = se_cur = se_ref = se_cand = x_cost
        se_acc_ref = se_acc_cand = 0.0
        se_nonmono = 0
        num_invalid = 0
        last_successful = True
        while True:
            if last_successful and x_cost < min_cost:
                min_cost = x_cost
                st["final_cost"] = min_cost
                state["best"] = x.copy()
            if st["iterations"] >= max_it:
                return done(1)
            if last_successful:
                self.exit_checks.append((grad_max, o["gradient_tolerance"]))
            if last_successful and grad_max <= o["gradient_tolerance"]:
                return done(0)
            self.exit_checks.append((radius, o["min_radius"]))
            if radius < o["min_radius"]:
                return done(0)
            st["iterations"] += 1
            it = st["iterations"]
            last_successful = False
            step = self.compute_step(radius)
            mcc = None
            if step is not None:
                mcc = self.model_cost_change(step)
                if not (mcc > 0.0):
                    step = None
            if step is None:
                num_invalid += 1
                radius = radius * 0.5
                trace[it] = (x_cost, radius, 0.0, -1.0)
                if num_invalid >= o["max_consecutive_invalid"]:
                    return done(2)
                continue
            num_invalid = 0
            with np.errstate(all="ignore"):
                cand = retract(x, self.e1, self.e2, step * self.scale)
            st["num_evals_cost"] += 1
            cand_cost = self.cost_at(cand)
            if not finite(cand_cost):
                cand_cost = DBL_MAX
            step_norm = norm12(x, cand, self.rev)
            self.checks.append((step_norm, o["parameter_tolerance"] * (x_norm + o["parameter_tolerance"]),
                                abs(x_cost - cand_cost), o["function_tolerance"] * x_cost))
            if step_norm <= o["parameter_tolerance"] * (x_norm + o["parameter_tolerance"]) or \
                    abs(x_cost - cand_cost) <= o["function_tolerance"] * x_cost:
                trace[it] = (cand_cost, radius, 0.0, 2.0)
                return done(0)
            with np.errstate(all="ignore"):
                rel = (se_cur - cand_cost) / mcc
                hist = (se_ref - cand_cost) / (se_acc_ref + mcc)
            quality = rel if rel > hist else hist
            self.qualities.append(quality)
            accepted = quality > o["min_relative_decrease"]
            if accepted:
                q = 2.0 * quality - 1.0
                den = 1.0 - (q * q) * q
                radius = radius / (den if den > 1.0 / 3.0 else 1.0 / 3.0)
                radius = radius if radius < o["max_radius"] else o["max_radius"]
                decrease = 2.0
                se_cur = cand_cost
                se_acc_cand = se_acc_cand + mcc
                se_acc_ref = se_acc_ref + mcc
                if se_cur < se_min:
                    se_min = se_cur
                    se_nonmono = 0
                    se_cand = se_cur
                    se_acc_cand = 0.0
                else:
                    se_nonmono += 1
                    if se_cur > se_cand:
                        se_cand = se_cur
                        se_acc_cand = 0.0
                if se_nonmono == max_nonmono:
                    se_ref = se_cand
                    se_acc_ref = se_acc_cand
            else:
                radius = radius / decrease
                decrease = decrease * 2.0
            trace[it] = (cand_cost, radius, quality, 1.0 if accepted else 0.0)
            if not accepted:
                continue
            x = cand
            state["last"] = x
            x_norm = norm12(x, None, self.rev)
            x_cost = self.eval_jac(x)
            grad_max = self.grad_max()
            st["num_evals_jac"] += 1
            last_successful = True
            if not finite(x_cost):
                return done(2)


def solve(pair, opts=None, reverse_sums=False):
    """pair: dict(model, f1, f2, idx).  -> dict(model, summary, trace, last_model, solver)."""
    s = Solver(pair["model"], pair["f1"], pair["f2"], pair["idx"], opts, reverse_sums)
    out = s.solve()
    out["solver"] = s
    return out


def difference(a, b):
    """Largest |a - b| / max(1, |b|) over two equal-shaped sets of doubles."""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    if len(a) == 0:
        return 0.0
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(all="ignore"):
        d = np.where(both_nan | (a == b), 0.0, np.abs(a - b) / np.maximum(1.0, np.abs(b)))
    return float(np.nan_to_num(d, nan=np.inf).max())


def result_difference(x, y):
    return max(difference(x["model"], y["model"]), difference(x["trace"], y["trace"]),
               difference(x["summary"]["final_cost"], y["summary"]["final_cost"]),
               difference(x["summary"]["initial_cost"], y["summary"]["initial_cost"]))


def write_problem(path, pairs, opts):
    """The problem file of tools/relpose_refine_serial.cpp for a list of pairs under one set of options."""
    off = np.concatenate([[0], np.cumsum([len(p["f1"]) for p in pairs])]).astype(float)
    cnt = np.array([len(p["idx"]) for p in pairs], float)
    idx = np.zeros(int(off[-1]))
    for k, p in enumerate(pairs):
        idx[int(off[k]):int(off[k]) + len(p["idx"])] = p["idx"]
    cat = lambda key, w: np.concatenate([np.asarray(p[key], float).reshape(-1, w) for p in pairs]).reshape(-1) if pairs else np.zeros(0)
    np.concatenate([np.array([len(pairs)] + [opts[k] for k in OPT_ORDER], float), off, cnt, cat("model", 12), cat("f1", 3), cat("f2", 3),
                    idx]).tofile(str(path))


def read_result(path, n_pairs, opts):
    """-> list of dict(model, summary, trace) from the serial build's result file."""
    raw = np.fromfile(str(path))
    rows = opts["max_num_iterations"] + 1
    assert len(raw) == n_pairs * (18 + 4 * rows), (len(raw), n_pairs, rows)
    out = []
    for p in range(n_pairs):
        h = raw[18 * p:18 * p + 18]
        summ = dict(iterations=int(h[0]), num_evals_cost=int(h[1]), num_evals_jac=int(h[2]), termination=int(h[3]),
                    initial_cost=h[4], final_cost=h[5])
        out.append(dict(model=h[6:18].reshape(3, 4).copy(), summary=summ,
                        trace=raw[18 * n_pairs + 4 * rows * p:18 * n_pairs + 4 * rows * (p + 1)].reshape(rows, 4).copy()))
    return out


# ---- scenes --------------------------------------------------------------------------------------------------------
def perturbed(model, seed, rot=0.01, trans=0.05, length=1.0):
    """The true model moved by a seeded rotation of `rot` rad and its direction by about `trans`, t of `length`."""
    rng = np.random.default_rng(seed)
    R = model[:, :3] @ T.rotation_about(rng.normal(size=3), rot)
    t = model[:, 3] / np.linalg.norm(model[:, 3]) + rng.normal(size=3) * trans
    out = np.zeros((3, 4))
    out[:, :3] = R
    out[:, 3] = t / np.linalg.norm(t) * length
    return out


def clean_pair(seed, m, n=None, noise_px=0.3, rot=0.01, trans=0.05, length=1.0, baseline=0.3, order="ascending"):
    """A pair of n correspondences without outliers whose list names m of them, from a perturbed true model.
    order: "ascending" = the first m; "shuffled" = a seeded choice in no order that ends on the pair's last index."""
    n = m if n is None else n
    sc = T.make_scene(seed, max(n, 1), outliers=0.0, noise_px=noise_px, baseline=baseline)
    if order == "ascending":
        idx = np.arange(m, dtype=np.int32)
    else:
        rng = np.random.default_rng(seed + 500)
        idx = rng.permutation(n - 1)[:m - 1].astype(np.int32)
        idx = np.concatenate([idx, [n - 1]]).astype(np.int32)
    return dict(model=perturbed(sc["model"], seed + 900, rot, trans, length), f1=sc["f1"][:n], f2=sc["f2"][:n], idx=idx, truth=sc["model"])


def ransac_pair(i):
    """Scene i of twoview_ref.SCENES with RANSAC seed 7: the restatement's own RANSAC model and inliers."""
    sc = T.scene(i)
    r = T.ransac(sc["f1"], sc["f2"], seed=T.RANSAC_SEED)
    return dict(model=r["model"], f1=sc["f1"], f2=sc["f2"], idx=r["inliers"], truth=sc["model"])


SIZES = (5, 63, 64, 65, 129, 300)


def nan_pair():
    p = clean_pair(31, 40)
    p["f2"] = p["f2"].copy()
    p["f2"][17, 1] = np.nan
    return p


def test_scenes():
    """name -> (pair, opts): the scenes of tests/test_gpu_relpose_refine.py (the table in its header)."""
    d = default_opts
    out = {"m0": (clean_pair(10, 0, n=20), d()), "m4": (clean_pair(11, 4, n=20), d())}
    for k, m in enumerate(SIZES):
        out["m%d" % m] = (clean_pair(20 + k, m), d())
    out["m4096"] = (clean_pair(27, 4096), d())
    out["shuffled"] = (clean_pair(28, 90, n=140, order="shuffled"), d())
    out["it0"] = (clean_pair(22, 64), d(max_num_iterations=0))
    out["it1"] = (clean_pair(22, 64), d(max_num_iterations=1))
    out["long_t"] = (clean_pair(29, 80, length=0.3), d())
    out["nan"] = (nan_pair(), d())
    out["rotation"] = (clean_pair(30, 120, baseline=1e-9), d())
    out["rej"] = (clean_pair(32, 100, rot=0.25, trans=0.8), d(initial_radius=1e16))
    out["invalid"] = (clean_pair(33, 60), d(initial_radius=1e-310, min_radius=0.0, min_lm_diagonal=0.0))
    return out


test_scenes.__test__ = False


def batch_scenes():
    """70 pairs of mixed sizes, perturbations (so iteration counts) and list orders, under the default options."""
    rng = np.random.default_rng(77)
    out = []
    for k in range(70):
        m = int(rng.integers(0, 200))
        n = m + int(rng.integers(0, 40))
        out.append(clean_pair(200 + k, m, n=max(n, 1), rot=float(rng.uniform(0.001, 0.012)), trans=float(rng.uniform(0.005, 0.06)),
                              order="shuffled" if (k % 3 == 0 and m >= 2) else "ascending"))
    return out
