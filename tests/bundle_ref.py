"""numpy restatement of the bundle-adjustment rules of include/ebo.h (B1-B9), and the scenes the tests solve.

One float64 operation per numpy operation, in the association the rules state; vectorised only across independent
outputs (observations, points, entries of a matrix), never inside a stated sum.  `reverse_sums=True` takes the stated
sums in descending order: the frame and point sums of B5, the point order of B8's reduced system and right-hand side,
the observation order of the points' back-substitution, and the trees of B9 (entries reversed before they are dealt
to the lanes, each lane adding from its last entry).  The elimination order of the factorisation and of the two
triangular solves is the algorithm, not a sum's order, and stays; so do dot and dot6.
"""
import numpy as np

LANES = 256
DBL_MAX = 1.7976931348623157e308
DBL_MIN = 2.2250738585072014e-308
MAX_FRAMES, MAX_POINTS, MAX_OBS = 24, 4096, 65535


def default_opts(**over):
    o = dict(max_num_iterations=50, use_nonmonotonic=0, function_tolerance=1e-6, gradient_tolerance=1e-10,
             parameter_tolerance=1e-8, initial_radius=1e4, max_radius=1e16, min_radius=1e-32, min_relative_decrease=1e-3,
             min_lm_diagonal=1e-6, max_lm_diagonal=1e32, max_consecutive_nonmonotonic=5, max_consecutive_invalid=5,
             jacobi_scaling=1)
    o.update(over)
    return o


def dot3(a0, a1, a2, b0, b1, b2):
    return (a0 * b0 + a1 * b1) + a2 * b2


def finite(v):
    return v >= -DBL_MAX and v <= DBL_MAX


def tree(v, is_max=False, rev=False):
    v = np.asarray(v, dtype=np.float64)
    n = len(v)
    rows = (n + LANES - 1) // LANES
    pad = np.zeros(max(rows, 1) * LANES)
    pad[:n] = v[::-1] if rev else v
    m = pad.reshape(-1, LANES)
    acc = np.zeros(LANES)
    for r in (range(m.shape[0] - 1, -1, -1) if rev else range(m.shape[0])):
        acc = np.where(m[r] > acc, m[r], acc) if is_max else acc + m[r]
    s = LANES // 2
    while s:
        a, b = acc[:s].copy(), acc[s:2 * s].copy()
        acc[:s] = np.where(b > a, b, a) if is_max else a + b
        s //= 2
    return acc[0]


def project_parts(cam, q):
    fx, fy, cx, cy, k1, k2, _k3, p1, p2 = cam
    xP = q[:, 0] / q[:, 2]
    yP = q[:, 1] / q[:, 2]
    r2 = xP * xP + yP * yP
    rad = (1.0 + k1 * r2) + (k2 * r2) * r2
    tx = ((2.0 * p1) * xP) * yP + p2 * (r2 + (2.0 * xP) * xP)
    ty = ((2.0 * p2) * yP) * xP + p1 * (r2 + (2.0 * yP) * yP)
    xD = xP * rad + tx
    yD = yP * rad + ty
    return xP, yP, r2, rad, fx * xD + cx, fy * yD + cy


def observe(cam, T, X, uv, huber, want_jac):
    """B1-B3 for n observations.  T (n, 12), X (n, 3), uv (n, 2) -> r (corrected when want_jac), rho, A, q."""
    fx, fy, cx, cy, k1, k2, _k3, p1, p2 = cam
    d0, d1, d2 = X[:, 0] - T[:, 3], X[:, 1] - T[:, 7], X[:, 2] - T[:, 11]
    q = np.stack([dot3(T[:, j], T[:, 4 + j], T[:, 8 + j], d0, d1, d2) for j in range(3)], axis=1)
    with np.errstate(all="ignore"):
        xP, yP, r2, rad, uh, vh = project_parts(cam, q)
        r0 = uv[:, 0] - uh
        r1 = uv[:, 1] - vh
        s = r0 * r0 + r1 * r1
        b = huber * huber
        out = s > b
        root = np.sqrt(np.where(out, s, 1.0))
        rho = np.where(out, (2.0 * huber) * root - b, s)
        rho1 = huber / root
        rho1 = np.where(rho1 > DBL_MIN, rho1, DBL_MIN)
        rho1 = np.where(out, rho1, 1.0)
        if not want_jac:
            return np.stack([r0, r1], axis=1), rho, None, q
        sr = np.sqrt(rho1)
        r = np.stack([r0 * sr, r1 * sr], axis=1)
        dr = k1 + (2.0 * k2) * r2
        xx2, yy2, xy2 = (2.0 * xP) * xP, (2.0 * yP) * yP, (2.0 * xP) * yP
        dxx = ((rad + xx2 * dr) + (2.0 * p1) * yP) + (6.0 * p2) * xP
        dxy = (xy2 * dr + (2.0 * p1) * xP) + (2.0 * p2) * yP
        dyy = ((rad + yy2 * dr) + (2.0 * p2) * xP) + (6.0 * p1) * yP
        iz = 1.0 / q[:, 2]
        A = np.empty((len(q), 2, 3))
        A[:, 0, 0] = (fx * (dxx * iz)) * sr
        A[:, 0, 1] = (fx * (dxy * iz)) * sr
        A[:, 0, 2] = (fx * (-((dxx * xP + dxy * yP) * iz))) * sr
        A[:, 1, 0] = (fy * (dxy * iz)) * sr
        A[:, 1, 1] = (fy * (dyy * iz)) * sr
        A[:, 1, 2] = (fy * (-((dxy * xP + dyy * yP) * iz))) * sr
    return r, rho, A, q


def jacobians(A, q, T):
    """B3: unscaled Jc (n, 2, 6) and Jp (n, 2, 3)."""
    n = len(q)
    Jc = np.empty((n, 2, 6))
    Jp = np.empty((n, 2, 3))
    for k in range(2):
        Jc[:, k, 0:3] = A[:, k, :]
        Jc[:, k, 3] = A[:, k, 2] * q[:, 1] - A[:, k, 1] * q[:, 2]
        Jc[:, k, 4] = A[:, k, 0] * q[:, 2] - A[:, k, 2] * q[:, 0]
        Jc[:, k, 5] = A[:, k, 1] * q[:, 0] - A[:, k, 0] * q[:, 1]
        for j in range(3):
            Jp[:, k, j] = -dot3(A[:, k, 0], A[:, k, 1], A[:, k, 2], T[:, 4 * j], T[:, 4 * j + 1], T[:, 4 * j + 2])
    return Jc, Jp


def retract(T, ups, om):
    """B4 for n poses: T (n, 12), ups, om (n, 3)."""
    hx, hy, hz = om[:, 0] * 0.5, om[:, 1] * 0.5, om[:, 2] * 0.5
    n = np.sqrt(1.0 + ((hx * hx + hy * hy) + hz * hz))
    x, y, z, w = hx / n, hy / n, hz / n, 1.0 / n
    x2, y2, z2 = 2.0 * x, 2.0 * y, 2.0 * z
    twx, twy, twz = x2 * w, y2 * w, z2 * w
    txx, txy, txz = x2 * x, y2 * x, z2 * x
    tyy, tyz, tzz = y2 * y, z2 * y, z2 * z
    C = [[1.0 - (tyy + tzz), txy - twz, txz + twy], [txy + twz, 1.0 - (txx + tzz), tyz - twx],
         [txz - twy, tyz + twx, 1.0 - (txx + tyy)]]
    out = np.empty_like(T)
    for i in range(3):
        for j in range(3):
            out[:, 4 * i + j] = dot3(T[:, 4 * i], T[:, 4 * i + 1], T[:, 4 * i + 2], C[0][j], C[1][j], C[2][j])
        out[:, 4 * i + 3] = T[:, 4 * i + 3] + dot3(T[:, 4 * i], T[:, 4 * i + 1], T[:, 4 * i + 2], ups[:, 0], ups[:, 1], ups[:, 2])
    return out


def sort_observations(F, of, op, uv):
    key = np.asarray(op, np.int64) * F + np.asarray(of, np.int64)
    order = np.argsort(key, kind="stable")
    return np.asarray(of, np.int32)[order], np.asarray(op, np.int32)[order], np.asarray(uv, np.float64).reshape(-1, 2)[order]


class Solver:
    """One problem.  poses (F, 3, 4), fixed (F,), points (P, 3), observations in any order."""

    def __init__(self, poses, fixed, points, of, op, uv, cam, huber, fix_points=False, opts=None, reverse_sums=False):
        self.o = opts or default_opts()
        self.cam = tuple(float(c) for c in cam)
        self.huber = float(huber)
        self.fix = bool(fix_points)
        self.rev = bool(reverse_sums)
        self.pose0 = np.array(poses, np.float64).reshape(-1, 12)
        self.pt0 = np.array(points, np.float64).reshape(-1, 3)
        self.F, self.P = len(self.pose0), len(self.pt0)
        self.of, self.op, self.uv = sort_observations(self.F, of, op, uv)
        self.N = len(self.of)
        self.fixed = np.asarray(fixed).astype(bool)
        self.free = ~self.fixed
        self.flist = np.nonzero(self.free)[0]
        self.fslot = np.full(self.F, -1)
        self.fslot[self.flist] = np.arange(len(self.flist))
        self.dim = 6 * len(self.flist)
        self.table = np.full((self.P, self.F), -1)
        self.table[self.op, self.of] = np.arange(self.N)
        self.pstart = np.searchsorted(self.op, np.arange(self.P + 1), side="left")
        count = self.pstart[1:] - self.pstart[:-1]
        self.active = np.ones(self.P, bool) if self.fix else count >= 2
        self.count = count
        self.oact = self.active[self.op] if self.N else np.zeros(0, bool)
        self.ofree = self.free[self.of] if self.N else np.zeros(0, bool)
        self.scale = np.ones(6 * self.F + 3 * self.P)
        # what the guard of tests/test_bundle_cpu.py looks at: every step quality, and both sides of every convergence test
        self.qualities, self.checks = [], []
        self.exit_checks = []    # (value, threshold) of every gradient_tolerance and min_radius test taken
        self.failed_pivots = []  # the pivot every factorisation that broke off stopped at
        self.pfree = np.concatenate([np.repeat(self.free, 6), np.repeat(self.active & (not self.fix), 3)])
        self.mask12 = np.concatenate([np.repeat(self.free, 12), np.repeat(self.active & (not self.fix), 3)])

    # ---- evaluation ----
    def cost_at(self, pose, pt):
        rho = np.zeros(self.N)
        a = self.oact
        if a.any():
            _, rho_a, _, _ = observe(self.cam, pose[self.of[a]], pt[self.op[a]], self.uv[a], self.huber, False)
            rho[a] = rho_a
        return 0.5 * tree(rho, rev=self.rev)

    def eval_jac(self, pose, pt):
        N, F = self.N, self.F
        self.res = np.zeros((N, 2))
        self.Jc = np.zeros((N, 2, 6))
        self.Jp = np.zeros((N, 2, 3))
        rho = np.zeros(N)
        a = self.oact
        if a.any():
            T = pose[self.of[a]]
            r, rho_a, A, q = observe(self.cam, T, pt[self.op[a]], self.uv[a], self.huber, True)
            Jc, Jp = jacobians(A, q, T)
            sc = self.scale[:6 * F].reshape(F, 6)[self.of[a]]
            sp = self.scale[6 * F:].reshape(-1, 3)[self.op[a]]
            self.res[a] = r
            rho[a] = rho_a
            self.Jc[a] = Jc * sc[:, None, :]
            self.Jp[a] = Jp * sp[:, None, :]
        with np.errstate(all="ignore"):
            self.W = self.Jc[:, 0, :, None] * self.Jp[:, 0, None, :] + self.Jc[:, 1, :, None] * self.Jp[:, 1, None, :]
        cost = 0.5 * tree(rho, rev=self.rev)
        self.sums()
        return cost

    def sums(self):
        F, P = self.F, self.P
        U = np.zeros((F, 6, 6))
        g = np.zeros((F, 6))
        with np.errstate(all="ignore"):
            for l in (range(P - 1, -1, -1) if self.rev else range(P)):
                if not self.active[l]:
                    continue
                o = self.table[l]
                m = (o >= 0) & self.free
                i = o[m]
                J0, J1 = self.Jc[i, 0], self.Jc[i, 1]
                U[m] = U[m] + (J0[:, :, None] * J0[:, None, :] + J1[:, :, None] * J1[:, None, :])
                g[m] = g[m] + (J0 * self.res[i, 0, None] + J1 * self.res[i, 1, None])
            V = np.zeros((P, 3, 3))
            gl = np.zeros((P, 3))
            if not self.fix and P:
                for j in range(int(self.count.max()) if self.N else 0):
                    m = self.active & (self.count > j)
                    i = (self.pstart[1:][m] - 1 - j) if self.rev else (self.pstart[:-1][m] + j)
                    J0, J1 = self.Jp[i, 0], self.Jp[i, 1]
                    V[m] = V[m] + (J0[:, :, None] * J0[:, None, :] + J1[:, :, None] * J1[:, None, :])
                    gl[m] = gl[m] + (J0 * self.res[i, 0, None] + J1 * self.res[i, 1, None])
        self.U, self.g, self.V, self.gl = U, g, V, gl

    def param_diag(self):
        return np.concatenate([np.einsum("kaa->ka", self.U).reshape(-1), np.einsum("laa->la", self.V).reshape(-1)])

    def grad_max(self):
        gr = np.concatenate([self.g.reshape(-1), self.gl.reshape(-1)])
        with np.errstate(all="ignore"):
            v = np.where(self.pfree, np.abs(gr / self.scale), 0.0)
        return tree(v, is_max=True, rev=self.rev)

    def norm(self, pose, pt, pose_b=None, pt_b=None):
        d = np.concatenate([pose.reshape(-1), pt.reshape(-1)])
        if pose_b is not None:
            d = d - np.concatenate([pose_b.reshape(-1), pt_b.reshape(-1)])
        with np.errstate(all="ignore"):
            return np.sqrt(tree(np.where(self.mask12, d * d, 0.0), rev=self.rev))

    def damp(self, d, radius):
        o = self.o
        d = np.where(d > o["min_lm_diagonal"], d, o["min_lm_diagonal"])
        d = np.where(d < o["max_lm_diagonal"], d, o["max_lm_diagonal"])
        l = np.sqrt(d / radius)
        return l * l

    # ---- B7, B8: the step; returns None for an invalid one ----
    def compute_step(self, radius):
        F, P, n = self.F, self.P, self.dim
        invalid = False
        with np.errstate(all="ignore"):
            if not self.fix:
                M = self.V.copy()
                for i in range(3):
                    M[:, i, i] = M[:, i, i] + self.damp(M[:, i, i], radius)
                C = np.empty_like(M)
                for i in range(3):
                    for j in range(3):
                        i1, i2, j1, j2 = (i + 1) % 3, (i + 2) % 3, (j + 1) % 3, (j + 2) % 3
                        C[:, i, j] = M[:, i1, j1] * M[:, i2, j2] - M[:, i1, j2] * M[:, i2, j1]
                det = dot3(M[:, 0, 0], M[:, 0, 1], M[:, 0, 2], C[:, 0, 0], C[:, 0, 1], C[:, 0, 2])
                if (~(det > 0.0) & self.active).any():
                    invalid = True
                Vinv = np.transpose(C, (0, 2, 1)) / det[:, None, None]
                iv = Vinv[self.op] if self.N else np.zeros((0, 3, 3))
                Y = np.empty((self.N, 6, 3))
                for b in range(3):
                    Y[:, :, b] = dot3(self.W[:, :, 0], self.W[:, :, 1], self.W[:, :, 2], iv[:, None, 0, b], iv[:, None, 1, b], iv[:, None, 2, b])
            rowf = np.repeat(self.flist, 6)
            rowa = np.tile(np.arange(6), len(self.flist))
            S = np.zeros((n, n))
            rhs = np.zeros(n)
            if n:
                same = rowf[:, None] == rowf[None, :]
                Ublk = self.U[rowf[:, None], rowa[:, None], rowa[None, :]]
                S = np.where(same, Ublk, 0.0)
                dg = np.arange(n)
                S[dg, dg] = S[dg, dg] + self.damp(S[dg, dg], radius)
                rhs = self.g[rowf, rowa].copy()
                if not self.fix:
                    for l in (range(P - 1, -1, -1) if self.rev else range(P)):
                        if not self.active[l]:
                            continue
                        oi = self.table[l][rowf]
                        seen = oi >= 0
                        if not seen.any():
                            continue
                        Yr = Y[oi, rowa]
                        Wc = self.W[oi, rowa]
                        term = (Yr[:, None, 0] * Wc[None, :, 0] + Yr[:, None, 1] * Wc[None, :, 1]) + Yr[:, None, 2] * Wc[None, :, 2]
                        S = np.where(seen[:, None] & seen[None, :], S - term, S)
                        tr = dot3(Yr[:, 0], Yr[:, 1], Yr[:, 2], self.gl[l, 0], self.gl[l, 1], self.gl[l, 2])
                        rhs = np.where(seen, rhs - tr, rhs)
            self.S = S.copy()
            self.rhs = rhs.copy()
            # Cholesky, lower, column by column
            L = S
            for k in range(n):
                d = L[k, k]
                if not (d > 0.0 and finite(d)):
                    invalid = True
                    self.failed_pivots.append(float(d))
                    break
                L[k, k] = np.sqrt(d)
                L[k + 1:, k] = L[k + 1:, k] / L[k, k]
                L[k + 1:, k + 1:] = L[k + 1:, k + 1:] - L[k + 1:, k, None] * L[None, k + 1:, k]
            if invalid:
                return None
            vec = rhs
            sol = np.zeros(n)
            for k in range(n):
                y = vec[k] / L[k, k]
                vec[k + 1:] = vec[k + 1:] - L[k + 1:, k] * y
                sol[k] = y
            x = np.zeros(n)
            for k in range(n - 1, -1, -1):
                xk = sol[k] / L[k, k]
                sol[:k] = sol[:k] - L[k, :k] * xk
                x[k] = xk
            step = np.zeros(6 * F + 3 * P)
            fs = -x
            step[:6 * F].reshape(F, 6)[self.flist] = fs.reshape(-1, 6)
            bad = ~np.isfinite(fs)
            if bad.any():
                invalid = True
            if not self.fix and P:
                e = self.gl.copy()
                for j in range(int(self.count.max()) if self.N else 0):
                    m = self.active & (self.count > j)
                    i = (self.pstart[1:][m] - 1 - j) if self.rev else (self.pstart[:-1][m] + j)
                    k = self.fslot[self.of[i]]
                    fr = k >= 0
                    mi = np.nonzero(m)[0][fr]
                    i, k = i[fr], k[fr]
                    if len(i) == 0:
                        continue
                    d = x.reshape(-1, 6)[k]
                    w = self.W[i]
                    for b in range(3):
                        t = w[:, 0, b] * d[:, 0] + w[:, 1, b] * d[:, 1]
                        t = t + w[:, 2, b] * d[:, 2]
                        t = t + w[:, 3, b] * d[:, 3]
                        t = t + w[:, 4, b] * d[:, 4]
                        t = t + w[:, 5, b] * d[:, 5]
                        e[mi, b] = e[mi, b] - t
                ps = np.empty((P, 3))
                for a in range(3):
                    ps[:, a] = -dot3(Vinv[:, a, 0], Vinv[:, a, 1], Vinv[:, a, 2], e[:, 0], e[:, 1], e[:, 2])
                ps = np.where(self.active[:, None], ps, 0.0)
                if (~np.isfinite(ps)).any():
                    invalid = True
                step[6 * F:] = ps.reshape(-1)
        return None if invalid else step

    def model_cost_change(self, step):
        F = self.F
        red = np.zeros(self.N)
        a = self.oact
        with np.errstate(all="ignore"):
            if a.any():
                sf = step[:6 * F].reshape(F, 6)[self.of[a]]
                sp = step[6 * F:].reshape(-1, 3)[self.op[a]]
                term = []
                for k in range(2):
                    J = self.Jc[a, k]
                    mc = J[:, 0] * sf[:, 0] + J[:, 1] * sf[:, 1]
                    for c in range(2, 6):
                        mc = mc + J[:, c] * sf[:, c]
                    mc = np.where(self.ofree[a], mc, 0.0)
                    Jp = self.Jp[a, k]
                    mp = 0.0 if self.fix else dot3(Jp[:, 0], Jp[:, 1], Jp[:, 2], sp[:, 0], sp[:, 1], sp[:, 2])
                    mr = mc + mp
                    term.append(mr * (self.res[a, k] + mr / 2.0))
                red[a] = term[0] + term[1]
            return -tree(red, rev=self.rev)

    def candidate(self, pose, pt, step):
        F = self.F
        s = step * self.scale
        sf = s[:6 * F].reshape(F, 6)
        cp = pose.copy()
        fl = self.flist
        if len(fl):
            cp[fl] = retract(pose[fl], sf[fl, 0:3], sf[fl, 3:6])
        cq = pt.copy()
        if not self.fix:
            a = self.active
            cq[a] = pt[a] + s[6 * F:].reshape(-1, 3)[a]
        return cp, cq

    # ---- B9 ----
    def solve(self):
        o = self.o
        max_it = o["max_num_iterations"]
        trace = np.zeros((max_it + 1, 4))
        x_pose, x_pt = self.pose0.copy(), self.pt0.copy()
        best_pose, best_pt = self.pose0.copy(), self.pt0.copy()
        st = dict(iterations=0, num_evals_cost=0, num_evals_jac=1, termination=1)
        radius, decrease = o["initial_radius"], 2.0
        max_nonmono = o["max_consecutive_nonmonotonic"] if o["use_nonmonotonic"] else 0
        x_cost = self.eval_jac(x_pose, x_pt)
        st["initial_cost"] = min_cost = x_cost
        trace[0] = (x_cost, radius, 0.0, 1.0)

        def done(term):
            st["termination"] = term
            st["final_cost"] = min_cost
            return dict(poses=best_pose.reshape(-1, 3, 4), points=best_pt, summary=st, trace=trace,
                        last_poses=x_pose.reshape(-1, 3, 4), last_points=x_pt)  # last_*: the iterate the solve stopped at

        if not finite(x_cost):
            return done(2)
        if o["jacobi_scaling"]:
            with np.errstate(all="ignore"):
                self.scale = np.where(self.pfree, 1.0 / (1.0 + np.sqrt(self.param_diag())), 1.0)
            x_cost = self.eval_jac(x_pose, x_pt)
        grad_max = self.grad_max()
        x_norm = self.norm(x_pose, x_pt)
        se_min = se_cur = se_ref = se_cand = x_cost
        se_acc_ref = se_acc_cand = 0.0
        se_nonmono = 0
        num_invalid = 0
        last_successful = True
        while True:
            if last_successful and x_cost < min_cost:
                min_cost = x_cost
                best_pose, best_pt = x_pose.copy(), x_pt.copy()
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
            c_pose, c_pt = self.candidate(x_pose, x_pt, step)
            st["num_evals_cost"] += 1
            cand_cost = self.cost_at(c_pose, c_pt)
            if not finite(cand_cost):
                cand_cost = DBL_MAX
            step_norm = self.norm(x_pose, x_pt, c_pose, c_pt)
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
            x_pose, x_pt = c_pose, c_pt
            x_norm = self.norm(x_pose, x_pt)
            x_cost = self.eval_jac(x_pose, x_pt)
            grad_max = self.grad_max()
            st["num_evals_jac"] += 1
            last_successful = True
            if not finite(x_cost):
                return done(2)


def solve(problem, huber, fix_points=False, opts=None, reverse_sums=False):
    s = Solver(problem["poses"], problem["fixed"], problem["points"], problem["of"], problem["op"], problem["uv"], problem["cam"],
               huber, fix_points, opts, reverse_sums)
    out = s.solve()
    out["solver"] = s
    return out


# the option fields of the problem file: five in its head, the rest of ebo_solver_opts in its order at its end (mode, which
# the bundle adjustment never reads, is not carried)
HEAD_OPTS = ("max_num_iterations", "use_nonmonotonic", "function_tolerance", "gradient_tolerance", "parameter_tolerance")
TAIL_OPTS = ("initial_radius", "max_radius", "min_radius", "min_relative_decrease", "min_lm_diagonal", "max_lm_diagonal",
             "max_consecutive_nonmonotonic", "max_consecutive_invalid", "jacobi_scaling")


def write_problem(path, pr, huber, fix_points, opts):
    """The problem file of tools/bundle_adjust_serial.cpp and tests/cpp/bundle_lines_test.cpp: raw float64, a head of 19
    (F, P, N, fix_points, the five HEAD_OPTS, huber, the camera's nine), the arrays with the observations sorted by
    (point, frame), then the nine TAIL_OPTS: every field of opts reaches the reader.  The tail comes last so that a
    reader of the arrays alone, and a file written without it (the defaults then), stay valid."""
    of, op, uv = sort_observations(len(pr["poses"]), pr["of"], pr["op"], pr["uv"])
    assert set(opts) == set(HEAD_OPTS + TAIL_OPTS), sorted(opts)
    head = [len(pr["poses"]), len(pr["points"]), len(of), int(fix_points), *[opts[k] for k in HEAD_OPTS], huber, *pr["cam"]]
    np.concatenate([np.array(head, float), np.asarray(pr["poses"], float).reshape(-1), np.asarray(pr["fixed"], float),
                    np.asarray(pr["points"], float).reshape(-1), of.astype(float), op.astype(float), uv.reshape(-1),
                    np.array([opts[k] for k in TAIL_OPTS], float)]).tofile(str(path))


# ---- scenes ----------------------------------------------------------------------------------------------------------
CAM = (200.0, 198.0, 120.0, 90.0, -0.05, 0.01, 0.0, 0.001, -0.0005)
IDENTITY_CAM = (1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)


def rot(w):
    th = np.linalg.norm(w)
    if th == 0:
        return np.eye(3)
    k = w / th
    K = np.array([[0, -k[2], k[1]], [k[2], 0, -k[0]], [-k[1], k[0], 0]])
    return np.eye(3) + np.sin(th) * K + (1 - np.cos(th)) * (K @ K)


def project_np(cam, q):
    q = np.atleast_2d(q)
    _, _, _, _, u, v = project_parts(cam, q)
    return np.stack([u, v], axis=1)


def scene(seed, F, P, n_fixed=2, views=None, noise=0.0, outliers=0.0, outlier_px=30.0, perturb_pose=0.01, perturb_pt=0.03, cam=CAM,
          fixed=None, baseline=0.25):
    """A synthetic window: cameras on a line looking down +z at a cloud 4-8 in front.  views: None = every point in every
    frame, or (lo, hi): each point seen by a seeded lo..hi frames.  Returns the problem with perturbed free poses and
    points; the true values under "true_poses" / "true_points"."""
    rng = np.random.default_rng(seed)
    poses = np.zeros((F, 3, 4))
    for k in range(F):
        poses[k, :, :3] = rot(rng.normal(0, 0.03, 3))
        poses[k, :, 3] = np.array([baseline * k, 0.0, 0.0]) + rng.normal(0, 0.03, 3)
    pts = np.stack([rng.uniform(-1.5, 1.5 + baseline * F, P), rng.uniform(-1.2, 1.2, P), rng.uniform(4.0, 8.0, P)], axis=1)
    of, op = [], []
    for l in range(P):
        if views is None:
            fr = np.arange(F)
        else:
            m = int(rng.integers(views[0], min(views[1], F) + 1))
            fr = np.sort(rng.choice(F, size=m, replace=False))
        of += list(fr)
        op += [l] * len(fr)
    of, op = np.array(of, np.int32), np.array(op, np.int32)
    q = np.einsum("nji,nj->ni", poses[of, :, :3], pts[op] - poses[of, :, 3])
    uv = project_np(cam, q) + rng.normal(0, 1.0, (len(of), 2)) * noise
    if outliers > 0:
        bad = rng.random(len(of)) < outliers
        uv[bad] += rng.uniform(-outlier_px, outlier_px, (int(bad.sum()), 2))
    fixed = np.array(fixed if fixed is not None else [k < n_fixed for k in range(F)], np.uint8)
    start = poses.copy()
    for k in range(F):
        if not fixed[k]:
            start[k, :, :3] = poses[k, :, :3] @ rot(rng.normal(0, perturb_pose, 3))
            start[k, :, 3] = poses[k, :, 3] + rng.normal(0, perturb_pose, 3)
    spts = pts + rng.normal(0, perturb_pt, pts.shape)
    shuffle = rng.permutation(len(of))  # the entry sorts: hand the observations over in no order
    return dict(poses=start, fixed=fixed, points=spts, of=of[shuffle], op=op[shuffle], uv=uv[shuffle], cam=cam, true_poses=poses,
                true_points=pts)


def refine_scene(seed, P, noise=0.002):
    """One free frame, constant points, the identity camera: the pose refinement (fix_points)."""
    s = scene(seed, 1, P, n_fixed=0, noise=0.0, cam=IDENTITY_CAM, perturb_pose=0.02, perturb_pt=0.0)
    rng = np.random.default_rng(seed + 77)
    s["uv"] = s["uv"] + rng.normal(0, noise, s["uv"].shape)
    s["points"] = s["true_points"].copy()
    return s


HUBER = 0.8
REFINE_SIZES = [int(v) for v in np.linspace(4, 200, 64)]


def difference(a, b):
    """Largest |a - b| / max(1, |b|) over two equal-shaped sets of doubles (what the tests call a difference)."""
    a, b = np.asarray(a, np.float64).reshape(-1), np.asarray(b, np.float64).reshape(-1)
    if len(a) == 0:
        return 0.0
    both_nan = np.isnan(a) & np.isnan(b)
    with np.errstate(all="ignore"):
        d = np.where(both_nan | (a == b), 0.0, np.abs(a - b) / np.maximum(1.0, np.abs(b)))
    return float(np.nan_to_num(d, nan=np.inf).max())


def result_difference(x, y):
    return max(difference(x["poses"], y["poses"]), difference(x["points"], y["points"]), difference(x["trace"], y["trace"]),
               difference(x["summary"]["final_cost"], y["summary"]["final_cost"]),
               difference(x["summary"]["initial_cost"], y["summary"]["initial_cost"]))


def edge_scene():
    """4 frames (0, 1 fixed; 3 free and without observations), 8 points: point 0 seen once, point 1 by the fixed frames only."""
    s = scene(6, 4, 8, fixed=[1, 1, 0, 0])
    keep = s["of"] != 3
    keep &= ~((s["op"] == 0) & (s["of"] != 2))
    keep &= ~((s["op"] == 1) & (s["of"] >= 2))
    for k in ("of", "op", "uv"):
        s[k] = s[k][keep]
    return s


def nan_scene():
    s = scene(1, 3, 4)
    s["points"] = s["points"].copy()
    s["points"][1, 0] = np.nan
    return s


def test_scenes():
    """name -> (problem, fix_points, opts): the scenes of tests/test_gpu_bundle.py, (a)-(f) of its header."""
    out = {
        "a": (scene(1, 3, 4), False, default_opts()),
        "b": (scene(2, 2, 5), False, default_opts()),
        "c": (scene(3, 24, 40, views=(2, 24), noise=0.3), False, default_opts()),
        "d": (scene(4, 5, 300, views=(2, 5), noise=0.3, outliers=0.1, baseline=0.8), False, default_opts()),
        "edge": (edge_scene(), False, default_opts()),
        "it0": (scene(1, 3, 4), False, default_opts(max_num_iterations=0)),
        "it1": (scene(1, 3, 4), False, default_opts(max_num_iterations=1)),
        "nan": (nan_scene(), False, default_opts()),
    }
    for i, n in enumerate(REFINE_SIZES):
        out["e%02d" % i] = (refine_scene(100 + i, n), True, default_opts())
    return out


test_scenes.__test__ = False


def big_scene():
    """A problem at both limits: 16 frames, 4096 points each seen by all 16, one observation dropped: 65535."""
    s = scene(33, 16, 4096, views=(16, 16), noise=0.3)
    for k in ("of", "op", "uv"):
        s[k] = s[k][:-1]
    return s


def branch_scenes():
    """name -> (problem, fix_points, opts): the scenes of tests/test_gpu_bundle_branches.py, one per branch of B9 that
    test_scenes() never takes and per option it never varies (the table in that module's header; what each must show is
    asserted by test_bundle_cpu.py::test_the_branch_scenes_take_their_branches)."""
    a = scene(1, 3, 4)
    noisy = scene(22, 4, 30, noise=0.3, outliers=0.1, perturb_pose=0.2, perturb_pt=0.8)
    far = scene(23, 3, 12, perturb_pose=0.3, perturb_pt=1.5)
    wild = scene(68, 3, 12, perturb_pose=0.3, perturb_pt=1.5)
    d = default_opts
    return {
        "rej": (noisy, False, d()),
        "rej_mrd": (noisy, False, d(min_relative_decrease=0.5)),
        "rej4": (far, False, d(initial_radius=1e16)),
        "nonmono": (far, False, d(initial_radius=1e16, use_nonmonotonic=1)),
        "nonmono_cut": (far, False, d(initial_radius=1e16, use_nonmonotonic=1, max_num_iterations=8)),
        "nonmono_m5": (wild, False, d(initial_radius=1e16, use_nonmonotonic=1)),
        "nonmono_m2": (wild, False, d(initial_radius=1e16, use_nonmonotonic=1, max_consecutive_nonmonotonic=2)),
        "invalid": (edge_scene(), False, d(min_lm_diagonal=0.0)),
        "invalid3": (edge_scene(), False, d(min_lm_diagonal=0.0, max_consecutive_invalid=3)),
        "minrad": (a, False, d(initial_radius=1e-33)),
        "gtol": (a, False, d(function_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=1e-6)),
        "ptol": (a, False, d(function_tolerance=0.0, gradient_tolerance=0.0)),
        "ptol4": (a, False, d(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=1e-4)),
        "maxrad": (a, False, d(max_radius=2e4, function_tolerance=0.0)),
        "lmclip": (a, False, d(min_lm_diagonal=0.1, max_lm_diagonal=0.1, initial_radius=1.0)),
        "noscale": (a, False, d(jacobi_scaling=0)),
        "noscale_clip": (a, False, d(jacobi_scaling=0, min_lm_diagonal=0.1, max_lm_diagonal=0.1, initial_radius=1.0)),
        "ftol3": (noisy, False, d(function_tolerance=1e-3)),
        "fix24": (scene(31, 24, 60, n_fixed=0, views=(3, 24), noise=0.3, perturb_pose=0.03, perturb_pt=0.0), True, d()),
        "dense24": (scene(32, 24, 30, noise=0.3), False, d()),
        "big": (big_scene(), False, d(max_num_iterations=2)),
    }
