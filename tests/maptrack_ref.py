"""numpy restatement of include/ebo.h's "pose from events against a map" (E1-E9), and the scenes its tests solve.

One float64 operation per numpy operation, in the association the rules state; vectorised only across independent
outputs (points, entries of a matrix), never inside a stated sum.  The update (B4), the tree (B9) and the trust region
are bundle_ref's functions or follow bundle_ref.Solver.solve line by line.  Test infrastructure: nothing here is the
product."""
import numpy as np

import bundle_ref as B
import rotation_ref as R

DBL_MAX = B.DBL_MAX
Z_MIN = 0.05
RESULT_INTS = ("termination", "iterations", "num_evals_jac", "num_evals_cost", "visible_start", "visible_final")
RESULT_DOUBLES = ("initial_cost", "final_cost", "scale")
OPT_FIELDS = B.HEAD_OPTS + B.TAIL_OPTS


def default_opts(**over):
    return B.default_opts(**over)


def tri(a, b):
    return a * (a + 1) // 2 + b


def image_max(img):
    """E1: the largest pixel that is > 0, 0 when there is none; NaN pixels are never taken."""
    with np.errstate(all="ignore"):
        v = img[img > 0.0]
    return float(v.max()) if v.size else 0.0


def project(cam, T, X, z_min, w, h):
    """E2 for n points at pose T (12,) -> q (n, 3), iz, xP, yP, u, v, visible."""
    fx, fy, cx, cy = cam
    with np.errstate(all="ignore"):
        d0, d1, d2 = X[:, 0] - T[9], X[:, 1] - T[10], X[:, 2] - T[11]
        q = np.stack([B.dot3(T[j], T[3 + j], T[6 + j], d0, d1, d2) for j in range(3)], axis=1)
        iz = 1.0 / q[:, 2]
        xP = q[:, 0] * iz
        yP = q[:, 1] * iz
        u = fx * xP + cx
        v = fy * yP + cy
        vis = (q[:, 2] > z_min) & (u >= 0.0) & (u < float(w - 1)) & (v >= 0.0) & (v < float(h - 1))
    return q, iz, xP, yP, u, v, vis


def point_terms(cam, img, s, T, X, z_min, scale, want_j=True):
    """E2-E5 -> r (n,), J (n, 6) scaled (None without want_j), visible (n,)."""
    h, w = img.shape
    fx, fy = cam[0], cam[1]
    n = len(X)
    q, iz, xP, yP, u, v, vis = project(cam, T, X, z_min, w, h)
    r = np.ones(n)
    J = np.zeros((n, 6)) if want_j else None
    if vis.any():
        q, iz, xP, yP, u, v = q[vis], iz[vis], xP[vis], yP[vis], u[vis], v[vis]
        x0, y0 = np.floor(u), np.floor(v)
        al, be = u - x0, v - y0
        ial, ibe = 1.0 - al, 1.0 - be
        ix, iy = x0.astype(np.int64), y0.astype(np.int64)
        b00, b10, b01, b11 = img[iy, ix], img[iy, ix + 1], img[iy + 1, ix], img[iy + 1, ix + 1]
        with np.errstate(all="ignore"):
            b = ibe * (ial * b00 + al * b10) + be * (ial * b01 + al * b11)
            r[vis] = 1.0 - s * b
            if want_j:
                Du = ibe * (b10 - b00) + be * (b11 - b01)
                Dv = ial * (b01 - b00) + al * (b11 - b10)
                au, av = Du * fx, Dv * fy
                A0 = -(s * (au * iz))
                A1 = -(s * (av * iz))
                A2 = s * ((au * xP + av * yP) * iz)
                q0, q1, q2 = q[:, 0], q[:, 1], q[:, 2]
                Jv = np.stack([-A0, -A1, -A2, A1 * q2 - A2 * q1, A2 * q0 - A0 * q2, A0 * q1 - A1 * q0], axis=1)
                J[vis] = Jv * scale[None, :]
    return r, J, vis


def tree12(v):
    return B.tree(np.asarray(v, np.float64))


def to34(T):
    """A pose of this section (R row-major, then t) as bundle_ref's [3][4]."""
    return np.concatenate([T[0:3], T[9:10], T[3:6], T[10:11], T[6:9], T[11:12]])


def from34(T):
    return np.concatenate([T[0:3], T[4:7], T[8:11], T[3:4], T[7:8], T[11:12]])


def retract(T, step6):
    """B4 (bundle_ref's operations on the same numbers; only where they are kept differs)."""
    return from34(B.retract(to34(T)[None, :], step6[None, 0:3], step6[None, 3:6])[0])


class Solver:
    """One unit: an image, the points, a start pose (12,)."""

    def __init__(self, cam, img, points, pose, z_min=Z_MIN, opts=None):
        self.cam = tuple(float(c) for c in cam[:4])
        self.img = np.asarray(img, np.float64)
        self.X = np.asarray(points, np.float64).reshape(-1, 3)
        self.pose0 = np.array(pose, np.float64).reshape(12)
        self.z_min = float(z_min)
        self.o = opts or default_opts()
        self.scale = np.ones(6)
        self.qualities, self.checks, self.exit_checks, self.failed_pivots = [], [], [], []
        self.flags = []

    def cost_at(self, T):
        r, _, vis = point_terms(self.cam, self.img, self.s, T, self.X, self.z_min, self.scale, False)
        with np.errstate(all="ignore"):
            return 0.5 * B.tree(r * r), int(vis.sum())

    def eval_jac(self, T):
        r, J, vis = point_terms(self.cam, self.img, self.s, T, self.X, self.z_min, self.scale, True)
        self.r, self.J = r, J
        with np.errstate(all="ignore"):
            self.U = np.zeros((6, 6))
            for a in range(6):
                for b in range(a + 1):
                    self.U[a, b] = self.U[b, a] = B.tree(J[:, a] * J[:, b])
            self.g = np.array([B.tree(J[:, a] * r) for a in range(6)])
            cost = 0.5 * B.tree(r * r)
        self.vis_x = int(vis.sum())
        self.vis_mask = vis
        return cost

    def grad_max(self):
        with np.errstate(all="ignore"):
            return B.tree(np.abs(self.g / self.scale), is_max=True)

    def norm(self, a, b=None):
        with np.errstate(all="ignore"):
            d = a if b is None else a - b
            return np.sqrt(tree12(d * d))

    def damp(self, d, radius):
        o = self.o
        d = d if d > o["min_lm_diagonal"] else o["min_lm_diagonal"]
        d = d if d < o["max_lm_diagonal"] else o["max_lm_diagonal"]
        with np.errstate(all="ignore"):
            l = np.sqrt(np.float64(d) / radius)
            return l * l

    def compute_step(self, radius):
        with np.errstate(all="ignore"):
            L = self.U.copy()
            for a in range(6):
                L[a, a] = L[a, a] + self.damp(L[a, a], radius)
            vec = self.g.copy()
            n = 6
            for k in range(n):
                d = L[k, k]
                if not (d > 0.0 and B.finite(d)):
                    self.failed_pivots.append(float(d))
                    return None
                L[k, k] = np.sqrt(d)
                L[k + 1:, k] = L[k + 1:, k] / L[k, k]
                L[k + 1:, k + 1:] = L[k + 1:, k + 1:] - L[k + 1:, k, None] * L[None, k + 1:, k]
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
            step = -x
        return step if np.isfinite(step).all() else None

    def model_cost_change(self, step):
        J, r = self.J, self.r
        with np.errstate(all="ignore"):
            mr = J[:, 0] * step[0] + J[:, 1] * step[1]
            for c in range(2, 6):
                mr = mr + J[:, c] * step[c]
            m = np.where(self.vis_mask, mr * (r + mr / 2.0), 0.0)
            return -B.tree(m)

    def solve(self):
        o = self.o
        max_it = o["max_num_iterations"]
        trace = np.zeros((max_it + 1, 4))
        res = {k: 0 for k in RESULT_INTS}
        res.update({k: 0.0 for k in RESULT_DOUBLES})
        res["termination"] = 2
        x = self.pose0.copy()
        best = self.pose0.copy()
        out = dict(pose=best, result=res, trace=trace, solver=self)
        bmax = image_max(self.img)
        if not (bmax > 0.0 and B.finite(bmax)):
            return out
        self.s = 1.0 / np.float64(bmax)
        res["scale"] = float(self.s)
        radius, decrease = o["initial_radius"], 2.0
        max_nonmono = o["max_consecutive_nonmonotonic"] if o["use_nonmonotonic"] else 0
        x_cost = self.eval_jac(x)
        res["num_evals_jac"] = 1
        res["visible_start"] = res["visible_final"] = vis_x = self.vis_x
        res["initial_cost"] = min_cost = x_cost
        res["termination"] = 1
        trace[0] = (x_cost, radius, 0.0, 1.0)

        def done(term):
            res["termination"] = term
            res["final_cost"] = min_cost
            out["pose"] = best
            out["last_pose"] = x
            return out

        if not B.finite(x_cost):
            return done(2)
        if o["jacobi_scaling"]:
            with np.errstate(all="ignore"):
                self.scale = 1.0 / (1.0 + np.sqrt(np.diag(self.U).copy()))
            x_cost = self.eval_jac(x)
        grad_max = self.grad_max()
        x_norm = self.norm(x)
        se_min = se_cur = se_ref = se_cand = x_cost
        se_acc_ref = se_acc_cand = 0.0
        se_nonmono = 0
        num_invalid = 0
        last_successful = True
        while True:
            if last_successful and x_cost < min_cost:
                min_cost = x_cost
                best = x.copy()
                res["visible_final"] = vis_x
            if res["iterations"] >= max_it:
                return done(1)
            if last_successful:
                self.exit_checks.append((grad_max, o["gradient_tolerance"]))
            if last_successful and grad_max <= o["gradient_tolerance"]:
                return done(0)
            self.exit_checks.append((radius, o["min_radius"]))
            if radius < o["min_radius"]:
                return done(0)
            res["iterations"] += 1
            it = res["iterations"]
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
                self.flags.append(-1)
                if num_invalid >= o["max_consecutive_invalid"]:
                    return done(2)
                continue
            num_invalid = 0
            c = retract(x, step * self.scale)
            res["num_evals_cost"] += 1
            cand_cost, vis_c = self.cost_at(c)
            if not B.finite(cand_cost):
                cand_cost = DBL_MAX
            step_norm = self.norm(x, c)
            self.checks.append((step_norm, o["parameter_tolerance"] * (x_norm + o["parameter_tolerance"]),
                                abs(x_cost - cand_cost), o["function_tolerance"] * x_cost))
            if step_norm <= o["parameter_tolerance"] * (x_norm + o["parameter_tolerance"]) or \
                    abs(x_cost - cand_cost) <= o["function_tolerance"] * x_cost:
                trace[it] = (cand_cost, radius, 0.0, 2.0)
                self.flags.append(2)
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
            self.flags.append(1 if accepted else 0)
            if not accepted:
                continue
            x = c
            vis_x = vis_c
            x_norm = self.norm(x)
            x_cost = self.eval_jac(x)
            grad_max = self.grad_max()
            res["num_evals_jac"] += 1
            last_successful = True
            if not B.finite(x_cost):
                return done(2)


def solve_units(pr, opts=None):
    """Every unit of a problem (dict of cam, images [n][h][w], points, unit_image, poses [n][12], z_min, opts) -> list of
    dicts (pose, result, trace)."""
    o = opts or pr.get("opts") or default_opts()
    out = []
    for u, im in enumerate(pr["unit_image"]):
        out.append(Solver(pr["cam"], pr["images"][im], pr["points"], pr["poses"][u], pr.get("z_min", Z_MIN), o).solve())
    return out


def winner(results):
    """Among a window's units: the lowest final cost whose termination is not 2, ties to the lowest index; None: lost."""
    best = None
    for i, r in enumerate(results):
        if r["termination"] == 2:
            continue
        if best is None or r["final_cost"] < results[best]["final_cost"]:
            best = i
    return best


def starts13(pose, t_step, r_step):
    """The prediction and +- one step along each of B4's six update directions."""
    out = [np.asarray(pose, np.float64).reshape(12).copy()]
    for a in range(6):
        for sign in (1.0, -1.0):
            s = np.zeros(6)
            s[a] = sign * (t_step if a < 3 else r_step)
            out.append(retract(out[0], s))
    return np.stack(out)


# ---- the serial tool's files ------------------------------------------------------------------------------------------

def write_problem(path, pr, opts=None):
    o = opts or pr.get("opts") or default_opts()
    images = np.asarray(pr["images"], np.float64)
    n, h, w = images.shape
    head = [w, h, n, len(pr["points"]), len(pr["unit_image"]), pr.get("z_min", Z_MIN), *pr["cam"][:4], *[o[k] for k in OPT_FIELDS]]
    np.concatenate([np.array(head, float), images.reshape(-1), np.asarray(pr["points"], float).reshape(-1),
                    np.asarray(pr["unit_image"], float), np.asarray(pr["poses"], float).reshape(-1)]).tofile(str(path))


def read_result(path, n_units, max_it):
    rows = max_it + 1
    a = np.fromfile(str(path), dtype=np.float64).reshape(n_units, 21 + 4 * rows)
    out = []
    for u in range(n_units):
        res = {k: int(a[u, 12 + i]) for i, k in enumerate(RESULT_INTS)}
        res.update({k: a[u, 18 + i] for i, k in enumerate(RESULT_DOUBLES)})
        out.append(dict(pose=a[u, :12].copy(), result=res, trace=a[u, 21:].reshape(rows, 4).copy()))
    return out


def same_bits(a, b):
    """Bit-equal doubles; a NaN equals any NaN (IEEE 754 leaves a NaN's sign and payload to the implementation, and the
    host's and the device's default NaNs differ in the sign)."""
    a, b = np.ascontiguousarray(a, np.float64), np.ascontiguousarray(b, np.float64)
    if a.shape != b.shape:
        return False
    both = np.isnan(a) & np.isnan(b)
    return np.array_equal(np.where(both, 0, a.view(np.uint64)), np.where(both, 0, b.view(np.uint64)))


def same_unit(got, want):
    """Every double and integer of a unit: pose, result, trace."""
    if not same_bits(got["pose"], want["pose"]) or not same_bits(got["trace"], want["trace"]):
        return False
    for k in RESULT_INTS:
        if int(got["result"][k]) != int(want["result"][k]):
            return False
    return all(same_bits(got["result"][k], want["result"][k]) for k in RESULT_DOUBLES)


# ---- scenes -------------------------------------------------------------------------------------------------------------

IDENTITY = np.array([1.0, 0, 0, 0, 1.0, 0, 0, 0, 1.0, 0, 0, 0])
SMALL = dict(w=37, h=29, cam=(30.0, 31.0, 18.0, 14.25))
MID = dict(w=64, h=48, cam=(60.0, 60.0, 32.0, 24.0))


def pose_of(Rm, t):
    return np.concatenate([np.asarray(Rm, np.float64).reshape(9), np.asarray(t, np.float64).reshape(3)])


def displaced(pose, rng, dt, dr):
    """pose moved by dt along a random translation direction and dr rad about a random axis (on the right)."""
    d = rng.normal(size=3)
    a = rng.normal(size=3)
    T = np.asarray(pose, np.float64)
    Rm = T[:9].reshape(3, 3)
    return pose_of(Rm @ B.rot(a / np.linalg.norm(a) * dr), T[9:] + Rm @ (d / np.linalg.norm(d) * dt))


def map_points(rng, geo, n, depths=(2.0, 4.0), margin=6.0):
    """n world points seen from the identity pose inside the image's margin, split evenly over the depths."""
    fx, fy, cx, cy = geo["cam"]
    u = rng.uniform(margin, geo["w"] - 1 - margin, n)
    v = rng.uniform(margin, geo["h"] - 1 - margin, n)
    z = np.array([depths[i * len(depths) // n] for i in range(n)]) if n >= len(depths) else np.full(n, depths[0])
    return np.stack([(u - cx) / fx * z, (v - cy) / fy * z, z], axis=1)


def pixels_of(geo, pose, X):
    q, _, _, _, u, v, _ = project(geo["cam"], np.asarray(pose, np.float64).reshape(12), X, -np.inf, 1 << 30, 1 << 30)
    return np.stack([u, v], axis=1)


def scene_events(rng, geo, X, pose=IDENTITY, per_point=8, jitter=0.3, noise=0.3):
    """Integer-pixel events: per_point per map point around its projection, and noise * that many anywhere."""
    uv = pixels_of(geo, pose, X)
    e = np.repeat(uv, per_point, axis=0) + rng.normal(0, jitter, (len(uv) * per_point, 2))
    e = np.rint(e).astype(np.int64)
    n_noise = int(noise * len(e))
    e = np.concatenate([e, np.stack([rng.integers(0, geo["w"], n_noise), rng.integers(0, geo["h"], n_noise)], axis=1)])
    keep = (e[:, 0] >= 0) & (e[:, 0] < geo["w"]) & (e[:, 1] >= 0) & (e[:, 1] < geo["h"])
    return e[keep]


def count_image(geo, e):
    img = np.zeros((geo["h"], geo["w"]))
    np.add.at(img, (e[:, 1], e[:, 0]), 1.0)
    return img


def event_image(geo, e, sigma=1.0):
    """The blurred event image at zero omega: V4's count image through V5's blur."""
    return R.blur(count_image(geo, e), R.blur_weights(sigma))


def recovery_scene(seed, dt=0.06, dr=0.02, n=120):
    """The issue's two-depth scene: 64 x 48, f = 60, n points half at Z = 2 and half at Z = 4, 8 events a point jittered
    by 0.3 px and rounded, 30 % noise events, blur 1; the truth is the identity pose."""
    rng = np.random.default_rng(seed)
    X = map_points(rng, MID, n)
    ev = scene_events(rng, MID, X)
    start = displaced(IDENTITY, rng, dt, dr)
    return dict(geo=MID, cam=MID["cam"], points=X, events=ev, image=event_image(MID, ev), truth=IDENTITY.copy(), start=start)


def reprojection_error(geo, X, pose, truth):
    d = pixels_of(geo, pose, X) - pixels_of(geo, truth, X)
    return float(np.mean(np.sqrt((d * d).sum(axis=1))))


def random_image(rng, geo, blobs=40, sigma=1.0):
    e = np.stack([rng.integers(0, geo["w"], blobs * 6), rng.integers(0, geo["h"], blobs * 6)], axis=1)
    return event_image(geo, e, sigma)


def problem(geo, images, points, unit_image, poses, z_min=Z_MIN, opts=None):
    return dict(cam=geo["cam"], images=np.ascontiguousarray(images, np.float64), points=np.ascontiguousarray(points, np.float64),
                unit_image=np.ascontiguousarray(unit_image, np.int32), poses=np.ascontiguousarray(poses, np.float64).reshape(-1, 12),
                z_min=z_min, opts=opts or default_opts())


def aligned_problem(seed, geo, n_points, n_units, n_images=None, dt=0.04, dr=0.015, opts=None, per_point=6):
    """n_images images of the same map seen from the identity pose with different events; unit u starts displaced from it
    and names image u mod n_images."""
    rng = np.random.default_rng(seed)
    n_images = n_images or min(n_units, 3)
    X = map_points(rng, geo, n_points, margin=4.0)
    images = np.stack([event_image(geo, scene_events(rng, geo, X, per_point=per_point)) for _ in range(n_images)])
    poses = np.stack([displaced(IDENTITY, rng, dt, dr) for _ in range(n_units)])
    return problem(geo, images, X, np.arange(n_units) % n_images, poses, opts=opts)


def border_problem():
    """Points exactly on the four visibility borders, q2 exactly at z_min, a NaN point, inside points; poses: identity, one
    with a NaN entry, one with an infinite entry."""
    geo = SMALL
    fx, fy, cx, cy = geo["cam"]
    w, h = geo["w"], geo["h"]
    rng = np.random.default_rng(5)

    def at(u, v, z=2.0):
        return [(u - cx) / fx * z, (v - cy) / fy * z, z]

    pts = [at(0.0, 10.0), at(w - 1.0, 10.0), at(12.0, 0.0), at(12.0, h - 1.0), at(w - 2.0, h - 2.0), at(0.0, 0.0),
           [0.0, 0.0, 0.5], [np.nan, 0.1, 2.0], [0.1, 0.1, -2.0], at(10.5, 9.25), at(20.75, 17.5), at(7.0, 7.0)]
    X = np.array(pts)
    img = random_image(rng, geo)
    nanp = IDENTITY.copy()
    nanp[4] = np.nan
    infp = IDENTITY.copy()
    infp[9] = np.inf
    return problem(geo, img[None], X, [0, 0, 0], [IDENTITY, nanp, infp], z_min=0.5)


def visibility_problem():
    """Unit 0: the whole scene in view; unit 1: about half out of view; unit 2: every point invisible."""
    pr = aligned_problem(11, SMALL, 80, 1, n_images=1)
    half = pose_of(np.eye(3), [0.9, 0.0, 0.0])
    away = pose_of(np.eye(3), [0.0, 0.0, 10.0])
    return problem(SMALL, pr["images"], pr["points"], [0, 0, 0], [pr["poses"][0], half, away])


def degenerate_problem():
    """Images: all zero, constant, a one-pixel spike, a NaN no tap reads, a NaN a tap reads, an infinity, all negative."""
    geo = SMALL
    pr = aligned_problem(12, geo, 30, 1, n_images=1)
    base = pr["images"][0]
    h, w = base.shape
    zero = np.zeros_like(base)
    const = np.full_like(base, 0.7)
    spike = zero.copy()
    uv = np.floor(pixels_of(geo, pr["poses"][0], pr["points"][:1])[0]).astype(int)
    spike[uv[1], uv[0]] = 3.0
    taps = np.zeros((h, w), bool)
    p = np.floor(pixels_of(geo, IDENTITY, pr["points"])).astype(int)
    for dx in range(-3, 5):
        for dy in range(-3, 5):
            taps[np.clip(p[:, 1] + dy, 0, h - 1), np.clip(p[:, 0] + dx, 0, w - 1)] = True
    free = np.argwhere(~taps)
    assert len(free), "no pixel far from every point"
    nan_far = base.copy()
    nan_far[free[0][0], free[0][1]] = np.nan
    nan_read = base.copy()
    nan_read[uv[1], uv[0]] = np.nan
    inf = base.copy()
    inf[free[0][0], free[0][1]] = np.inf
    images = np.stack([zero, const, spike, nan_far, nan_read, inf, -base])
    return problem(geo, images, pr["points"], np.arange(len(images)), np.repeat(pr["poses"][:1], len(images), axis=0))


def branch_problems():
    """name -> problem: one per branch of B9 a scene can reach (asserted by tests/test_maptrack_cpu.py)."""
    d = default_opts
    base = lambda **kw: aligned_problem(21, SMALL, 60, 1, n_images=1, opts=d(**kw))
    far = lambda **kw: aligned_problem(22, MID, 120, 1, n_images=1, dt=0.35, dr=0.12, opts=d(**kw))
    # an image that varies along x only: Dv = 0 exactly, the column of the y translation is zero, and without a floor
    # under the damping its pivot is 0: every step is invalid
    one = base()
    stripes = np.repeat(np.exp(-(np.arange(SMALL["w"]) - 18.0) ** 2 / 50.0)[None, :], SMALL["h"], axis=0)
    flat = problem(SMALL, stripes[None], one["points"], [0], one["poses"], opts=d(min_lm_diagonal=0.0))
    flat3 = dict(flat, opts=d(min_lm_diagonal=0.0, max_consecutive_invalid=3))
    return {
        "plain": base(),
        "rej": far(),
        "rej_r16": far(initial_radius=1e16),
        "nonmono": far(initial_radius=1e16, use_nonmonotonic=1),
        "nonmono_m2": far(initial_radius=1e16, use_nonmonotonic=1, max_consecutive_nonmonotonic=2),
        "invalid": flat,
        "invalid3": flat3,
        "it0": base(max_num_iterations=0),
        "it1": base(max_num_iterations=1),
        "minrad": base(initial_radius=1e-33),
        "gtol": base(function_tolerance=0.0, parameter_tolerance=0.0, gradient_tolerance=2.0),
        "ptol": base(function_tolerance=0.0, gradient_tolerance=0.0, parameter_tolerance=1e-4),
        "ftol": base(function_tolerance=1e-3),
        "maxrad": base(initial_radius=5e-3, max_radius=1e-2, function_tolerance=0.0),
        "lmclip": base(min_lm_diagonal=0.1, max_lm_diagonal=0.1, initial_radius=1.0),
        "noscale": base(jacobi_scaling=0),
        "mrd": far(min_relative_decrease=0.5),
    }


POINT_COUNTS = (1, 5, 255, 256, 257, 600)


def size_problems():
    """(geometry name, points, units) -> problem: the tree's partial boundary, lanes with unequal trip counts, one to 70 units."""
    out = {}
    for gname, geo in (("small", SMALL), ("mid", MID)):
        for n in POINT_COUNTS:
            out[(gname, n, 3)] = aligned_problem(100 + n, geo, n, 3, opts=default_opts(max_num_iterations=12))
    out[("small", 40, 1)] = aligned_problem(31, SMALL, 40, 1)
    out[("small", 40, 70)] = aligned_problem(32, SMALL, 40, 70, n_images=5, opts=default_opts(max_num_iterations=10))
    return out


def gpu_problems():
    """Every scene the device is held to, bit for bit: name -> problem."""
    out = {"size_%s_%d_%d" % k: v for k, v in size_problems().items()}
    out.update({"branch_" + k: v for k, v in branch_problems().items()})
    out["border"] = border_problem()
    out["visibility"] = visibility_problem()
    out["degenerate"] = degenerate_problem()
    return out
