"""The inputs of the objective sweep (tests/test_gpu_eval_sweep.py), shared with the CPU tests that check the
oracle against a second restatement on them (tests/test_eval_consts_cpu.py): functor constants away from the
reference's defaults, pixel pile-ups around the wrap count of the fixed-point value image, and patch shapes
from 1x1 to remainder patches.  All deterministic.  A plain module, not a conftest."""
import math

import numpy as np

# sigma_compensate values: the library-exp path (sigma < 1, outer taps below the fixed-point grid), 1/sqrt(pi) +- one
# ulp (norm = 1/(2 pi sigma^2) crosses 0.5: the fixed-point exponent steps), the switch between the two exp paths at
# sigma = 1, and large sigma (nearly flat taps far below the fixed-point grid's top)
_RSQRT_PI = 1.0 / math.sqrt(math.pi)
SIGMAS = [0.25, 0.5, math.nextafter(_RSQRT_PI, 0.0), _RSQRT_PI, math.nextafter(_RSQRT_PI, 1.0), 0.75,
          math.nextafter(1.0, 0.0), 1.0, math.nextafter(1.0, 2.0), 1.5, 4.0, 30.0, 1e3]
# the sigma_compensate and sigma_st ranges ebo_create admits (include/ebo.h): the ranges this sweep covers
SIGMA_MIN, SIGMA_MAX = 0.25, 1e3
SIGMA_ST_MIN, SIGMA_ST_MAX = 1.0, 10.0
SIGMA_STS = [1.0, 1.5, 3.0, 10.0]
MAX_RESIDUALS = [1.0, 1e3, 1e6]
SCALES = [1e-6, 1e-3, 0.1]
FD_STEPS = [1e-8, 1e-6, 1e-3]
PILE_SIGMAS = [1.0, 0.5, 0.25]
PILE_FACTORS = [0.99, 1.01, 4.0]
PILE_SPREADS = [0, 2]

# the window geometry: 61 x 43 pixels in 20 x 20 patches = a 3 x 2 grid whose last column is 21 wide and whose
# last row is 23 high (feature_detector.cpp:332-346): regular, remainder-column, remainder-row and corner patches
IMAGE_W, IMAGE_H, PATCH = 61, 43, 20
T_END = 20000        # every patch has an event at t = 0 and at t = T_END: reference time 10000 us everywhere
T_EDGE = 9000        # events 1 ms (at scale 1e-3) before the reference time: the warped fraction follows the flow
PILE_XY = (10, 10)   # the pile-up pixel, inside patch 0
PILE_T = 4000


def norm_of(sigma):
    return 1.0 / ((2 * math.pi) * (sigma * sigma))


def fixed_exponent(sigma):
    """The fixed-point exponent k of the value image for this sigma (ebo_api.cpp make_consts): the least k >= 0
    with norm < 2^(k-1).  A pixel of the image holds values below 2^(12+k)."""
    k = 0
    while norm_of(sigma) >= math.ldexp(0.5, k):
        k += 1
    return k


def unit_exponent(sigma, n_ev):
    """The exponent a unit of n_ev events gets (unit_fix_grid in ebo_kernels.hip): n_ev * norm < 2^(11 + k)."""
    k = fixed_exponent(sigma)
    while n_ev * norm_of(sigma) >= math.ldexp(1.0, 11 + k):
        k += 1
    return k


def wrap_count(sigma):
    """Events on one pixel, each adding its central tap (= norm at zero fraction), that fill 2^(12+k)."""
    return int(math.ldexp(1.0, 12 + fixed_exponent(sigma)) / norm_of(sigma))


class Case:
    def __init__(self, name, sigma=1.0, sigma_st=1.5, max_res=1e3, scale=1e-3, fd_step=None, pile=None,
                 spread=0, seed=0):
        self.name, self.sigma, self.sigma_st, self.max_res = name, sigma, sigma_st, max_res
        self.scale, self.fd_step, self.pile, self.spread, self.seed = scale, fd_step, pile, spread, seed

    def __repr__(self):
        return self.name

    def ctx_kw(self, ebo, loss):
        """ebo.Context keyword arguments (functor constants set afterwards by apply_consts)."""
        kw = dict(image_w=IMAGE_W, image_h=IMAGE_H, patch_w=PATCH, patch_h=PATCH, scale=self.scale, tv_weight=0.0,
                  loss=loss, max_events=1 << 20)
        if self.fd_step is not None:
            kw.update(grad=ebo.GRAD_CENTRAL, fd_step=self.fd_step)
        return kw

    def apply_consts(self, k):
        """Fill an ebo_functor_consts / orc FunctorConsts in place."""
        k.sigma_compensate = self.sigma
        k.sigma_st = self.sigma_st
        k.max_possible_residual = self.max_res
        return k

    def params(self, ebo, loss):
        p = ebo.default_params(**self.ctx_kw(ebo, loss))
        self.apply_consts(p.k)
        return p

    def oparams(self, orc, loss):
        p = orc.default_params(image_w=IMAGE_W, image_h=IMAGE_H, patch_w=PATCH, patch_h=PATCH, scale=self.scale,
                               tv_weight=0.0, loss=loss)
        self.apply_consts(p.k)
        return p

    def consts(self, orc):
        return self.apply_consts(orc.default_consts())

    def with_max_res(self, max_res):
        c = Case(self.name, self.sigma, self.sigma_st, max_res, self.scale, self.fd_step, self.pile, self.spread,
                 self.seed)
        return c

    def edge_flow(self):
        """A flow that moves the T_EDGE events by one pixel minus 1e-7: warped fractions of +-(1 - 1e-7)."""
        return (1.0 - 1e-7) / (1000.0 * self.scale)


def _cases():
    out = [Case("sigma=%r" % s, sigma=s, seed=i) for i, s in enumerate(SIGMAS)]
    out += [Case("sigma_st=%r" % s, sigma_st=s, seed=100 + i) for i, s in enumerate(SIGMA_STS)]
    out += [Case("max_res=%r" % m, max_res=m, seed=200 + i) for i, m in enumerate(MAX_RESIDUALS)]
    out += [Case("scale=%r" % s, scale=s, seed=300 + i) for i, s in enumerate(SCALES)]
    out += [Case("fd_step=%r" % h, fd_step=h, seed=400 + i) for i, h in enumerate(FD_STEPS)]
    for s in PILE_SIGMAS:
        for f in PILE_FACTORS:
            for sp in PILE_SPREADS:
                out.append(Case("pile sigma=%r N=%.2fx spread=%d" % (s, f, sp), sigma=s,
                                pile=int(round(f * wrap_count(s))), spread=sp, seed=500))
    return out


CASES = _cases()
CASE_IDS = [c.name for c in CASES]


def grid_rects():
    rects = []
    for py in range(IMAGE_H // PATCH):
        for px in range(IMAGE_W // PATCH):
            w = IMAGE_W - px * PATCH if px == IMAGE_W // PATCH - 1 else PATCH
            h = IMAGE_H - py * PATCH if py == IMAGE_H // PATCH - 1 else PATCH
            rects.append((px * PATCH, py * PATCH, w, h))
    return rects


def _patch_events(rng, rect, n, margin=0):
    """n events in rect (+ margin), first at t = 0 and last at T_END, T_EDGE events on the rect's left column
    and top row (x or y = 0 at the image origin: warped coordinates in (-1, 0) there)."""
    x, y, w, h = rect
    ex = rng.integers(max(x - margin, 0), x + w + margin, n)
    ey = rng.integers(max(y - margin, 0), y + h + margin, n)
    t = np.sort(rng.integers(1, T_END, n))
    t[0], t[-1] = 0, T_END
    k = min(24, n - 2)
    sel = rng.choice(np.arange(1, n - 1), k, replace=False)
    t[sel] = T_EDGE
    ex[sel[: k // 2]] = x
    ey[sel[k // 2:]] = y
    o = np.argsort(t, kind="stable")
    return ex[o], ey[o], t[o]


def window(case, orc):
    """The sorted window of the case: a few hundred events per grid patch, the pile-up (if any) in patch 0."""
    rng = np.random.default_rng(case.seed)
    xs, ys, ts = [], [], []
    for rect in grid_rects():
        x, y, t = _patch_events(rng, rect, int(rng.integers(150, 320)))
        xs.append(x), ys.append(y), ts.append(t)
    if case.pile:
        n, s = case.pile, case.spread
        xs.append(PILE_XY[0] + rng.integers(-s, s + 1, n))
        ys.append(PILE_XY[1] + rng.integers(-s, s + 1, n))
        ts.append(np.full(n, PILE_T))
    x, y, t = np.concatenate(xs), np.concatenate(ys), np.concatenate(ts)
    o = np.argsort(t, kind="stable")
    sign = np.where(rng.random(len(t)) < 0.5, -1, 1)
    return orc.make_events(x[o], y[o], t[o], sign[o])


def patch_rects():
    """ebo_set_patches rects: 1x1 and 1xN at the origin, 1x1 inside, a regular 20 x 20 and a 13 x 23 one."""
    return [(0, 0, 1, 1), (0, 0, 1, 9), (30, 17, 1, 1), (7, 11, 20, 20), (40, 5, 13, 23)]


def patch_lists(case, orc):
    """(events, offsets, rects) for ebo_set_patches: each rect with its own list of events around it."""
    rng = np.random.default_rng(case.seed + 7)
    evs, offs = [], [0]
    for rect in patch_rects():
        x, y, t = _patch_events(rng, rect, int(rng.integers(120, 260)), margin=3)
        sign = np.where(rng.random(len(t)) < 0.5, -1, 1)
        evs.append(orc.make_events(x, y, t, sign))
        offs.append(offs[-1] + len(t))
    return evs, offs, patch_rects()


def flow_sets(case, n):
    """Flows per patch at which every case is evaluated, none exactly zero (edge-loss ties, test_gpu_random.py):
    random ones, and +-(1 pixel - 1e-7) for the T_EDGE events in alternating signs."""
    rng = np.random.default_rng(case.seed + 11)
    f1 = rng.uniform(-1.2, 1.2, (n, 2))
    f1[np.abs(f1) < 1e-3] = 1e-3
    e = case.edge_flow()
    f2 = np.array([[e, -e], [-e, e], [e, e], [-e, -e]] * (n // 4 + 1))[:n]
    return [f1, f2]
