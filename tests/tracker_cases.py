"""The inputs of the tracker-layer shape and edge tests (tests/test_gpu_tracker_shapes.py), shared with the CPU tests
that check the oracle against second restatements on them (tests/test_tracker_cases_cpu.py): a gradient grid that does
not vanish at the border, patch shapes at which the lane strides and the reductions of csrc/ebo_optimizer.inc change,
solve problems built by the rule of test_optimizer._batch, poses that put samples exactly on the edges of the functor's
inside test and of the bicubic clamps, images smaller than the 4x4 neighbourhood, and rects / warps for the two
nearest-neighbour map kernels (k_estimate_num_events, k_patch_warp_image).  All deterministic.  A plain module, not a
conftest; it needs no GPU.

Out of scope: translations beyond +-2^20.  The 10-bit map forms int(rint(t * 1024)); past 2^31 / 1024 = 2^21 that is
the conversion of an out-of-range double, which neither the restatement (lrint) nor the kernel (static_cast<int>)
defines.  The map cases stop at +-1e5 (1024 t < 1.1e8, far inside int)."""
import math

import numpy as np

from test_optimizer import pose_of

W, H = 64, 48


def gradient_grid():
    """[H][W][2]: white noise smoothed circularly with the binomial [1 4 6 4 1] / 16 along both axes, the 4 px margin
    cut off, times 3.  Mean |g| 0.70 on the first row, 0.58 on the first column, 0.64 overall: a clamp that is off by
    one at a border changes values of the size of the patch's maximum."""
    g = np.random.default_rng(7).normal(0.0, 1.0, (H + 8, W + 8, 2))
    k = np.array([1.0, 4.0, 6.0, 4.0, 1.0]) / 16.0
    for axis in (0, 1):
        g = sum(k[i] * np.roll(g, i - 2, axis=axis) for i in range(5))
    return np.ascontiguousarray(g[4:-4, 4:-4] * 3.0)


# (pw, ph): the smallest shapes at which the strides over 64 / 128 / 192 / 256 lanes and the wave reductions change
SHAPES = [(1, 1), (3, 3), (8, 8), (13, 5), (11, 11), (16, 8), (43, 3), (17, 15), (16, 16), (1, 40), (40, 1),
          (25, 25), (21, 27), (40, 33), (37, 37), (54, 55), (60, 50)]
REFUSED_SHAPE = (55, 55)                                # 3025 pixels: EBO_ERR_UNSUPPORTED
BIG_SHAPES = [(40, 33), (37, 37), (54, 55), (60, 50)]   # 64 KB, the first above it, ..., the admitted 3000 pixels
MAX_PIXELS = 3000


def lds_bytes(pw, ph):
    """optimizer_lds_bytes of ebo_kernels.hip: 128 reduction doubles + p and five derivatives per pixel"""
    return (128 + 6 * pw * ph) * 8


def _item(rect, pose, flow, seed, **kw):
    pw, ph = int(rect[2]), int(rect[3])
    raw = np.random.default_rng([1234, seed]).integers(-3, 4, (ph, pw)).astype(np.float64) + 0.25
    return dict(rect=tuple(float(v) for v in rect), pose=np.asarray(pose, dtype=np.float64), flow=float(flow), raw=raw, **kw)


def _corner(rng, room):
    """uniform(-3, room + 3): up to 3 px over either border (a patch larger than the image: the ends in order)"""
    lo, hi = sorted((-3.0, room + 3.0))
    return float(rng.uniform(lo, hi))


def shape_items():
    """One patch of every admitted shape on the W x H grid.  Every fourth rect has a fractional corner, every third a
    fractional size (optimizer_stage truncates it); small rotations, so that samples are off the grid."""
    rng = np.random.default_rng(41)
    out = []
    for i, (pw, ph) in enumerate(SHAPES):
        x0 = float(np.floor(_corner(rng, W - pw)))
        y0 = float(np.floor(_corner(rng, H - ph)))
        if i % 4 == 0:
            x0, y0 = x0 + 0.37, y0 - 0.21
        fw, fh = (pw + 0.9, ph + 0.9) if i % 3 == 1 else (float(pw), float(ph))
        pose = pose_of(float(rng.uniform(-0.08, 0.08)), float(rng.uniform(-1.5, 1.5)), float(rng.uniform(-1.5, 1.5)))
        if (pw, ph) == (1, 1):
            x0, y0 = 30.37, 20.79    # its one sample inside the image
        if (pw, ph) == (60, 50):
            pose[:2] *= 1.25         # 60 < W: a scaled rotation (the functor takes any complex number) spreads the samples
            pose[2:] = (-3.0, -2.0)  # over all four borders
        out.append(_item((x0, y0, fw, fh), pose, float(rng.uniform(-7, 7)), 100 + i, name="%dx%d" % (pw, ph)))
    return out


def big_item(pw, ph):
    return next(it for it in shape_items() if it["name"] == "%dx%d" % (pw, ph))


def refused_item():
    pw, ph = REFUSED_SHAPE
    return _item((2.0, -3.0, float(pw), float(ph)), pose_of(0.01, 0.5, 0.5), 0.4, 99, name="55x55")


def small_item():
    """The 3x3 patch that shares a call with the large ones and follows a refused call"""
    return big_item(3, 3)


# ---- border samples for the functor -------------------------------------------------------------------------------
_WL, _HL = math.nextafter(float(W), 0.0), math.nextafter(float(H), 0.0)
IDENT = (1.0, 0.0, 0.0, 0.0)


def border_items():
    """4x3 patches (non-square, under one wave) whose samples sit on the edges of `wx >= imgW || wy >= imgH || wx < 0 ||
    wy < 0` and of the 4x4 clamps.  Every pose is exact in floating point: wx, wy of a case are what its name says, with
    no rounding.  `inside`: the number of samples inside the image, by hand."""
    out = []
    n = [0]

    def add(name, corner, pose, inside, flow=0.6, size=(4.0, 3.0)):
        n[0] += 1
        out.append(_item((corner[0], corner[1], size[0], size[1]), pose, flow, 200 + n[0], name=name, inside=inside))

    # identity: wx = px + x0 (px = 0..3), wy = py + y0 (py = 0..2)
    add("corner 0", (0.0, 0.0), IDENT, 12)
    add("corner -0.0", (-0.0, -0.0), IDENT, 12)
    add("corner -1", (-1.0, -1.0), IDENT, 3 * 2)                    # column -1 and row -1 outside
    add("corner W-1", (W - 1.0, H - 1.0), IDENT, 1)                 # only (W-1, H-1)
    add("corner W-2", (W - 2.0, H - 2.0), IDENT, 2 * 2)
    add("corner -0.5", (-0.5, -0.5), IDENT, 3 * 2)                  # -0.5 outside, 0.5 .. 2.5 in the clamped first cell
    add("corner W-1.5", (W - 1.5, H - 1.5), IDENT, 2 * 2)           # W-1.5 and W-0.5 inside, W+0.5 outside
    add("corner W-2.5", (W - 2.5, H - 2.5), IDENT, 3 * 3)
    # the last representable value below W (resp. H) at px = 2 (py = 1): px = 3 (py = 2) is outside by one ulp of W
    add("last below W", (_WL - 2.0, _HL - 1.0), IDENT, 3 * 2)
    add("last below W, y inside", (_WL - 2.0, 20.0), IDENT, 3 * 3)
    add("last below H, x inside", (30.0, _HL - 1.0), IDENT, 4 * 2)
    # exact turns, integer corners and translations: every wx, wy is an integer
    #   quarter turn (0, 1): wx = tx - Y, wy = X + ty
    add("quarter turn on the border", (0.0, 0.0), (0.0, 1.0, 2.0, -1.0), 3 * 3)        # wx = 2,1,0; wy = -1,0,1,2
    add("quarter turn at W", (0.0, 0.0), (0.0, 1.0, float(W), H - 2.0), 2 * 2)         # wx = W,W-1,W-2; wy = H-2..H+1
    #   half turn (-1, 0): wx = tx - X, wy = ty - Y
    add("half turn on the border", (0.0, 0.0), (-1.0, 0.0, 2.0, 1.0), 3 * 2)           # wx = 2,1,0,-1; wy = 1,0,-1
    add("half turn, -0.0", (0.0, 0.0), (-1.0, 0.0, -0.0, -0.0), 1)                     # wx = -0.0 at X = 0: inside
    add("half turn at W", (1.0, 1.0), (-1.0, 0.0, W + 1.0, H + 1.0), 3 * 2)            # wx = W..W-3, wy = H..H-2
    #   three-quarter turn (0, -1): wx = Y + tx, wy = ty - X
    add("three-quarter turn on the border", (0.0, 0.0), (0.0, -1.0, -1.0, 2.0), 2 * 3)  # wx = -1,0,1; wy = 2,1,0,-1
    add("three-quarter turn at W", (0.0, 0.0), (0.0, -1.0, W - 2.0, H + 1.0), 2 * 2)    # wx = W-2,W-1,W; wy = H+1..H-2
    # all samples in the first cell [0, 1) and in the last two columns / rows [W - 2, W): scaled identities (the functor
    # does not ask for a unit complex number), exact binary fractions
    add("all in [0, 1)", (0.0, 0.0), (0.25, 0.0, 0.125, 0.25), 12)                      # wx = .125 .. .875, wy = .25 .. .75
    add("all in [W-2, W)", (0.0, 0.0), (0.5, 0.0, W - 1.875, H - 1.75), 12)             # wx = W-1.875 .. W-.375
    return out


TINY_IMAGES = [(1, 1), (2, 3), (3, 2), (4, 4)]   # (w, h): smaller than, or just, the 4x4 neighbourhood


def tiny_grid(w, h):
    return np.random.default_rng([11, w, h]).normal(0.0, 1.0, (h, w, 2))


def tiny_items(w, h):
    """A rect one pixel larger than the image all round; off-grid samples, so that every tap of every sample clamps (and
    both ends of a row of taps clamp at once)."""
    rect = (-1.0, -1.0, w + 2.0, h + 2.0)
    poses = [IDENT, (1.0, 0.0, 0.5, 0.25), (1.0, 0.0, -0.25, 0.75), tuple(pose_of(0.3, 0.4, -0.2)), (0.5, 0.0, 0.75, 0.625)]
    return [_item(rect, p, 0.9 + k, 300 + 10 * w + h + 100 * k, name="%dx%d image, pose %d" % (w, h, k))
            for k, p in enumerate(poses)]


def inside_count(item, w=W, h=H):
    """The functor's inside test in exact rational arithmetic (fractions): what `inside` states, recomputed"""
    from fractions import Fraction as F
    c, s, tx, ty = (F(float(v)) for v in item["pose"])
    x0, y0 = F(item["rect"][0]), F(item["rect"][1])
    n = 0
    for py in range(int(item["rect"][3])):
        for px in range(int(item["rect"][2])):
            X, Y = px + x0, py + y0
            wx, wy = c * X - s * Y + tx, s * X + c * Y + ty
            n += int(0 <= wx < w and 0 <= wy < h)
    return n


# ---- solve problems -----------------------------------------------------------------------------------------------
N_SOLVE = 512
# The problems (by index) that fail the admission gate of test_gpu_optimizer_branches (the oracle's own summary moves
# when the nabla moves by 1e-12 relative): none.  tests/test_tracker_cases_cpu.py recomputes the list and compares.
DROPPED = ()

_solve_cache = {}


def solve_problems(orc, n=N_SOLVE):
    """n problems on the W x H grid by the rule of test_optimizer._batch, the shapes cycling through SHAPES: nabla =
    -prediction at a true warp x 40 + N(0, 0.02) noise (normalised), start = a small rotation and the flow +- 0.3,
    corners in uniform(-3, W - pw + 3) so that patches hang over the border."""
    if n in _solve_cache:
        return _solve_cache[n]
    grad = gradient_grid()
    rng = np.random.default_rng(20)
    items = []
    for i in range(n):
        pw, ph = SHAPES[i % len(SHAPES)]
        rect = (_corner(rng, W - pw), _corner(rng, H - ph), float(pw), float(ph))
        if i % 4 == 0:
            rect = (np.floor(rect[0]) + 0.37, np.floor(rect[1]) - 0.21, float(pw), float(ph))
        theta = float(rng.uniform(-0.06, 0.06))
        t = (float(rng.uniform(-1.2, 1.2)), float(rng.uniform(-1.2, 1.2)))
        flow = float(rng.uniform(0, 2 * np.pi))
        zero = np.zeros((ph, pw))
        pred, _, _ = orc.optimizer_cost(grad, rect, zero, pose_of(theta, *t), flow, want_jac=False)
        raw = (-pred).reshape(zero.shape) * 40 + rng.normal(0, 0.02, zero.shape)
        items.append(dict(rect=rect, raw=raw, nabla=orc.normalize_nabla(raw), shape=(pw, ph),
                          start=(pose_of(float(rng.uniform(-0.02, 0.02)), 0.0, 0.0), flow + float(rng.uniform(-0.3, 0.3)))))
    _solve_cache[n] = items
    return items


def kept_problems(orc):
    return [it for i, it in enumerate(solve_problems(orc)) if i not in DROPPED]


_oracle_cache = {}


def oracle_solves(orc):
    """-> per kept problem (pose, flow, (iterations, termination, evals cost, evals jac, initial cost, final cost)), once"""
    if "s" not in _oracle_cache:
        grad = gradient_grid()
        out = []
        for it in kept_problems(orc):
            p, f, s = orc.optimizer_solve(grad, it["rect"], it["nabla"], it["start"][0], it["start"][1])
            out.append((p, f, (s.iterations, s.termination, s.num_evals_cost, s.num_evals_jac, s.initial_cost, s.final_cost)))
        _oracle_cache["s"] = out
    return _oracle_cache["s"]


# ---- the nearest-neighbour maps -----------------------------------------------------------------------------------
def map_grid():
    return np.random.default_rng(9).normal(0.0, 1.5, (H, W, 2))


QUARTER_TURNS = [(1.0, 0.0), (0.0, 1.0), (-1.0, 0.0), (0.0, -1.0)]
MAP_RECTS_INSIDE = [(10.0, 8.0, 7.0, 13.0), (10.0, 8.0, 13.0, 7.0), (31.0, 17.0, 1.0, 1.0), (5.0, 3.0, 1.0, 40.0),
                    (3.0, 5.0, 40.0, 1.0), (20.0, 11.0, 25.0, 25.0)]
# partly outside the image, or touching its border: patch_warp_image skips these (its border test), the estimate does not
MAP_RECTS_OUTSIDE = [(0.0, 0.0, 64.0, 48.0), (-3.0, -2.0, 13.0, 7.0), (58.0, 40.0, 7.0, 13.0), (-5.0, 44.0, 13.0, 7.0),
                     (60.0, -6.0, 7.0, 13.0)]
# exact .5 corners and sizes: cv::Rect2d -> cv::Rect rounds half to even (10, 12, 6, 8 and 11, 12, 8, 6)
MAP_RECTS_HALF = [(10.5, 11.5, 6.5, 7.5), (11.5, 12.5, 7.5, 5.5)]


def exact_map_cases():
    """(rect, pose, flow) with the identity or an exact quarter / half turn and integer translations: the fixed-point
    map is exact, X = c x - s y + tx, Y = s x + c y + ty, and a direct loop is a second restatement"""
    out = []
    shifts = [(0, 0), (3, -2), (63, 47), (-7, 50), (20, 10)]
    k = 0
    for rect in MAP_RECTS_INSIDE + MAP_RECTS_OUTSIDE + MAP_RECTS_HALF:
        cx, cy = int(rect[0] + rect[2] / 2), int(rect[1] + rect[3] / 2)
        for c, s in QUARTER_TURNS:
            c, s = int(c), int(s)
            # the turn about the rect's centre pixel, then a shift: some stay on the image, some leave it in part or whole
            ox, oy = cx - (c * cx - s * cy), cy - (s * cx + c * cy)
            for dx, dy in shifts[k % 2::2] + [((k * 7) % 23 - 11, (k * 5) % 17 - 8)]:
                out.append((rect, np.array([float(c), float(s), float(ox + dx), float(oy + dy)]), 0.3 + 0.37 * k))
                k += 1
    return out


def tie_cases():
    """(rect, pose, flow, (dx, dy)): identity rotation, translations at the rounding ties of the 10-bit map and at its
    floor.  dx, dy: the integer source shift, floor((rint(1024 t) + 512) / 1024) with rint to even.
      t = (2k + 1) / 2048: 1024 t = k + 1/2 exactly.  k = 511 -> 512 (even) -> shift 1; k = 510 -> 510 -> shift 0;
      k = 512 -> 512 -> 1; k = -513: -512.5 -> -512 -> shift 0 (away from zero would give -1); k = -512: -511.5 -> -512
      -> 0; k = 1535 -> 1536 -> 2; k = -1537: -1536.5 -> -1536 -> -1."""
    out = []
    rect = (20.0, 11.0, 13.0, 7.0)
    for i, k in enumerate((511, 510, 512, -513, -512, 1535, -1537, 4, 5, -4, -5)):
        t = (2 * k + 1) / 2048.0
        d = (int(round(t * 1024.0)) + 512) // 1024   # Python's round(): half to even; //: floor
        out.append((rect, np.array([1.0, 0.0, t, 0.0]), 0.7 + i, (d, 0)))
        out.append((rect, np.array([1.0, 0.0, 0.0, t]), 0.2 + i, (0, d)))
    return out


def floor_cases():
    """Identity rotation, fractional translations that leave the fixed-point source coordinate of the rect's first column
    (row) in (-1, 0) -- `>> 10` gives -1, outside; a division would give 0, inside -- and of its last column (row) in
    [W - 1, W) resp. just past it.  (rect, pose, flow, (dx, dy)) with the integer shift as in tie_cases."""
    out = []
    rect = (20.0, 11.0, 13.0, 7.0)
    for i, frac in enumerate((-0.7, -0.9, -0.51, -1.2)):
        for axis in (0, 1):
            t = -(rect[axis]) + frac   # the first column / row reads from frac: rounds to -1 (frac = -1.2: -1, too)
            d = (int(round(t * 1024.0)) + 512) // 1024
            pose = np.array([1.0, 0.0, t if axis == 0 else 0.0, t if axis == 1 else 0.0])
            out.append((rect, pose, 1.1 + i + axis, (d, 0) if axis == 0 else (0, d)))
    for i, frac in enumerate((0.3, 0.49, 0.6)):
        for axis in (0, 1):
            last = rect[axis] + rect[2 + axis] - 1
            t = ((W, H)[axis] - 1 - last) + frac   # the last column / row reads from W - 1 + frac
            d = (int(round(t * 1024.0)) + 512) // 1024
            pose = np.array([1.0, 0.0, t if axis == 0 else 0.0, t if axis == 1 else 0.0])
            out.append((rect, pose, 2.3 + i + axis, (d, 0) if axis == 0 else (0, d)))
    return out


def random_map_cases():
    """Rotations over (-pi, pi], translations up to +-1e5, every rect"""
    rng = np.random.default_rng(77)
    rects = MAP_RECTS_INSIDE + MAP_RECTS_OUTSIDE + MAP_RECTS_HALF
    out = []
    for i in range(78):
        rect = rects[i % len(rects)]
        th = float(rng.uniform(-np.pi, np.pi)) if i % 13 else np.pi
        span = (4.0, 40.0, 12.0, 25.0, 4.0, 40.0, 1e3, 1e5)[i % 8]
        t = rng.uniform(-span, span, 2)
        if i % 8 < 6:   # keep the rect's centre near the image: rotate about it, then shift
            cx, cy = rect[0] + rect[2] / 2, rect[1] + rect[3] / 2
            t = np.array([cx - (np.cos(th) * cx - np.sin(th) * cy), cy - (np.sin(th) * cx + np.cos(th) * cy)]) + t * 0.2
        out.append((rect, np.array([np.cos(th), np.sin(th), t[0], t[1]]), float(rng.uniform(-7, 7))))
    out.append((rects[5], np.array([1.0, 0.0, 1e5, -1e5]), 0.5))
    out.append((rects[5], np.array([1.0, 0.0, -1e5, 1e5]), 0.5))
    return out


def map_cases():
    """Every (rect, pose, flow) that goes to estimate_num_events and patch_warp_image"""
    return ([c[:3] for c in exact_map_cases()] + [c[:3] for c in tie_cases()] + [c[:3] for c in floor_cases()]
            + random_map_cases())


def rint_even(v):
    return int(round(v))  # Python's round() on a float: half to even, as lrint / rint in the default rounding mode


def direct_map(grad, rect, pose, shift=None):
    """The warped gradient over the rect, [h][w][2], by a direct loop.  pose = the identity or an exact turn with integer
    translations (shift None): X = c x - s y + tx in integers.  shift = (dx, dy): identity rotation, X = x + dx."""
    x0, y0, w, h = (rint_even(v) for v in rect)
    Hh, Ww = grad.shape[:2]
    c, s = int(pose[0]), int(pose[1])
    if shift is None:
        assert (float(c), float(s)) == (pose[0], pose[1]) and c * c + s * s == 1
        tx, ty = int(pose[2]), int(pose[3])
        assert (float(tx), float(ty)) == (pose[2], pose[3])
    else:
        assert (c, s) == (1, 0)
        tx, ty = shift
    out = np.zeros((h, w, 2))
    for y in range(y0, y0 + h):
        for x in range(x0, x0 + w):
            X, Y = c * x - s * y + tx, s * x + c * y + ty
            if 0 <= x < Ww and 0 <= y < Hh and 0 <= X < Ww and 0 <= Y < Hh:   # the warped image is image-sized
                out[y - y0, x - x0] = grad[Y, X]
    return out


def direct_estimate_sum(grad, rect, pose, flow, shift=None):
    """The extension of test_num_events.direct to the exact turns and to a stated shift: the double sum (row-major)"""
    g = direct_map(grad, rect, pose, shift)
    a = 0.6 * float(np.cos(np.float32(flow)))
    b = 0.6 * float(np.sin(np.float32(flow)))
    s = 0.0
    for v in np.abs(g[..., 0] * a + g[..., 1] * b).ravel():
        s += float(v)
    return s


def fixed_point_sum(grad, rect, pose, flow):
    """The estimate's double sum through the 10-bit fixed-point map for ANY pose, in Python integers (row-major)"""
    x0, y0, w, h = (rint_even(v) for v in rect)
    Hh, Ww = grad.shape[:2]
    c, s, tx, ty = (float(v) for v in pose)
    a = 0.6 * float(np.cos(np.float32(flow)))
    b = 0.6 * float(np.sin(np.float32(flow)))
    tot = 0.0
    for y in range(y0, y0 + h):
        X0 = rint_even((-s * y + tx) * 1024.0) + 512
        Y0 = rint_even((c * y + ty) * 1024.0) + 512
        for x in range(x0, x0 + w):
            X = (X0 + rint_even(c * x * 1024.0)) >> 10   # Python's >> on a negative int is the arithmetic shift
            Y = (Y0 + rint_even(s * x * 1024.0)) >> 10
            if 0 <= x < Ww and 0 <= y < Hh and 0 <= X < Ww and 0 <= Y < Hh:
                tot += abs(grad[Y, X, 0] * a + grad[Y, X, 1] * b)
    return tot


# rects no entry has an answer for: EBO_ERR_RANGE from ebo_estimate_num_events and ebo_patch_warp_image
BAD_MAP_RECTS = [(10.0, 10.0, -25.0, -25.0), (10.0, 10.0, -1.0, 5.0), (10.0, 10.0, 5.0, 32768.0),
                 (10.0, 10.0, float("nan"), 5.0), (10.0, 10.0, 5.0, float("inf")), (float("nan"), 10.0, 5.0, 5.0),
                 (10.0, float("inf"), 5.0, 5.0), (float("-inf"), 10.0, 5.0, 5.0)]

# ---- the normalisation --------------------------------------------------------------------------------------------
NORMALIZE_SHAPES = [(1, 1), (8, 8), (13, 5), (16, 16), (257, 1), (60, 50)]   # 1, 64, 65, 256, 257, 3000 pixels
