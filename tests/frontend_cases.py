"""The inputs of the image front end sweep (tests/test_gpu_front_end_sweep.py), shared with the CPU test that
runs them through the instrumented restatement (tests/test_front_end_cpu.py): images, masks, parameter sets and
point sets, all deterministic.  A plain module, not a conftest."""
import functools
import math

import numpy as np

import frontend_ref as F

# ---- images ------------------------------------------------------------------------------------------------
GRADIENT_SIZES = [(1, 1), (1, 9), (9, 1), (2, 2), (2, 3), (3, 2), (31, 7), (32, 8), (33, 9), (65, 17), (640, 480),
                  (4100, 3), (3, 4100)]  # (w, h)
GRADIENT_CONTENTS = ("random", "extremes", "constant", "fixture")


def random_image(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(h, w), dtype=np.uint8)


def extremes_image(w, h, seed):
    return (np.random.default_rng(seed).integers(0, 2, size=(h, w)) * 255).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _frames():
    return F.frames()


def fixture_image(w, h, k=0):
    """Fixture frame k tiled (and cropped) to [h][w]."""
    f = _frames()[k]
    return np.ascontiguousarray(np.tile(f, (-(-h // f.shape[0]), -(-w // f.shape[1])))[:h, :w])


@functools.lru_cache(maxsize=None)
def _textured(w, h, seed, sigma):
    return F.textured(h, w, seed=seed, sigma=sigma)


def textured_image(w, h, seed, sigma=1.5):
    return _textured(w, h, seed, sigma)[32:32 + h, 32:32 + w].copy()


def checker(w, h, period, lo=0, hi=255):
    yy, xx = np.indices((h, w))
    return np.where(((xx // period) + (yy // period)) % 2 == 1, hi, lo).astype(np.uint8)


def edge_image(w, h, seed):
    """Texture in the top third, a straight vertical step at x = w // 2 below it."""
    img = np.where(np.arange(w)[None, :] >= w // 2, 200, 30).repeat(h, axis=0).astype(np.uint8)
    top = max(1, h // 3)
    img[:top] = random_image(w, top, seed)
    return img


def gradient_image(content, w, h, seed):
    if content == "random":
        return random_image(w, h, seed)
    if content == "extremes":
        return extremes_image(w, h, seed)
    if content == "constant":
        return np.full((h, w), 77, np.uint8)
    return fixture_image(w, h, seed % 3)


def gradient_cases():
    for i, (w, h) in enumerate(GRADIENT_SIZES):
        for j, content in enumerate(GRADIENT_CONTENTS):
            yield "%s %dx%d" % (content, w, h), gradient_image(content, w, h, 100 * i + j)
    for k in range(3):
        yield "frame%d" % k, _frames()[k]


# ---- corners -----------------------------------------------------------------------------------------------
BLOCK_SIZES = (1, 2, 3, 4, 5, 6, 7)
HARRIS_KS = (0.04, 0.0, -0.04, 0.25)
QUALITY_LEVELS = (0.0, 0.01, 0.5, 1.0)
MIN_DISTANCES = (0.0, 0.5, 1.0, math.sqrt(2.0), 2.0, 10.0, 10.5, 1e9, math.inf)
CORNER_MASKS = ("none", "reference", "zero", "nonbinary", "edge")
CORNER_SIZES = ((3, 3), (4, 4), (17, 17), (240, 180), (640, 480), (4100, 3))  # (w, h)
CORNER_IMAGES = ("random", "textured", "checker4", "checker1", "flat", "fixture")
MAX_CORNERS = (1, 7, 100, 1000, 8192)
N_CORNER_CASES = 126


def corner_image(kind, w, h, seed):
    if kind == "random":
        return random_image(w, h, seed)
    if kind == "textured":
        return textured_image(w, h, seed % 4)
    if kind == "checker4":
        return checker(w, h, 4)  # 0/255: the largest moments (R up to 2.3e14 at block_size 7)
    if kind == "checker1":
        return checker(w, h, 1, 40, 210)  # every Sobel derivative cancels: R == 0
    if kind == "flat":
        return np.full((h, w), 128, np.uint8)
    return fixture_image(w, h, seed % 3)


def corner_mask(kind, w, h, seed):
    if kind == "none":
        return None
    if kind == "reference":
        return F.reference_mask(w, h, max(1, min(12, min(w, h) // 4)))
    if kind == "zero":
        return np.zeros((h, w), np.uint8)
    if kind == "nonbinary":
        return np.random.default_rng(seed).choice(np.array([0, 7, 255], np.uint8), size=(h, w))
    # "edge": over the straight part of edge_image only, where R <= 0 (max R over the mask is not positive)
    m = np.zeros((h, w), np.uint8)
    m[h // 2:, max(0, w // 2 - 3):w // 2 + 3] = 1
    return m


def _cycle(values, n, rng):
    """n values, each of `values` once per len(values) (in a fresh random order each round)."""
    out = []
    while len(out) < n:
        out += [values[k] for k in rng.permutation(len(values))]
    return out[:n]


@functools.lru_cache(maxsize=None)
def _corner_plan():
    rng = np.random.default_rng(20261015)
    dims = [BLOCK_SIZES, HARRIS_KS, QUALITY_LEVELS, MIN_DISTANCES, CORNER_MASKS, CORNER_SIZES, CORNER_IMAGES,
            MAX_CORNERS]
    cols = [_cycle(d, N_CORNER_CASES, rng) for d in dims]
    return list(zip(*cols))


def corner_cases():
    """(name, image, mask, kwargs of good_features): a covering design over every value of every parameter (each
    value appears at least once; the combinations vary).  The "edge" mask comes with edge_image."""
    for i, (bs, k, q, md, mk, (w, h), kind, mc) in enumerate(_corner_plan()):
        img = edge_image(w, h, i) if mk == "edge" else corner_image(kind, w, h, i)
        mask = corner_mask(mk, w, h, i)
        kw = dict(max_corners=mc, quality_level=q, min_distance=md, block_size=bs, harris_k=k)
        name = "%d: %s %dx%d mask=%s %s" % (i, "edge" if mk == "edge" else kind, w, h, mk, kw)
        yield name, img, mask, kw


# selection boundaries: candidate counts around the batch width (64) and the LDS sort limit (4096)
SELECT_COUNTS = (0, 1, 63, 64, 65, 4095, 4096, 4097, 8193)
SELECT_W, SELECT_H = 640, 480


@functools.lru_cache(maxsize=None)
def select_base(kind):
    """The image the selection cases mask down, and its full candidate list (quality_level 0, block_size 3):
    random noise (distinct responses, 17548 candidates) or the 0/255 4-pixel checker (one tied response)."""
    img = random_image(SELECT_W, SELECT_H, 11) if kind == "noise" else checker(SELECT_W, SELECT_H, 4)
    return img, F.candidates(img, None, 0.0, 3, 0.04)


def select_mask(kind, n, seed=0):
    """A mask that leaves exactly n of select_base(kind)'s candidates: with quality_level 0 the threshold does not
    depend on the mask, and neither does the non-maximum suppression, so the candidates are the masked subset."""
    img, cand = select_base(kind)
    keep = np.sort(np.random.default_rng(seed + n).choice(len(cand), size=n, replace=False))
    m = np.zeros(img.size, np.uint8)
    m[cand[keep]] = 1
    return m.reshape(img.shape)


def select_max_corners(n):
    return sorted({v for v in (1, 63, 64, 65, n - 1, n, n + 1, 8192) if 1 <= v <= 8192})


# ---- LK ----------------------------------------------------------------------------------------------------
LK_WINDOWS = ((3, 3), (4, 4), (20, 21), (5, 41), (41, 5), (3, 341), (341, 3), (31, 33), (32, 32))
LK_MAX_LEVELS = (0, 1, 3, 7)
LK_MAX_COUNTS = (1, 2, 30, 100, 1000)
LK_EPSILONS = (0.0, 0.01, 10.0, 100.0)
LK_MIN_EIGS = (0.0, 1e-4, 1e-2, 1e3)


@functools.lru_cache(maxsize=None)
def lk_pair(kind):
    """Image pairs (older, newer), uint8 [h][w]."""
    if kind == "tex640":  # a large shift: the pyramid is needed
        return F.shifted(_textured(640, 480, 21, 2.5), 480, 640, 37.3, -22.6)
    if kind == "tex640s":
        return F.shifted(_textured(640, 480, 22, 2.5), 480, 640, 2.3, -1.1)
    if kind == "noise640":  # unrelated: the iterations wander, out of the level too
        return random_image(640, 480, 31), random_image(640, 480, 32)
    if kind == "small16x12":  # smaller than the window
        return F.shifted(_textured(16, 12, 23, 1.5), 12, 16, 1.0, 0.5)
    if kind == "odd641x479":  # odd sizes: the pyramid rounds up, 8 levels
        return F.shifted(_textured(641, 479, 24, 2.0), 479, 641, 5.5, 3.25)
    if kind == "flat":
        f = np.full((48, 64), 90, np.uint8)
        return f, f.copy()
    if kind == "edge":  # one straight edge: G has rank 1
        a = np.where(np.arange(96)[None, :] >= 40, 180, 40).repeat(72, axis=0).astype(np.uint8)
        return a, np.roll(a, 2, axis=1)
    raise KeyError(kind)


def lk_levels(w, h, win, max_level):
    """The level count ebo_lk_track uses and the level sizes of the pyramid (ebo.h)."""
    sizes = [(w, h)]
    while len(sizes) < 8:
        cw, ch = sizes[-1]
        nw, nh = (cw + 1) // 2, (ch + 1) // 2
        if nw < 2 or nh < 2 or (nw == cw and nh == ch):
            break
        sizes.append((nw, nh))
    n = 1
    while n - 1 < max_level and n < len(sizes) and sizes[n][0] > win[0] and sizes[n][1] > win[1]:
        n += 1
    return n, sizes


def bound_points(w, h, win, max_level):
    """Points whose floor(p) (p = point / 2^l - half) is -win-1, -win, w_l-1 or w_l in x or y, at level 0 and at the
    top level, with fractional parts 0 and .5."""
    n, sizes = lk_levels(w, h, win, max_level)
    hx, hy = (win[0] - 1) * 0.5, (win[1] - 1) * 0.5
    pts = []
    for lvl in sorted({0, n - 1}):
        lw, lh = sizes[lvl]
        s = float(1 << lvl)
        for f in (0.0, 0.5):
            for k in (-win[0] - 1, -win[0], lw - 1, lw):
                pts.append(((k + f + hx) * s, (lh * 0.5 + hy) * s))
            for k in (-win[1] - 1, -win[1], lh - 1, lh):
                pts.append(((lw * 0.5 + hx) * s, (k + f + hy) * s))
    return pts


def special_points(w, h, win):
    """Fractional parts that round weights half to even, far-away points and -0.0."""
    hx, hy = (win[0] - 1) * 0.5, (win[1] - 1) * 0.5
    cx, cy = float(w // 2), float(h // 2)
    pts = []
    for f in (0.5, 0.25, 0.75, 2.0 ** -15, 3 * 2.0 ** -15, 0.5 + 2.0 ** -15):
        pts += [(cx + f + hx, cy + hy), (cx + hx, cy + f + hy), (cx + f + hx, cy + f + hy), (cx + f, cy + 0.25)]
    pts += [(1e6, cy), (-1e6, cy), (cx, 1e9), (-1e9, -1e9), (-0.0, -0.0), (-0.0, cy), (cx, -0.0)]
    return pts


def interior_points(w, h, n, seed):
    rng = np.random.default_rng(seed)
    return list(zip(rng.uniform(0, w, n), rng.uniform(0, h, n)))


# (pair, win, max_level, max_count, epsilon, min_eig_threshold, interior points): every listed value at least once
LK_CONFIGS = (
    ("tex640", (21, 21), 3, 30, 0.01, 1e-4, 32),
    ("tex640", (4, 4), 7, 100, 0.0, 0.0, 24),
    ("tex640", (20, 21), 1, 2, 0.01, 1e-2, 24),
    ("tex640", (31, 33), 3, 1000, 10.0, 1e-4, 16),
    ("tex640", (32, 32), 3, 1, 100.0, 1e-4, 16),
    ("noise640", (21, 21), 3, 100, 0.0, 0.0, 24),
    ("noise640", (5, 41), 1, 30, 0.01, 1e-4, 24),
    ("noise640", (41, 5), 3, 100, 0.01, 0.0, 24),
    ("noise640", (3, 3), 7, 1, 0.01, 1e-4, 32),
    ("noise640", (3, 3), 0, 1, 10.0, 0.0, 32),  # one step out of the level, taken by the epsilon exit
    ("tex640s", (3, 341), 3, 30, 0.01, 1e-4, 16),
    ("tex640s", (341, 3), 0, 30, 0.01, 1e3, 8),
    ("tex640s", (7, 7), 0, 2, 10.0, 0.0, 32),
    ("small16x12", (21, 21), 3, 30, 0.01, 1e-4, 16),
    ("small16x12", (3, 3), 7, 100, 0.0, 0.0, 16),
    ("odd641x479", (3, 3), 7, 30, 0.01, 1e-4, 32),
    ("odd641x479", (20, 21), 7, 1000, 0.0, 1e-2, 16),
    ("flat", (21, 21), 3, 30, 0.01, 1e-4, 8),
    ("edge", (7, 7), 3, 30, 0.01, 0.0, 16),
)


def lk_cases():
    """(name, pair kind, points float32 [n][2], kwargs of lk_track)."""
    for i, (kind, win, ml, mc, eps, me, n_int) in enumerate(LK_CONFIGS):
        a, _ = lk_pair(kind)
        h, w = a.shape
        pts = interior_points(w, h, n_int, 1000 + i) + bound_points(w, h, win, ml) + special_points(w, h, win)
        kw = dict(win=win, max_level=ml, max_count=mc, epsilon=eps, min_eig_threshold=me)
        yield "%d: %s %s" % (i, kind, kw), kind, np.array(pts, dtype=np.float32), kw


@functools.lru_cache(maxsize=None)
def lk_restated(kind):
    lk = F.LK()
    for im in lk_pair(kind):
        lk.add_image(im)
    return lk


def tie_cases():
    """Tied responses (the 0/255 4-pixel checker: candidates in 2 x 2 clusters every 4 pixels, one response) in a
    rectangle of more than 4096 candidates (global sort) and one of fewer (LDS sort), with min_distance at a
    distance that occurs (3, 5) and one ulp on either side; min_distance 0 keeps the whole tie order."""
    img = checker(SELECT_W, SELECT_H, 4)
    for (x0, y0, x1, y1) in ((200, 160, 360, 288), (100, 100, 196, 196)):
        mask = np.zeros(img.shape, np.uint8)
        mask[y0:y1, x0:x1] = 1
        for d in (3.0, 5.0):
            for md in (float(np.nextafter(d, 0.0)), d, float(np.nextafter(d, math.inf))):
                kw = dict(max_corners=8192, quality_level=0.0, min_distance=md, block_size=3, harris_k=0.04)
                yield "checker rect %s min_distance=%r" % ((x0, y0, x1, y1), md), img, mask, kw
        for mc in (4097, 8192):
            kw = dict(max_corners=mc, quality_level=0.0, min_distance=0.0, block_size=3, harris_k=0.04)
            yield "checker rect %s order max_corners=%d" % ((x0, y0, x1, y1), mc), img, mask, kw
