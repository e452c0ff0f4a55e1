"""CPU restatement of the image front end of include/ebo.h (ebo_image_gradients, ebo_good_features,
ebo_lk_add_image + ebo_lk_track), written from the rules in that header, plus a reader for the PNG
fixtures under tests/golden/frontend.  Test infrastructure: the device must agree with this bit for bit
(gradients, corners, LK positions, status and err).

good_features / greedy and LK.track take an optional `trace`, a collections.Counter that counts the branch each
candidate or point took (the names are in CORNER_BRANCHES and LK_BRANCHES); results do not depend on it."""
import math
import os
import struct
import zlib

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "frontend")
FRAMES = [os.path.join(GOLDEN, "frame_%08d.png" % i) for i in range(3)]

F32 = np.float32

# the branches a trace counts (what tests/test_front_end_cpu.py requires the GPU sweep to reach)
LK_BRANCHES = (
    "skip_bounds_upper",       # floor(p) outside the level at a level > 0: the level is skipped
    "status0_bounds_l0",       # ... at level 0: status 0 before iterating
    "skip_mineig_upper",       # minEig < threshold or D < FLT_EPSILON at a level > 0: the level is skipped
    "status0_mineig_l0",       # ... at level 0: status 0
    "iter_oob_upper",          # floor(q) outside the level inside the iteration at a level > 0: break, next level
    "iter_oob_l0",             # ... at level 0: status 0
    "eps_exit",                # dx^2 + dy^2 <= epsilon^2
    "half_step_exit",          # |delta + delta_prev| < 0.01: result -= delta / 2
    "max_count_exhausted",     # max_count iterations without an exit
    "final_check_fail",        # status 1 until the level-0 position check of the result
    "err_computed",            # status 1 and err computed
)
CORNER_BRANCHES = (
    "zero_candidates",         # an empty candidate list
    "sort_lds",                # 1 .. 4096 candidates: the device sorts in LDS
    "sort_global",             # more than 4096: the global bitonic sort
    "max_corners_cutoff",      # candidates left over when max_corners were accepted
    "reject_in_batch",         # too close only to corners accepted in its own batch of 64 sorted candidates
    "reject_earlier_batch",    # too close to a corner accepted in an earlier batch
    "accept_near_rejected",    # accepted although closer than min_distance to a rejected candidate
    "accept_at_min_distance",  # accepted at exactly min_distance ((dx*dx + dy*dy) == min_distance^2) from a corner
)


def _hit(trace, key, n=1):
    if trace is not None:
        trace[key] += n


# ---- PNG (8-bit grey, not interlaced) ------------------------------------------------------------
def read_png_gray8(path):
    data = open(path, "rb").read()
    assert data[:8] == b"\x89PNG\r\n\x1a\n", "not a PNG"
    pos, idat, hdr = 8, [], None
    while pos < len(data):
        length, kind = struct.unpack(">I4s", data[pos:pos + 8])
        body = data[pos + 8:pos + 8 + length]
        pos += 12 + length
        if kind == b"IHDR":
            hdr = struct.unpack(">IIBBBBB", body)
        elif kind == b"IDAT":
            idat.append(body)
        elif kind == b"IEND":
            break
    w, h, depth, ctype, _, _, interlace = hdr
    assert depth == 8 and ctype == 0 and interlace == 0, "only 8-bit grey, non-interlaced PNGs"
    raw = zlib.decompress(b"".join(idat))
    out = np.zeros((h, w), dtype=np.uint8)
    prev = np.zeros(w, dtype=np.int32)
    for y in range(h):
        f = raw[y * (w + 1)]
        line = np.frombuffer(raw, dtype=np.uint8, count=w, offset=y * (w + 1) + 1).astype(np.int32)
        cur = np.zeros(w, dtype=np.int32)
        if f == 0:
            cur = line
        elif f == 2:
            cur = (line + prev) & 255
        else:  # 1 (sub), 3 (average), 4 (Paeth) depend on the left neighbour: per pixel
            for x in range(w):
                a = cur[x - 1] if x else 0
                b = prev[x]
                c = prev[x - 1] if x else 0
                if f == 1:
                    p = a
                elif f == 3:
                    p = (a + b) >> 1
                elif f == 4:
                    pa, pb, pc = abs(b - c), abs(a - c), abs(a + b - 2 * c)
                    p = a if pa <= pb and pa <= pc else (b if pb <= pc else c)
                else:
                    raise ValueError("bad PNG filter %d" % f)
                cur[x] = (line[x] + p) & 255
        out[y] = cur
        prev = cur
    return out


def frames():
    return [read_png_gray8(p) for p in FRAMES]


def refl(i, n):
    """BORDER_REFLECT_101 for any integer (array) index."""
    i = np.asarray(i)
    if n == 1:
        return np.zeros_like(i)
    period = 2 * n - 2
    i = np.abs(i) % period
    return np.where(i < n, i, period - i)


# ---- ebo_image_gradients ---------------------------------------------------------------------------
def log_table():
    return np.array([math.log(v * (1.0 / 255.0) + 10e-2) / 8 for v in range(256)])


def image_gradients(img):
    h, w = img.shape
    L = log_table()[img]
    ys, xs = refl(np.arange(-1, h + 1), h), refl(np.arange(-1, w + 1), w)
    Lp = L[ys][:, xs]
    r = Lp[:, 2:] - Lp[:, :-2]
    s = (Lp[:, :-2] + 2.0 * Lp[:, 1:-1]) + Lp[:, 2:]
    gx = (r[:-2] + 2.0 * r[1:-1]) + r[2:]
    gy = s[2:] - s[:-2]
    return gx, gy


# ---- ebo_good_features -----------------------------------------------------------------------------
def harris_response(img, block_size=3, k=0.04):
    h, w = img.shape
    I = img.astype(np.int64)
    ys, xs = refl(np.arange(-1, h + 1), h), refl(np.arange(-1, w + 1), w)
    P = I[ys][:, xs]
    dx = (P[:-2, 2:] + 2 * P[1:-1, 2:] + P[2:, 2:]) - (P[:-2, :-2] + 2 * P[1:-1, :-2] + P[2:, :-2])
    dy = (P[2:, :-2] + 2 * P[2:, 1:-1] + P[2:, 2:]) - (P[:-2, :-2] + 2 * P[:-2, 1:-1] + P[:-2, 2:])
    lo = block_size // 2
    ys, xs = refl(np.arange(-lo, h - lo + block_size - 1), h), refl(np.arange(-lo, w - lo + block_size - 1), w)
    sums = []
    for m in (dx * dx, dx * dy, dy * dy):
        mp = m[ys][:, xs]
        acc = np.zeros((h, w), dtype=np.int64)
        for j in range(block_size):
            for i in range(block_size):
                acc += mp[j:j + h, i:i + w]
        sums.append(acc)
    A, B, C = sums
    det = (A * C - B * B).astype(np.float64)
    tr = (A + C).astype(np.float64)
    return det - k * (tr * tr)


def candidates(img, mask=None, quality_level=0.01, block_size=3, harris_k=0.04):
    """Steps 1-5 of ebo_good_features: the candidates' raster indices y*w + x in selection order."""
    h, w = img.shape
    R = harris_response(img, block_size, harris_k)
    m = np.ones((h, w), dtype=bool) if mask is None else (np.asarray(mask) != 0)
    max_val = R[m].max() if m.any() else 0.0
    thr = quality_level * max_val
    T = np.where(R > thr, R, 0.0)
    keep = np.zeros((h, w), dtype=bool)
    if h >= 3 and w >= 3:
        inner = T[1:-1, 1:-1]
        nb = np.max(np.stack([T[1 + j:h - 1 + j, 1 + i:w - 1 + i] for j in (-1, 0, 1) for i in (-1, 0, 1)]), axis=0)
        keep[1:-1, 1:-1] = (inner != 0) & (inner == nb)
    keep &= m
    idx = np.flatnonzero(keep)
    r = R.ravel()[idx]
    order = np.lexsort((-idx, -r))  # R descending, ties: larger raster index first
    return idx[order]


def good_features(img, mask=None, max_corners=100, quality_level=0.01, min_distance=10.0, block_size=3,
                  harris_k=0.04, trace=None):
    cand = candidates(img, mask, quality_level, block_size, harris_k)
    return greedy(cand, img.shape[1], max_corners, min_distance, trace)


def greedy(sorted_idx, w, max_corners, min_distance, trace=None):
    md2 = min_distance * min_distance
    acc = []
    ax, ay = np.zeros(0, dtype=np.int64), np.zeros(0, dtype=np.int64)
    apos = np.zeros(0, dtype=np.int64)  # position of each accepted corner in the sorted list
    rx, ry = [], []  # rejected candidates (trace only)
    if trace is not None:
        _hit(trace, "zero_candidates" if len(sorted_idx) == 0 else
             ("sort_lds" if len(sorted_idx) <= 4096 else "sort_global"))
    for pos, p in enumerate(sorted_idx):
        if len(acc) >= max_corners:
            _hit(trace, "max_corners_cutoff")
            break
        x, y = int(p % w), int(p // w)
        d2 = ((ax - x) ** 2 + (ay - y) ** 2).astype(np.float64)
        close = d2 < md2
        if len(acc) and np.any(close):
            if trace is not None:
                # the device checks the corners of earlier batches first, then the survivors of its own batch
                _hit(trace, "reject_earlier_batch" if np.any(apos[close] // 64 < pos // 64) else "reject_in_batch")
                rx.append(x)
                ry.append(y)
            continue
        if trace is not None:
            if np.any(d2 == md2):
                _hit(trace, "accept_at_min_distance")
            if rx and np.any((np.subtract(rx, x) ** 2 + np.subtract(ry, y) ** 2).astype(np.float64) < md2):
                _hit(trace, "accept_near_rejected")
        acc.append((x, y))
        ax, ay, apos = np.append(ax, x), np.append(ay, y), np.append(apos, pos)
    return np.array(acc, dtype=np.float32).reshape(-1, 2)


def reference_mask(w, h, patch_extent):
    """FeatureDetector::reset's mask_: a border of patchExtent (feature_detector.cpp:39-45)."""
    m = np.zeros((h, w), dtype=np.uint8)
    m[patch_extent:h - patch_extent, patch_extent:w - patch_extent] = 1
    return m


def reference_max_corners(w, h, patch_extent):
    return w * h // ((2 * patch_extent + 1) * (2 * patch_extent + 1))


# ---- ebo_lk_add_image / ebo_lk_track ---------------------------------------------------------------
def pyr_down(src):
    sh, sw = src.shape
    dh, dw = (sh + 1) // 2, (sw + 1) // 2
    k = np.array([1, 4, 6, 4, 1], dtype=np.int64)
    S = src.astype(np.int64)
    rows = refl(2 * np.arange(dh)[:, None] + np.arange(5)[None, :] - 2, sh)  # [dh][5]
    cols = refl(2 * np.arange(dw)[:, None] + np.arange(5)[None, :] - 2, sw)
    acc = np.zeros((dh, dw), dtype=np.int64)
    for j in range(5):
        rs = np.zeros((dh, dw), dtype=np.int64)
        for i in range(5):
            rs += k[i] * S[rows[:, j]][:, cols[:, i]]
        acc += k[j] * rs
    return ((acc + 128) >> 8).astype(np.uint8)


def scharr(img):
    h, w = img.shape
    I = img.astype(np.int64)
    ym, yp = refl(np.arange(h) - 1, h), refl(np.arange(h) + 1, h)
    xm, xp = refl(np.arange(w) - 1, w), refl(np.arange(w) + 1, w)
    v0 = 3 * (I[ym] + I[yp]) + 10 * I
    v1 = I[yp] - I[ym]
    return v0[:, xp] - v0[:, xm], 3 * (v1[:, xm] + v1[:, xp]) + 10 * v1


def pyramid(img):
    levels = [img]
    while len(levels) < 8:
        h, w = levels[-1].shape
        nh, nw = (h + 1) // 2, (w + 1) // 2
        if nw < 2 or nh < 2 or (nw == w and nh == h):
            break
        levels.append(pyr_down(levels[-1]))
    return levels


def _weights(a, b):
    one, s = F32(1), F32(16384)
    w00 = int(np.rint((one - a) * (one - b) * s))
    w01 = int(np.rint(a * (one - b) * s))
    w10 = int(np.rint((one - a) * b * s))
    return w00, w01, w10, 16384 - w00 - w01 - w10


def _sample(im, x0, y0, ox, oy, wts):
    h, w = im.shape
    xs, ys = x0 + ox, y0 + oy
    a, b = refl(xs, w), refl(xs + 1, w)
    c, d = refl(ys, h), refl(ys + 1, h)
    I = im.astype(np.int64)
    w00, w01, w10, w11 = wts
    return (I[c, a] * w00 + I[c, b] * w01 + I[d, a] * w10 + I[d, b] * w11 + 256) >> 9


def _dsample(D, x0, y0, ox, oy, wts):
    h, w = D.shape
    out = 0
    for (dx, dy, wt) in ((0, 0, wts[0]), (1, 0, wts[1]), (0, 1, wts[2]), (1, 1, wts[3])):
        xs, ys = x0 + ox + dx, y0 + oy + dy
        ok = (xs >= 0) & (xs < w) & (ys >= 0) & (ys < h)
        out = out + np.where(ok, D[np.clip(ys, 0, h - 1), np.clip(xs, 0, w - 1)], 0) * wt
    return (out + 8192) >> 14


class LK:
    """ebo_lk_add_image + ebo_lk_track."""

    def __init__(self):
        self.pyrs = []

    def add_image(self, img):
        levels = pyramid(np.asarray(img, dtype=np.uint8))
        self.pyrs = (self.pyrs + [(levels, [scharr(l) for l in levels])])[-2:]

    def track(self, prev_xy, win=(21, 21), max_level=3, max_count=30, epsilon=0.01, min_eig_threshold=1e-4,
              trace=None):
        if len(self.pyrs) < 2:
            raise RuntimeError("two images are needed")
        (Ilv, Dlv), (Jlv, _) = self.pyrs
        ww, wh = win
        n_levels = 1
        while n_levels - 1 < max_level and n_levels < len(Ilv) and Ilv[n_levels].shape[1] > ww and \
                Ilv[n_levels].shape[0] > wh:
            n_levels += 1
        eps = min(epsilon, 10.0)
        eps2 = eps * eps
        max_count = min(max_count, 100)
        pts = np.asarray(prev_xy, dtype=np.float32).reshape(-1, 2)
        nxt = np.zeros_like(pts)
        st = np.ones(len(pts), dtype=np.uint8)
        err = np.zeros(len(pts), dtype=np.float32)
        oy, ox = np.divmod(np.arange(ww * wh), ww)
        for k, (px0, py0) in enumerate(pts):
            nxt[k], st[k], err[k] = self._one(Ilv, Dlv, Jlv, n_levels, F32(px0), F32(py0), ox, oy, ww, wh, max_count,
                                              eps2, F32(min_eig_threshold), trace)
        return nxt, st, err

    @staticmethod
    def _one(Ilv, Dlv, Jlv, n_levels, px0, py0, ox, oy, ww, wh, max_count, eps2, min_eig, trace=None):
        hx, hy = F32(ww - 1) * F32(0.5), F32(wh - 1) * F32(0.5)
        scale = F32(1.0 / (1 << 20))
        ok = True
        resX = resY = F32(0)
        Ival = Ix = Iy = None
        for level in range(n_levels - 1, -1, -1):
            I, J = Ilv[level], Jlv[level]
            DX, DY = Dlv[level]
            h, w = I.shape
            sc = F32(1.0 / (1 << level))
            prevX, prevY = px0 * sc, py0 * sc
            if level == n_levels - 1:
                resX, resY = prevX, prevY
            else:
                resX, resY = resX * F32(2), resY * F32(2)
            prevX, prevY = prevX - hx, prevY - hy
            ipx, ipy = int(np.floor(prevX)), int(np.floor(prevY))
            if ipx < -ww or ipx >= w or ipy < -wh or ipy >= h:
                _hit(trace, "status0_bounds_l0" if level == 0 else "skip_bounds_upper")
                if level == 0:
                    ok = False
                continue
            wts = _weights(prevX - F32(ipx), prevY - F32(ipy))
            Ival = _sample(I, ipx, ipy, ox, oy, wts)
            Ix = _dsample(DX, ipx, ipy, ox, oy, wts)
            Iy = _dsample(DY, ipx, ipy, ox, oy, wts)
            A11 = F32(int(np.sum(Ix * Ix))) * scale
            A12 = F32(int(np.sum(Ix * Iy))) * scale
            A22 = F32(int(np.sum(Iy * Iy))) * scale
            D = A11 * A22 - A12 * A12
            dd = A11 - A22
            disc = dd * dd + (F32(4) * A12) * A12
            minEig = ((A22 + A11) - np.sqrt(disc)) / F32(2 * ww * wh)
            if minEig < min_eig or D < F32(1.19209290e-7):
                _hit(trace, "status0_mineig_l0" if level == 0 else "skip_mineig_upper")
                if level == 0:
                    ok = False
                continue
            D = F32(1) / D
            qx, qy = resX - hx, resY - hy
            pdx = pdy = F32(0)
            for it in range(max_count):
                iqx, iqy = int(np.floor(qx)), int(np.floor(qy))
                if iqx < -ww or iqx >= w or iqy < -wh or iqy >= h:
                    _hit(trace, "iter_oob_l0" if level == 0 else "iter_oob_upper")
                    if level == 0:
                        ok = False
                    break
                wj = _weights(qx - F32(iqx), qy - F32(iqy))
                diff = _sample(J, iqx, iqy, ox, oy, wj) - Ival
                B1 = F32(int(np.sum(diff * Ix))) * scale
                B2 = F32(int(np.sum(diff * Iy))) * scale
                dx = (A12 * B2 - A22 * B1) * D
                dy = (A12 * B1 - A11 * B2) * D
                qx, qy = qx + dx, qy + dy
                resX, resY = qx + hx, qy + hy
                if float(dx) * float(dx) + float(dy) * float(dy) <= eps2:
                    _hit(trace, "eps_exit")
                    break
                if it > 0 and float(abs(dx + pdx)) < 0.01 and float(abs(dy + pdy)) < 0.01:
                    _hit(trace, "half_step_exit")
                    resX, resY = resX - dx * F32(0.5), resY - dy * F32(0.5)
                    break
                pdx, pdy = dx, dy
            else:
                _hit(trace, "max_count_exhausted")
        e = F32(0)
        if ok:
            I, J = Ilv[0], Jlv[0]
            h, w = I.shape
            qx, qy = resX - hx, resY - hy
            iqx, iqy = int(np.floor(qx)), int(np.floor(qy))
            if iqx < -ww or iqx >= w or iqy < -wh or iqy >= h:
                _hit(trace, "final_check_fail")
                ok = False
            else:
                _hit(trace, "err_computed")
                diff = _sample(J, iqx, iqy, ox, oy, _weights(qx - F32(iqx), qy - F32(iqy))) - Ival
                e = F32(int(np.sum(np.abs(diff)))) / F32(32 * ww * wh)
        return (resX, resY), int(ok), e


def textured(h, w, seed=0, sigma=2.0):
    """A smoothed random texture, uint8 [h + 64][w + 64] (shifted() cuts the [h][w] view), for the flow tests
    (float64 separable Gaussian, rounded)."""
    rng = np.random.default_rng(seed)
    big = rng.uniform(0, 255, size=(h + 64, w + 64))
    r = int(3 * sigma)
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    tmp = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 1, big)
    out = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), 0, tmp)
    out = (out - out.mean()) * 4 + 128
    return np.clip(np.rint(out), 0, 255).astype(np.uint8)


def shifted(big, h, w, dx, dy):
    """The [h][w] view of `big` at offset (32, 32) and the same view of `big` moved by (dx, dy): a Fourier shift of
    the smooth texture (exact for a band-limited image; the wrap-around stays outside the view), rounded."""
    a = big[32:32 + h, 32:32 + w]
    H, W = big.shape
    fy, fx = np.fft.fftfreq(H)[:, None], np.fft.fftfreq(W)[None, :]
    moved = np.real(np.fft.ifft2(np.fft.fft2(big.astype(np.float64)) * np.exp(-2j * np.pi * (fx * dx + fy * dy))))
    return a.copy(), np.clip(np.rint(moved[32:32 + h, 32:32 + w]), 0, 255).astype(np.uint8)
