"""CPU only: a plain restatement (Python ints and floats) of where the edge loss stores a unit -- the warp to the canvas
(warp_event, csrc/ebo_kernels.hip), the geometry of a unit's box and the quantities the kernel counts from it (edge_box_of,
edge_box_rows, edge_unit: csrc/ebo_edge.inc), the fit tests (npx <= capPx on the 28 B form, edge_box_fits_alias on the 20 B
and compact forms) and the arithmetic of edge_launch_setup (csrc/ebo_api.cpp) that gives the capacities.  For
tests/edge_fit_cases.py, tests/test_edge_fit_cases_cpu.py and tests/test_gpu_edge_fit.py.  Nothing here calls the library."""
import math

LDS_BUDGET = 160 * 1024                  # kLdsBudget
HEADER_BYTES = (168 + 1024) * 8          # kEdgeHeader doubles
TWICE_BYTES = 80 * 1024 - 256            # what one of two workgroups per CU may take
LIST_CAP, LM_INTS, LIST_SLACK = 2048, 128, 64   # kEdgeListCap, kEdgeLmInts (k_solve_edge's state), the list's slack
BYTES_28, BYTES_20 = 3 * 8 + 4, 2 * 8 + 4

FORM_28, FORM_20, FORM_COMPACT, FORM_SLICE = "lds28", "lds20", "compact", "slice"


def ref_time(t_first_us, t_last_us):
    """mid_timestamp (ebo_api.cpp): the int32 truncation of the mean of a unit's first and last stamp -- ebo_set_patches
    takes the list's first and last event, the grid loader the earliest and latest stamp of the patch"""
    half = float(t_first_us + t_last_us) * 0.5
    assert -2147483648.0 < half < 2147483648.0
    return int(half)


def warp(x, y, t_us, t_ref_us, rect, flow, scale=1e-3):
    """warp_event: (pxc, pyc, cx, cy) of the centre tap in canvas coordinates, or None when the taps miss the canvas"""
    rx, ry, rw, rh = rect
    tau = float(t_ref_us - t_us) * scale
    cx = float(x) + tau * flow[0]
    cy = float(y) + tau * flow[1]
    bx, by = int(cx), int(cy)  # truncation towards zero
    pxc, pyc = bx - rx + rw, by - ry + rh
    if pxc + 3 < 0 or pxc - 3 >= 3 * rw or pyc + 3 < 0 or pyc - 3 >= 3 * rh:
        return None
    return pxc, pyc, cx, cy


def tap_bounds(events, rect, flow, scale=1e-3, t_ref_us=None):
    """(xmin, xmax, ymin, ymax) of the accepted centre taps of a unit's events (x, y, t_us), or None if none is accepted;
    and the distance of the nearest warped coordinate from an integer"""
    if t_ref_us is None:
        ts = [e[2] for e in events]
        t_ref_us = ref_time(min(ts), max(ts))
    xs, ys, away = [], [], 1.0
    for x, y, t in events:
        w = warp(x, y, t, t_ref_us, rect, flow, scale)
        if w is None:
            continue
        xs.append(w[0])
        ys.append(w[1])
        for v in w[2:]:
            away = min(away, abs(v - round(v)))
    if not xs:
        return None, away
    return (min(xs), max(xs), min(ys), max(ys)), away


class Box:
    """edge_box_of + edge_box_rows + the regions edge_unit derives (its work counters)"""

    def __init__(self, xmin, xmax, ymin, ymax, W3, H3):
        self.taps = (xmin, xmax, ymin, ymax)
        self.W3, self.H3 = W3, H3
        self.x0, self.x1 = max(xmin - 3, 0), min(xmax + 3, W3 - 1)
        self.y0, self.y1 = max(ymin - 3, 0), min(ymax + 3, H3 - 1)
        self.bx0, self.by0 = max(self.x0 - 8, 0), max(self.y0 - 8, 0)
        self.bc = min(self.x1 + 8, W3 - 1) - self.bx0 + 1
        self.br = min(self.y1 + 8, H3 - 1) - self.by0 + 1
        # edge_box_rows
        self.iy0 = max(self.y0 - 1, 0)
        self.iRows = min(self.y1 + 1, H3 - 1) - self.iy0 + 1
        self.qy0 = max(min(max(self.y0 - 4, 0), self.y0) - 1, 0)
        self.qRows = min(max(min(self.y1 + 3, H3 - 2), self.y1) + 1, H3 - 1) - self.qy0 + 1
        # edge_unit: the eigenvalue region and the grid of 5x5 windows
        self.ex0, self.ex1 = max(self.x0 - 4, 0), min(self.x1 + 3, W3 - 2)
        self.ey0, self.ey1 = max(self.y0 - 4, 0), min(self.y1 + 3, H3 - 2)
        self.ew, self.eh = self.ex1 - self.ex0 + 1, self.ey1 - self.ey0 + 1
        half = lambda v: int(v / 2)  # C's division truncates
        self.cyLo, self.cxLo = max(2, half(self.ey0 - 2 + 1) * 2), max(2, half(self.ex0 - 2 + 1) * 2)
        self.cyHi, self.cxHi = min(self.ey1 + 2, H3 - 4), min(self.ex1 + 2, W3 - 4)
        self.nwy = (self.cyHi - self.cyLo) // 2 + 1 if self.cyHi >= self.cyLo else 0
        self.nwx = (self.cxHi - self.cxLo) // 2 + 1 if self.cxHi >= self.cxLo else 0

    npx = property(lambda s: s.bc * s.br)
    nI = property(lambda s: s.bc * s.iRows)
    nE = property(lambda s: s.bc * s.qRows)
    eigen_px = property(lambda s: s.ew * s.eh)
    windows = property(lambda s: s.nwy * s.nwx)

    def alias_ints(self, cnt4):
        """the left side of edge_box_fits_alias, in 4-byte ints: I and E as doubles, the claim counters behind E"""
        return 2 * (self.nI + self.nE) + ((self.nE + 7) >> 3 if cnt4 else self.nE)

    def key(self):
        return (self.bc, self.br, self.iRows, self.qRows)

    def __repr__(self):
        return "Box(taps=%r, %dx%d=%d, iRows=%d, qRows=%d)" % (self.taps, self.bc, self.br, self.npx, self.iRows, self.qRows)


def alias_cap_ints(cap_px, cnt4):
    return 4 * cap_px + ((cap_px >> 3) if cnt4 else cap_px)


def fits_alias(box, cap_px, max_px, cnt4):
    """edge_box_fits_alias"""
    return box.alias_ints(cnt4) <= alias_cap_ints(cap_px, cnt4) and box.npx <= max_px


def fits_28(box, cap_px):
    return box.npx <= cap_px


class Setup:
    """what edge_launch_setup decides"""

    def __repr__(self):
        return "Setup(%s)" % ", ".join("%s=%r" % kv for kv in sorted(vars(self).items()))


def _env_size(env, name, dflt):
    v = env.get(name)
    return dflt if v is None or v == "" else int(v)


def launch_setup(max_rw, max_rh, patch_w, patch_h, custom, n_units=1, for_solve=False, n_cus=256, env=None):
    """edge_launch_setup for one flow set.  custom: units from ebo_set_patches (their largest rect is the regular one).
    env: the A/B switches EBO_EDGE_LAYOUT, EBO_EDGE_LDS_KB, EBO_EDGE_COMPACT, EBO_EDGE_COMPACT_KB (the A/B build only;
    the shipped library reads none).  n_cus enters only through `more than eight units per CU`."""
    env = env or {}
    S = Setup()
    S.env = dict(env)
    canvas = 9 * max_rw * max_rh
    fits_twice = HEADER_BYTES + canvas * BYTES_20 + 64 <= TWICE_BYTES
    regular = canvas if custom else 9 * patch_w * patch_h
    regular_fits_twice = HEADER_BYTES + regular * BYTES_20 + 64 <= TWICE_BYTES
    only_alias = (HEADER_BYTES + regular * BYTES_28 + 64 > LDS_BUDGET and
                  HEADER_BYTES + (regular * 9 // 10) * BYTES_20 + 64 <= LDS_BUDGET and regular <= 8 * 1024)
    layout_env = env.get("EBO_EDGE_LAYOUT")
    S.alias = (int(layout_env) != 0) if layout_env is not None else (fits_twice or regular_fits_twice or only_alias)
    per_px = BYTES_20 if S.alias else BYTES_28
    lds_env = env.get("EBO_EDGE_LDS_KB") is not None
    lds_bytes = min(_env_size(env, "EBO_EDGE_LDS_KB", 160) * 1024, LDS_BUDGET)
    if S.alias and layout_env is None and not lds_env and not fits_twice and regular_fits_twice:
        lds_bytes = TWICE_BYTES
    lds_bytes = min(lds_bytes, HEADER_BYTES + canvas * per_px + 64)
    S.cap_px = (lds_bytes - HEADER_BYTES) // per_px
    two_per_cu = S.alias and HEADER_BYTES + S.cap_px * per_px <= TWICE_BYTES
    S.block = 256 if two_per_cu else (512 if for_solve else 768)
    S.lds_bytes = HEADER_BYTES + S.cap_px * per_px
    S.canvas_px = canvas
    S.max_lds_px = min(canvas, 4 * (LIST_CAP - LM_INTS - LIST_SLACK))
    S.cs_stride = S.max_lds_px if S.alias else S.cap_px
    S.has_slice = S.cap_px < canvas or S.max_lds_px < canvas
    # the compact form
    S.compact_cap = S.compact_max_px = S.compact_list_cap = S.compact_bytes = 0
    S.compact = False
    force = env.get("EBO_EDGE_COMPACT")
    eligible = S.alias and S.block == 256 and not for_solve and 2 * S.lds_bytes <= LDS_BUDGET
    want = (int(force) != 0) if force is not None else n_units > 8 * n_cus
    if eligible and want:
        budget = _env_size(env, "EBO_EDGE_COMPACT_KB", 52) * 1024
        max_px = min((canvas + 7) & ~7, (budget // 13) & ~7)
        list_cap = ((max_px // 4 + 64) + 1) & ~1
        hdr = (168 + list_cap // 2) * 8
        cap = (((budget - hdr) * 2 // 33) & ~7) if budget > hdr else 0
        cap = min(cap, max_px)
        nbytes = hdr + cap * 16 + cap // 2
        if cap >= 1024 and nbytes <= budget:
            S.compact = True
            S.compact_cap, S.compact_max_px, S.compact_list_cap, S.compact_bytes = cap, max_px, list_cap, nbytes
    return S


def form_of(box, S):
    """the storage form the launch gives a unit with this box"""
    if S.compact and fits_alias(box, S.compact_cap, S.compact_max_px, True):
        return FORM_COMPACT
    if S.alias:
        return FORM_20 if fits_alias(box, S.cap_px, S.cs_stride, False) else FORM_SLICE
    return FORM_28 if fits_28(box, S.cap_px) else FORM_SLICE


# ---- the eigenvalue image and the claims of the 5x5 windows, loosely (numpy doubles; not bit for bit) ------------------------
def eigen_image(I, sigma_st=1.5):
    """the larger eigenvalue of the structure tensor of image I [H3][W3] (forward differences on the (H3-1) x (W3-1)
    gradient domain, 7x7 Gaussian window), as calculateEdgeLoss forms it; zero outside the gradient domain"""
    import numpy as np
    H3, W3 = I.shape
    gx = I[:-1, 1:] - I[:-1, :-1]
    gy = I[1:, :-1] - I[:-1, :-1]
    g = np.array([math.exp(-0.5 / (sigma_st * sigma_st) * k * k) for k in range(-3, 4)])
    norm = 1.0 / ((2 * math.pi) * sigma_st * sigma_st)

    def smooth(a):
        p = np.pad(a, 3)
        rows = sum(g[k] * p[:, k:k + a.shape[1]] for k in range(7))
        return norm * sum(g[k] * rows[k:k + a.shape[0], :] for k in range(7))
    s00, s01, s11 = smooth(gx * gx), smooth(gx * gy), smooth(gy * gy)
    tr, det = s00 + s11, s00 * s11 - s01 * s01
    E = np.zeros((H3, W3))
    E[:-1, :-1] = 0.5 * (tr + np.sqrt(np.maximum(tr * tr - 4.0 * det, 0.0)))
    return E


def window_claims(E, box):
    """{(x, y): windows} -- how many of the box's 5x5 windows (centres cxLo, cxLo + 2 .. cxHi, likewise in y) have their
    positive maximum at the pixel; E restricted to the box's eigenvalue region, as the kernel stores it"""
    import numpy as np
    M = np.zeros_like(E)
    M[box.ey0:box.ey1 + 1, box.ex0:box.ex1 + 1] = E[box.ey0:box.ey1 + 1, box.ex0:box.ex1 + 1]
    claims = {}
    for cy in range(box.cyLo, box.cyHi + 1, 2):
        for cx in range(box.cxLo, box.cxHi + 1, 2):
            w = M[cy - 2:cy + 3, cx - 2:cx + 3]
            if w.max() > 0.0:
                j, i = np.unravel_index(np.argmax(w), w.shape)
                key = (cx - 2 + int(i), cy - 2 + int(j))
                claims[key] = claims.get(key, 0) + 1
    return claims


def counter_index(box, x, y):
    """the index of canvas pixel (x, y) among the box's claim counters (4-bit fields on the compact form: word p >> 3,
    field p & 7): the counters cover E's stored rows"""
    return (y - box.qy0) * box.bc + (x - box.bx0)
