"""CPU model of the LDS-array cycles of k_eval3's two tap passes: a numpy restatement of the
canonical order (order_deal.h), warp_event and eval_unit3's box rule on synth's windows, and on it the access rules of
the LDS for lane = event and one fixed tap per instruction:

    ds_add_u64   4 groups of 16 contiguous lanes over 16 bank pairs; every lane on a busy bank pair costs a cycle
                 (equal addresses serialise)
    ds_read_b64  2 groups of 32 lanes over 32 bank pairs; every DISTINCT address on a busy bank pair costs a cycle
                 (equal addresses are one access)

All 49 taps of an instruction sequence shift every lane's word alike, so an event-wave costs 49 x (one atomic + one read) of
its base words  (pyc - 3 - y0) * cols + (pxc - 3 - x0).  Counts, not measurements.

usage: lds_conflict_model.py [config=3] [windows=2] [patch step=5] [block=128] [flow scales=0,0.5,1]

Prints, per flow scale, the cycles of an atomic and of a read instruction in the canonical order and the tap cycles per
64 events of: the canonical order, a random permutation, and the bank deal (events sorted by the residue of their base
word modulo 32 resp. 16, dealt to lanes by deal_positions).  The last line scales the canonical figure to a number of
events (default: the headline's 25.6 M) for comparison with a measured SQ_LDS_IDX_ACTIVE.

tools/ab/bank_deal_ceiling.py loads windows in the dealt order and times the unchanged kernel on them."""
import os
import sys

import numpy as np

SCALE = 1e-3       # ebo_default_params: compensateScale
MIN_EVENTS = 100   # compensateMinNumEvents
ORDER_STRIDE = 127
SORT_MAX = 8192
REJECT = -(1 << 40)  # base word of an event warp_event rejects (its lane idles)


def order_stride(n):
    if n < 3:
        return 1
    st = ORDER_STRIDE % n or 1
    while np.gcd(st, n) != 1:
        st += 1
    return st


def canonical(x, y, sign, dt):
    """indices of a unit's events in the canonical order: ascending packed record, dealt with stride 127"""
    lo = (x.astype(np.int64) & 0x7FFF) | ((sign > 0).astype(np.int64) << 15) | ((y.astype(np.int64) & 0x7FFF) << 16)
    rec = (lo | ((dt.astype(np.int64) & 0xFFFFFFFF) << 32)).astype(np.uint64)
    n = len(rec)
    rank = np.argsort(rec, kind="stable")
    if n < 2 or n > SORT_MAX:
        return np.arange(n)
    return rank[(np.arange(n, dtype=np.int64) * order_stride(n)) % n]


def mid_time(a, b):
    return int(float(int(a) + int(b)) * 0.5)


def window_units(ev, image, patch):
    """the events of each grid patch of one window, in list order: [(positions in ev)] per patch, row-major"""
    iw, ih = image
    pw, ph = patch
    npx, npy = iw // pw, ih // ph
    pid = np.minimum(ev["y"] // ph, npy - 1).astype(np.int64) * npx + np.minimum(ev["x"] // pw, npx - 1)
    order = np.argsort(pid, kind="stable")
    bounds = np.searchsorted(pid[order], np.arange(npx * npy + 1))
    return [order[bounds[p]:bounds[p + 1]] for p in range(npx * npy)]


def box_base_words(x, y, dt, rect, flow, cap, scale=SCALE):
    """(base, cols, rows) of events given as source pixel and dt = t_ref - t: the word of each one's first tap in the LDS
    image (REJECT where warp_event drops the event) and the pitch and rows of eval_unit3's box (0, 0 where no event lands)"""
    rx, ry, rw, rh = (int(v) for v in rect)
    tau = dt.astype(np.float64) * scale
    cx = x.astype(np.float64) + tau * flow[0]
    cy = y.astype(np.float64) + tau * flow[1]
    pxc = np.trunc(cx).astype(np.int64) - rx + rw
    pyc = np.trunc(cy).astype(np.int64) - ry + rh
    ok = (pxc + 3 >= 0) & (pxc - 3 < 3 * rw) & (pyc + 3 >= 0) & (pyc - 3 < 3 * rh)
    base = np.full(len(x), REJECT, np.int64)
    if not ok.any():
        return base, 0, 0
    x0, x1 = max(pxc[ok].min() - 3, 0), min(pxc[ok].max() + 3, 3 * rw - 1)
    y0, y1 = max(pyc[ok].min() - 3, 0), min(pyc[ok].max() + 3, 3 * rh - 1)
    bw = x1 - x0 + 1
    cols = (bw | 1) if (bw | 1) <= cap else bw
    # (an event at the canvas edge takes the clipped path; its taps still start at this word, possibly outside the box)
    base[ok] = (pyc[ok] - 3 - y0) * cols + (pxc[ok] - 3 - x0)
    return base, int(cols), int(y1 - y0 + 1)


def unit_base_words(evu, rect, flow, cap, scale=SCALE):
    """One unit of events `evu` (any order): (idx, base) -- idx the positions in evu in the canonical order, base as
    box_base_words gives it for them."""
    if len(evu) == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    x, y, t = evu["x"].astype(np.int64), evu["y"].astype(np.int64), evu["t_us"].astype(np.int64)
    dt = mid_time(t.min(), t.max()) - t
    idx = canonical(x, y, evu["sign"], dt)
    return idx, box_base_words(x[idx], y[idx], dt[idx], rect, flow, cap, scale)[0]


DEAL_KEYS, DEAL_MIN_ROUNDS, DEAL_MAX_ROUNDS, DEAL_MAX_BLOCK = 17, 2, 12, 256  # csrc/eval_deal.h


def deal_admitted(n, block, tiles, cap, cols, rows):
    """eval_deal.h's rule: by event count, block size and row tiles, and the list (16-bit indices at the end of the image
    area) must fit behind the largest sub-band and behind the sort's scratch"""
    if tiles != 1 or block > DEAL_MAX_BLOCK or n < DEAL_MIN_ROUNDS * block or n > DEAL_MAX_ROUNDS * block or cols == 0:
        return False
    lst = (n + 3) // 4
    scratch = (DEAL_KEYS * block + 1) // 2 + lst
    band = min(max(cap // cols, 1), rows) * cols
    return lst + max(band, scratch) <= cap


def unpack_records(rec):
    """x, y, dt of packed records (x:15 | polarity:1 | y:15 | 0 in the low word, int32 dt in the high one)"""
    rec = np.asarray(rec, dtype=np.uint64)
    lo = (rec & np.uint64(0xFFFFFFFF)).astype(np.int64)
    x = ((lo & 0x7FFF) ^ 0x4000) - 0x4000
    y = (((lo >> 16) & 0x7FFF) ^ 0x4000) - 0x4000
    dt = (rec >> np.uint64(32)).astype(np.uint32).astype(np.int32).astype(np.int64)
    return x, y, dt


def dealt_list(rec, rect, flow, block, cap, tiles=1, scale=SCALE):
    """eval_unit3's dealt list of a unit from its records in device order (the canonical one): entry q the position of the
    event that lane q mod block takes in round q div block; empty where the unit is not dealt"""
    x, y, dt = unpack_records(rec)
    base, cols, rows = box_base_words(x, y, dt, rect, flow, cap, scale)
    if not deal_admitted(len(rec), block, tiles, cap, cols, rows):
        return np.zeros(0, np.uint16)
    return dealt_order(base, block, 16).astype(np.uint16)


def deal_positions(n, block, group=32):
    """The bank deal's layout: where list position q = round * block + lane takes its event from the SORTED order.
    With rounds = n // block full rounds and rem = n % block lanes in the last one (lanes 0 .. rem-1, as today: no
    wave-round is added), lane L owns the slot (L mod group) * (block / group) + L div group and a slot owns consecutive
    sorted elements, one per round its lane is live in: the lanes of a group (the sort key's modulus) sit block / group
    slots, about one bin, apart.  -> sorted index per list position [n], a permutation of 0 .. n-1."""
    per = block // group
    full, rem = divmod(n, block)
    lane = np.arange(block)
    slot = (lane % group) * per + lane // group
    count = full + (lane < rem)            # events of the lane
    by_slot = np.zeros(block, np.int64)
    by_slot[slot] = count
    start_of_slot = np.concatenate([[0], np.cumsum(by_slot)[:-1]])
    q = np.arange(n)
    return start_of_slot[slot[q % block]] + q // block


def dealt_order(base, block, mod):
    """indices into a unit's canonical order in the dealt list order: a stable counting sort by the key (residue of the
    base word modulo `mod`; rejected events last), ties by canonical lane then round, laid out by deal_positions"""
    n = len(base)
    key = np.where(base == REJECT, mod, base % mod)
    e = np.arange(n)
    srt = np.lexsort((e // block, e % block, key))
    return srt[deal_positions(n, block, mod)]


def wave_matrix(base, block):
    """[event-waves][64] base words of the list `base` as the kernel deals it (e = tid + k * blockDim), REJECT in idle lanes;
    only the waves with a live lane"""
    n = len(base)
    rounds = -(-n // block)
    m = np.full(rounds * block, REJECT, np.int64)
    m[:n] = base
    m = m.reshape(-1, 64)
    live = np.zeros(rounds * block, bool)
    live[:n] = True
    return m[live.reshape(-1, 64).any(axis=1)]


def atomic_cycles(m):
    """per event-wave: sum over the four 16-lane groups of the fullest bank pair"""
    g = m.reshape(-1, 4, 16)
    res = np.where(g == REJECT, 16, g % 16)
    cnt = (res[..., None] == np.arange(16)).sum(axis=2)
    return cnt.max(axis=2).sum(axis=1)


def read_cycles(m):
    """per event-wave: sum over the two 32-lane groups of the most distinct addresses on one bank pair"""
    g = np.sort(m.reshape(-1, 2, 32), axis=2)
    first = np.ones(g.shape, bool)
    first[..., 1:] = g[..., 1:] != g[..., :-1]
    res = np.where((g == REJECT) | ~first, 32, g % 32)
    cnt = (res[..., None] == np.arange(32)).sum(axis=2)
    return cnt.max(axis=2).sum(axis=1)


def unit_cycles(base, block):
    """(atomic cycles, read cycles, event-waves) of one instruction of each kind over a unit's list"""
    m = wave_matrix(base, block)
    return int(atomic_cycles(m).sum()), int(read_cycles(m).sum()), len(m)


def active_units(config, windows, step, synth):
    cfg = synth.CONFIGS[config]
    _, _, rects = synth.grid_rects(cfg["image"], cfg["patch"])
    for w in range(windows):
        ev, gt = synth.make_window(config, window=w)
        units = window_units(ev, cfg["image"], cfg["patch"])
        for p in range(0, len(rects), step):
            yield ev[units[p]], rects[p], gt[p]


def main(argv):
    pkg_dir = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, pkg_dir)
    import synth

    config = int(argv[1]) if len(argv) > 1 else 3
    windows = int(argv[2]) if len(argv) > 2 else 2
    step = int(argv[3]) if len(argv) > 3 else 5
    block = int(argv[4]) if len(argv) > 4 else 128
    scales = [float(v) for v in (argv[5] if len(argv) > 5 else "0,0.5,1").split(",")]
    cap = int(argv[6]) if len(argv) > 6 else 2542
    headline_events = float(argv[7]) if len(argv) > 7 else 25.6e6
    rng = np.random.default_rng(1)
    print("config %d, windows 0-%d, every %d. patch, %d lanes per workgroup, image capacity %d" % (config, windows - 1, step, block, cap))
    print("flows | atomic, read cycles per instruction (canonical) | tap cycles per 64 events: canonical / random / "
          "deal mod 32 / deal mod 16 | event-waves canonical, dealt")
    for s in scales:
        tot = {k: np.zeros(3, np.int64) for k in ("canonical", "random", "deal32", "deal16")}
        events = 0
        units = dealt = 0
        for ev, rect, flow in active_units(config, windows, step, synth):
            if len(ev) <= MIN_EVENTS:
                continue
            x, y, t = ev["x"].astype(np.int64), ev["y"].astype(np.int64), ev["t_us"].astype(np.int64)
            dt = mid_time(t.min(), t.max()) - t
            idx = canonical(x, y, ev["sign"], dt)
            base, cols, rows = box_base_words(x[idx], y[idx], dt[idx], rect, flow * s, cap)
            units += 1
            dealt += deal_admitted(len(base), block, 1, cap, cols, rows)
            events += len(base)
            tot["canonical"] += unit_cycles(base, block)
            tot["random"] += unit_cycles(base[rng.permutation(len(base))], block)
            tot["deal32"] += unit_cycles(base[dealt_order(base, block, 32)], block)
            tot["deal16"] += unit_cycles(base[dealt_order(base, block, 16)], block)
        per64 = {k: 49.0 * (v[0] + v[1]) / (events / 64.0) for k, v in tot.items()}
        c = tot["canonical"]
        print("%.1f x gt | %.2f, %.2f | %.0f / %.0f / %.0f / %.0f | %d, %d  (%d events; eval_deal.h deals %d of %d units, %.2f %% not)"
              % (s, c[0] / c[2], c[1] / c[2], per64["canonical"], per64["random"], per64["deal32"], per64["deal16"],
                 c[2], tot["deal32"][2], events, dealt, units, 100.0 * (units - dealt) / max(units, 1)))
        if s == 0.5:
            print("          canonical tap cycles of %.3g events: %.3e LDS-array cycles per launch"
                  % (headline_events, per64["canonical"] * headline_events / 64.0))


if __name__ == "__main__":
    main(sys.argv)
