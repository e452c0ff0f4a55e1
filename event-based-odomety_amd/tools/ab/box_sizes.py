"""CPU count of k_eval3's bounding boxes: a numpy restatement of warp_event and of eval_unit3's
box rule on synth's windows, and from it how many units need more than one sequential sub-band at a given image
capacity.  Counts, not measurements: what a smaller LDS share per workgroup costs in re-warped events, before any GPU run.

usage: box_sizes.py [config=3] [windows=6] [capacities=2272,2400,2512,2540,2656]

Per flow scale (0, 0.5, 1.0 x ground truth): box pixels (pitch x rows) mean / p99 / max over the active units, and per
capacity the share of active units with more than one sub-band.  tests/test_gpu_eval_capacity_edges.py uses unit_boxes
and sub_bands to place its units' boxes at a capacity's edges."""
import os
import sys

import numpy as np

SCALE = 1e-3       # ebo_default_params: compensateScale
MIN_EVENTS = 100   # compensateMinNumEvents: a unit is active with more events than this


def ref_time(t_first, t_last):
    """int32 truncation of the mean of a unit's first and last timestamp (mid_timestamp, ebo_api.cpp)"""
    return int(np.int32(float(t_first + t_last) * 0.5))


def unit_centres(ev, rect, flow, scale=SCALE):
    """(pxc, pyc) of the events of the patch `rect` = (x, y, w, h) warped by `flow`: the canvas column and row of each
    event's centre tap, for the events warp_event keeps (a 7 x 7 footprint that touches the 3w x 3h canvas); and the number
    of events the patch holds.  Events are bucketed by their own pixel (the grid rule) and sorted by time."""
    rx, ry, rw, rh = (int(v) for v in rect)
    x, y = ev["x"].astype(np.int64), ev["y"].astype(np.int64)
    m = (x >= rx) & (x < rx + rw) & (y >= ry) & (y < ry + rh)
    n = int(m.sum())
    if n == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64), 0
    tp = ev["t_us"][m].astype(np.int64)
    tau = (ref_time(tp[0], tp[-1]) - tp).astype(np.float64) * scale
    cx = x[m].astype(np.float64) + tau * flow[0]
    cy = y[m].astype(np.float64) + tau * flow[1]
    pxc = np.trunc(cx).astype(np.int64) - rx + rw
    pyc = np.trunc(cy).astype(np.int64) - ry + rh
    ok = (pxc + 3 >= 0) & (pxc - 3 < 3 * rw) & (pyc + 3 >= 0) & (pyc - 3 < 3 * rh)
    return pxc[ok], pyc[ok], n


def unit_boxes(ev, rects, flows, scale=SCALE, min_events=MIN_EVENTS):
    """Per unit of the grid `rects` [P][4] (x, y, w, h) at `flows` [P][2]: (active, x0, y0, bw, rows) of the box
    eval_unit3 forms -- the warped events' centre pixels, widened by the 7 x 7 footprint and clipped by the canvas.
    bw = rows = 0 where no event lands; inactive units (min_events events or fewer) are all zero."""
    rects = np.asarray(rects)
    out = np.zeros((len(rects), 5), dtype=np.int64)
    for p, rect in enumerate(rects):
        pxc, pyc, n = unit_centres(ev, rect, flows[p], scale)
        if n <= min_events:
            continue
        out[p, 0] = 1
        if len(pxc) == 0:
            continue
        rw, rh = int(rect[2]), int(rect[3])
        x0, x1 = max(pxc.min() - 3, 0), min(pxc.max() + 3, 3 * rw - 1)
        y0, y1 = max(pyc.min() - 3, 0), min(pyc.max() + 3, 3 * rh - 1)
        out[p, 1:] = (x0, y0, x1 - x0 + 1, y1 - y0 + 1)
    return out


def pitch(bw, cap):
    """the odd pitch of the LDS image (an even one only where the odd one exceeds the capacity)"""
    return (bw | 1) if (bw | 1) <= cap else bw


def sub_bands(bw, rows, cap):
    """sequential sub-bands of a bw x rows box in an image of `cap` pixels (one row tile)"""
    if bw == 0:
        return 0
    max_rows = max(cap // pitch(bw, cap), 1)
    return -(-rows // max_rows)


def main(argv):
    pkg_dir = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
    sys.path.insert(0, pkg_dir)
    import synth

    config = int(argv[1]) if len(argv) > 1 else 3
    windows = int(argv[2]) if len(argv) > 2 else 6
    caps = [int(v) for v in (argv[3] if len(argv) > 3 else "2272,2400,2512,2540,2656").split(",")]
    cfg = synth.CONFIGS[config]
    _, _, rects = synth.grid_rects(cfg["image"], cfg["patch"])
    loaded = [synth.make_window(config, window=w) for w in range(windows)]
    print("config %d, %d windows, %d units" % (config, windows, windows * len(rects)))
    print("flows | box pixels mean / p99 / max | share of active units with > 1 sub-band at " + " / ".join(map(str, caps)))
    for s in (0.0, 0.5, 1.0):
        boxes = np.concatenate([unit_boxes(ev, rects, gt * s) for ev, gt in loaded])
        b = boxes[boxes[:, 0] == 1]
        px = np.array([pitch(int(bw), 1 << 30) * int(r) for bw, r in b[:, 3:5]])
        shares = [np.mean([sub_bands(int(bw), int(r), cap) > 1 for bw, r in b[:, 3:5]]) for cap in caps]
        print("%.1f x gt | %.0f / %.0f / %d | %s  (%d active)" % (s, px.mean(), np.percentile(px, 99), px.max(),
              " / ".join("%.2f %%" % (100 * v) for v in shares), len(b)))


if __name__ == "__main__":
    main(sys.argv)
