#!/usr/bin/env python3
"""Times the space-sweep depth map (ebo_dsi_add_windows, ebo_dsi_depth) on one device, by stream events
(ebo_timer_begin / _end around the call, median of --repeats after one warm-up; the calls are synchronous, so the figure
holds the pose upload and the final wait) and by wall clock.  The yardstick is measured in the same process on the same
resident windows: ebo_rotation_image with no output asked for, the nearest existing kernel -- the same four fixed-point
taps per event on ONE image, where the sweep has them on every plane.  No ratio is asserted anywhere.

Shapes: 256 windows of the reference defaults (240 x 180, 15 k events) and 128 windows of C3 (346 x 260, 200 k events),
synth.make_stream's translating windows, at 64 planes.  A volume accepts 2^21 events (rule M4), fewer than either shape
holds: a timed call votes the leading windows that fit (139 and 10), through the use mask, with all of them resident.
The poses translate along x by 0.4 over the voted windows, so that the planes map a patch to different places.

    python3 tools/time_dsi.py [--repeats 11] [--shapes default,c3] [--vote tile|global] [--planes N]

--vote binds the A/B build (libebo_hip_ab.so) and forces the vote's form: the LDS tile per (patch, plane), or every tap
as a global atomic; --planes forces the planes a workgroup walks.  All give the same bits (the volume is an integer sum).

Prints one JSON line per shape."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

SHAPES = {"default": (0, 256), "c3": (3, 128)}
MAX_EVENTS = 1 << 21


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=11)
    ap.add_argument("--shapes", default="default,c3")
    ap.add_argument("--nz", type=int, default=64)
    ap.add_argument("--vote", choices=("tile", "global"))
    ap.add_argument("--planes", type=int, default=0)
    args = ap.parse_args()
    if args.vote or args.planes:  # the A/B build
        os.environ["EBO_LIB_PATH"] = os.path.join(ROOT, "event-based-odomety_amd", "libebo_hip_ab.so")
        os.environ["EBO_DSI_TILE"] = "0" if args.vote == "global" else "1"
        os.environ["EBO_DSI_PLANES"] = str(args.planes)
    import torch  # noqa: F401  before the library: one HIP runtime per process (tests/conftest.py)
    ebo = importlib.import_module("event-based-odomety_amd")
    synth = importlib.import_module("event-based-odomety_amd.synth")
    for shape in args.shapes.split(","):
        cfg_idx, Wn = SHAPES[shape]
        cfg = synth.CONFIGS[cfg_idx]
        ev, offsets, _ = synth.make_stream(cfg_idx, Wn)
        w, h = cfg["image"]
        cam = (200.0 * w / 240.0, 200.0 * w / 240.0, (w - 1) / 2.0, (h - 1) / 2.0)
        offsets = np.asarray(offsets, dtype=np.int64)
        inside = (ev["x"] >= 0) & (ev["x"] < w) & (ev["y"] >= 0) & (ev["y"] < h)
        counted = np.concatenate([[0], np.cumsum(inside)])[offsets]  # in-sensor events before each window
        voted = int(np.searchsorted(counted, MAX_EVENTS, side="right") - 1)
        use = (np.arange(Wn) < voted).astype(np.uint8)
        poses = np.zeros((Wn, 12))
        poses[:, 0] = poses[:, 4] = poses[:, 8] = 1.0
        poses[:voted, 9] = np.linspace(-0.2, 0.2, voted)
        ref = poses[voted // 2].copy()
        prm = ebo.default_depth_params(nz=args.nz)
        with ebo.Context(image_w=w, image_h=h, patch_w=cfg["patch"][0], patch_h=cfg["patch"][1], loss=ebo.LOSS_VARIANCE,
                         tv_weight=0.0, max_windows=Wn, max_events=len(ev)) as c:
            c.set_windows(ev, offsets)

            def timed(call, before=None):
                dev, wall = [], []
                for i in range(args.repeats + 1):
                    if before:
                        before()
                    c.synchronize()
                    t0 = time.perf_counter()
                    c.timer_begin()
                    call()
                    ms = c.timer_end()
                    if i:
                        dev.append(ms)
                        wall.append((time.perf_counter() - t0) * 1e3)
                return statistics.median(dev), statistics.median(wall)

            t_add = timed(lambda: c.dsi_add_windows(poses, use), before=lambda: c.dsi_begin(cam, ref, prm))
            Hq = c.dsi_volume()
            t_depth = timed(lambda: c.dsi_depth())
            kept = c.dsi_depth(max_points=0)[4]
            c.dsi_end()
            om = np.zeros((Wn, 3))
            t_rot = timed(lambda: c.rotation_image(cam, om, votes=False, image=False))
        n_ev = int(counted[voted])
        print(json.dumps(dict(shape=shape, vote=args.vote or "shipped", planes_forced=args.planes, windows_resident=Wn, windows_voted=voted,
                              image=[w, h], nz=args.nz, events_voted=n_ev, votes_sum=int(Hq.sum(dtype=np.uint64)), kept=int(kept),
                              add_windows_ms=round(t_add[0], 4), add_windows_wall_ms=round(t_add[1], 4),
                              depth_ms=round(t_depth[0], 4), depth_wall_ms=round(t_depth[1], 4),
                              rotation_image_ms=round(t_rot[0], 4), rotation_image_events=int(inside.sum()),
                              ns_per_event_plane=round(t_add[0] * 1e6 / (n_ev * args.nz), 5),
                              rotation_ns_per_event=round(t_rot[0] * 1e6 / int(inside.sum()), 5))), flush=True)


if __name__ == "__main__":
    main()
