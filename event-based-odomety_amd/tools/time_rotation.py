#!/usr/bin/env python3
"""Times the rotational contrast maximisation (ebo_eval_rotation_device, ebo_solve_rotation) on one
device: a batched evaluation with and without the gradient, by stream events (ebo_timer_begin / _end, median of
--repeats launches after one warm-up), and a whole solve from omega = 0 by wall clock.  The yardstick is measured in the
same process on the same loaded windows: ebo_count_image_device(EBO_COUNT_WARPED), the nearest existing kernel -- one
integer add per event where the vote has four, plus the image passes and the gather.  No ratio is asserted anywhere.

Shapes: 256 windows of the reference defaults (240 x 180, 15 k events) and 128 windows of C3 (346 x 260, 200 k events),
synth.make_stream's translating windows: the timing does not depend on what the events show.

    python3 tools/time_rotation.py [--repeats 21] [--shapes default,c3] [--vote tile|global]

--vote binds the A/B build (libebo_hip_ab.so) and forces the vote's design: the shipped LDS tile per patch, or every tap
as a global atomic.  Both give the same bits (the vote image is an integer sum).

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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=21)
    ap.add_argument("--shapes", default="default,c3")
    ap.add_argument("--sigma", type=float, default=1.0)
    ap.add_argument("--vote", choices=("tile", "global"))
    args = ap.parse_args()
    if args.vote:  # the A/B build: the shipped vote (LDS tiles) or every tap as a global atomic
        os.environ["EBO_LIB_PATH"] = os.path.join(ROOT, "event-based-odomety_amd", "libebo_hip_ab.so")
        os.environ["EBO_ROTATION_TILE"] = "1" if args.vote == "tile" else "0"
    import torch  # before the library: one HIP runtime per process (tests/conftest.py)
    ebo = importlib.import_module("event-based-odomety_amd")
    synth = importlib.import_module("event-based-odomety_amd.synth")
    for shape in args.shapes.split(","):
        cfg_idx, Wn = SHAPES[shape]
        cfg = synth.CONFIGS[cfg_idx]
        ev, offsets, flows = synth.make_stream(cfg_idx, Wn)
        w, h = cfg["image"]
        cam = (200.0 * w / 240.0, 200.0 * w / 240.0, (w - 1) / 2.0, (h - 1) / 2.0)
        prm = ebo.RotationParams(args.sigma)
        with ebo.Context(image_w=w, image_h=h, patch_w=cfg["patch"][0], patch_h=cfg["patch"][1], loss=ebo.LOSS_VARIANCE,
                         tv_weight=0.0, max_windows=Wn, max_events=len(ev)) as c:
            c.set_windows(ev, offsets)
            om = np.random.default_rng(7).uniform(-3.0, 3.0, (Wn, 3))
            d_om = torch.from_numpy(om).to("cuda")
            d_r = torch.zeros(Wn, dtype=torch.float64, device="cuda")
            d_g = torch.zeros((Wn, 3), dtype=torch.float64, device="cuda")
            d_flows = torch.from_numpy(np.ascontiguousarray(flows)).to("cuda")
            d_img = torch.zeros((Wn, h, w), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()

            def timed(call):
                call()
                c.synchronize()
                ms = []
                for _ in range(args.repeats):
                    c.timer_begin()
                    call()
                    ms.append(c.timer_end())
                return statistics.median(ms)

            t_grad = timed(lambda: c.eval_rotation_device(cam, d_om.data_ptr(), d_r.data_ptr(), d_g.data_ptr(), prm))
            t_value = timed(lambda: c.eval_rotation_device(cam, d_om.data_ptr(), d_r.data_ptr(), 0, prm))
            t_count = timed(lambda: c.count_image_device(ebo.COUNT_WARPED, d_flows.data_ptr(), d_img.data_ptr()))
            t0 = time.perf_counter()
            sol, summ = c.solve_rotation(cam, prm)
            t_solve = (time.perf_counter() - t0) * 1e3
        print(json.dumps(dict(shape=shape, vote=args.vote or "shipped", windows=Wn, image=[w, h], events=int(len(ev)), sigma_blur=args.sigma,
                              eval_grad_ms=round(t_grad, 4), eval_value_ms=round(t_value, 4), count_warped_ms=round(t_count, 4),
                              grad_over_count=round(t_grad / t_count, 2), solve_wall_ms=round(t_solve, 2),
                              solve_rounds=max(s.evaluations for s in summ),
                              solve_evaluations=sum(s.evaluations for s in summ))), flush=True)


if __name__ == "__main__":
    main()
