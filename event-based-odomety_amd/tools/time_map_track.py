#!/usr/bin/env python3
"""time_map_track.py -- what ebo_map_track costs next to the same rules run serially on the host.

Three cases at 240 x 180 with a map of 3000 points seen from the identity pose, every window with its own events of that
map (8 a point, 30 % noise, blur 1) and every start displaced by 0.04 and 0.015 rad:
    64 windows x 1 start, 64 windows x 13 starts (+- 0.05 and +- 0.015 rad), 1 window x 13 starts.
Device: the median of --repeats calls after one warm-up; the kernel by stream events around ebo_map_track_device on
arrays already on the device (the poses are put back before every call, outside the bracket), the call by wall clock
around the host form ebo_map_track, uploads and downloads included.  Serial: tools/map_track_serial.cpp (g++ -O2
-ffp-contract=off), one host thread, every unit of the case one after the other, one run.  No ratio is asserted anywhere.

usage: time_map_track.py [--repeats 21] [--points 3000] [--no-serial]

Prints one JSON line per case."""
import argparse
import importlib
import json
import os
import statistics
import subprocess
import sys
import tempfile
import time

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402

GEO = dict(w=240, h=180, cam=(200.0, 200.0, 119.5, 89.5))
CASES = (("64x1", 64, 1), ("64x13", 64, 13), ("1x13", 1, 13))


def main():
    par = argparse.ArgumentParser()
    par.add_argument("--repeats", type=int, default=21)
    par.add_argument("--points", type=int, default=3000)
    par.add_argument("--no-serial", action="store_true")
    args = par.parse_args()
    import torch  # before the library: one HIP runtime per process (tests/conftest.py)
    import maptrack_ref as M
    ebo = importlib.import_module("event-based-odomety_amd")
    rng = np.random.default_rng(1)
    X = M.map_points(rng, GEO, args.points, margin=8.0)
    images = np.stack([M.event_image(GEO, M.scene_events(rng, GEO, X)) for _ in range(64)])
    firsts = [M.displaced(M.IDENTITY, rng, 0.04, 0.015) for _ in range(64)]
    o = ebo.default_map_track_opts()
    exe = None
    tmp = tempfile.TemporaryDirectory()
    if not args.no_serial:
        exe = os.path.join(tmp.name, "map_track_serial")
        subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", exe,
                               os.path.join(HERE, "map_track_serial.cpp")])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        for label, nw, ns in CASES:
            starts = np.concatenate([M.starts13(f, 0.05, 0.015)[:ns] for f in firsts[:nw]])
            ui = np.repeat(np.arange(nw), ns).astype(np.int32)
            n = len(ui)
            d_img, d_pts, d_ui, d_pose0 = dev(images[:nw]), dev(X), dev(ui), dev(starts)
            d_pose = d_pose0.clone()
            d_res = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
            torch.cuda.synchronize()

            def device_call():
                c.map_track_device(GEO["cam"], GEO["w"], GEO["h"], nw, d_img.data_ptr(), len(X), d_pts.data_ptr(), n, d_ui.data_ptr(),
                                   d_pose.data_ptr(), d_res.data_ptr(), 0.05, o)

            kernel_ms, call_ms = [], []
            for rep in range(args.repeats + 1):
                d_pose.copy_(d_pose0)
                torch.cuda.synchronize()
                c.timer_begin()
                device_call()
                ms = c.timer_end()
                t0 = time.perf_counter()
                _, res, _ = c.map_track(GEO["cam"], images[:nw], X, ui, starts, 0.05, o)
                wall = (time.perf_counter() - t0) * 1e3
                if rep:  # the first is the warm-up
                    kernel_ms.append(ms)
                    call_ms.append(wall)
            got = ebo.Context.map_track_results(d_res.cpu().numpy())
            assert [r["iterations"] for r in got] == [r["iterations"] for r in res]
            out = dict(case=label, windows=nw, starts=ns, units=n, points=len(X), image=[GEO["w"], GEO["h"]],
                       kernel_ms=round(statistics.median(kernel_ms), 4), call_ms=round(statistics.median(call_ms), 4),
                       iterations_total=int(sum(r["iterations"] for r in res)), iterations_max=int(max(r["iterations"] for r in res)),
                       evaluations_total=int(sum(r["num_evals_jac"] + r["num_evals_cost"] for r in res)),
                       terminations=[int(sum(r["termination"] == t for r in res)) for t in (0, 1, 2)])
            if exe:
                pr = M.problem(GEO, images[:nw], X, ui, starts, opts=M.default_opts())
                M.write_problem(os.path.join(tmp.name, "p.f64"), pr)
                line = subprocess.check_output([exe, os.path.join(tmp.name, "p.f64"), os.path.join(tmp.name, "r.f64"), "1"], text=True)
                ser = json.loads(line)
                assert ser["iterations"] == out["iterations_total"], (ser, out)  # the same solves
                out["serial_ms"] = round(ser["ms_median"], 2)
                out["serial_over_kernel"] = round(ser["ms_median"] / out["kernel_ms"], 1)
            print(json.dumps(out), flush=True)
    tmp.cleanup()


if __name__ == "__main__":
    main()
