#!/usr/bin/env python3
"""time_abs_pose.py -- what ebo_absolute_pose_ransac costs, phase by phase, next to the serial loop on the host.

One process.  One keyframe (n = 200 points, 30 % outliers, 1000 hypotheses) and 64 keyframes in one call; after a warm-up,
the median of 21 calls of: the hypothesis kernel, the counting kernel, the host walk, the inlier list (events on the
context's stream, ebo_two_view_timing) and the whole call (wall clock; the remainder is uploads and copies).  Next to
it the single-thread time of the same rules compiled for the host (tools/abs_pose_serial.cpp, g++ -O2) with the serial
early stop: the honest comparison, since the serial loop stops after some ten hypotheses where the device
evaluates all 1000.

usage: time_abs_pose.py [--frames 64] [--n 200] [--hypotheses 1000] [--repeats 21] [--no-serial]
Prints a table and one JSON line."""
import argparse
import importlib
import json
import os
import subprocess
import sys
import tempfile

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(os.path.dirname(HERE))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402


def main():
    par = argparse.ArgumentParser()
    par.add_argument("--frames", type=int, default=64)
    par.add_argument("--n", type=int, default=200)
    par.add_argument("--hypotheses", type=int, default=1000)
    par.add_argument("--repeats", type=int, default=21)
    par.add_argument("--no-serial", action="store_true")
    args = par.parse_args()
    import abspose_ref as apr
    ebo = importlib.import_module("event-based-odomety_amd")
    scenes = [apr.make_scene(100 + i, args.n, 0.3, 0.3) for i in range(args.frames)]
    prm = ebo.two_view_params(seed=apr.RANSAC_SEED, max_iterations=args.hypotheses, threshold=apr.THRESHOLD)
    names = ("hypotheses", "counting", "host_walk", "inlier_list", "call")
    out = {"n": args.n, "hypotheses": args.hypotheses, "repeats": args.repeats}
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        c.two_view_timing(True)
        for label, k in (("one_frame", 1), ("%d_frames" % args.frames, args.frames)):
            f1 = np.concatenate([s["f"] for s in scenes[:k]])
            f2 = np.concatenate([s["points"] for s in scenes[:k]])
            offsets = np.arange(k + 1) * args.n
            for _ in range(3):
                res = c.absolute_pose_ransac(offsets, f1, f2, prm)
            rows = []
            for _ in range(args.repeats):
                c.absolute_pose_ransac(offsets, f1, f2, prm)
                rows.append(c.two_view_timing(True))
            med = np.median(np.array(rows), axis=0)
            out[label] = dict(zip(names, (round(float(v), 4) for v in med)))
            out[label]["iterations"] = [r["iterations"] for r in res][:8]
            out[label]["found"] = int(sum(r["found"] for r in res))
    if not args.no_serial:
        with tempfile.TemporaryDirectory() as d:
            exe = os.path.join(d, "abs_pose_serial")
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe, os.path.join(HERE, "abs_pose_serial.cpp")])
            ms, its = [], []
            for i, s in enumerate(scenes[:min(args.frames, 8)]):
                s["f"].tofile(os.path.join(d, "f1.f64"))
                s["points"].tofile(os.path.join(d, "f2.f64"))
                r = json.loads(subprocess.check_output([exe, os.path.join(d, "f1.f64"), os.path.join(d, "f2.f64"), str(apr.RANSAC_SEED),
                                                        str(i), str(args.hypotheses), str(args.repeats), repr(apr.THRESHOLD)]).decode())
                ms.append(r["ms_median"])
                its.append(r["iterations"])
            out["serial_host"] = {"ms_first_frame": ms[0], "ms_mean_per_frame": round(float(np.mean(ms)), 4), "iterations": its}
    print("%-12s %12s %12s %12s %12s %12s" % (("phase [ms]",) + names))
    for label in [k for k in out if isinstance(out[k], dict) and "call" in out[k]]:
        print("%-12s %12.4f %12.4f %12.4f %12.4f %12.4f" % ((label,) + tuple(out[label][k] for k in names)))
    if "serial_host" in out:
        print("serial host loop, one thread: %.4f ms for the first frame (%d hypotheses), %.4f ms per frame over %d frames" % (
            out["serial_host"]["ms_first_frame"], out["serial_host"]["iterations"][0], out["serial_host"]["ms_mean_per_frame"],
            len(out["serial_host"]["iterations"])))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
