#!/usr/bin/env python3
"""time_align.py -- what ebo_align_sim3 costs next to the same rules run serially on the host.

One process.  Three cases on one noisy helix trajectory: one segment of 200 poses; 64 segments of 200 poses of a
12800-pose trajectory; and every prefix 3 .. 2000 of a 2000-pose trajectory (1998 segments, two million points read),
what the reference computes one keyframe at a time.  After a warm-up, the median of 21 calls of the kernel (events on
the context's stream, ebo_two_view_timing slot 0) and of the whole call (wall clock; the remainder is the host's
checks, uploads and copies).  Next to each the single-thread time of the device's own text compiled for the host
(tools/align_sim3_serial.cpp, g++ -O2), which aligns every segment of the call one after the other: the median of 21
runs.

usage: time_align.py [--repeats 21] [--no-serial]
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
    par.add_argument("--repeats", type=int, default=21)
    par.add_argument("--no-serial", action="store_true")
    args = par.parse_args()
    import align_ref as A
    ebo = importlib.import_module("event-based-odomety_amd")
    gt1, est1 = A.trajectory(200)
    gt64, est64 = A.trajectory(12800, span=3.0 * 64)
    gtp, estp = A.trajectory(2000, span=30.0)
    cases = (("one_segment", gt1, est1, [(0, 200)]),
             ("64_segments", gt64, est64, [(200 * k, 200 * (k + 1)) for k in range(64)]),
             ("prefixes_2000", gtp, estp, [(0, k) for k in range(3, 2001)]))
    out = {"repeats": args.repeats}
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        c.two_view_timing(True)
        for label, gt, est, segs in cases:
            for _ in range(2):
                res = c.align_sim3(gt, est, segs)
            rows = []
            for _ in range(args.repeats):
                c.align_sim3(gt, est, segs)
                ms = c.two_view_timing(True)
                rows.append((ms[0], ms[4]))
            med = np.median(np.array(rows), axis=0)
            out[label] = {"kernel_ms": round(float(med[0]), 4), "call_ms": round(float(med[1]), 4), "segments": len(segs),
                          "points_read": int(sum(e - b for b, e in segs)), "statuses": sorted(set(r["status"] for r in res)),
                          "last_rmse": float(res[-1]["rmse"])}
    if not args.no_serial:
        with tempfile.TemporaryDirectory() as d:
            exe = os.path.join(d, "align_sim3_serial")
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-o", exe,
                                   os.path.join(HERE, "align_sim3_serial.cpp")])
            for label, gt, est, segs in cases:
                A.write_problem(os.path.join(d, "p.f64"), gt, est, segs, False)
                r = json.loads(subprocess.check_output([exe, os.path.join(d, "p.f64"), os.path.join(d, "r.f64"), str(args.repeats)]).decode())
                out["serial_" + label] = {"ms": r["ms_median"]}
    print("%-14s %12s %12s %10s %12s %22s" % ("case", "kernel [ms]", "call [ms]", "segments", "points read", "one host thread [ms]"))
    for label, _, _, _ in cases:
        r = out[label]
        serial = "%.4f" % out["serial_" + label]["ms"] if ("serial_" + label) in out else "-"
        print("%-14s %12.4f %12.4f %10d %12d %22s" % (label, r["kernel_ms"], r["call_ms"], r["segments"], r["points_read"], serial))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
