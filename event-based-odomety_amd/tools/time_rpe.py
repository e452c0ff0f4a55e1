#!/usr/bin/env python3
"""time_rpe.py -- what ebo_trajectory_rpe costs next to the same rules run serially on the host.

One process.  Three cases on one noisy helix trajectory with orientations, each at deltas 1, 2, 5 and 10: one segment of
200 poses; 64 segments of 200 poses of a 12800-pose trajectory; and every prefix 3 .. 2000 of a 2000-pose trajectory
(1998 segments, 7992 units, eight million pairs), an evaluation after every keyframe done in one call.  After a warm-up,
the median of 21 calls of the kernel (events on the context's stream, ebo_two_view_timing slot 0) and of the whole call
(wall clock; the remainder is the host's checks, uploads and copies).  Next to each the single-thread time of the device's
own text compiled for the host (tools/rpe_serial.cpp, g++ -O2), which evaluates every unit of the call one after the
other: the median of 21 runs.

usage: time_rpe.py [--repeats 21] [--no-serial]
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

DELTAS = [1, 2, 5, 10]


def main():
    par = argparse.ArgumentParser()
    par.add_argument("--repeats", type=int, default=21)
    par.add_argument("--no-serial", action="store_true")
    args = par.parse_args()
    import rpe_ref as T
    ebo = importlib.import_module("event-based-odomety_amd")
    gt1, est1 = T.helix(200, 1, 1e-2)
    gt64, est64 = T.helix(12800, 2, 1e-2, span=3.0 * 64)
    gtp, estp = T.helix(2000, 3, 1e-2, span=30.0)
    cases = (("one_segment", gt1, est1, [(0, 200)]),
             ("64_segments", gt64, est64, [(200 * k, 200 * (k + 1)) for k in range(64)]),
             ("prefixes_2000", gtp, estp, [(0, k) for k in range(3, 2001)]))
    out = {"repeats": args.repeats, "deltas": DELTAS}
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        c.two_view_timing(True)
        for label, gt, est, segs in cases:
            for _ in range(2):
                res = c.trajectory_rpe(gt, est, segs, DELTAS)
            rows = []
            for _ in range(args.repeats):
                c.trajectory_rpe(gt, est, segs, DELTAS)
                ms = c.two_view_timing(True)
                rows.append((ms[0], ms[4]))
            med = np.median(np.array(rows), axis=0)
            out[label] = {"kernel_ms": round(float(med[0]), 4), "call_ms": round(float(med[1]), 4), "units": len(res),
                          "pairs": int(sum(r["count"] for r in res)), "statuses": sorted(set(r["status"] for r in res)),
                          "last_trans_rmse": float(res[-1]["trans_rmse"]), "last_rot_rmse": float(res[-1]["rot_rmse"])}
    if not args.no_serial:
        with tempfile.TemporaryDirectory() as d:
            exe = os.path.join(d, "rpe_serial")
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-o", exe,
                                   os.path.join(HERE, "rpe_serial.cpp")])
            for label, gt, est, segs in cases:
                T.write_problem(os.path.join(d, "p.f64"), gt, est, segs, DELTAS)
                r = json.loads(subprocess.check_output([exe, os.path.join(d, "p.f64"), os.path.join(d, "r.f64"), str(args.repeats)]).decode())
                out["serial_" + label] = {"ms": r["ms_median"]}
    print("%-14s %12s %12s %8s %10s %22s" % ("case", "kernel [ms]", "call [ms]", "units", "pairs", "one host thread [ms]"))
    for label, _, _, _ in cases:
        r = out[label]
        serial = "%.4f" % out["serial_" + label]["ms"] if ("serial_" + label) in out else "-"
        print("%-14s %12.4f %12.4f %8d %10d %22s" % (label, r["kernel_ms"], r["call_ms"], r["units"], r["pairs"], serial))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
