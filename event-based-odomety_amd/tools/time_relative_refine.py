#!/usr/bin/env python3
"""time_relative_refine.py -- what ebo_relative_pose_refine costs next to the same rules run serially on the host.

One process.  One keyframe pair (about 150 listed inliers of 190 correspondences, 0.3 px noise, the model a perturbed
truth; ebo_default_ba_opts) and 64 such pairs in one call.  After a warm-up, the median of 21 calls of the kernel (events
on the context's stream, ebo_two_view_timing slot 0) and of the whole call (wall clock; the remainder is the host's
checks, uploads and copies).  Next to each the single-thread time of the device's own text compiled for the host
(tools/relpose_refine_serial.cpp, g++ -O2), which solves every pair of the call one after the other: the median of 21
runs.

usage: time_relative_refine.py [--pairs 64] [--inliers 150] [--repeats 21] [--no-serial]
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
    par.add_argument("--pairs", type=int, default=64)
    par.add_argument("--inliers", type=int, default=150)
    par.add_argument("--repeats", type=int, default=21)
    par.add_argument("--no-serial", action="store_true")
    args = par.parse_args()
    import relpose_ref as R
    ebo = importlib.import_module("event-based-odomety_amd")
    rng = np.random.default_rng(5)
    pairs = []
    for i in range(args.pairs):
        m = args.inliers + int(rng.integers(-10, 11))
        pairs.append(R.clean_pair(900 + i, m, n=m + 40, rot=0.006, trans=0.03, order="shuffled"))
    cases = (("one_pair", pairs[:1]), ("%d_pairs" % args.pairs, pairs))
    out = {"inliers": args.inliers, "repeats": args.repeats}
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        c.two_view_timing(True)
        for label, prs in cases:
            for _ in range(2):
                res = c.relative_pose_refine(prs)
            rows = []
            for _ in range(args.repeats):
                c.relative_pose_refine(prs)
                ms = c.two_view_timing(True)
                rows.append((ms[0], ms[4]))
            med = np.median(np.array(rows), axis=0)
            its = [r["summary"]["iterations"] for r in res]
            out[label] = {"kernel_ms": round(float(med[0]), 4), "call_ms": round(float(med[1]), 4),
                          "listed_inliers": int(sum(len(p["idx"]) for p in prs)), "iterations_mean": round(float(np.mean(its)), 2),
                          "terminations": sorted(set(r["summary"]["termination"] for r in res))}
    if not args.no_serial:
        with tempfile.TemporaryDirectory() as d:
            exe = os.path.join(d, "relpose_refine_serial")
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-o", exe,
                                   os.path.join(HERE, "relpose_refine_serial.cpp")])
            for label, prs in cases:
                R.write_problem(os.path.join(d, "p.f64"), prs, R.default_opts())
                r = json.loads(subprocess.check_output([exe, os.path.join(d, "p.f64"), os.path.join(d, "r.f64"), str(args.repeats)]).decode())
                out["serial_" + label] = {"ms": r["ms_median"], "iterations": r["iterations"]}
    print("%-12s %12s %12s %16s %12s %22s" % ("case", "kernel [ms]", "call [ms]", "listed inliers", "iterations", "one host thread [ms]"))
    for label, _ in cases:
        r = out[label]
        serial = "%.4f" % out["serial_" + label]["ms"] if ("serial_" + label) in out else "-"
        print("%-12s %12.4f %12.4f %16d %12.2f %22s" % (label, r["kernel_ms"], r["call_ms"], r["listed_inliers"], r["iterations_mean"], serial))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
