#!/usr/bin/env python3
"""time_track_errors.py -- what ebo_track_errors costs next to the same rules run serially on the host.

One process.  Three cases, each at the thresholds 1, 2, 5 and 10 px, against ground-truth tracks of 48 frame samples
(2 s of a DAVIS at 24 frames a second): one track of 2000 samples; 100 tracks of 2000 samples (400 units, 200 000
samples); and 100 prefixes of one 2000-sample track, 20, 40, .., 2000 samples long (tracks that die at different ages).
After a warm-up, the median of 21 calls of the kernel (events on the context's stream, ebo_two_view_timing slot 0) and
of the whole call (wall clock; the remainder is the host's checks, uploads and copies).  Next to each the single-thread
time of the device's own text compiled for the host (tools/track_errors_serial.cpp, g++ -O2), which evaluates every unit
of the call one after the other: the median of 21 runs; its results must equal the device's bit for bit.

usage: time_track_errors.py [--repeats 21] [--no-serial]
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

TAUS = [1.0, 2.0, 5.0, 10.0]
SAMPLES = 2000
FRAMES = 48


def drifting(V, gt, n, seed):
    """An estimated track of n samples that drifts away from the ground truth by up to 12 px over its life."""
    t, xy = V.est_track(gt, n, seed, noise=0.4)
    drift = np.linspace(0.0, 12.0, n) * (0.3 + 0.7 * ((seed * 37) % 100) / 100.0)
    return t, xy + np.stack([drift, -0.5 * drift], axis=1)


def main():
    par = argparse.ArgumentParser()
    par.add_argument("--repeats", type=int, default=21)
    par.add_argument("--no-serial", action="store_true")
    args = par.parse_args()
    import trackerr_ref as V
    ebo = importlib.import_module("event-based-odomety_amd")
    gts = [V.gt_track(FRAMES, 1000 + k) for k in range(100)]
    ests = [drifting(V, g, SAMPLES, 2000 + k) for k, g in enumerate(gts)]
    long_t, long_xy = ests[0]
    prefixes = [(long_t[:20 * (k + 1)], long_xy[:20 * (k + 1)]) for k in range(100)]
    cases = (("one_track", ests[:1], gts[:1]), ("100_tracks", ests, gts), ("100_prefixes", prefixes, gts[:1] * 100))
    out = {"repeats": args.repeats, "taus": TAUS}
    device = {}
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        c.two_view_timing(True)
        for label, ee, gg in cases:
            for _ in range(2):
                res = c.track_errors(ee, gg, TAUS)
            rows = []
            for _ in range(args.repeats):
                c.track_errors(ee, gg, TAUS)
                ms = c.two_view_timing(True)
                rows.append((ms[0], ms[4]))
            med = np.median(np.array(rows), axis=0)
            device[label] = res
            out[label] = {"kernel_ms": round(float(med[0]), 4), "call_ms": round(float(med[1]), 4), "units": len(res),
                          "samples": int(sum(len(t) for t, _ in ee)), "inliers": int(sum(r["n_inliers"] for r in res)),
                          "statuses": sorted(set(r["status"] for r in res)), "cut": int(sum(r["cut"] >= 0 for r in res))}
    if not args.no_serial:
        with tempfile.TemporaryDirectory() as d:
            exe = os.path.join(d, "track_errors_serial")
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-I", os.path.join(ROOT, "include"), "-o", exe,
                                   os.path.join(HERE, "track_errors_serial.cpp")])
            for label, ee, gg in cases:
                V.write_problem(os.path.join(d, "p.bin"), ee, gg, TAUS)
                r = json.loads(subprocess.check_output([exe, os.path.join(d, "p.bin"), os.path.join(d, "r.bin"), str(args.repeats)]).decode())
                got, _ = V.read_result(os.path.join(d, "r.bin"), len(device[label]), out[label]["samples"])
                out["serial_" + label] = {"ms": r["ms_median"], "equal": all(V.same_result(a, b) for a, b in zip(got, device[label]))}
    print("%-14s %12s %12s %8s %10s %10s %22s" % ("case", "kernel [ms]", "call [ms]", "units", "samples", "inliers", "one host thread [ms]"))
    for label, _, _ in cases:
        r = out[label]
        serial = "%.4f" % out["serial_" + label]["ms"] if ("serial_" + label) in out else "-"
        print("%-14s %12.4f %12.4f %8d %10d %10d %22s" % (label, r["kernel_ms"], r["call_ms"], r["units"], r["samples"], r["inliers"], serial))
    print(json.dumps(out))
    if any(not v.get("equal", True) for k, v in out.items() if k.startswith("serial_")):
        sys.exit("the host build of the device text differs from the device")


if __name__ == "__main__":
    main()
