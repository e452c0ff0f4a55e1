#!/usr/bin/env python3
"""time_triangulate_tracks.py -- what ebo_triangulate_tracks and ebo_landmark_scores cost next to the same rules run
serially on the host.

One process.  Two shapes over one set of keyframes, every landmark seen by a run of consecutive keyframes with pixel
noise 0.3 at f = 200 and a planted outlier in a third of the longer tracks: a live map, 2 000 landmarks of 2-10
observations, and a recording's worth, 200 000 landmarks of 2-24 observations.  After a warm-up, the median of
`repeats` calls of the kernel (events on the context's stream, ebo_two_view_timing slot 0) and of the whole call (wall
clock; the remainder is the host's checks, uploads and copies), for the triangulation and for the audit of its points.
Next to each the single-thread time of the device's own rule functions compiled for the host
(tools/landmark_serial.cpp, g++ -O2), one landmark after the other.

--lanes 16 | 64 binds the A/B build (libebo_hip_ab.so) and forces the lanes per landmark: four landmarks per wave or a
wave per landmark (csrc/ebo_landmark.inc).

usage: time_triangulate_tracks.py [--repeats 21] [--serial-repeats 3] [--no-serial] [--lanes 16|64]
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

SHAPES = (("live_map", 2000, 2, 10), ("recording", 200000, 2, 24))


def make_shape(L, seed, n, lo, hi):
    """n landmarks of lo .. hi observations over 24 keyframes, built without a Python loop per landmark."""
    rng = np.random.default_rng(seed)
    K = 24
    P = L.make_keyframes(rng, K)
    counts = rng.integers(lo, hi + 1, size=n)
    offsets = np.concatenate([[0], np.cumsum(counts)]).astype(np.int32)
    total = int(offsets[-1])
    lm = np.repeat(np.arange(n), counts)
    within = np.arange(total) - offsets[lm]
    first = (rng.uniform(size=n) * (K - counts + 1)).astype(np.int64)
    k = (first[lm] + within).astype(np.int32)
    mid = P[:, :, 3].mean(axis=0)
    X = mid + np.stack([rng.uniform(-3.0, 3.0, n), rng.uniform(-0.5, 0.5, n), rng.uniform(2.0, 6.0, n)], axis=1)
    xc = np.einsum("oji,oj->oi", P[k][:, :, :3], X[lm] - P[k][:, :, 3])
    uv = L.FOCAL * xc[:, :2] / xc[:, 2:3] + rng.normal(size=(total, 2)) * 0.3
    # a planted outlier, 40 px off, as the last observation of a third of the tracks with more than three
    last = offsets[1:] - 1
    hit = last[(counts > 3) & (rng.uniform(size=n) < 1.0 / 3.0)]
    uv[hit, 1] += 40.0
    f = np.concatenate([uv / L.FOCAL, np.ones((total, 1))], axis=1)
    return dict(poses=P, offsets=offsets, obs_pose=k, obs_f=f / np.linalg.norm(f, axis=1, keepdims=True))


def main():
    par = argparse.ArgumentParser()
    par.add_argument("--repeats", type=int, default=21)
    par.add_argument("--serial-repeats", type=int, default=3)
    par.add_argument("--no-serial", action="store_true")
    par.add_argument("--lanes", choices=("16", "64"))
    args = par.parse_args()
    if args.lanes:
        os.environ["EBO_LIB_PATH"] = os.path.join(ROOT, "event-based-odomety_amd", "libebo_hip_ab.so")
        os.environ["EBO_LANDMARK_LANES"] = args.lanes
    import landmark_ref as L
    ebo = importlib.import_module("event-based-odomety_amd")
    shapes = [(label, make_shape(L, 50 + i, n, lo, hi)) for i, (label, n, lo, hi) in enumerate(SHAPES)]
    out = {"repeats": args.repeats, "lanes": args.lanes or "default"}
    points = {}
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        c.two_view_timing(True)
        for label, b in shapes:
            tri = lambda: c.triangulate_tracks(b["poses"], b["offsets"], b["obs_pose"], b["obs_f"], scores=False, flags=False)
            res = tri()
            points[label] = np.where(res["status"][:, None] == 0, res["point"], 1.0)
            aud = lambda: c.landmark_scores(b["poses"], b["offsets"], b["obs_pose"], b["obs_f"], points[label], scores=False, flags=False)
            for what, fn in (("triangulate", tri), ("audit", aud)):
                r = fn()
                rows = []
                for _ in range(args.repeats):
                    fn()
                    ms = c.two_view_timing(True)
                    rows.append((ms[0], ms[4]))
                med = np.median(np.array(rows), axis=0)
                out["%s_%s" % (what, label)] = {"kernel_ms": round(float(med[0]), 4), "call_ms": round(float(med[1]), 4),
                                                "landmarks": len(r["status"]), "observations": int(b["offsets"][-1]),
                                                "statuses": np.bincount(r["status"], minlength=6).tolist()}
    if not args.no_serial:
        prm = L.default_params()
        with tempfile.TemporaryDirectory() as d:
            exe = os.path.join(d, "landmark_serial")
            subprocess.check_call(["g++", "-std=c++17", "-O2", "-ffp-contract=off", "-Wno-unknown-pragmas", "-o", exe,
                                   os.path.join(HERE, "landmark_serial.cpp")])
            for label, b in shapes:
                for what, pts in (("triangulate", None), ("audit", points[label])):
                    L.write_problem(os.path.join(d, "p.f64"), b, prm, pts)
                    r = json.loads(subprocess.check_output([exe, os.path.join(d, "p.f64"), os.path.join(d, "r.f64"),
                                                            str(args.serial_repeats)]).decode())
                    out["serial_%s_%s" % (what, label)] = {"ms": r["ms_median"]}
    print("%-24s %12s %12s %10s %12s %22s" % ("case", "kernel [ms]", "call [ms]", "landmarks", "observations", "one host thread [ms]"))
    for label, _ in shapes:
        for what in ("triangulate", "audit"):
            key = "%s_%s" % (what, label)
            r = out[key]
            serial = "%.3f" % out["serial_" + key]["ms"] if ("serial_" + key) in out else "-"
            print("%-24s %12.4f %12.4f %10d %12d %22s" % (key, r["kernel_ms"], r["call_ms"], r["landmarks"], r["observations"], serial))
    print(json.dumps(out))


if __name__ == "__main__":
    main()
