"""Replaying a recording: ms per window for reference-default windows (240x180, 20x20 patches, 15 000 events, edge
loss + TV, EBO_SOLVE_GLOBAL), every window with both of the reference's images (compensated and integrated).
  (a) today's per-window path: ebo_compensate_events_contrast, then ebo_set_window + ebo_count_image(INTEGRATED)
  (b) ebo_compensate_windows at 16, 64 and 256 windows per chunk (and at 256 without images: what the images cost)
  (c) the facade's tools::EventPump at windowBatch 1, 64 and 256 (tests/cpp/replay_batch_test.cpp, `time` mode)
usage: time_replay.py [--windows N] [--parts abc] [--driver-timeout S]"""
import argparse
import importlib
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
ebo = importlib.import_module("event-based-odomety_amd")
synth = importlib.import_module("event-based-odomety_amd.synth")
LIBDIR = os.path.join(ROOT, "event-based-odomety_amd")
KW = dict(image_w=240, image_h=180, patch_w=20, patch_h=20, loss=ebo.LOSS_EDGE)


def per_window(ev, offsets, n):
    with ebo.Context(**KW, max_events=15000, max_windows=1) as c:
        opts = ebo.default_solver()
        best = None
        for rep in range(2):  # the first pass loads the code objects and sizes the work tables
            t0 = time.perf_counter()
            for w in range(n):
                sub = ev[int(offsets[w]):int(offsets[w + 1])]
                c.compensate_events_contrast(sub, opts)
                c.set_window(sub)
                c.count_image(ebo.COUNT_INTEGRATED)
            dt = time.perf_counter() - t0
            best = dt if rep == 0 or dt < best else best
    return best * 1e3 / n


def batched(ev, offsets, n, chunk, images=True):
    with ebo.Context(**KW, max_events=15000 * chunk, max_windows=chunk) as c:
        opts = ebo.default_solver()
        best = None
        for rep in range(2):
            t0 = time.perf_counter()
            _, _, _, _, status = c.compensate_windows(ev, offsets[:n + 1], opts, images=images)
            dt = time.perf_counter() - t0
            assert not status.any()
            best = dt if rep == 0 or dt < best else best
    return best * 1e3 / n


def facade(ev, batches, timeout_s):
    with tempfile.TemporaryDirectory() as tmp:
        exe = os.path.join(tmp, "replay_batch_test")
        subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", exe,
                               os.path.join(ROOT, "tests", "cpp", "replay_batch_test.cpp"),
                               "-L" + LIBDIR, "-lebo_hip", "-Wl,-rpath," + LIBDIR, "-Wl,-rpath,/opt/rocm/lib"])
        rec = os.path.join(tmp, "recording.bin")
        ebo.write_events_bin(rec, ev)
        out = subprocess.run(["timeout", "-k", "10", str(timeout_s), exe, "time", rec] + [str(b) for b in batches],
                             capture_output=True, text=True)
        if out.returncode:
            raise SystemExit("replay_batch_test time: exit %d\n%s%s" % (out.returncode, out.stdout, out.stderr))
        return out.stdout


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--windows", type=int, default=512)
    ap.add_argument("--parts", default="abc")
    ap.add_argument("--driver-timeout", type=int, default=900)
    a = ap.parse_args()
    cfg = dict(name="reference default", image=(240, 180), patch=(20, 20), events=15000, index=0)
    ev, offsets, _ = synth.make_stream(cfg, a.windows)
    print("recording: %d windows of 15000 events, edge loss + TV, EBO_SOLVE_GLOBAL" % a.windows, flush=True)
    if "a" in a.parts:
        n = min(a.windows, 64)
        print("(a) per-window calls            : %.4f ms/window (%d windows)" % (per_window(ev, offsets, n), n), flush=True)
    if "b" in a.parts:
        for chunk in (16, 64, 256):
            print("(b) ebo_compensate_windows %3d   : %.4f ms/window" % (chunk, batched(ev, offsets, a.windows, chunk)),
                  flush=True)
        print("(b) ebo_compensate_windows 256, flows only (no images): %.4f ms/window"
              % batched(ev, offsets, a.windows, 256, images=False), flush=True)
    if "c" in a.parts:
        print("(c) EventPump (facade):", flush=True)
        sys.stdout.write(facade(ev, (1, 64, 256), a.driver_timeout))


if __name__ == "__main__":
    main()
