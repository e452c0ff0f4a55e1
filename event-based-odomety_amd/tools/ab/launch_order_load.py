"""What the launch-order table (csrc/launch_order.h) costs where it is built -- at load -- and what a load followed by ONE
solve nets: two builds of the shipped library in one process, interleaved.

usage: launch_order_load.py <config> <windows> --parent LIB [--reps 7]

Per build (`parent` = LIB, `new` = this tree's libebo_hip.so), wall clock around calls that end synchronised, ms:
  resident      ebo_set_windows_device of the batch's raw events already in device memory
  host          ebo_set_windows of the same events from pageable host memory
  solve         ebo_solve_device (per-patch solve, default options) on the loaded batch
  load+solve    resident load, then one solve, timed together: what real use does with a batch
  one window    ebo_set_window of the batch's first window alone, and one value+Jacobian ebo_eval_device of it (us)
Median and best of the repetitions after one warm-up."""
import argparse
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from launch_order_ab import PKG_DIR, load_instance  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", type=int)
    ap.add_argument("windows", type=int)
    ap.add_argument("--parent", required=True)
    ap.add_argument("--reps", type=int, default=7)
    args = ap.parse_args()
    libs = [("parent", load_instance("ebo_ll_parent", os.path.abspath(args.parent))),
            ("new", load_instance("ebo_ll_new", os.path.join(PKG_DIR, "libebo_hip.so")))]
    import importlib.util
    spec = importlib.util.spec_from_file_location("ebo_ll_synth", os.path.join(PKG_DIR, "synth.py"))
    synth = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(synth)
    cfg = synth.CONFIGS[args.config]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0)), args.windows))) as pool:
        evs = [e for e, _ in pool.map(lambda w: synth.make_window(args.config, window=w), range(args.windows))]
    offs = np.zeros(args.windows + 1, dtype=np.uint64)
    offs[1:] = np.cumsum([len(e) for e in evs])
    ev = np.ascontiguousarray(np.concatenate(evs), dtype=libs[0][1].EVENT_DTYPE)
    first = ev[:int(offs[1])]
    d_raw = torch.from_numpy(ev.view(np.uint8)).to("cuda")
    stream = torch.cuda.current_stream()
    iw, ih = cfg["image"]
    pw, ph = cfg["patch"]
    S = {}
    for name, lib in libs:
        kw = dict(image_w=iw, image_h=ih, patch_w=pw, patch_h=ph, loss=lib.LOSS_VARIANCE, grad=lib.GRAD_JET, tv_weight=0.0)
        c = lib.Context(max_events=len(ev), max_windows=args.windows, **kw)
        c.set_stream(stream.cuda_stream)
        c1 = lib.Context(max_events=len(first), max_windows=1, **kw)
        c1.set_stream(stream.cuda_stream)
        nf = args.windows * c.P
        S[name] = dict(lib=lib, c=c, c1=c1, opts=lib.default_solver(mode=lib.SOLVE_INDEPENDENT),
                       d_sol=torch.zeros((nf, 2), dtype=torch.float64, device="cuda"),
                       d_stats=torch.zeros((nf, 4), dtype=torch.int32, device="cuda"),
                       d_f1=torch.zeros((c.P, 2), dtype=torch.float64, device="cuda"),
                       d_o1=torch.zeros((c.P, 3), dtype=torch.float64, device="cuda"))
    torch.cuda.synchronize()

    def wall(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    def solve(s):
        s["c"].solve_device(s["opts"], s["d_sol"].data_ptr(), s["d_stats"].data_ptr())

    def load_solve(s):
        s["c"].set_windows_device(d_raw.data_ptr(), offs)
        solve(s)

    def eval_one(s):
        for _ in range(50):
            s["c1"].eval_device(s["d_f1"].data_ptr(), 1, s["d_o1"].data_ptr())

    legs = [("resident load", lambda s: s["c"].set_windows_device(d_raw.data_ptr(), offs), 1.0, "ms"),
            ("host load", lambda s: s["c"].set_windows(ev, offs), 1.0, "ms"),
            ("solve", solve, 1.0, "ms"),
            ("load+solve", load_solve, 1.0, "ms"),
            ("one window load", lambda s: s["c1"].set_window(first), 1.0, "ms"),
            ("one window eval", eval_one, 1e3 / 50, "us")]
    print("config %d x %d windows, %d events, %d units" % (args.config, args.windows, len(ev), args.windows * (S["new"]["c"].P + 1)))
    for label, fn, k, unit in legs:
        t = {name: [] for name, _ in libs}
        for rep in range(args.reps + 1):
            for name, _ in libs:
                v = wall(lambda: fn(S[name])) * k
                if rep:
                    t[name].append(v)
        p, n = np.array(t["parent"]), np.array(t["new"])
        print("%-16s parent median %9.3f best %9.3f | new median %9.3f best %9.3f %s | median %+.3f (%+.1f %%)"
              % (label, np.median(p), p.min(), np.median(n), n.min(), unit, np.median(n) - np.median(p),
                 100.0 * (np.median(n) / np.median(p) - 1.0)), flush=True)
    for s in S.values():
        s["c"].close()
        s["c1"].close()


if __name__ == "__main__":
    main()
