"""The launch order of a batch's units (csrc/launch_order.h), measured: k_eval3 and k_solve_independent over the same
windows with the units handed out in index order, heaviest first (the default) and lightest first (the expected worst
case), all in ONE process on one GPU, the variants interleaved so that clock drift hits them alike.

usage: launch_order_ab.py <config> <windows> [--what eval|solve|both] [--reps 5] [--launches 40] [--parent LIB]

The three orders come from libebo_hip_ab.so (EBO_EVAL_ORDER, read when the windows are loaded: every variant loads them
into a context of its own); `shipped` is libebo_hip.so; `--parent LIB` adds another build of the shipped library, e.g.
the parent commit's, as `parent`.  Prints per variant the median and the range of the per-launch time over the
repetitions, and whether every variant's output has the bits of the first.  No oracle involved."""
import argparse
import importlib.util
import os
import sys

import numpy as np
import torch

PKG_DIR = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
ROOT = os.path.dirname(PKG_DIR)
sys.path.insert(0, ROOT)


def load_instance(name, lib_path=None):
    """One more instance of the ctypes plumbing, bound to lib_path (a name ending in _ab binds libebo_hip_ab.so)."""
    if lib_path:
        os.environ["EBO_LIB_PATH"] = lib_path
    else:
        os.environ.pop("EBO_LIB_PATH", None)
    pkg = os.path.join(PKG_DIR, "__init__.py")
    spec = importlib.util.spec_from_file_location(name, pkg, submodule_search_locations=[PKG_DIR])
    mod = importlib.util.module_from_spec(spec)
    sys.modules[name] = mod
    spec.loader.exec_module(mod)
    mod.lib()
    os.environ.pop("EBO_LIB_PATH", None)
    return mod


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("config", type=int)
    ap.add_argument("windows", type=int)
    ap.add_argument("--what", choices=("eval", "solve", "both"), default="eval")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--launches", type=int, default=40)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--c4-rows", type=int, default=0, help="load only the first N grid rows of every window through "
                    "set_patches, as the c4 workload's shards are (0: whole windows through set_windows)")
    args = ap.parse_args()

    shipped = load_instance("ebo_lo_shipped", os.path.join(PKG_DIR, "libebo_hip.so"))
    ab = load_instance("ebo_lo_ab")
    variants = [("index", ab, "index"), ("heaviest", ab, None), ("light", ab, "light"), ("shipped", shipped, None)]
    if args.parent:
        variants.insert(0, ("parent", load_instance("ebo_lo_parent", os.path.abspath(args.parent)), None))
    spec = importlib.util.spec_from_file_location("ebo_lo_synth", os.path.join(PKG_DIR, "synth.py"))
    synth = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(synth)

    cfg = synth.CONFIGS[args.config]
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0)), args.windows))) as pool:
        made = list(pool.map(lambda w: synth.make_window(args.config, window=w), range(args.windows)))
    gt = np.stack([g for _, g in made])
    iw, ih = cfg["image"]
    pw, ph = cfg["patch"]
    rects = offs = None
    if args.c4_rows:
        npx, npy, all_rects = synth.grid_rects(cfg["image"], cfg["patch"])
        rows = min(args.c4_rows, npy)
        evs, cnts = [], []
        for e, _ in made:
            gx = np.minimum(e["x"] // pw, npx - 1)
            gy = np.minimum(e["y"] // ph, npy - 1)
            sel = np.flatnonzero(gy < rows)
            pid = gy[sel] * npx + gx[sel]
            o = np.argsort(pid, kind="stable")
            evs.append(e[sel[o]])
            cnts.append(np.bincount(pid, minlength=rows * npx))
        ev = np.concatenate(evs)
        offs = np.zeros(args.windows * rows * npx + 1, dtype=np.uint64)
        offs[1:] = np.cumsum(np.concatenate(cnts))
        rects = np.tile(all_rects[:rows * npx], (args.windows, 1))
        gt = gt[:, :rows * npx]
    else:
        ev = np.concatenate([e for e, _ in made])
        offs = np.zeros(args.windows + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(e) for e, _ in made])
    del made

    stream = torch.cuda.current_stream()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ctxs = []
    for name, lib, order in variants:
        if order:
            os.environ["EBO_EVAL_ORDER"] = order
        else:
            os.environ.pop("EBO_EVAL_ORDER", None)
        ctx = lib.Context(image_w=iw, image_h=ih, patch_w=pw, patch_h=ph, loss=lib.LOSS_VARIANCE, grad=lib.GRAD_JET,
                          tv_weight=0.0, max_events=len(ev), max_windows=args.windows)
        ctx.set_stream(stream.cuda_stream)
        if rects is not None:
            ctx.set_patches(ev, offs, rects)
        else:
            ctx.set_windows(ev, offs)
        ctxs.append(ctx)
    os.environ.pop("EBO_EVAL_ORDER", None)
    nf = gt.shape[0] * gt.shape[1]
    n_ev = np.array([ctxs[0].patch_info(p, w)[0] for w in range(ctxs[0].n_windows) for p in range(ctxs[0].cur_patches)])
    print("config %d x %d windows: %d events, %d flow slots; events per unit min %d mean %.0f max %d"
          % (args.config, args.windows, len(ev), nf, n_ev.min(), n_ev.mean(), n_ev.max()), flush=True)

    def timed(fn, launches):
        torch.cuda.synchronize()
        e0.record(stream)
        for _ in range(launches):
            fn()
        e1.record(stream)
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / launches

    cases = []
    if args.what in ("eval", "both"):
        cases += [("eval jac %.1f x gt" % s, s, 1) for s in (0.0, 0.5, 1.0)] + [("eval value 0.5 x gt", 0.5, 0)]
    if args.what in ("solve", "both"):
        cases += [("solve_device", None, None)]
    d_out = torch.zeros((nf, 3), dtype=torch.float64, device="cuda")
    d_sol = torch.zeros((nf, 2), dtype=torch.float64, device="cuda")
    d_stats = torch.zeros((nf, 4), dtype=torch.int32, device="cuda")
    for label, scale, jac in cases:
        solve = scale is None
        d_flows = None if solve else torch.from_numpy(np.ascontiguousarray(gt * scale)).to("cuda")
        launches = max(1, args.launches // 10) if solve else args.launches
        times = {name: [] for name, _, _ in variants}
        outs = {}
        for rep in range(args.reps + 1):  # (the first repetition is the warm-up)
            for (name, lib, _), ctx in zip(variants, ctxs):
                if solve:
                    opts = lib.default_solver(mode=lib.SOLVE_INDEPENDENT)
                    fn = lambda: ctx.solve_device(opts, d_sol.data_ptr(), d_stats.data_ptr())
                else:
                    fn = lambda: ctx.eval_device(d_flows.data_ptr(), jac, d_out.data_ptr())
                t = timed(fn, launches)
                if rep:
                    times[name].append(t)
                else:
                    outs[name] = ((d_sol.cpu().numpy().copy(), d_stats.cpu().numpy().copy()) if solve
                                  else (d_out.cpu().numpy().copy(),))
        first = variants[0][0]
        for name, _, _ in variants:
            v = np.array(times[name])
            same = all(np.array_equal(a, b) for a, b in zip(outs[name], outs[first]))
            print("%-22s %-9s median %8.4f ms  min %8.4f  max %8.4f  (%+.2f %% vs %s)  bits %s"
                  % (label, name, np.median(v), v.min(), v.max(),
                     100.0 * (np.median(v) / np.median(times[first]) - 1.0), first, "same" if same else "DIFFER"), flush=True)
    for ctx in ctxs:
        ctx.close()


if __name__ == "__main__":
    main()
