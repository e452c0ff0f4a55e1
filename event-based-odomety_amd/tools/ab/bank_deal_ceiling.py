"""What a bank deal of ZERO cost is worth to k_eval3: the dealt order of lds_conflict_model.py is
computed on the host for the very flows that are evaluated, the windows are loaded in it (A/B library, EBO_KEEP_ORDER=1:
a unit keeps its list order; host bucketing, which is stable) and the UNCHANGED kernel is timed against the canonical
load, by tools/ab_eval.py's method (3 launches, then 20 timed ones by events on the stream), alternating, two repetitions.
The value image is an integer sum, so r must have the same bits in every order; J differs by summation order only.

    bank_deal_ceiling.py [config=3] [windows=128] [flow scale=0.5] [block=128] [capacity=2542]
    bank_deal_ceiling.py ... --pmc <order> [--launches 3]    one load, a few launches: the program of a counter run
        (rocprofv3 --pmc SQ_LDS_IDX_ACTIVE SQ_LDS_BANK_CONFLICT SQ_WAIT_INST_LDS SQ_BUSY_CYCLES, summarised by pmc_summary.py)
    --cache DIR keeps the prepared event lists between calls

orders: library (the library's own canonical order, no switch), canonical (the same order computed here and kept: the
control of the method), deal32 / deal16 (sorted by the residue of the first tap's word modulo 32 / 16 and dealt)."""
import importlib
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
os.environ.setdefault("EBO_LIB_PATH", os.path.join(ROOT, "event-based-odomety_amd", "libebo_hip_ab.so"))
ebo = importlib.import_module("event-based-odomety_amd")
synth = importlib.import_module("event-based-odomety_amd.synth")
import lds_conflict_model as model

ORDERS = ("library", "canonical", "deal32", "deal16")


def ordered_window(ev, gt, cfg, rects, scale, block, cap):
    """{order: the window's events, units in grid order, each unit's events in that order}"""
    out = {k: [] for k in ORDERS[1:]}
    for p, pos in enumerate(model.window_units(ev, cfg["image"], cfg["patch"])):
        evu = ev[pos]
        idx, base = model.unit_base_words(evu, rects[p], gt[p] * scale, cap)
        canon = evu[idx]
        out["canonical"].append(canon)
        for mod in (32, 16):
            out["deal%d" % mod].append(canon[model.dealt_order(base, block, mod)] if len(base) > model.MIN_EVENTS else canon)
    return {k: np.concatenate(v) for k, v in out.items()}


def prepare(config, windows, scale, block, cap, cache):
    tag = "c%d_w%d_s%g_b%d_%d" % (config, windows, scale, block, cap)
    path = os.path.join(cache, tag + ".npz") if cache else None
    if path and os.path.exists(path):
        z = np.load(path)
        return {k: z[k] for k in ORDERS}, z["offsets"], z["gt"]
    cfg = synth.CONFIGS[config]
    _, _, rects = synth.grid_rects(cfg["image"], cfg["patch"])
    from concurrent.futures import ThreadPoolExecutor

    def one(w):
        ev, gt = synth.make_window(config, window=w)
        d = ordered_window(ev, gt, cfg, rects, scale, block, cap)
        d["library"] = ev
        return d, gt
    with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
        made = list(pool.map(one, range(windows)))
    lists = {k: np.concatenate([d[k] for d, _ in made]) for k in ORDERS}
    offsets = np.zeros(windows + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(d["library"]) for d, _ in made])
    gt = np.stack([g for _, g in made])
    if path:
        os.makedirs(cache, exist_ok=True)
        np.savez(path, offsets=offsets, gt=gt, **lists)
    return lists, offsets, gt


def load(cfg, ev, offsets, windows, keep, stream):
    ctx = ebo.Context(image_w=cfg["image"][0], image_h=cfg["image"][1], patch_w=cfg["patch"][0], patch_h=cfg["patch"][1],
                      loss=ebo.LOSS_VARIANCE, tv_weight=0.0, max_events=len(ev), max_windows=windows)
    ctx.set_stream(stream.cuda_stream)
    os.environ["EBO_BUCKET"] = "host"
    if keep:
        os.environ["EBO_KEEP_ORDER"] = "1"
    ctx.set_windows(ev, offsets)
    os.environ.pop("EBO_KEEP_ORDER", None)
    return ctx


def main():
    argv = [a for a in sys.argv[1:]]
    opt = {}
    for name in ("--pmc", "--launches", "--cache"):
        if name in argv:
            i = argv.index(name)
            opt[name] = argv[i + 1]
            del argv[i:i + 2]
    config = int(argv[0]) if len(argv) > 0 else 3
    windows = int(argv[1]) if len(argv) > 1 else 128
    scale = float(argv[2]) if len(argv) > 2 else 0.5
    block = int(argv[3]) if len(argv) > 3 else 128
    cap = int(argv[4]) if len(argv) > 4 else 2542
    cfg = synth.CONFIGS[config]
    lists, offsets, gt = prepare(config, windows, scale, block, cap, opt.get("--cache"))
    stream = torch.cuda.current_stream()
    d_flows = torch.from_numpy(gt * scale).to("cuda")
    names = [opt["--pmc"]] if "--pmc" in opt else list(ORDERS)
    ctxs = {k: load(cfg, lists[k], offsets, windows, k != "library", stream) for k in names}
    P = ctxs[names[0]].P
    d_out = torch.zeros((windows * P, 3), dtype=torch.float64, device="cuda")
    if "--pmc" in opt:
        for _ in range(int(opt.get("--launches", 3))):
            ctxs[names[0]].eval_device(d_flows.data_ptr(), 1, d_out.data_ptr())
        torch.cuda.synchronize()
        print("%s: %d launches of %d events" % (names[0], int(opt.get("--launches", 3)), len(lists[names[0]])))
        return
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ref = None
    for rep in range(2):
        for k in names:
            res = []
            for jac in (1, 0):
                for _ in range(3):
                    ctxs[k].eval_device(d_flows.data_ptr(), jac, d_out.data_ptr())
                torch.cuda.synchronize()
                e0.record(stream)
                for _ in range(20):
                    ctxs[k].eval_device(d_flows.data_ptr(), jac, d_out.data_ptr())
                e1.record(stream)
                torch.cuda.synchronize()
                res.append(e0.elapsed_time(e1) / 20)
                if jac:
                    out = d_out.cpu().numpy().copy()
            ref = out if ref is None else ref
            print("cfg %d win %d flows %.1f*gt block %d rep %d [%-9s] jac %7.4f ms | val %7.4f ms | r %s | max|dJ| / max|J| %.1e"
                  % (config, windows, scale, block, rep, k, res[0], res[1],
                     "same bits" if np.array_equal(out[:, 0], ref[:, 0]) else "DIFFERS",
                     np.abs(out[:, 1:] - ref[:, 1:]).max() / np.abs(ref[:, 1:]).max()), flush=True)
    for c in ctxs.values():
        c.close()


if __name__ == "__main__":
    main()
