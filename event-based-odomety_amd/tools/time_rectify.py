"""What rectifying events at load costs (include/ebo.h: ebo_set_rectification), measured in ONE process:
the same call without a rectification, with the rectified camera that keeps K and with the fitted rectified camera
(ebo_fit_rectified_camera: no event leaves the sensor), alternating, after a warm-up; device times from HIP events
(ebo_timer_begin / _end on the context's stream), wall times where the call is host-bound.

usage: time_rectify.py [--step ingest|images|setup|all] [--windows 128] [--events 200000] [--reps 21]

  ingest  ebo_set_windows8_device (resident 8-byte records) and ebo_set_windows8 (pinned host records, PCIe included)
          on C3 windows, with / without: the ratio is the cost of the table read in the count and scatter passes
  images  the warped count image and ebo_compensate_windows on windows loaded with / without (with a rectification
          the stray unit holds the events that leave the sensor)
  setup   ebo_set_rectification (map build + flag read-back) for three sensor sizes; ebo_camera_unproject for 100 and
          100 000 points

Run each step under its own time limit (timeout -k 10 <seconds> python time_rectify.py --step ...)."""
import argparse
import importlib
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
ebo = importlib.import_module("event-based-odomety_amd")
synth = importlib.import_module("event-based-odomety_amd.synth")

# the DAVIS240C calibration of the reference's camera test, scaled to the sensor at hand
K = (-0.368436311798, 0.150947243557, 0.0, -0.000296130534385, -0.000759431726241)


def lens(w, h):
    return (199.092366542 * w / 240.0, 198.82882047 * h / 180.0, 132.192071378 * w / 240.0, 110.712660011 * h / 180.0) + K


def stream(config, windows, events, distinct=16):
    """`windows` windows of `events` events: `distinct` generated ones, repeated (the records are relative to their
    window's base time, so a repeated window is as good as a new one for the loaders)."""
    distinct = min(distinct, windows)
    ev, offsets, gt = synth.make_stream(config, distinct, n_events=events)
    t_base = np.array([int(ev["t_us"][int(offsets[w])]) for w in range(distinct)], dtype=np.int64)
    ev8 = [ebo.pack_events8(ev[int(offsets[w]):int(offsets[w + 1])], t_base[w]) for w in range(distinct)]
    pick = [w % distinct for w in range(windows)]
    all8 = np.concatenate([ev8[w] for w in pick])
    off = np.concatenate([[0], np.cumsum([len(ev8[w]) for w in pick])]).astype(np.uint64)
    return ev, offsets, gt, all8, t_base[pick], off, np.stack([gt[w] for w in pick])


MODES = ("plain", "same K", "fitted")


def set_mode(ctx, cam, mode):
    if mode == "plain":
        ctx.clear_rectification()
    elif mode == "same K":
        ctx.set_rectification(cam)
    else:
        ctx.set_rectification_camera(cam, ctx.fit_rectified_camera(cam))


def alternate(ctx, cam, fn, reps, device_clock=True):
    """median ms of fn() in the three modes, alternating; the switch is outside the clock"""
    out = {m: [] for m in MODES}
    for rep in range(reps + 2):
        for rectify in MODES:
            set_mode(ctx, cam, rectify)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if device_clock:
                ctx.timer_begin()
            fn()
            ms = ctx.timer_end() if device_clock else None
            ctx.synchronize()
            wall = (time.perf_counter() - t0) * 1e3
            if rep >= 2:  # two warm-up rounds
                out[rectify].append(ms if device_clock else wall)
    return tuple(statistics.median(out[m]) for m in MODES)


def report(**kw):
    print(json.dumps(kw), flush=True)


def step_ingest(args):
    cfg = synth.CONFIGS[3]
    w, h = cfg["image"]
    _, _, _, all8, t_base, off, _ = stream(3, args.windows, args.events)
    n = len(all8)
    ctx = ebo.Context(image_w=w, image_h=h, patch_w=cfg["patch"][0], patch_h=cfg["patch"][1], loss=ebo.LOSS_VARIANCE,
                      tv_weight=0.0, max_events=n, max_windows=args.windows)
    pin8 = torch.from_numpy(all8.view(np.uint8).reshape(-1, 8)).pin_memory()
    d8 = pin8.to("cuda")
    cam = lens(w, h)
    for name, fn in (("ebo_set_windows8_device (resident)", lambda: ctx.set_windows8(d8.data_ptr(), t_base, off, device=True)),
                     ("ebo_set_windows8 (pinned host, PCIe included)", lambda: ctx.set_windows8(pin8.data_ptr(), t_base, off))):
        for clock in (True, False):
            a, b, f = alternate(ctx, cam, fn, args.reps, device_clock=clock)
            report(step="ingest", call=name, clock="hip events" if clock else "wall", windows=args.windows, events=n,
                   ms_plain=round(a, 4), ms_rectified=round(b, 4), ms_fitted=round(f, 4), ratio=round(b / a, 4),
                   ratio_fitted=round(f / a, 4), gev_s_plain=round(n / a / 1e6, 2), gev_s_rectified=round(n / b / 1e6, 2),
                   gev_s_fitted=round(n / f / 1e6, 2))
    ctx.close()


def step_images(args):
    cfg = synth.CONFIGS[3]
    w, h = cfg["image"]
    windows = min(args.windows, 32)
    ev, offsets, gt, all8, t_base, off, flows = stream(3, windows, args.events)
    n = len(all8)
    ctx = ebo.Context(image_w=w, image_h=h, patch_w=cfg["patch"][0], patch_h=cfg["patch"][1], loss=ebo.LOSS_VARIANCE,
                      tv_weight=0.0, max_events=n, max_windows=windows)
    d8 = torch.from_numpy(all8.view(np.uint8).reshape(-1, 8)).to("cuda")
    d_flows = torch.from_numpy(np.ascontiguousarray(flows)).to("cuda")
    d_img = torch.zeros((windows, h, w), dtype=torch.float64, device="cuda")
    cam = lens(w, h)
    times = {}
    for rectify in MODES:
        set_mode(ctx, cam, rectify)
        ctx.set_windows8(d8.data_ptr(), t_base, off, device=True)
        stray = sum(ctx.window_info(k)[1] - sum(ctx.patch_info(p, k)[0] for p in range(ctx.P)) for k in range(windows))
        ms = []
        for rep in range(args.reps + 2):
            ctx.timer_begin()
            ctx.count_image_device(ebo.COUNT_WARPED, d_flows.data_ptr(), d_img.data_ptr())
            ms.append(ctx.timer_end())
        times[rectify] = (statistics.median(ms[2:]), stray)
    report(step="images", call="ebo_count_image_device (warped)", windows=windows, events=n,
           ms_plain=round(times["plain"][0], 4), ms_rectified=round(times["same K"][0], 4),
           ms_fitted=round(times["fitted"][0], 4), ratio=round(times["same K"][0] / times["plain"][0], 4),
           ratio_fitted=round(times["fitted"][0] / times["plain"][0], 4), stray_events_plain=int(times["plain"][1]),
           stray_events_rectified=int(times["same K"][1]), stray_events_fitted=int(times["fitted"][1]))
    # ebo_compensate_windows: the generated windows themselves (24-byte host records), wall clock
    few = min(len(offsets) - 1, 8)
    sub, suboff = ev[:int(offsets[few])], offsets[:few + 1]
    opts = ebo.default_solver(mode=ebo.SOLVE_INDEPENDENT, max_num_iterations=10)
    a, b, f = alternate(ctx, cam, lambda: ctx.compensate_windows(sub, suboff, opts), max(3, args.reps // 4), device_clock=False)
    report(step="images", call="ebo_compensate_windows (independent, 10 iterations)", windows=few, events=len(sub),
           ms_plain=round(a, 3), ms_rectified=round(b, 3), ms_fitted=round(f, 3), ratio=round(b / a, 4),
           ratio_fitted=round(f / a, 4))
    ctx.close()


def step_setup(args):
    for w, h in ((240, 180), (346, 260), (1280, 720)):
        ctx = ebo.Context(image_w=w, image_h=h, patch_w=40, patch_h=20, loss=ebo.LOSS_VARIANCE)
        cam = lens(w, h)
        ms = []
        for rep in range(args.reps + 2):
            t0 = time.perf_counter()
            ctx.set_rectification(cam)
            ms.append((time.perf_counter() - t0) * 1e3)
        report(step="setup", call="ebo_set_rectification", sensor="%dx%d" % (w, h), ms_wall=round(statistics.median(ms[2:]), 4),
               table_bytes=4 * w * h)
        ctx.close()
    ctx = ebo.Context(loss=ebo.LOSS_VARIANCE)
    rng = np.random.default_rng(0)
    for n in (100, 100_000):
        uv = np.stack([rng.uniform(0, 240, n), rng.uniform(0, 180, n)], axis=1)
        d_uv = torch.from_numpy(uv).to("cuda")
        d_out = torch.zeros((n, 3), dtype=torch.float64, device="cuda")
        wall, dev = [], []
        for rep in range(args.reps + 2):
            t0 = time.perf_counter()
            ctx.camera_unproject(lens(240, 180), uv)
            wall.append((time.perf_counter() - t0) * 1e3)
            ctx.timer_begin()
            ctx.camera_unproject_device(lens(240, 180), n, d_uv.data_ptr(), d_out.data_ptr())
            dev.append(ctx.timer_end())
        report(step="setup", call="ebo_camera_unproject", points=n, ms_wall_host_form=round(statistics.median(wall[2:]), 4),
               ms_device_form=round(statistics.median(dev[2:]), 4))
    ctx.close()


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--step", default="all", choices=["ingest", "images", "setup", "all"])
    ap.add_argument("--windows", type=int, default=128)
    ap.add_argument("--events", type=int, default=200_000)
    ap.add_argument("--reps", type=int, default=21)
    a = ap.parse_args()
    for name, fn in (("ingest", step_ingest), ("images", step_images), ("setup", step_setup)):
        if a.step in (name, "all"):
            fn(a)
