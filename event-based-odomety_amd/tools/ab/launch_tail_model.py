"""Two CPU models of the end of a k_eval3 launch: how much of the launch is the chip draining
its last workgroups when units are handed out in index order, and how much a heaviest-first order (csrc/launch_order.h)
gets back.  Models, not measurements: the counts are real (synth's windows, bucketed by the grid rule), the machine is not.

usage: launch_tail_model.py [config=3] [windows=128]

  slots   1792 independent slots (256 CUs x 7 resident workgroups); a workgroup lasts c0 + n_ev, c0 in {0, 100, 300};
          the next workgroup in launch order takes the slot that frees first.
  xcd     workgroup q runs on XCD q % 8: 32 CUs x 7 slots each, an in-order queue per XCD; the residents of a CU share
          it (processor sharing) and its throughput saturates at s = 3, 4 or 7 residents: each of k residents advances at
          min(1, s / k).

Both are printed as makespan / ideal, ideal = total work / capacity, for the index order, heaviest first and lightest
first.  Units at or below min_events (inactive) and the stray buckets weigh nothing: their workgroups return at once."""
import heapq
import os
import sys

import numpy as np

PKG_DIR = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, PKG_DIR)
import synth  # noqa: E402

MIN_EVENTS = 100  # ebo_default_params
CUS, SLOTS, XCDS = 256, 7, 8


def unit_counts(config, windows):
    """[windows][P + 1] events per unit: the grid's patches (the last column / row absorbs the remainder), then the stray
    bucket, which synth never fills."""
    cfg = synth.CONFIGS[config]
    iw, ih = cfg["image"]
    pw, ph = cfg["patch"]
    npx, npy = iw // pw, ih // ph
    from concurrent.futures import ThreadPoolExecutor

    def one(w):
        ev, _ = synth.make_window(config, window=w)
        pid = np.minimum(ev["y"] // ph, npy - 1) * npx + np.minimum(ev["x"] // pw, npx - 1)
        return np.append(np.bincount(pid, minlength=npx * npy), 0)
    with ThreadPoolExecutor(max(1, min(16, len(os.sched_getaffinity(0))))) as pool:
        return np.stack(list(pool.map(one, range(windows))))


def orders(key):
    idx = np.arange(len(key))
    return {"index": idx, "heaviest": np.argsort(-key, kind="stable"), "lightest": np.argsort(key, kind="stable")}


def model_slots(work, order, c0, slots=CUS * SLOTS):
    free = [0.0] * slots
    heapq.heapify(free)
    end = 0.0
    total = 0.0
    for u in order:
        d = (c0 + work[u]) if work[u] > 0 else 0.0
        t = heapq.heappop(free) + d
        heapq.heappush(free, t)
        end = max(end, t)
        total += d
    return end / (total / slots)


def model_xcd(work, order, sat, cus=CUS // XCDS, slots=SLOTS):
    """max over the XCDs of the time its queue takes / (all work / (256 CUs x sat))"""
    worst = 0.0
    for x in range(XCDS):
        queue = [work[u] for u in order[x::XCDS] if work[u] > 0]
        rem = np.zeros((cus, slots))  # remaining work of each resident, 0 = free slot
        nxt = 0
        for s in range(slots):  # the first residents, dealt round the CUs
            for cu in range(cus):
                if nxt < len(queue):
                    rem[cu, s] = queue[nxt]
                    nxt += 1
        now = 0.0
        while True:
            live = rem > 0
            k = live.sum(axis=1)
            if not k.any():
                break
            rate = np.minimum(1.0, sat / np.maximum(k, 1))  # per resident of the CU
            first = np.where(live, rem, np.inf).min(axis=1) / rate  # time until the CU's next completion
            dt = first.min()
            now += dt
            rem = np.where(live, rem - dt * rate[:, None], 0.0)
            done = live & (rem <= 1e-9)
            rem[done] = 0.0
            for cu, s in zip(*np.nonzero(done)):  # in order: the next of the queue takes the slot that came free
                if nxt < len(queue):
                    rem[cu, s] = queue[nxt]
                    nxt += 1
        worst = max(worst, now)
    return worst / (float(np.sum(work)) / (CUS * sat))


def main():
    config = int(sys.argv[1]) if len(sys.argv) > 1 else 3
    windows = int(sys.argv[2]) if len(sys.argv) > 2 else 128
    n = unit_counts(config, windows)
    patches = n[:, :-1]
    act = patches[patches > MIN_EVENTS]
    print("%s x %d windows: %d units, %d active" % (synth.CONFIGS[config]["name"], windows, n.size, act.size))
    print("events per active unit: min %d  mean %.0f  max %d" % (act.min(), act.mean(), act.max()))
    q = np.array([np.percentile(w[w > MIN_EVENTS], (5, 50, 95)) for w in patches])
    print("within one window (mean over windows): 5 %% / 50 %% / 95 %% = %.0f / %.0f / %.0f" % tuple(q.mean(axis=0)))
    print("workgroups per launch %d = %.1f waves of %d resident" % (n.size, n.size / (CUS * SLOTS), CUS * SLOTS))
    work = np.where(n > MIN_EVENTS, n, 0).astype(np.float64)
    work[:, -1] = 0.0
    work = work.reshape(-1)
    od = orders(work)
    print("\nmakespan / ideal        %10s %10s %10s" % tuple(od))
    for c0 in (0, 100, 300):
        print("slots  c0 = %-3d         " % c0 + " ".join("%10.3f" % model_slots(work, o, c0) for o in od.values()), flush=True)
    for sat in (3, 4, 7):
        print("xcd    saturation at %d  " % sat + " ".join("%10.3f" % model_xcd(work, o, sat) for o in od.values()), flush=True)


if __name__ == "__main__":
    main()
