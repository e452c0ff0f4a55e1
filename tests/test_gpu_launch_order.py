"""k_eval3 and k_solve_independent take their unit through a launch-order table, heaviest first (csrc/launch_order.h;
DESIGN.md 4.1 item 15).  Which workgroup evaluates a unit must change no bit: libebo_hip_ab.so with the default order is
compared with EBO_EVAL_ORDER=index (the identity table) and =light (lightest first), and the shipped library with the
`index` run, every array with np.array_equal.

The mixed batch: a 64 x 48 sensor in 16 x 16 patches (12 per window), 3 windows, per-patch counts 0, 1, min_events,
min_events + 1, 63, 64, 65 and ~600 dealt differently in every window plus events outside the sensor, so active, inactive
and stray units share one launch and the table is far from the identity.  Times in [0, 20000] us at scale 1e-3."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T_END = 20000
MIN_EVENTS = 8
COUNTS = [0, 1, MIN_EVENTS, MIN_EVENTS + 1, 63, 64, 65, 600, 300, 17, 128, 590]
ORDERS = (("index", "index"), ("heaviest", None), ("light", "light"))


def _window(lib, rng, counts, w, strays=5):
    """One window of the 64 x 48 sensor: counts[p] events inside patch p (a drifting cloud), `strays` outside the sensor."""
    xs, ys, ts = [], [], []
    for p, n in enumerate(counts):
        x0, y0 = 16 * (p % 4), 16 * (p // 4)
        t = rng.integers(0, T_END + 1, n)
        v = rng.uniform(-0.5, 0.5, 2)
        s = rng.uniform(0, 16, n)
        xs.append(x0 + np.clip(5 + 0.3 * s + v[0] * (t - T_END / 2) * 1e-3, 0, 15).astype(int))
        ys.append(y0 + np.clip(s - v[1] * (t - T_END / 2) * 1e-3, 0, 15).astype(int))
        ts.append(t)
    xs.append(np.full(strays, 70))  # outside the sensor: the stray bucket
    ys.append(rng.integers(0, 48, strays))
    ts.append(rng.integers(0, T_END + 1, strays))
    x, y, t = np.concatenate(xs), np.concatenate(ys), np.concatenate(ts)
    t[0], t[-1] = 0, T_END  # pin the window's reference time
    o = np.argsort(t, kind="stable")
    return lib.make_events(x[o], y[o], t[o] + w * 2 * T_END)


def _mixed(lib, seed=3, windows=3, shift=0):
    rng = np.random.default_rng(seed)
    evs = [_window(lib, rng, np.roll(COUNTS, 5 * w + shift), w) for w in range(windows)]
    offs = np.concatenate([[0], np.cumsum([len(e) for e in evs])]).astype(np.uint64)
    return np.concatenate(evs), offs


def _ctx(lib, n_events, windows, **kw):
    args = dict(image_w=64, image_h=48, patch_w=16, patch_h=16, scale=1e-3, tv_weight=0.0, loss=lib.LOSS_VARIANCE,
                min_events=MIN_EVENTS, max_events=max(n_events, 1), max_windows=windows)
    args.update(kw)
    return lib.Context(lib.default_params(**args))


def _under_orders(ebo, ebo_ab, monkeypatch, run, env=None):
    """run(lib) under index / heaviest / light in the A/B library and in the shipped one -> {name: result};
    asserts that every result (a tuple of arrays or lists) equals the `index` run's."""
    out = {}
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)
    try:
        for name, order in ORDERS:
            if order:
                monkeypatch.setenv("EBO_EVAL_ORDER", order)
            else:
                monkeypatch.delenv("EBO_EVAL_ORDER", raising=False)
            out[name] = run(ebo_ab)
        monkeypatch.delenv("EBO_EVAL_ORDER", raising=False)
        out["shipped"] = run(ebo)
    finally:
        for k in ["EBO_EVAL_ORDER"] + list(env or {}):
            monkeypatch.delenv(k, raising=False)
    ref = out["index"]
    for name, res in out.items():
        assert len(res) == len(ref)
        for a, b in zip(res, ref):
            if isinstance(a, np.ndarray):
                assert np.array_equal(a, b), name
            else:
                assert a == b, name
    return ref


def _eval_all(lib, c, flows, n_slots):
    """(r, J, r value-only) of ebo_eval and the [n][3] outputs of ebo_eval_device with and without the Jacobian."""
    import torch
    r, J = c.eval(flows)
    r1, _ = c.eval(flows, want_jac=False)
    d_flows = torch.from_numpy(np.ascontiguousarray(flows, dtype=np.float64).reshape(-1, 2)).to("cuda")
    d_out = torch.full((n_slots, 3), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    res = [r, J, r1]
    for jac in (1, 0):
        c.eval_device(d_flows.data_ptr(), jac, d_out.data_ptr())
        c.synchronize()
        res.append(d_out.cpu().numpy().copy())
    return tuple(res)


def test_units_of_the_mixed_batch(ebo):
    """The batch holds what it is meant to: inactive units (0, 1, min_events events), active ones from min_events + 1 to
    600, a stray bucket per window, and weights in a different place in every window."""
    ev, offs = _mixed(ebo)
    with _ctx(ebo, len(ev), 3) as c:
        c.set_windows(ev, offs)
        info = [[c.patch_info(p, w)[:2] for p in range(c.P)] for w in range(3)]
    assert c.P == 12
    for w in range(3):
        n = [i[0] for i in info[w]]
        assert sorted(n) == sorted(COUNTS)
        assert [i[1] for i in info[w]] == [k > MIN_EVENTS for k in n]
    assert len({tuple(i[0] for i in info[w]) for w in range(3)}) == 3


def _expected_table(c, kind):
    """numpy's stable sort of the keys the library documents: n_ev of an active unit, 0 of any other."""
    if getattr(c, "_custom", None):
        info = [c.patch_info(p) for p in range(c.cur_patches)]
    else:  # P patches and the stray bucket (never active) per window
        info = [c.patch_info(p, w) if p < c.P else (0, False, 0) for w in range(c.n_windows) for p in range(c.P + 1)]
    key = np.array([n if act else 0 for n, act, _ in info], dtype=np.int64)
    if kind == "index":
        return np.arange(len(key))
    return np.argsort(key if kind == "light" else -key, kind="stable")


@pytest.mark.parametrize("path", ["device", "device-resident", "patches"])
def test_the_device_holds_the_documented_table(ebo, ebo_ab, monkeypatch, path):
    """The table read back from device memory (ebo_launch_order) is numpy's stable argsort of the keys: heaviest first in
    the shipped library and by default in the A/B one, the identity and lightest first under the switch -- after
    ebo_set_windows, ebo_set_windows_device and ebo_set_patches, and after a reload with other counts."""
    import torch
    ev, offs = _mixed(ebo)
    ev2, offs2 = _mixed(ebo, seed=8, windows=2, shift=3)

    def load(lib, c, e, o):
        if path == "device":
            c.set_windows(e, o)
        elif path == "device-resident":
            d = torch.from_numpy(np.ascontiguousarray(e, dtype=lib.EVENT_DTYPE).view(np.uint8)).to("cuda")
            torch.cuda.synchronize()
            c.set_windows_device(d.data_ptr(), o)
            c.synchronize()
        else:  # every grid patch of every window as a patch of its own, events grouped by patch
            rects, chunks, counts = [], [], []
            for w in range(len(o) - 1):
                ew = e[int(o[w]):int(o[w + 1])]
                ew = ew[(ew["x"] >= 0) & (ew["x"] < 64)]
                pid = (ew["y"] // 16) * 4 + ew["x"] // 16
                for p in range(12):
                    chunks.append(ew[pid == p])
                    counts.append(len(chunks[-1]))
                    rects.append((16 * (p % 4), 16 * (p // 4), 16, 16))
            c.set_patches(np.concatenate(chunks), np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), rects)

    for lib, order, kind in ((ebo, None, "heaviest"), (ebo_ab, None, "heaviest"), (ebo_ab, "index", "index"), (ebo_ab, "light", "light")):
        if order:
            monkeypatch.setenv("EBO_EVAL_ORDER", order)
        else:
            monkeypatch.delenv("EBO_EVAL_ORDER", raising=False)
        try:
            with _ctx(lib, len(ev), 3) as c:
                for e, o in ((ev, offs), (ev2, offs2)):
                    load(lib, c, e, o)
                    got = c.launch_order()
                    want = _expected_table(c, kind)
                    assert len(got) == len(want) and np.array_equal(got, want), (kind, path)
                    if kind != "index":
                        assert not np.array_equal(got, np.arange(len(got)))  # the batch is mixed: far from the identity
        finally:
            monkeypatch.delenv("EBO_EVAL_ORDER", raising=False)


@pytest.mark.parametrize("scale", [0.0, 1.0])
def test_mixed_weights_eval_and_eval_device(ebo, ebo_ab, monkeypatch, scale):
    ev, offs = _mixed(ebo)
    flows = np.random.default_rng(4).uniform(-0.6, 0.6, (3, 12, 2)) * scale

    def run(lib):
        with _ctx(lib, len(ev), 3) as c:
            c.set_windows(ev, offs)
            return _eval_all(lib, c, flows, 36)
    r, J, r1, dj, dv = _under_orders(ebo, ebo_ab, monkeypatch, run)
    assert np.isfinite(r).all() and np.isfinite(J).all()
    assert np.array_equal(r, r1) and np.array_equal(dj[:, 0], r.reshape(-1)) and np.array_equal(dv[:, 0], r.reshape(-1))
    assert (r != 0).sum() == 3 * sum(k > MIN_EVENTS for k in COUNTS)  # every active unit was evaluated, nobody else


def test_central_differences_five_flow_sets(ebo, ebo_ab, monkeypatch):
    """grad = EBO_GRAD_CENTRAL: five flow sets and k_combine_variance, which reads a unit's partial sums by unit index."""
    ev, offs = _mixed(ebo)
    flows = np.random.default_rng(5).uniform(-0.6, 0.6, (3, 12, 2))

    def run(lib):
        with _ctx(lib, len(ev), 3, grad=lib.GRAD_CENTRAL) as c:
            c.set_windows(ev, offs)
            return _eval_all(lib, c, flows, 36)
    r, J, _, _, _ = _under_orders(ebo, ebo_ab, monkeypatch, run)
    assert (J != 0).any()


def test_row_tiles_of_a_frame_sized_patch(ebo, ebo_ab, synth, monkeypatch):
    """One 240 x 180 patch per frame (configs[0] of the baseline): the launch plan cuts a unit's rows into several tiles (asserted), the
    non-fused path.  Three windows of 1500, 4000 and 2500 events: the table takes window 1, then 2, then 0, then the strays."""
    evs = [synth.make_window(1, window=w, n_events=n)[0] for w, n in enumerate((1500, 4000, 2500))]
    ev = np.concatenate(evs)
    offs = np.concatenate([[0], np.cumsum([len(e) for e in evs])]).astype(np.uint64)
    flows = np.array([[[0.3, -0.2]], [[-0.4, 0.1]], [[0.2, 0.5]]])

    def run(lib):
        with lib.Context(image_w=240, image_h=180, patch_w=240, patch_h=180, loss=lib.LOSS_VARIANCE, tv_weight=0.0,
                         max_events=len(ev), max_windows=3) as c:
            c.set_windows(ev, offs)
            assert c.eval_launch_shape(True)[0] > 1 and c.eval_launch_shape(False)[0] > 1  # row tiles: the non-fused path
            return _eval_all(lib, c, flows, 3)
    r, J, _, _, _ = _under_orders(ebo, ebo_ab, monkeypatch, run)
    assert (r != 0).all() and (J != 0).all()


def test_row_tiles_with_unequal_units_of_set_patches(ebo, ebo_ab, synth, monkeypatch):
    """ebo_set_patches: four frame-sized rects with 3000, 40 (inactive: min_events is 100), 5000 and 900 events -- tiles > 1 and the table 2, 0, 3, 1."""
    evs = [synth.make_window(1, window=w, n_events=n)[0] for w, n in enumerate((3000, 40, 5000, 900))]
    ev = np.concatenate(evs)
    offs = np.concatenate([[0], np.cumsum([len(e) for e in evs])]).astype(np.uint64)
    rects = [(0, 0, 240, 180)] * 4
    flows = np.random.default_rng(6).uniform(-0.5, 0.5, (4, 2))

    def run(lib):
        with lib.Context(image_w=240, image_h=180, patch_w=240, patch_h=180, loss=lib.LOSS_VARIANCE, tv_weight=0.0,
                         max_events=len(ev), max_windows=4) as c:
            c.set_patches(ev, offs, rects)
            assert c.eval_launch_shape(True)[0] > 1  # row tiles: the non-fused path
            return _eval_all(lib, c, flows, 4)
    r, _, _, _, _ = _under_orders(ebo, ebo_ab, monkeypatch, run)
    assert list(r.reshape(-1) != 0) == [True, False, True, True]


@pytest.mark.parametrize("lists", [True, False], ids=["window-lists", "mode-table"])
def test_lock_step_solve_modes_and_thinned_rounds(ebo, ebo_ab, synth, monkeypatch, lists):
    """A lock-step solve of six windows: its rounds carry a per-slot mode table with all three modes (0 a finished
    window, 1 a cost round, 2 a Jacobian round) and, once the batch has thinned out, go as window lists (the LiveWindows
    path, which does not use the table at all).  EBO_SOLVE_NO_COMPACT keeps every round on the mode table."""
    ev, offsets, _ = synth.make_stream(0, 6)

    def run(lib):
        with lib.Context(image_w=240, image_h=180, patch_w=20, patch_h=20, loss=lib.LOSS_VARIANCE, max_events=len(ev),
                         max_windows=6) as c:
            c.set_windows(ev, offsets)
            opts = lib.default_solver()
            opts.max_num_iterations = 15
            flows, summ = c.solve(opts)
            return flows.copy(), [(s.iterations, s.final_cost, s.termination, s.num_evals_cost, s.num_evals_jac) for s in summ]
    flows, summ = _under_orders(ebo, ebo_ab, monkeypatch, run, env=None if lists else {"EBO_SOLVE_NO_COMPACT": "1"})
    assert len({s[0] for s in summ}) > 1  # the windows do not stop together: finished windows (mode 0), thinned rounds
    assert (flows != 0).any()


def test_reload_on_one_context_equals_a_fresh_one(ebo, ebo_ab, monkeypatch):
    """set_windows twice on one context, the second time with other counts per unit (and fewer windows): the table is
    rebuilt with the units, the second result is that of a fresh context."""
    ev1, offs1 = _mixed(ebo, seed=7, windows=3)
    ev2, offs2 = _mixed(ebo, seed=8, windows=2, shift=3)
    flows = np.random.default_rng(9).uniform(-0.6, 0.6, (2, 12, 2))

    def run(lib):
        with _ctx(lib, max(len(ev1), len(ev2)), 3) as c:
            c.set_windows(ev1, offs1)
            c.eval(np.zeros((3, 12, 2)))
            c.set_windows(ev2, offs2)
            again = _eval_all(lib, c, flows, 24)
        with _ctx(lib, max(len(ev1), len(ev2)), 3) as c:
            c.set_windows(ev2, offs2)
            fresh = _eval_all(lib, c, flows, 24)
        for a, b in zip(again, fresh):
            assert np.array_equal(a, b)
        return again
    _under_orders(ebo, ebo_ab, monkeypatch, run)


def test_recorded_graph_replays_the_direct_call(ebo, ebo_ab, monkeypatch):
    """ebo_eval_device recorded into a graph and replayed on unchanged windows: the recording holds the table's address,
    which no load moves."""
    import torch
    ev, offs = _mixed(ebo, seed=10)
    flows = np.random.default_rng(11).uniform(-0.6, 0.6, (36, 2))

    def run(lib):
        with _ctx(lib, len(ev), 3) as c:
            stream = torch.cuda.Stream()
            c.set_stream(stream.cuda_stream)
            c.set_windows(ev, offs)
            d_flows = torch.from_numpy(flows).to("cuda")
            d_out = torch.zeros((36, 3), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            step = lambda: c.eval_device(d_flows.data_ptr(), 1, d_out.data_ptr())
            step()
            c.synchronize()
            direct = d_out.cpu().numpy().copy()
            g = c.record(step)
            d_out.fill_(-3.0)
            torch.cuda.synchronize()
            g.launch(2)
            c.synchronize()
            replayed = d_out.cpu().numpy().copy()
            g.close()
        assert np.array_equal(direct, replayed)
        return (direct,)
    (direct,) = _under_orders(ebo, ebo_ab, monkeypatch, run)
    assert (direct[:, 0] != 0).sum() == 3 * sum(k > MIN_EVENTS for k in COUNTS)


def test_solve_device_on_the_mixed_batch(ebo, ebo_ab, monkeypatch):
    """k_solve_independent takes the same table: flows and statistics of the mixed batch under the three orders."""
    import torch
    ev, offs = _mixed(ebo, seed=12)

    def run(lib):
        with _ctx(lib, len(ev), 3) as c:
            c.set_windows(ev, offs)
            opts = lib.default_solver(mode=lib.SOLVE_INDEPENDENT, max_num_iterations=12)
            d_sol = torch.full((36, 2), -5.0, dtype=torch.float64, device="cuda")
            d_stats = torch.full((36, 4), -5, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            c.solve_device(opts, d_sol.data_ptr(), d_stats.data_ptr())
            c.synchronize()
            return d_sol.cpu().numpy().copy(), d_stats.cpu().numpy().copy()
    sol, stats = _under_orders(ebo, ebo_ab, monkeypatch, run)
    assert (sol != -5.0).all() and (stats != -5).all()  # every flow slot was written, whatever workgroup took its unit
    active = np.concatenate([np.roll(COUNTS, 5 * w) > MIN_EVENTS for w in range(3)])
    assert (stats[~active] == 0).all() and (stats[active, 1] > 0).all()
    assert (np.abs(sol[active]).max(axis=1) > 0).any()  # the solves moved
