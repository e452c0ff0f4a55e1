"""k_eval3 and k_solve_independent take a unit's bounding box from the load's per-column / per-row time extents where
those give it exactly, and from a pass over the events elsewhere (csrc/box_extents.h, ebo_extents.inc; DESIGN.md 4.1
item 17).  The box is the same either way, so every output is: libebo_hip_ab.so under EBO_EVAL_BOX=events is compared
with =extents, and the shipped library with both, bit for bit (the arrays' bytes, so NaN results compare too).  The table
read back from device memory is compared with a numpy restatement after every loading path, and the number of units
that took each path with what the numpy restatement of the rule predicts, so no scene passes with the new path unused.

The scene: a 64 x 48 sensor cut in 12 x 12 patches -- five columns, the last one the remainder column of 16 x 12
patches -- by four rows, 2 windows of ~1000 events, times in [0, 20000] us at scale 1e-3 (|tau| <= 10 around a unit's
mid-time).  Per window: dense and sparse patches, one whose events lie on three columns only (empty table entries), an
empty and a two-event patch (inactive at min_events = 8) and events outside the sensor (the stray bucket)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

T_END = 20000
SCALE = 1e-3
MIN_EVENTS = 8
W, H, PW, PH = 64, 48, 12, 12
NPX, NPY = 5, 4
P = NPX * NPY
STRIDE, ENT = 258, 2
I32MAX, I32MIN = np.iinfo(np.int32).max, np.iinfo(np.int32).min
COUNTS = [120, 60, 0, 33, 90, 2, 75, 40, 64, 65, 110, 9, 50, 20, 128, 30, 45, 63, 80, 25]  # per patch; rolled per window
BOXES = (("events", "events"), ("extents", "extents"), ("default", None))


def _rect(p):
    px, py = p % NPX, p // NPX
    return PW * px, PH * py, (W - PW * px) if px == NPX - 1 else PW, PH


def _window(lib, rng, counts, w, strays=4, moving=False):
    xs, ys, ts = [], [], []
    for p, n in enumerate(counts):
        x0, y0, rw, rh = _rect(p)
        if moving:  # a slanted edge drifting through the patch: something for a solve to find
            t = rng.integers(0, T_END + 1, n)
            v = rng.uniform(-0.4, 0.4, 2)
            s = rng.uniform(0, rh, n)
            xs.append(x0 + np.clip(4 + 0.3 * s + v[0] * (t - T_END / 2) * SCALE, 0, rw - 1).astype(int))
            ys.append(y0 + np.clip(s - v[1] * (t - T_END / 2) * SCALE, 0, rh - 1).astype(int))
            ts.append(t)
            continue
        if p % 7 == 3:  # three columns only: the other columns' table entries stay empty
            xs.append(x0 + rng.choice([1, 4, rw - 2], n))
        else:
            xs.append(x0 + rng.integers(0, rw, n))
        ys.append(y0 + rng.integers(0, rh, n))
        ts.append(rng.integers(0, T_END + 1, n))
    xs.append(np.full(strays, W + 6))  # outside the sensor: the stray bucket
    ys.append(rng.integers(0, H, strays))
    ts.append(rng.integers(0, T_END + 1, strays))
    x, y, t = np.concatenate(xs), np.concatenate(ys), np.concatenate(ts)
    t[0], t[-1] = 0, T_END
    o = np.argsort(t, kind="stable")
    return lib.make_events(x[o], y[o], t[o] + w * 2 * T_END)


_scenes = {}


def _scene(lib, seed=21, windows=2, shift=0, moving=False):
    key = (seed, windows, shift, moving)
    if key not in _scenes:
        rng = np.random.default_rng(seed)
        evs = [_window(lib, rng, np.roll(COUNTS, 3 * w + shift), w, moving=moving) for w in range(windows)]
        offs = np.concatenate([[0], np.cumsum([len(e) for e in evs])]).astype(np.uint64)
        ev = np.concatenate(evs)
        ev.setflags(write=False)
        _scenes[key] = (ev, offs)
    return _scenes[key]


def _ctx(lib, n_events, windows, sigma=None, **kw):
    args = dict(image_w=W, image_h=H, patch_w=PW, patch_h=PH, scale=SCALE, tv_weight=0.0, loss=lib.LOSS_VARIANCE,
                min_events=MIN_EVENTS, max_events=max(n_events, 1), max_windows=windows)
    args.update(kw)
    p = lib.default_params(**args)
    if sigma is not None:
        p.k.sigma_compensate = sigma
    return lib.Context(p)


# ---- numpy restatements -------------------------------------------------------------------------------------------
def _unpack(rec):
    lo = (rec & np.uint64(0xFFFFFFFF)).astype(np.int64)
    dt = (rec >> np.uint64(32)).astype(np.uint32).view(np.int32).astype(np.int64)
    x = ((lo & 0x7FFF) ^ 0x4000) - 0x4000
    y = (((lo >> 16) & 0x7FFF) ^ 0x4000) - 0x4000
    return x, y, dt


def _slot(rec, rect, stray=False):
    """k_unit_extents' slot of one unit from its packed records."""
    s = np.empty(STRIDE, dtype=np.int64)
    s[:ENT] = 0
    s[ENT::2], s[ENT + 1::2] = I32MAX, I32MIN
    x0, y0, rw, rh = rect
    if stray or rw > 64 or rh > 64:
        return s.astype(np.int32)
    x, y, dt = _unpack(rec)
    cx, cy = x - x0, y - y0
    inside = (cx >= 0) & (cx < rw) & (cy >= 0) & (cy < rh)
    for k, d in zip(np.concatenate([cx[inside], rw + cy[inside]]), np.concatenate([dt[inside], dt[inside]])):
        s[ENT + 2 * k] = min(s[ENT + 2 * k], d)
        s[ENT + 2 * k + 1] = max(s[ENT + 2 * k + 1], d)
    s[0] = 1 if inside.all() else 0
    return s.astype(np.int32)


def _table(c, rects=None):
    if rects is not None:
        return np.stack([_slot(c.unit_records(0, i), r) for i, r in enumerate(rects)])
    return np.stack([_slot(c.unit_records(w, b), _rect(b) if b < P else (0, 0, 1, 1), stray=b == P)
                     for w in range(c.n_windows) for b in range(P + 1)])


def _rule(slot, rect, m0, m1):
    """box_from_slot: (admitted, (xmin, xmax, ymin, ymax)) of one unit at one flow."""
    if slot[0] != 1:
        return False, None
    x0, y0, rw, rh = rect
    ent = slot[ENT:ENT + 2 * (rw + rh)].reshape(-1, 2).astype(np.int64)
    src = np.concatenate([x0 + np.arange(rw), y0 + np.arange(rh)]).astype(np.float64)
    m = np.concatenate([np.full(rw, m0), np.full(rh, m1)])
    live = ent[:, 0] <= ent[:, 1]
    with np.errstate(all="ignore"):
        cc = src[:, None] + (ent.astype(np.float64) * SCALE) * m[:, None]  # one rounding per operation
        conv = np.abs(cc) < 1073741824.0
    if not conv[live].all():
        return False, None
    pos = np.trunc(np.where(conv, cc, 0.0)).astype(np.int64) - np.concatenate([np.full(rw, x0), np.full(rh, y0)])[:, None] \
        + np.concatenate([np.full(rw, rw), np.full(rh, rh)])[:, None]
    cols, rows = pos[:rw][live[:rw]], pos[rw:][live[rw:]]
    if cols.size == 0:
        return True, None
    box = (cols.min(), cols.max(), rows.min(), rows.max())
    ok = box[0] >= -3 and box[1] <= 3 * rw + 2 and box[2] >= -3 and box[3] <= 3 * rh + 2
    return ok, box


def _predict(c, table, flows):
    """(units on the event pass, units on the table, admitted units whose box reaches into the canvas margin) among the
    active grid units of the loaded windows."""
    ev = tab = margin = 0
    for w in range(c.n_windows):
        for b in range(P):
            if not c.patch_info(b, w)[1]:
                continue
            ok, box = _rule(table[w * (P + 1) + b], _rect(b), *flows[w, b])
            tab += ok
            ev += not ok
            rw, rh = _rect(b)[2:]
            margin += bool(ok and box and (box[0] < 3 or box[1] > 3 * rw - 4 or box[2] < 3 or box[3] > 3 * rh - 4))
    return ev, tab, margin


# ---- running the same thing under both boxes -------------------------------------------------------------------------
def _same(a, b):
    if isinstance(a, np.ndarray):
        return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()
    return a == b


def _under_boxes(ebo, ebo_ab, monkeypatch, run, env=None, shipped=True):
    """run(lib) under events / extents / no switch in the A/B library and (unless env changes the launch shape, which
    the shipped library does not read) in the shipped one; every result must have the `events` run's bytes."""
    out = {}
    try:
        for k, v in (env or {}).items():
            monkeypatch.setenv(k, v)
        for name, box in BOXES:
            if box:
                monkeypatch.setenv("EBO_EVAL_BOX", box)
            else:
                monkeypatch.delenv("EBO_EVAL_BOX", raising=False)
            out[name] = run(ebo_ab)
        monkeypatch.delenv("EBO_EVAL_BOX", raising=False)
        if shipped:
            out["shipped"] = run(ebo)
    finally:
        for k in ["EBO_EVAL_BOX"] + list(env or {}):
            monkeypatch.delenv(k, raising=False)
    ref = out["events"]
    for name, res in out.items():
        assert len(res) == len(ref)
        for i, (a, b) in enumerate(zip(res, ref)):
            assert _same(a, b), (name, i)
    return ref


def _eval_all(c, flows, counts=False):
    """(r, J, r value-only) of ebo_eval and the [n][3] outputs of ebo_eval_device with and without the Jacobian; with
    counts (A/B library), also the box path counts after each launch."""
    import torch
    n = flows.reshape(-1, 2).shape[0]
    seen = []
    r, J = c.eval(flows)
    seen.append(c.box_path_counts() if counts else None)
    r1, _ = c.eval(flows, want_jac=False)
    seen.append(c.box_path_counts() if counts else None)
    d_flows = torch.from_numpy(np.ascontiguousarray(flows, dtype=np.float64).reshape(-1, 2)).to("cuda")
    d_out = torch.full((n, 3), -7.0, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    res = [r, J, r1]
    for jac in (1, 0):
        c.eval_device(d_flows.data_ptr(), jac, d_out.data_ptr())
        c.synchronize()
        seen.append(c.box_path_counts() if counts else None)
        res.append(d_out.cpu().numpy().copy())
    return tuple(res), seen


def _flows(name, windows=2):
    rng = np.random.default_rng(31)
    if name == "zero":
        return np.zeros((windows, P, 2))
    if name == "mid":  # +-5 pixels at the ends of the window: every warped event far inside the canvas
        return rng.uniform(-0.5, 0.5, (windows, P, 2))
    if name == "negative":
        return -rng.uniform(0.05, 0.5, (windows, P, 2))
    if name == "border":
        # 1.0 .. 2.2 pixels per ms graded over the patches, signs mixed: 10 .. 22 pixels at |tau| = 10 against a margin
        # of 12 + 3 -- the lower grades put the box into the canvas's edge (clipped footprints), the higher ones lose events
        g = np.linspace(1.0, 2.2, P)
        f = np.stack([g * np.where(np.arange(P) % 2, 1.0, -1.0), 0.6 * g * np.where(np.arange(P) % 3, -1.0, 1.0)], axis=1)
        return np.stack([f, -f[::-1]][:windows])
    if name == "nan":
        f = rng.uniform(-0.5, 0.5, (windows, P, 2))
        f[0, 0, 0] = np.nan
        f[0, 4, 1] = np.nan
        f[1, 6] = np.nan
        f[1, 10, 0] = np.inf
        f[1, 9, 1] = 1e300
        return f
    raise KeyError(name)


# ---- the table ----------------------------------------------------------------------------------------------------------
def _load(lib, c, path, ev, offs):
    import torch
    if path == "host":
        c.set_windows(ev, offs)
    elif path == "device":
        d = torch.from_numpy(np.array(ev, dtype=lib.EVENT_DTYPE).view(np.uint8)).to("cuda")
        torch.cuda.synchronize()
        c.set_windows_device(d.data_ptr(), offs)
        c.synchronize()
    return None


def _patch_scene(lib):
    """ebo_set_patches: six rects of their own -- two grid rects, a 30 x 20 one, a 64 x 64 one (the table's limit), a
    70 x 20 one (no table) and a one-column 1 x 40 one -- with events inside them."""
    rng = np.random.default_rng(41)
    rects = [(0, 0, 12, 12), (48, 36, 16, 12), (10, 5, 30, 20), (0, 0, 64, 64), (2, 3, 70, 20), (33, 4, 1, 40)]
    counts = [40, 55, 200, 300, 150, 30]
    chunks = []
    for (x0, y0, rw, rh), n in zip(rects, counts):
        t = np.sort(rng.integers(0, T_END + 1, n))
        chunks.append(lib.make_events(x0 + rng.integers(0, rw, n), y0 + rng.integers(0, rh, n), t))
    return np.concatenate(chunks), np.concatenate([[0], np.cumsum(counts)]).astype(np.uint64), rects


@pytest.mark.parametrize("path", ["host", "device", "patches"])
def test_the_device_holds_the_restated_table(ebo, ebo_ab, path):
    """After ebo_set_windows, ebo_set_windows_device and ebo_set_patches, and after a reload with fewer units on the same
    context, the table read back is the numpy restatement: status, per-column and per-row (dtMin, dtMax), empty entries."""
    ev, offs = _scene(ebo)
    ev1, offs1 = _scene(ebo, seed=22, windows=1, shift=5)
    for lib in (ebo, ebo_ab):
        if path == "patches":
            pev, poffs, rects = _patch_scene(lib)
            with lib.Context(lib.default_params(image_w=96, image_h=80, patch_w=PW, patch_h=PH, scale=SCALE, tv_weight=0.0,
                                                loss=lib.LOSS_VARIANCE, min_events=MIN_EVENTS, max_events=len(pev),
                                                max_windows=2)) as c:
                c.set_patches(pev, poffs, rects)
                got, want = c.unit_extents(), _table(c, rects)
                assert got.shape == want.shape and np.array_equal(got, want)
                assert list(got[:, 0]) == [1, 1, 1, 1, 0, 1]
                c.set_patches(pev[:int(poffs[3])], poffs[:4], rects[:3])  # fewer units
                got, want = c.unit_extents(), _table(c, rects[:3])
                assert got.shape == (3, STRIDE) and np.array_equal(got, want)
            continue
        with _ctx(lib, len(ev), 2) as c:
            for e, o in ((ev, offs), (ev1, offs1)):
                _load(lib, c, path, e, o)
                got, want = c.unit_extents(), _table(c)
                assert got.shape == ((len(o) - 1) * (P + 1), STRIDE)
                assert np.array_equal(got, want), path
                status = got[:, 0].reshape(-1, P + 1)
                assert (status[:, :P] == 1).all() and (status[:, P] == 0).all()  # grid units tabled, the stray bucket not
                ent = got[:, ENT:].reshape(len(got), -1, 2)
                assert ((ent[:, :, 0] == I32MAX) == (ent[:, :, 1] == I32MIN)).all()
                assert ((ent[:, :PW, 0] != I32MAX).sum(axis=1) == 3).any()  # a three-column patch: its other columns empty


# ---- bit for bit --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zero", "mid", "negative", "border", "nan"])
def test_eval_and_eval_device_bit_for_bit(ebo, ebo_ab, monkeypatch, name):
    """Active, inactive (0 and 2 events) and stray units in one launch, at flows from zero to NaN."""
    ev, offs = _scene(ebo)
    flows = _flows(name)

    def run(lib):
        with _ctx(lib, len(ev), 2) as c:
            c.set_windows(ev, offs)
            return _eval_all(c, flows)[0]
    r, J, r1, dj, dv = _under_boxes(ebo, ebo_ab, monkeypatch, run)
    active = np.stack([np.roll(COUNTS, 3 * w) > MIN_EVENTS for w in range(2)])
    assert (r[~active] == 0).all()
    if name != "nan":
        assert np.isfinite(r).all() and (r[active] != 0).all() and (J[active] != 0).any()
    else:
        assert np.isnan(r[0, 0]) and np.isnan(r[1, 6]) and np.isfinite(r[0, 1])


def test_one_event_units(ebo, ebo_ab, monkeypatch):
    """min_events = 0: a unit of ONE event is active; its column's and its row's extents are that event's dt twice."""
    rng = np.random.default_rng(51)
    x = np.array([PW * (p % NPX) + 5 for p in range(P)])
    y = np.array([PH * (p // NPX) + 7 for p in range(P)])
    t = np.sort(rng.integers(0, T_END + 1, P))
    t[0], t[-1] = 0, T_END
    ev = ebo.make_events(x, y, t)
    offs = np.array([0, P], dtype=np.uint64)
    flows = np.random.default_rng(52).uniform(-0.8, 0.8, (1, P, 2))

    def run(lib):
        with _ctx(lib, P, 1, min_events=0) as c:
            c.set_windows(ev, offs)
            tab = c.unit_extents()
            assert (tab[:P, 0] == 1).all() and ((tab[:P, ENT:] != I32MAX) & (tab[:P, ENT:] != I32MIN)).sum() == 4 * P
            return _eval_all(c, flows)[0]
    r = _under_boxes(ebo, ebo_ab, monkeypatch, run)[0]
    assert (r != 0).all()


@pytest.mark.parametrize("name", ["mid", "border"])
def test_set_patches_rects(ebo, ebo_ab, monkeypatch, name):
    """Rects of ebo_set_patches: 64 x 64 takes the table in two steps of 64 lanes, 70 x 20 has no table."""
    pev, poffs, rects = _patch_scene(ebo)
    f = np.random.default_rng(61).uniform(-0.5, 0.5, (len(rects), 2)) * (1.0 if name == "mid" else 6.0)

    def run(lib):
        with lib.Context(lib.default_params(image_w=96, image_h=80, patch_w=PW, patch_h=PH, scale=SCALE, tv_weight=0.0,
                                            loss=lib.LOSS_VARIANCE, min_events=MIN_EVENTS, max_events=len(pev),
                                            max_windows=2)) as c:
            c.set_patches(pev, poffs, rects)
            return _eval_all(c, f)[0]
    r = _under_boxes(ebo, ebo_ab, monkeypatch, run)[0]
    assert (r != 0).all()


@pytest.mark.parametrize("env", [{"EBO_EVAL_TILES": "2"}, {"EBO_LDS_KB": "4"}, {"EBO_LDS_KB": "4", "EBO_EVAL_TILES": "3"}],
                         ids=["tiles2", "lds4", "lds4-tiles3"])
@pytest.mark.parametrize("name", ["mid", "border"])
def test_row_tiles_and_sub_bands(ebo, ebo_ab, monkeypatch, env, name):
    """Row tiles (every tile's workgroup takes the same decision and the same box) and forced sub-bands.  The shipped
    library does not read the switches, so here the A/B library's two boxes are compared with each other."""
    pev, poffs, rects = _patch_scene(ebo)
    f = np.random.default_rng(62).uniform(-0.5, 0.5, (len(rects), 2)) * (1.0 if name == "mid" else 6.0)

    def run(lib):
        with lib.Context(lib.default_params(image_w=96, image_h=80, patch_w=PW, patch_h=PH, scale=SCALE, tv_weight=0.0,
                                            loss=lib.LOSS_VARIANCE, min_events=MIN_EVENTS, max_events=len(pev),
                                            max_windows=2)) as c:
            c.set_patches(pev, poffs, rects)
            if "EBO_EVAL_TILES" in env:
                assert c.eval_launch_shape()[0] == int(env["EBO_EVAL_TILES"])
            return _eval_all(c, f)[0]
    r = _under_boxes(ebo, ebo_ab, monkeypatch, run, env=env, shipped=False)[0]
    assert (r != 0).all()


@pytest.mark.parametrize("name", ["mid", "border"])
def test_sigma_below_one(ebo, ebo_ab, monkeypatch, name):
    """sigma = 0.5: the k_eval3<false> instantiation."""
    ev, offs = _scene(ebo)
    flows = _flows(name)

    def run(lib):
        with _ctx(lib, len(ev), 2, sigma=0.5) as c:
            c.set_windows(ev, offs)
            return _eval_all(c, flows)[0]
    _under_boxes(ebo, ebo_ab, monkeypatch, run)


@pytest.mark.parametrize("name", ["mid", "border"])
def test_central_differences(ebo, ebo_ab, monkeypatch, name):
    """EBO_GRAD_CENTRAL: five flow sets; each set's flow takes its own decision."""
    ev, offs = _scene(ebo)
    flows = _flows(name)

    def run(lib):
        with _ctx(lib, len(ev), 2, grad=lib.GRAD_CENTRAL) as c:
            c.set_windows(ev, offs)
            return _eval_all(c, flows)[0]
    _, J, _, _, _ = _under_boxes(ebo, ebo_ab, monkeypatch, run)
    assert (J != 0).any()


@pytest.mark.parametrize("lists", [True, False], ids=["window-lists", "mode-table"])
def test_lock_step_solve(ebo, ebo_ab, monkeypatch, lists):
    """A lock-step solve: rounds with per-slot modes 0 / 1 / 2 and, once windows finish, window lists."""
    ev, offs = _scene(ebo, seed=23, windows=2, moving=True)

    def run(lib):
        with _ctx(lib, len(ev), 2, tv_weight=1e3) as c:
            c.set_windows(ev, offs)
            opts = lib.default_solver()
            opts.max_num_iterations = 8
            flows, summ = c.solve(opts)
            return flows.copy(), [(s.iterations, s.final_cost, s.termination, s.num_evals_cost, s.num_evals_jac) for s in summ]
    flows, _ = _under_boxes(ebo, ebo_ab, monkeypatch, run, env=None if lists else {"EBO_SOLVE_NO_COMPACT": "1"})
    assert (flows != 0).any()


def test_solve_device(ebo, ebo_ab, monkeypatch):
    """k_solve_independent: every evaluation of a solve decides for its own flow; flows and statistics."""
    import torch
    ev, offs = _scene(ebo, seed=24, moving=True)

    def run(lib):
        with _ctx(lib, len(ev), 2) as c:
            c.set_windows(ev, offs)
            opts = lib.default_solver(mode=lib.SOLVE_INDEPENDENT, max_num_iterations=12)
            d_sol = torch.full((2 * P, 2), -5.0, dtype=torch.float64, device="cuda")
            d_stats = torch.full((2 * P, 4), -5, dtype=torch.int32, device="cuda")
            torch.cuda.synchronize()
            c.solve_device(opts, d_sol.data_ptr(), d_stats.data_ptr())
            c.synchronize()
            return d_sol.cpu().numpy().copy(), d_stats.cpu().numpy().copy()
    sol, stats = _under_boxes(ebo, ebo_ab, monkeypatch, run)
    active = np.concatenate([np.roll(COUNTS, 3 * w) > MIN_EVENTS for w in range(2)])
    assert (stats[~active] == 0).all() and (stats[active, 1] > 0).all()
    assert (np.abs(sol[active]).max(axis=1) > 0).any()


def test_recorded_graph_survives_a_reload(ebo, ebo_ab, monkeypatch):
    """ebo_eval_device recorded into a graph: the recording holds the table's address, which no load moves -- replayed
    after a reload of other events, it gives what a direct call gives then."""
    import torch
    ev, offs = _scene(ebo, seed=25)
    ev2, offs2 = _scene(ebo, seed=26, shift=4)
    flows = _flows("border").reshape(-1, 2)

    def run(lib):
        with _ctx(lib, max(len(ev), len(ev2)), 2) as c:
            stream = torch.cuda.Stream()
            c.set_stream(stream.cuda_stream)
            c.set_windows(ev, offs)
            d_flows = torch.from_numpy(flows.copy()).to("cuda")
            d_out = torch.zeros((2 * P, 3), dtype=torch.float64, device="cuda")
            torch.cuda.synchronize()
            step = lambda: c.eval_device(d_flows.data_ptr(), 1, d_out.data_ptr())
            step()
            c.synchronize()
            first = d_out.cpu().numpy().copy()
            g = c.record(step)
            d_out.fill_(-3.0)
            torch.cuda.synchronize()
            g.launch(2)
            c.synchronize()
            replayed = d_out.cpu().numpy().copy()
            assert _same(first, replayed)
            c.set_windows(ev2, offs2)
            step()
            c.synchronize()
            direct2 = d_out.cpu().numpy().copy()
            d_out.fill_(-3.0)
            torch.cuda.synchronize()
            g.launch(1)
            c.synchronize()
            replayed2 = d_out.cpu().numpy().copy()
            g.close()
            assert _same(direct2, replayed2) and not _same(first, direct2)
        return first, direct2
    _under_boxes(ebo, ebo_ab, monkeypatch, run)


# ---- which path ran -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["zero", "mid", "negative", "border", "nan"])
def test_path_counts_equal_the_rule(ebo, ebo_ab, monkeypatch, name):
    """The A/B library counts, per launch, the units whose box came from each path: equal to the numpy restatement of
    the rule on the table -- every active unit on the table where nothing is clipped, exactly the predicted units on the
    event pass in the border and NaN scenes, everybody on the event pass under EBO_EVAL_BOX=events -- and the shipped
    library says that it does not count."""
    ev, offs = _scene(ebo)
    flows = _flows(name)
    n_active = int(sum((np.roll(COUNTS, 3 * w) > MIN_EVENTS).sum() for w in range(2)))
    monkeypatch.delenv("EBO_EVAL_BOX", raising=False)
    with _ctx(ebo_ab, len(ev), 2) as c:
        c.set_windows(ev, offs)
        want_ev, want_tab, margin = _predict(c, c.unit_extents(), flows)
        assert want_ev + want_tab == n_active
        if name in ("zero", "mid", "negative"):
            assert want_ev == 0  # the no-clipping scenes: the table everywhere
        elif name == "border":
            assert want_ev >= 4 and want_tab >= 4 and margin >= 2  # both paths, and table boxes inside the canvas's edge
        else:
            assert want_ev == 5  # the five units with a NaN, an infinite or a huge component
        _, seen = _eval_all(c, flows, counts=True)
        assert seen == [(want_ev, want_tab)] * 4, name
        monkeypatch.setenv("EBO_EVAL_BOX", "events")
        try:
            _, seen = _eval_all(c, flows, counts=True)
        finally:
            monkeypatch.delenv("EBO_EVAL_BOX", raising=False)
        assert seen == [(n_active, 0)] * 4
    with _ctx(ebo, len(ev), 2) as c:
        c.set_windows(ev, offs)
        with pytest.raises(ebo.EboError):
            c.box_path_counts()
