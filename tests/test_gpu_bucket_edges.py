"""GPU tests of the device bucketing (csrc/ebo_bucket.inc: k_bucket_count, _scan, _chunk_scan, _scatter, _canon) at its
edges, against the plain restatement of tests/bucket_ref.py: the window and unit tables and -- through the read-back
ebo_unit_records -- every packed record of every unit in its place, on every loading path.  Everything compared is an
integer or a bit pattern; there is no tolerance anywhere.  tests/test_bucket_ref_cpu.py checks that each case holds the
edge it is named after.

Not readable through the ABI, and so pinned only through the (E) comparisons of evaluations and count images between
the paths: a unit's dt_win and flow_idx (the stray unit's events take them in COUNT_WARPED)."""
import numpy as np
import pytest

import bucket_ref as br

pytestmark = pytest.mark.gpu

PAD = 3  # records in front of the first window of a device buffer: offsets that do not start at 0
SHIPPED_PATHS = ("set_windows", "set_windows_device", "set_windows8", "set_windows8_device")


def context(mod, case, **kw):
    g = case.grid
    return mod.Context(image_w=g.image_w, image_h=g.image_h, patch_w=g.patch_w, patch_h=g.patch_h, loss=mod.LOSS_VARIANCE,
                       min_events=case.min_events, max_windows=len(case.offsets) - 1, max_events=max(len(case.ev), 1) + PAD, **kw)


def base_times(case):
    """per-window base times of the compact records that are NOT the first event's: some t_rel_us are negative"""
    if case.t_base is not None:
        return case.t_base
    first = [int(case.ev["t_us"][int(a)]) + 5 if b > a else 12345 for a, b in zip(case.offsets[:-1], case.offsets[1:])]
    return np.array(first, dtype=np.int64)


def compact(ebo, case):
    tb = base_times(case)
    parts = [ebo.pack_events8(case.ev[int(case.offsets[w]):int(case.offsets[w + 1])], tb[w]) for w in range(len(tb))]
    ev8 = np.concatenate(parts) if parts else np.zeros(0, dtype=ebo.EVENT8_DTYPE)
    if len(case.ev) > 1:
        assert (ev8["t_rel_us"] < 0).any()
    return ev8, tb


def on_device(records):
    """the records behind PAD junk ones, in device memory -> (tensor that owns them, pointer)"""
    import torch
    junk = np.full(PAD, 0x5A, dtype=np.uint8).repeat(records.dtype.itemsize)
    d = torch.from_numpy(np.concatenate([junk, np.ascontiguousarray(records).view(np.uint8).reshape(-1)])).to("cuda")
    torch.cuda.synchronize()
    return d, d.data_ptr()


def load(ebo, c, path, case):
    if path == "set_windows":
        c.set_windows(case.ev, case.offsets)
    elif path == "set_windows_device":
        keep, ptr = on_device(case.ev)
        c.set_windows_device(ptr, case.offsets + np.uint64(PAD))
    else:
        ev8, tb = compact(ebo, case)
        if path == "set_windows8":
            c.set_windows8(ev8, tb, case.offsets)
        else:
            keep, ptr = on_device(ev8)
            c.set_windows8(ptr, tb, case.offsets + np.uint64(PAD), device=True)


def check_against(c, ref, what):
    """window_info, patch_info of every patch, unit_records of every bucket, and the grid's rects"""
    P = c.P
    assert c.n_windows == len(ref)
    for p in range(P):
        assert c.patch_rect(p % c.npx, p // c.npx) == ref[0].buckets[p].rect, (what, p)
    for w, rw in enumerate(ref):
        assert len(rw.buckets) == P + 1
        assert c.window_info(w) == (rw.t_ref, rw.size), (what, w)
        for b, rb in enumerate(rw.buckets):
            if b < P:
                assert c.patch_info(b, w) == (rb.count, rb.active, rb.t_ref), (what, w, b)
            got = c.unit_records(w, b)
            assert got.dtype == np.uint64 and len(got) == rb.count, (what, w, b, len(got), rb.count)
            if not np.array_equal(got, rb.records):
                at = int(np.flatnonzero(got != rb.records)[0])
                raise AssertionError("%s: window %d bucket %d (%d records) differs first at position %d: %016x, expected %016x"
                                     % (what, w, b, rb.count, at, int(got[at]), int(rb.records[at])))


def evaluations(ebo, c, case):
    """r, J of the variance loss and both count images at a small random flow, for the bit-for-bit comparison of paths"""
    flows = np.random.default_rng(77).uniform(-1.0, 1.0, (c.n_windows, c.P, 2))
    r, J = c.eval(flows)
    return r, J, c.count_image(ebo.COUNT_INTEGRATED), c.count_image(ebo.COUNT_WARPED, flows)


def run_case(ebo, ebo_ab, monkeypatch, case, shipped=SHIPPED_PATHS):
    ref = br.reference(case)
    results = {}
    with context(ebo, case) as c:
        for path in shipped:
            load(ebo, c, path, case)
            check_against(c, ref, "%s %s" % (case.name, path))
            if case.eval:
                results[path] = evaluations(ebo, c, case)
    monkeypatch.setenv("EBO_BUCKET", "host")
    with context(ebo_ab, case) as c:
        c.set_windows(case.ev, case.offsets)
        check_against(c, ref, "%s EBO_BUCKET=host" % case.name)
        if case.eval:
            results["EBO_BUCKET=host"] = evaluations(ebo_ab, c, case)
    if case.eval:
        first = results[shipped[0]]
        assert np.any(first[0] != 0) and np.any(first[1] != 0) and first[2].sum() > 0
        for path, got in results.items():
            for a, b in zip(first, got):
                assert np.array_equal(a, b), (case.name, path)


CASES = {
    "sizes": br.case_sizes,
    "chunk_switch": lambda: br.case_chunk_switch(False),
    "chunk_switch_filler": lambda: br.case_chunk_switch(True),
    "skew": br.case_skew,
    "unit_sizes": br.case_unit_sizes,
    "ties": br.case_ties,
    "strays": br.case_strays,
    "min_events_0": lambda: br.case_min_events(0),
    "min_events_1": lambda: br.case_min_events(1),
    "min_events_100": lambda: br.case_min_events(100),
    "times": br.case_times,
    "finest": lambda: br.case_finest(br.FINE_FITS),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_path_equals_the_restatement(ebo, ebo_ab, monkeypatch, name):
    """The cases of bucket_ref.py (what each holds: test_bucket_ref_cpu.py).  chunk_switch and chunk_switch_filler share
    their first four windows: 256-event chunks without the filler window, 2048-event chunks with it (2^19 + 1 events),
    and both equal the restatement, hence each other.  unit_sizes: the unit of 8193 events is in list order on every
    path.  finest: 8100 patches, the finest grid the device path admits at this sensor shape."""
    run_case(ebo, ebo_ab, monkeypatch, CASES[name]())


def test_not_time_ordered_windows_load_as_the_ordered_ones(ebo, ebo_ab, monkeypatch):
    """The events between a window's first and last one in a random order: every path, the host sort included, gives the
    tables of the ordered load and -- for units of up to 8192 events -- its records.  The exception is the unit of 9000
    events of the second window, which keeps the order of the list on every path: there the restatement of the PERMUTED
    list is what is compared (test_bucket_ref_cpu.py::test_unordered_case: it differs from the ordered load's)."""
    perm, ordered = br.case_unordered(True), br.case_unordered(False)
    rp, ro = br.reference(perm), br.reference(ordered)
    for wp, wo in zip(rp, ro):
        for bp, bo in zip(wp.buckets, wo.buckets):
            assert bp[:6] == bo[:6] and (bp.count > br.SORT_MAX or np.array_equal(bp.records, bo.records))
    run_case(ebo, ebo_ab, monkeypatch, perm)


@pytest.mark.parametrize("seed", br.SWEEP_SEEDS)
def test_random_sweep(ebo, ebo_ab, monkeypatch, seed):
    run_case(ebo, ebo_ab, monkeypatch, br.case_sweep(seed))


def test_time_range_fault_fails_the_whole_call_and_the_next_load_succeeds(ebo, ebo_ab, monkeypatch):
    """A window at t = 0 and t = 2^32 has its mid time at 2^31: EBO_ERR_RANGE, alone or in the middle of a batch, on
    every path that can carry it (no compact record holds both stamps: ebo_pack_events8 refuses them)."""
    fault, good = br.case_time_fault(), br.case_strays()
    alone = br.make_case("time_fault_alone", br.G16, [fault.ev[int(fault.offsets[1]):int(fault.offsets[2])]])
    with pytest.raises(ebo.EboError) as ei:
        ebo.pack_events8(alone.ev, 1 << 31)
    assert ei.value.code == ebo.ERR_RANGE
    ref = br.reference(good)

    def both(mod, c, paths):
        for path in paths:
            for bad in (alone, fault):
                with pytest.raises(mod.EboError) as ei:
                    load(mod, c, path, bad)
                assert ei.value.code == mod.ERR_RANGE, (path, bad.name)
            load(mod, c, path, good)
            check_against(c, ref, "after a refused load, " + path)

    with ebo.Context(image_w=70, image_h=50, patch_w=16, patch_h=12, loss=ebo.LOSS_VARIANCE, min_events=good.min_events,
                     max_windows=3, max_events=1000) as c:
        both(ebo, c, ("set_windows", "set_windows_device"))
    monkeypatch.setenv("EBO_BUCKET", "host")
    with ebo_ab.Context(image_w=70, image_h=50, patch_w=16, patch_h=12, loss=ebo.LOSS_VARIANCE, min_events=good.min_events,
                        max_windows=3, max_events=1000) as c:
        both(ebo_ab, c, ("set_windows",))


def test_grid_too_fine_for_the_device_histogram(ebo):
    """8190 patches: one more than k_bucket_count's LDS histogram holds (8140 slots).  set_windows falls back to the host
    sort and still equals the restatement; the device-only loaders refuse."""
    case = br.case_finest(br.FINE_TOO_FINE)
    with context(ebo, case) as c:
        assert c.P == 8190
        c.set_windows(case.ev, case.offsets)
        check_against(c, br.reference(case), "finest_91 set_windows")
        for path in SHIPPED_PATHS[1:]:
            with pytest.raises(ebo.EboError) as ei:
                load(ebo, c, path, case)
            assert ei.value.code == ebo.ERR_UNSUPPORTED, path


def test_set_patches_records_and_reference_times(ebo):
    """Three patch lists of 1, 200 and 9000 events, not time-ordered: canonical records for the first two, list order for
    the third, and the reference time of the first and last LISTED stamp (the functor's constructor)."""
    ev, offsets, rects = br.patches_case()
    want = br.patch_units(ev, offsets)
    with ebo.Context(image_w=64, image_h=48, patch_w=16, patch_h=12, loss=ebo.LOSS_VARIANCE, max_windows=1,
                     max_events=len(ev)) as c:
        c.set_patches(ev, offsets, rects)
        for i, (t_ref, records) in enumerate(want):
            n, _, t = c.patch_info(i, 0)
            assert (n, t) == (len(records), t_ref), i
            assert np.array_equal(c.unit_records(0, i), records), i


def test_unit_records_arguments_and_state(ebo):
    import ctypes as C
    case = br.case_strays()
    ref = br.reference(case)
    f = ebo.lib().ebo_unit_records
    f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
    with context(ebo, case) as c:
        c.set_windows(case.ev, case.offsets)
        P = c.P
        full = max(range(P), key=lambda b: ref[0].buckets[b].count)
        size = ref[0].buckets[full].count
        buf = np.zeros(size, dtype=np.uint64)
        n = C.c_size_t(0)
        ptr = buf.ctypes.data_as(C.c_void_p)
        for w, b in ((-1, 0), (1, 0), (0, -1), (0, P + 1)):
            assert f(c._h, w, b, ptr, size, C.byref(n)) == ebo.ERR_ARG, (w, b)
        assert f(c._h, 0, full, ptr, size, None) == ebo.ERR_ARG           # nowhere to report the size
        assert f(None, 0, full, ptr, size, C.byref(n)) == ebo.ERR_ARG
        assert f(c._h, 0, full, None, size, C.byref(n)) == ebo.ERR_ARG and n.value == size
        n.value = 0
        assert f(c._h, 0, full, ptr, size - 1, C.byref(n)) == ebo.ERR_ARG and n.value == size  # too small: n is reported
        assert not buf.any()                                              # and nothing was written
        assert f(c._h, 0, full, ptr, size, C.byref(n)) == 0 and n.value == size
        assert np.array_equal(buf, ref[0].buckets[full].records)
        stray = np.zeros(6, dtype=np.uint64)
        assert f(c._h, 0, P, stray.ctypes.data_as(C.c_void_p), 6, C.byref(n)) == 0 and n.value == 6  # the stray bucket
        assert np.array_equal(stray, ref[0].buckets[P].records)
        again = c.unit_records(0, full)
        assert np.array_equal(again, buf) and np.array_equal(c.unit_records(0, full), again)  # reads change nothing
        refused = []

        def body():
            try:
                c.unit_records(0, full)
            except ebo.EboError as exc:
                refused.append((exc.code, "recording" in str(exc)))
        g = c.record(body)
        assert refused == [(ebo.ERR_STATE, True)]
        g.close()
        check_against(c, ref, "after the refused read-back")
        ev, offsets, rects = br.patches_case()
    with ebo.Context(image_w=64, image_h=48, patch_w=16, patch_h=12, loss=ebo.LOSS_VARIANCE, max_windows=1,
                     max_events=len(ev)) as c:
        c.set_patches(ev, offsets, rects)
        big = np.zeros(9000, dtype=np.uint64)
        n = C.c_size_t(0)
        for w, b in ((1, 0), (0, 3), (0, -1)):  # after ebo_set_patches: window 0, bucket = the patch index
            assert f(c._h, w, b, big.ctypes.data_as(C.c_void_p), 9000, C.byref(n)) == ebo.ERR_ARG, (w, b)
        assert f(c._h, 0, 2, big.ctypes.data_as(C.c_void_p), 9000, C.byref(n)) == 0 and n.value == 9000
