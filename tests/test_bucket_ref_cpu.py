"""CPU checks of tests/bucket_ref.py, the restatement that tests/test_gpu_bucket_edges.py compares the device bucketing
with: the strided deal of the canonical order for every unit size it applies to (against its definition and against
the product's own csrc/order_deal.h, compiled for the host), and every edge case's content -- a case that does not
contain the edge it is named after fails here, not silently on the GPU."""
import os
import subprocess

import numpy as np
import pytest

import bucket_ref as br

HERE = os.path.dirname(os.path.abspath(__file__))
N_MAX = br.SORT_MAX + 1


def test_stride_is_coprime_and_the_deal_a_permutation_with_the_stated_inverse():
    for n in range(1, N_MAX + 1):
        st = br.order_stride(n)
        assert 1 <= st < max(n, 2) and br.gcd(st, n) == 1, (n, st)
        dealt = br.deal(np.arange(n, dtype=np.uint64)).astype(np.int64)  # dealt[q] = the rank at position q
        assert np.array_equal(np.sort(dealt), np.arange(n)), n
        if n >= 2:
            assert np.array_equal(dealt, (np.arange(n) * st) % n), n
            where = (np.arange(n) * br.order_inverse(st, n)) % n  # where[r] = the position of rank r
            assert np.array_equal(dealt[where], np.arange(n)), n
    # the sizes at which 127 mod n is 1, 0, or shares a factor with n and the search moves on
    assert [br.order_stride(n) for n in (1, 2, 3, 126, 127, 128, 254)] == [1, 1, 1, 1, 1, 127, 129]
    assert br.order_stride(8191) == 127 and br.order_stride(8192) == 127


def test_deal_equals_the_products_own(tmp_path):
    """csrc/order_deal.h (what k_bucket_canon and the host sort include) as the host compiles it."""
    exe = str(tmp_path / "order_deal_test")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-o", exe,
                           os.path.join(HERE, "cpp", "order_deal_test.cpp")])
    out = subprocess.run([exe, "1", str(N_MAX)], capture_output=True, text=True, timeout=120, check=True).stdout.split("\n")
    for n in range(1, N_MAX + 1):
        got = tuple(int(v) for v in out[n - 1].split())
        st = br.order_stride(n)
        assert got == (n, st, br.order_inverse(st, n) % n), (n, got)


def test_mid_time_truncates_toward_zero_in_float64():
    assert br.mid_time(-50000, -1) == -25000 and br.mid_time(-3, 0) == -1 and br.mid_time(3, 0) == 1
    assert br.mid_time(0, br.T_WIDE) == (1 << 31) - 1
    assert br.mid_time(-(1 << 32) + 1, 0) == -(1 << 31) + 1  # -2147483647.5
    for a, b in ((0, 1 << 32), (-(1 << 32), 0)):
        with pytest.raises(br.RangeError):
            br.mid_time(a, b)
    assert br.mid_time((1 << 62) + 1, -(1 << 62)) == 0  # the SUM is rounded to a double first, as the device does


def time_ordered(case):
    return all(np.all(np.diff(case.ev["t_us"][int(a):int(b)]) >= 0) for a, b in zip(case.offsets[:-1], case.offsets[1:]))


def signed_dt(records):
    return (records >> np.uint64(32)).astype(np.uint32).view(np.int32)


def test_sizes_case():
    case = br.case_sizes()
    ref = br.reference(case)
    assert tuple(w.size for w in ref) == br.SIZES == (0, 1, 2, 63, 64, 65, 255, 256, 257, 511, 513, 0, 1000, 0)
    assert ref[0].size == 0 and ref[-1].size == 0 and 0 in [w.size for w in ref[1:-1]]
    assert time_ordered(case) and case.eval
    for w in ref:
        assert sum(b.count for b in w.buckets) == w.size
        assert all(b.t_ref == w.t_ref and not b.active for b in w.buckets if b.count == 0)
    assert ref[-2].buckets[-1].count == 2 and any(b.active for b in ref[-2].buckets)


def test_chunk_switch_cases():
    small, big = br.case_chunk_switch(False), br.case_chunk_switch(True)
    sizes = [int(b - a) for a, b in zip(big.offsets[:-1], big.offsets[1:])]
    assert tuple(sizes[:4]) == br.CHUNK_WINDOWS == (2047, 2048, 2049, 4097) and len(sizes) == 5
    assert int(big.offsets[-1]) == (1 << 19) + 1       # above 2^19 events: 2048-event chunks
    assert int(small.offsets[-1]) == sum(br.CHUNK_WINDOWS) <= 1 << 19  # 256-event chunks
    n = int(small.offsets[-1])
    assert np.array_equal(small.ev, big.ev[:n]) and np.array_equal(small.offsets, big.offsets[:5])
    assert time_ordered(big)
    rs, rb = br.reference(small), br.reference(big)
    for a, b in zip(rs, rb):
        assert (a.t_ref, a.size) == (b.t_ref, b.size)
        for ua, ub in zip(a.buckets, b.buckets):
            assert ua[:5] == ub[:5] and np.array_equal(ua.records, ub.records)
    assert max(b.count for b in rb[4].buckets) > br.SORT_MAX  # the filler's units keep list order: the stable scatter alone


def buckets_of(case, w):
    """bucket per event of window w, from the restatement's rects"""
    rects = br.grid_rects(case.grid)
    e = case.ev[int(case.offsets[w]):int(case.offsets[w + 1])]
    out = np.full(len(e), len(rects))
    for k, (x, y, rw, rh) in enumerate(rects):
        out[(e["x"] >= x) & (e["x"] < x + rw) & (e["y"] >= y) & (e["y"] < y + rh)] = k
    return out


def test_skew_case():
    case = br.case_skew()
    P = 576
    assert len(br.grid_rects(case.grid)) == P
    walk = buckets_of(case, 0)
    assert len(walk) > 64 * 20 and len(walk) % 64
    for s in range(0, len(walk) - 63, 64):  # every full step of the scatter: 64 distinct buckets
        assert sorted(walk[s:s + 64]) == list(range(64))
    single = buckets_of(case, 1)
    assert len(single) == 700 and set(single) == {br.SKEW_SINGLE}
    alt = buckets_of(case, 2)
    assert np.array_equal(alt, np.array([br.SKEW_PAIR[0], br.SKEW_PAIR[1], P])[np.arange(len(alt)) % 3])
    ref = br.reference(case)
    assert [b.count for b in ref[1].buckets if b.count] == [700] and ref[2].buckets[P].count == 200
    assert time_ordered(case)


def test_unit_sizes_case():
    case = br.case_unit_sizes()
    w = br.reference(case)[0]
    assert tuple(b.count for b in w.buckets[:10]) == br.UNIT_SIZES == (1, 2, 3, 126, 127, 128, 254, 8191, 8192, 8193)
    assert all(1 <= b.count <= 8 for b in w.buckets[10:16]) and w.buckets[16].count == 0
    assert time_ordered(case) and case.eval
    for b in w.buckets[:9]:
        ranked = np.sort(b.records)
        assert np.array_equal(b.records, ranked[(np.arange(b.count) * br.order_stride(b.count)) % b.count])
    big = w.buckets[9]
    dt = signed_dt(big.records).astype(np.int64)
    assert np.all(np.diff(dt) <= 0)                           # list order of a time-ordered window: stamps never fall
    assert not np.array_equal(big.records, np.sort(big.records))  # ... which is neither the ranked order
    assert not np.array_equal(big.records, br.deal(np.sort(big.records)))  # nor the dealt one


def run_members(b):
    """{signed dt: lo words} of the runs of equal stamps of a bucket"""
    dt = signed_dt(b.records)
    lo = (b.records & np.uint64(0xFFFFFFFF)).astype(np.int64)
    return {int(d): lo[dt == d] for d in np.unique(dt) if (dt == d).sum() > 1}


def test_ties_case():
    case = br.case_ties()
    assert time_ordered(case) and case.eval and len(case.offsets) == 2
    w = br.reference(case)[0]
    for p, run in enumerate(br.TIE_MID_RUNS):
        b = w.buckets[p]
        runs = run_members(b)
        assert [len(v) for v in runs.values()] == [run], (p, runs)
        dt = signed_dt(b.records)
        (at,) = runs
        assert dt.min() < at < dt.max() and b.count == 40 + run  # in the middle of the unit
    assert br.TIE_MID_RUNS == (2, 31, 32, 33, 64) and br.RUN_MAX == 32
    first, last, mid = w.buckets[br.TIE_FIRST], w.buckets[br.TIE_LAST], w.buckets[br.TIE_REF]
    assert {k: len(v) for k, v in run_members(first).items()} == {int(signed_dt(first.records).max()): 5}  # earliest stamp
    assert {k: len(v) for k, v in run_members(last).items()} == {int(signed_dt(last.records).min()): 5}    # latest stamp
    assert {k: len(v) for k, v in run_members(mid).items()} == {0: 7}  # at the unit's reference time
    assert signed_dt(mid.records).min() < 0 < signed_dt(mid.records).max()
    for p, n in ((br.TIE_ALL20, 20), (br.TIE_ALL40, 40)):
        b = w.buckets[p]
        assert b.count == n and np.all(signed_dt(b.records) == 0)
    # inside the runs: records that differ only in x, only in y, only in polarity, and exact duplicates
    seen = set()
    for b in w.buckets[:10]:
        for lo in run_members(b).values():
            d = lo[:, None] ^ lo[None, :]
            off = ~np.eye(len(lo), dtype=bool)
            seen |= {"dup"} if np.any((d == 0) & off) else set()
            seen |= {"pol"} if np.any(d == 0x8000) else set()
            seen |= {"x"} if np.any((d != 0) & (d & ~0x7FFF == 0)) else set()
            seen |= {"y"} if np.any((d != 0) & (d & ~0x7FFF0000 == 0)) else set()
    assert seen == {"dup", "pol", "x", "y"}
    assert all(b.active for b in w.buckets[:16])


def test_strays_case():
    case = br.case_strays()
    w = br.reference(case)[0]
    P = 16
    stray = w.buckets[P]
    assert (stray.count, stray.rect, stray.t_ref, stray.active, stray.dt_win, stray.flow_idx) == (6, (0, 0, 1, 1), w.t_ref, False, 0, P - 1)
    lo = set((stray.records & np.uint64(0xFFFFFFFF)).tolist())
    e = case.ev
    for x, y in br.STRAY_POINTS:
        s = int(e["sign"][(e["x"] == x) & (e["y"] == y)][0])
        assert ((x & 0x7FFF) | ((s > 0) << 15) | ((y & 0x7FFF) << 16)) in lo
    assert set(br.STRAY_POINTS) >= {(-1, 5), (70, 5), (5, -1), (5, 50), (-16384, 16383), (16383, -16384)}
    rects = br.grid_rects(case.grid)
    assert rects[P - 1] == (48, 36, 22, 14) and rects[3] == (48, 0, 22, 12) and rects[12] == (0, 36, 16, 14)
    b = buckets_of(case, 0)
    at = np.flatnonzero((e["x"] == br.LAST_PIXEL[0]) & (e["y"] == br.LAST_PIXEL[1]))
    assert br.LAST_PIXEL == (69, 49) and len(at) >= 1 and np.all(b[at] == P - 1)
    assert np.array_equal(np.bincount(b, minlength=P + 1), [u.count for u in w.buckets])


@pytest.mark.parametrize("m", [0, 1, 100])
def test_min_events_case(m):
    case = br.case_min_events(m)
    w = br.reference(case)[0]
    assert case.min_events == m
    assert (w.buckets[0].count, w.buckets[0].active) == (m, False)
    assert (w.buckets[1].count, w.buckets[1].active) == (m + 1, True)
    assert (w.buckets[2].count, w.buckets[2].active, w.buckets[2].t_ref) == (0, False, w.t_ref)
    assert not w.buckets[16].active


def test_times_cases():
    case = br.case_times()
    ref = br.reference(case)
    t = case.ev["t_us"][:int(case.offsets[1])]
    assert (t.min(), t.max(), t[0], t[-1]) == (-50000, -1, -50000, -1)
    assert ref[0].t_ref == -25000 and (t[0] + t[-1]) // 2 == -25001  # toward zero, not toward minus infinity
    assert ref[1].size == 2 and ref[1].t_ref == (1 << 31) - 1
    assert [b.count for b in ref[1].buckets if b.count] == [2]
    rel = case.ev["t_us"][int(case.offsets[1]):] - case.t_base[1]
    assert rel.min() >= br.I32_MIN and rel.max() <= br.I32_MAX  # the compact record holds them
    assert np.any(case.ev["t_us"][:int(case.offsets[1])] - case.t_base[0] < 0)
    fault = br.case_time_fault()
    with pytest.raises(br.RangeError):
        br.reference(fault)
    assert len(fault.offsets) == 4  # the faulty window is the middle one


def test_unordered_case():
    perm, ordered = br.case_unordered(True), br.case_unordered(False)
    assert time_ordered(ordered) and not time_ordered(perm)
    rp, ro = br.reference(perm), br.reference(ordered)
    big = 0
    for w in range(2):
        a, b = int(perm.offsets[w]), int(perm.offsets[w + 1])
        assert np.array_equal(perm.ev[[a, b - 1]], ordered.ev[[a, b - 1]])  # first and last stay
        assert np.array_equal(np.sort(perm.ev[a:b], order=["t_us", "x", "y", "sign"]),
                              np.sort(ordered.ev[a:b], order=["t_us", "x", "y", "sign"]))
        assert np.any(np.diff(perm.ev["t_us"][a:b]) < 0)
        assert (rp[w].t_ref, rp[w].size) == (ro[w].t_ref, ro[w].size)
        for up, uo in zip(rp[w].buckets, ro[w].buckets):
            assert up[:6] == uo[:6]  # the tables do not depend on the order of the list
            if up.count <= br.SORT_MAX:
                assert np.array_equal(up.records, uo.records)  # nor do the records
            else:
                big += 1  # the exception: list order, which the permutation changed
                assert not np.array_equal(up.records, uo.records)
                assert np.array_equal(np.sort(up.records), np.sort(uo.records))
    assert big == 1 and rp[1].buckets[15].count == br.UNORDERED_BIG > br.SORT_MAX
    # a unit's first / last LISTED stamps are not its earliest / latest ones: what the host path used to take
    e = perm.ev[:int(perm.offsets[1])]
    b = buckets_of(perm, 0)
    differ = 0
    for k in range(16):
        t = e["t_us"][b == k]
        differ += br.mid_time(t[0], t[-1]) != br.mid_time(t.min(), t.max())
    assert differ >= 8


def test_finest_grid_cases():
    lds_budget = 160 * 1024
    fits = lambda g: (g.image_w * g.image_h + 1) * (2 * 8 + 4) + 8 <= lds_budget - 1024
    assert fits(br.FINE_FITS) and not fits(br.FINE_TOO_FINE)
    assert (lds_budget - 1024 - 8) // 20 == 8140
    for g, P in ((br.FINE_FITS, 8100), (br.FINE_TOO_FINE, 8190)):
        case = br.case_finest(g)
        ref = br.reference(case)
        assert len(ref[0].buckets) == P + 1 and ref[0].buckets[P].count == 3 and ref[1].buckets[P].count == 1
        assert max(b.count for w in ref for b in w.buckets[:P]) >= 2 and case.min_events == 0


def test_sweep_cases():
    short = long = empty = 0
    grids, quanta, mins = set(), set(), set()
    assert len(br.SWEEP_SEEDS) == 40
    for seed in br.SWEEP_SEEDS:
        case = br.case_sweep(seed)
        assert time_ordered(case) and 1 <= len(case.offsets) - 1 <= 6
        assert all(0 <= int(b - a) <= 6000 for a, b in zip(case.offsets[:-1], case.offsets[1:]))
        grids.add(case.grid)
        mins.add(case.min_events)
        quanta.add(int(case.name.rsplit("q", 1)[1]))
        for w in br.reference(case):
            assert 0 <= w.buckets[-1].count <= 5
            for b in w.buckets:
                if b.count == 0:
                    empty += 1
                    continue
                longest = br.stamp_runs(b.records).max()
                short += 2 <= longest <= br.RUN_MAX
                long += longest > br.RUN_MAX
    assert grids == {br.G16, br.G16R, br.G576} and quanta == {1, 7, 100, 2000} and mins == {0, 10, 100}
    assert short >= 20 and long >= 20 and empty >= 20, (short, long, empty)


def test_patches_case():
    ev, offsets, rects = br.patches_case()
    assert tuple(int(b - a) for a, b in zip(offsets[:-1], offsets[1:])) == br.PATCH_SIZES == (1, 200, 9000)
    units = br.patch_units(ev, offsets)
    for i in (1, 2):
        t = ev["t_us"][int(offsets[i]):int(offsets[i + 1])]
        assert np.any(np.diff(t) < 0)  # list order is not time order
        assert units[i][0] == br.mid_time(t[0], t[-1]) != br.mid_time(t.min(), t.max())
        assert br.stamp_runs(units[i][1]).max() == 2
    assert np.array_equal(units[1][1], br.deal(np.sort(units[1][1])))
    assert not np.array_equal(units[2][1], br.deal(np.sort(units[2][1])))
    assert len(rects) == 3
