"""CPU: the scenes of tests/plumbing_cases.py reach the edges they are named after, checked with the oracle alone.
Routing: the oracle's loop and the plain numpy selection agree on every call, and each "filling event" patch fills its
quota at the index it claims.  Patch images: the non-square images change under a swap of rows and columns, the ring
outside a rect contributes nothing while the ring inside contributes everything, each rounding tie lands where it is
listed, each time test passes or fails as listed, and the oracle refuses fractional and non-finite sizes.  Initial
field: lower_bound, rounding, overwriting, the zero-velocity rule and the nearest-fill tie as listed.  No GPU."""
import math

import numpy as np
import pytest

import plumbing_cases as K

CHUNKS, CALLS = K.route_calls()


# ---- routing ------------------------------------------------------------------------------------------------------------

def assert_routed(got, nxt, want, wnxt, what):
    assert len(got) == len(want), what
    for p in range(len(want)):
        assert np.array_equal(got[p], want[p]), (what, p)
    assert np.array_equal(nxt, wnxt), what


@pytest.mark.parametrize("call", CALLS, ids=[c["name"] for c in CALLS])
def test_route_oracle_is_the_plain_selection(orc, call):
    ev = CHUNKS[call["chunk"]]
    got, nxt = orc.route_events(ev, call["rects"], call["start"], call["take"], call["cap"])
    want, wnxt = K.route_select(ev, call["rects"], call["start"], call["take"], call["cap"])
    assert_routed(got, nxt, want, wnxt, call["name"])


def test_route_dense_chunks_are_dense():
    rx, ry, rw, rh = K.DENSE_RECT
    for n in K.ROUTE_LENGTHS:
        ev = K.dense_chunk(n)
        assert len(ev) == n
        assert np.all((rx <= ev["x"]) & (ev["x"] < rx + rw) & (ry <= ev["y"]) & (ev["y"] < ry + rh))
    for lane in (0, 63):
        ev = K.sparse_chunk(1025, lane)
        inside = np.flatnonzero((rx <= ev["x"]) & (ev["x"] < rx + rw) & (ry <= ev["y"]) & (ev["y"] < ry + rh))
        assert np.array_equal(inside, np.arange(lane, 1025, 64))   # exactly one per sub-step, at that lane


def test_route_filling_events_fill_where_they_claim(orc):
    call = next(c for c in CALLS if c["name"] == "quota")
    ev, n = CHUNKS[call["chunk"]], 1025
    got, nxt = orc.route_events(ev, call["rects"], call["start"], call["take"], call["cap"])
    seen = set()
    for p, (s, q) in enumerate(zip(call["start"].tolist(), call["take"].tolist())):
        if q <= n - s:   # the q-th event from start fills the quota: next is one behind it
            assert np.array_equal(got[p], np.arange(s, s + q)) and nxt[p] == s + q, (s, q)
        else:            # one more than the chunk holds: never filled
            assert np.array_equal(got[p], np.arange(s, n)) and nxt[p] == n, (s, q)
        seen.add(((q - 1) % 256, q <= n - s, s + q == n))   # the walk is aligned to start: the filling event's lane
    # the filling event at the last lane of a sub-step (63), of a step (255) and the first lane of the next (0 again)
    lanes = {k[0] for k in seen if k[1]}
    assert {0, 62, 63, 64, 254, 255}.issubset(lanes)
    assert any(k[2] for k in seen)                         # filled by the chunk's very last event: next == n
    assert any(not k[1] for k in seen)                     # never filled: next == n
    # the sparse chunks: the q-th inside event from start
    for lane in (0, 63):
        call = next(c for c in CALLS if c["name"] == "sparse%d" % lane)
        got, nxt = orc.route_events(CHUNKS[call["chunk"]], call["rects"], call["start"], call["take"], call["cap"])
        for p, (s, q) in enumerate(zip(call["start"].tolist(), call["take"].tolist())):
            inside = np.arange(lane, n, 64)
            inside = inside[inside >= s]
            assert np.array_equal(got[p], inside[:q])
            assert nxt[p] == (inside[q - 1] + 1 if q <= len(inside) else n)
        assert n in nxt.tolist() and any(len(g) == t for g, t in zip(got, call["take"].tolist()))


def test_route_take_and_cap(orc):
    c5 = next(c for c in CALLS if c["name"] == "cap5")
    got, nxt = orc.route_events(CHUNKS[c5["chunk"]], c5["rects"], c5["start"], c5["take"], c5["cap"])
    assert [len(g) for g in got] == [0, 0, 5, 5, 4, 0]
    assert nxt.tolist() == [0, 300, 5, 12, 68, 2000]     # take = 0: next == start, also past the chunk
    c1 = next(c for c in CALLS if c["name"] == "cap1")
    got, nxt = orc.route_events(CHUNKS[c1["chunk"]], c1["rects"], c1["start"], c1["take"], c1["cap"])
    assert [g.tolist() for g in got] == [[], [300], [1024], []] and nxt.tolist() == [0, 301, 1025, 1025]


def test_route_coordinates_reach_the_packed_ends(orc):
    call = next(c for c in CALLS if c["name"] == "coords")
    ev = CHUNKS["coords"]
    got, _ = orc.route_events(ev, call["rects"], call["start"], call["take"], call["cap"])
    for p in range(16):   # a 1 x 1 rect on each pair holds exactly that pair's five events
        rx, ry = call["rects"][p][:2]
        assert len(got[p]) == 5 and np.all(ev["x"][got[p]] == rx) and np.all(ev["y"][got[p]] == ry)
    neg, negrow, whole, pos, frac = got[16:]
    assert len(neg) == 20 and np.all(ev["x"][neg] < 0) and np.all(ev["y"][neg] < 0)
    assert len(negrow) == 10 and np.all(ev["y"][negrow] == -1)
    assert len(whole) == len(ev) == 80
    assert len(pos) == 20 and np.all(ev["x"][pos] >= 0) and np.all(ev["y"][pos] >= 0)
    assert len(frac) == 5 and np.all(ev["x"][frac] == 16383) and np.all(ev["y"][frac] == -16384)


def test_route_rect_shapes(orc):
    call = next(c for c in CALLS if c["name"] == "shapes")
    ev = CHUNKS["grid"]
    got, _ = orc.route_events(ev, call["rects"], call["start"], call["take"], call["cap"])
    nf = len(K.FRACTION_RECTS)
    for p, (rx, ry, rw, rh) in enumerate(K.FRACTION_RECTS):
        # the whole pixels of [rx, rx + rw): ceil(rx) .. ceil(rx + rw) - 1, on every border one in and one out
        x0, x1, y0, y1 = math.ceil(rx), math.ceil(rx + rw) - 1, math.ceil(ry), math.ceil(ry + rh) - 1
        want = [i for i in range(len(ev)) if x0 <= ev["x"][i] <= x1 and y0 <= ev["y"][i] <= y1]
        assert got[p].tolist() == want and len(want) == max(x1 - x0 + 1, 0) * max(y1 - y0 + 1, 0)
        assert ev["x"].min() < x0 and ev["x"].max() > x1 and ev["y"].min() < y0 and ev["y"].max() > y1
    assert [len(g) for g in got[:nf]] == [80, 70, 64, 81, 1, 0]
    for p in range(nf, nf + len(K.NOTHING_RECTS)):
        assert len(got[p]) == 0, p
    assert len(got[nf + len(K.NOTHING_RECTS)]) == 1600
    assert np.array_equal(got[-1], got[-2]) and np.array_equal(got[-1], got[0])   # identical rects: the same list


def test_route_second_call_continues(orc):
    first, moved = K.second_call()
    ev = CHUNKS[first["chunk"]]
    _, nxt = orc.route_events(ev, first["rects"], first["start"], first["take"], first["cap"])
    assert nxt.tolist() == [1, 63, 64, 65, 255, 256, 257, 300, 1025, 1025]
    got, nxt2 = orc.route_events(ev, moved, nxt, first["take"], first["cap"])
    want, wnxt = K.route_select(ev, moved, nxt, first["take"], first["cap"])
    assert_routed(got, nxt2, want, wnxt, "second")
    assert all(np.all(ev["x"][g] >= 106) for g in got) and len(got[0]) == 1 and len(got[-1]) == 0
    assert 0 < len(got[3]) and got[3][0] >= 65


# ---- patch images -------------------------------------------------------------------------------------------------------

def test_patch_nonsquare_images_are_not_symmetric(orc):
    for ev, rect in K.patches_nonsquare():
        img, _, _ = orc.patch_integrate(ev, rect)
        rows, cols = int(rect[3]), int(rect[2])
        assert img.shape == (rows, cols) and rows != cols
        if min(rows, cols) > 1:
            assert not np.array_equal(img, img.ravel().reshape(cols, rows).T)   # rows and columns swapped
        else:   # one pixel wide: the same words either way, but the events run along the long side only
            assert np.ptp(ev["x"]) == cols - 1 and np.ptp(ev["y"]) == rows - 1
        k = np.arange(max(rows, cols))
        extra = np.zeros((rows, cols))
        np.add.at(extra, (k % rows, k % cols), np.where(k % 2 == 0, k, -k))
        assert np.array_equal(img, 1 + extra)


def test_patch_limit_scenes_reach_the_last_pixel(orc):
    for ev, rect in K.patches_limit():
        img, _, _ = orc.patch_integrate(ev, rect)
        assert img.size in (16384, 16383) and img.shape == (int(rect[3]), int(rect[2]))
        want = np.zeros(img.shape)
        want[-1, -1] += 2
        want[0, 0] -= 1
        assert np.array_equal(img, want)    # the three events just outside leave nothing


def test_oracle_refuses_fractional_and_non_finite_sizes(orc):
    for rect, code in K.REFUSED:
        for mc in (False, True):
            # the device's limit of 16384 pixels is not the oracle's: it refuses what its image cannot hold
            want = 0 if rect[2:] == (129.0, 128.0) else -1
            assert K.orc_patch_status(rect, mc) == want, (rect, mc)
    assert sum(code == K.ERR_ARG for _, code in K.REFUSED) == 4
    assert K.orc_patch_status((0.0, 0.0, 8.0, 8.0), False) == 0 and K.orc_patch_status((0.5, 0.25, 8.0, 8.0), True) == 0


def test_patch_border_rings(orc):
    for ev, rect in K.patches_border():
        img, _, _ = orc.patch_integrate(ev, rect)
        want = np.zeros(img.shape)
        want[0, :] = want[-1, :] = want[:, 0] = want[:, -1] = 1   # all of the ring inside, none of the ring outside
        assert np.array_equal(img, want), rect
        assert (ev["sign"] == -1).sum() == 2 * (img.shape[0] + img.shape[1]) + 4


def test_patch_pileups(orc):
    (big, r0), (alt, r1), (neg, r2), (spread, r3) = K.patches_pileup()
    img, _, _ = orc.patch_integrate(big, r0)
    assert img[12, 12] == 70000 and np.count_nonzero(img) == 1
    img, _, _ = orc.patch_integrate(alt, r1)
    assert img[24, 24] == 1 and np.count_nonzero(img) == 1 and len(alt) == 70001
    img, _, _ = orc.patch_integrate(neg, r2)
    assert img[0, 0] == -1 and np.count_nonzero(img) == 1
    img, _, _ = orc.patch_integrate(spread, r3)
    assert len(spread) == 257 and np.count_nonzero(img) == 257 and np.abs(img).max() == 1


def test_patch_mc_ties_land_where_listed(orc):
    ev, rect, pre, last, mid = K.patch_mc_ties()
    img, upd = orc.patch_integrate_mc(ev, rect, pre, last, mid)
    assert upd
    want = np.zeros(img.shape)
    for (x, y, q), col in K.MC_TIES:
        assert (x + q / 4.0) % 1 in (0.25, 0.5, 0.75)
        if col is not None:
            want[y - int(rect[1]), col - int(rect[0])] += 1
    assert np.array_equal(img, want)
    assert want[:, 0].sum() == 2 and want[:, -1].sum() == 1 and want.sum() == len(K.MC_TIES) - 2


def test_patch_mc_time_tests_pass_as_listed(orc):
    for (ev, rect, pre, last, mid), (_, passes) in zip(K.patches_mc_time(), K.MC_TIME_TESTS):
        img, upd = orc.patch_integrate_mc(ev, rect, pre, last, mid)
        assert upd == passes, (pre, last, mid)
        plain, _, _ = orc.patch_integrate(ev, rect)
        assert np.array_equal(img, plain if passes else np.zeros(img.shape))   # direction zero: the plain image


def test_offset_layouts_leave_gaps():
    sizes = [15, 15, 6, 4]
    lay = K.offset_layouts(sizes)
    for name, (off, length) in lay.items():
        used = np.zeros(length, dtype=int)
        for o, s in zip(off, sizes):
            used[o:o + s] += 1
        assert used.max() == 1, name   # no overlap
        if name != "descending_dense":
            assert used[0] == 0 and used[-1] == 0 and np.count_nonzero(np.diff(used)) > 2, name
    assert lay["gaps"][0] == sorted(lay["gaps"][0]) and lay["gaps"][0][0] > 0
    for name in ("descending", "descending_dense"):
        assert lay[name][0] == sorted(lay[name][0], reverse=True)


# ---- initial field ------------------------------------------------------------------------------------------------------

W, H = K.FIELD_W, K.FIELD_H
FIELD = {name: (ts, tr) for name, ts, tr in K.field_scenes()}


def field(orc, name, use_average):
    ts, tr = FIELD[name]
    return orc.init_motion_field(W, H, ts, tr, use_average)


def test_field_geometry_leaves_the_last_workgroup_partly_idle():
    assert (W * H) % 256 not in (0,) and W * H > 256


@pytest.mark.parametrize("ts", K.LB_TIMESTAMPS)
def test_field_lower_bound(orc, ts):
    f, fixed = field(orc, "lower_bound_%d" % ts, False)
    three, two = K.LB_EXPECT[ts]
    want = []
    if three is not None:
        want.append([int(K.LB_TRAJ[three][0]), int(K.LB_TRAJ[three][1])])
    if two is not None:
        want.append([30, 10])
    assert fixed.tolist() == want
    if three is not None:
        a, b = K.LB_TRAJ[three], K.LB_TRAJ[three + 1]
        assert f[int(a[1]), int(a[0]), 0] == np.float32(1000.0 * (b[0] - a[0]) / (b[2] - a[2]))
    if not want:
        assert not f.any()


def test_field_without_fixed_points_is_zero(orc):
    for name in ("no_patches", "only_short"):
        for avg in (True, False):
            f, fixed = field(orc, name, avg)
            assert len(fixed) == 0 and not f.any()


def test_field_rounding_is_half_away_from_zero(orc):
    f, fixed = field(orc, "rounding", True)
    assert fixed.tolist() == [list(c[1]) for c in K.ROUND_CASES if c[1] is not None]
    for i, c in enumerate(K.ROUND_CASES):
        if c[1] is not None:
            assert f[c[1][1], c[1][0]].tolist() == [0.25 * (i + 1), -0.5 * (i + 1)]


def test_field_two_patches_on_one_pixel(orc):
    f, fixed = field(orc, "same_pixel", True)
    assert fixed.tolist() == [[12, 9], [30, 20], [12, 9]]
    assert f[9, 12].tolist() == [4.0, -1.0]                          # the later one stands
    assert f[0, 0].tolist() == [np.float32(2.0 / 3), np.float32(1.5 / 3)]  # the average counts all three
    f, _ = field(orc, "same_pixel", False)
    assert f[9, 11].tolist() == [4.0, -1.0]


def test_field_zero_velocity_fixed_point(orc):
    f, fixed = field(orc, "zero_velocity", True)
    avg = [np.float32(2.5 / 3), np.float32(-0.75 / 3)]
    assert fixed.tolist()[0] == [5, 5] and f[5, 5].tolist() == avg and f[0, 0].tolist() == avg   # it takes the average
    f, _ = field(orc, "zero_velocity", False)
    assert not f[5, 5].any() and not f[5, 6].any() and not f[0, 0].any()   # it stays zero, so do its neighbours
    assert f[22, 29].tolist() == [2.0, -1.0]
    for avg in (True, False):
        f, fixed = field(orc, "all_zero", avg)
        assert len(fixed) == 2 and not f.any()


def test_field_dt_zero(orc):
    f, fixed = field(orc, "dt_zero_inf", False)
    assert fixed.tolist() == [[8, 8], [30, 5]] and f[8, 8].tolist() == [math.inf, -math.inf]
    f, _ = field(orc, "dt_zero_inf", True)
    assert f[0, 0].tolist() == [math.inf, -math.inf] and f[5, 30].tolist() == [1.0, 1.0]
    f, fixed = field(orc, "dt_zero_nan", False)
    assert len(fixed) == 3 and math.isnan(f[20, 25, 0]) and f[20, 25, 1] == math.inf
    f, _ = field(orc, "dt_zero_nan", True)
    assert np.isnan(f[0, 0]).all()   # inf - inf in y, NaN in x


def test_field_nearest_tie_goes_to_the_first_in_the_list(orc):
    f, fixed = field(orc, "tie", False)
    assert fixed.tolist() == [[30, 14], [10, 14]]            # list order and raster order disagree
    assert np.all(f[:, 20, 0] == 1.0) and np.all(f[:, 20, 1] == 0.0)   # the whole equidistant column
    assert np.all(f[:, 19, 1] == 2.0) and np.all(f[:, 21, 0] == 1.0)


def test_field_many_points(orc):
    f, fixed = field(orc, "many", False)
    assert len(fixed) == 300 and fixed.min() == 0 and fixed[:, 0].max() == W - 1 and fixed[:, 1].max() == H - 1
    assert len({tuple(p) for p in fixed.tolist()}) < 300     # some pixels are fixed twice
