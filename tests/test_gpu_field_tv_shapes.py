"""The motion-field TV solve (csrc/field_tv.cpp, csrc/ebo_fieldtv.inc) at the shapes where its loop
structure changes, with the bars of tests/test_field_tv.py (derived in that file's docstring):

1. images of more than 262144 pixels, where the 1024 workgroups of the chunk-walking kernels take a
   second and third 256-pixel chunk (tall and narrow, because the oracle's banded Cholesky has band w);
2. one WIDE image of that size, where the stencil's i +- w reads cross chunk and band borders,
   against scipy's sparse direct solve (the oracle cannot take a band of 1300);
3. narrow and tiny images: coarse multigrid levels of width 2 and 1, owned sets of one column, one
   row or one pixel, the one-level (diagonal preconditioner) path, the first sizes with two levels;
4. (CPU) the launch shape restated here, which 1 and 2 rely on to prove that they are in the regime.

Measured on one CPU core: the oracle takes 2.0 s on 17 x 16383 (9 LM iterations), 9.9 s on
40 x 16383 (9 iterations) and 1.3 s for the 6 Huber iterations on 17 x 16383; lm_replay_scipy takes
14.5 s on 1300 x 210 (6 iterations).  Each oracle solve is computed once (multi_chunk_case) and
shared.  The tests print their oracle and device times (pytest -s).
"""
import time

import numpy as np
import pytest

from test_field_tv import lm_replay_scipy, make_case, run_device, ulp_report


# ------------------------------------------------------------------ the launch shape, restated
def tvf_grid(n):
    """csrc/ebo_kernels.hip tvf_grid: workgroups of the chunk-walking kernels."""
    chunks = (n + 255) // 256
    per_band = (chunks + 7) // 8
    return 8 * min(per_band, 128)


def tvf_chunks(n, block, grid):
    """csrc/ebo_fieldtv.inc tvf_chunks: the chunks workgroup `block` of `grid` walks, in order."""
    n_chunks = (n + 255) >> 8
    per_band = (n_chunks + 7) >> 3
    band, local = block & 7, block >> 3
    step = grid >> 3
    first = band * per_band + local
    end = min((band + 1) * per_band, n_chunks)
    return np.arange(first, max(first, end), step, dtype=np.int64)


def chunk_visits(n):
    """(times each chunk is visited, the visit number at which its workgroup reaches it, grid)."""
    grid = tvf_grid(n)
    n_chunks = (n + 255) // 256
    count = np.zeros(n_chunks, np.int64)
    visit = np.full(n_chunks, -1, np.int64)
    for b in range(grid):
        c = tvf_chunks(n, b, grid)
        assert len(c) == 0 or (c[0] >= 0 and c[-1] < n_chunks), (n, b)
        np.add.at(count, c, 1)
        visit[c] = np.arange(len(c))
    return count, visit, grid


def tvf_mg_dims(w, h):
    """csrc/ebo_kernels.hip tvf_mg_dims: halve both sides until a level has at most 256 nodes."""
    lv = [(w, h)]
    while lv[-1][0] * lv[-1][1] > 256 and len(lv) < 12:
        lv.append(((lv[-1][0] + 1) // 2, (lv[-1][1] + 1) // 2))
    return lv


@pytest.mark.parametrize("n", [1, 255, 256, 257, 2048, 2049, 262144, 262145, 278511, 655320, 921600,
                               16383 * 16383])
def test_restated_launch_shape_visits_every_chunk_once(n):
    """Every chunk 0 .. ceil(n/256)-1 exactly once over all (band, local); a grid <= 1024 that is a
    multiple of 8.  At the largest n the last pixel index is 2^28: the kernels' int arithmetic
    ((c << 8) + lane, band * perBand + local) stays below 2^31."""
    count, visit, grid = chunk_visits(n)
    assert grid <= 1024 and grid % 8 == 0 and grid >= 8
    assert np.all(count == 1), (n, np.flatnonzero(count != 1)[:8])
    assert np.all(visit >= 0)
    assert ((len(count) - 1) << 8) + 255 < 2 ** 31
    # more than one chunk per workgroup exactly above 1024 chunks
    assert (visit.max() >= 1) == (n > 262144)


# ------------------------------------------------------------------ building cases
def traj_through(x, y, k):
    """A track whose sample at t = 31000 (the one lower_bound(25000) finds) is exactly (x, y)."""
    v = 0.7e-3 * np.array([np.cos(1.0 + 2.3 * k), np.sin(1.0 + 2.3 * k)])
    return [(x + v[0] * (t - 30000), y + v[1] * (t - 30000), 1000 + t) for t in range(0, 60000, 10000)]


def random_tracks(w, h, n, seed):
    """make_case's tracks for a side below 5, where its margin of 2 pixels leaves no room: the
    sample at t = 31000 is uniform over the whole image, the last row and column included."""
    rng = np.random.default_rng(seed)
    traj = []
    for _ in range(n):
        v = rng.uniform(-1, 1, 2) * 1e-3  # px per us
        x0, y0 = rng.uniform(0, w - 1) - v[0] * 30000, rng.uniform(0, h - 1) - v[1] * 30000
        traj.append([(x0 + v[0] * t, y0 + v[1] * t, 1000 + t) for t in range(0, 60000, 10000)])
    return traj


def case_with_points(orc, w, h, n_random, seed, points, use_average=True):
    """Random tracks (make_case's where the image has room for them) followed by one track through
    each of `points`."""
    if n_random == 0:
        traj = []
    elif min(w, h) >= 5:
        traj = make_case(orc, w, h, n_random, seed, use_average=use_average)[0]
    else:
        traj = random_tracks(w, h, n_random, seed)
    traj = traj + [traj_through(x, y, k) for k, (x, y) in enumerate(points)]
    field, fixed = orc.init_motion_field(w, h, 25000, traj, use_average=use_average)
    return traj, field, fixed


def l1_opts(ebo, orc, iters):
    opts = ebo.default_solver()
    opts.use_nonmonotonic = 0
    opts.function_tolerance, opts.gradient_tolerance, opts.parameter_tolerance = 1e-6, 1e-10, 1e-8
    opts.max_num_iterations = iters  # IRLS on |.|: compare a fixed number of iterations
    oo = orc.default_solver(use_nonmonotonic=0, function_tolerance=1e-6, gradient_tolerance=1e-10,
                            parameter_tolerance=1e-8, max_num_iterations=iters)
    return opts, oo


def assert_matches_oracle(field, fixed, out, s, cg, field_o, fixed_o, ref, so):
    """The bars of test_device_field_tv_matches_oracle."""
    assert np.array_equal(field, field_o) and np.array_equal(fixed, fixed_o)
    assert (s.iterations, s.termination) == (so.iterations, so.termination)
    print("iterations %d cg %d initial %.17g final %.17g oracle initial %.17g final %.17g"
          % (s.iterations, cg, s.initial_cost, s.final_cost, so.initial_cost, so.final_cost))
    assert s.initial_cost == pytest.approx(so.initial_cost, rel=1e-12)
    assert s.final_cost == pytest.approx(so.final_cost, rel=1e-10)
    diff, frac, ok = ulp_report(out, ref)
    print("field: max |diff| %.3e, fraction differing %.3e" % (diff.max(), frac))
    assert ok and frac <= 1e-3, (diff.max(), frac)
    assert cg > 0


# ------------------------------------------------------------------ 1. several chunks per workgroup
# (w, h, chunks, chunks per band, most chunks one workgroup walks)
MULTI_CHUNK = [(17, 16383, 1088, 136, 2), (40, 16383, 2560, 320, 3)]
MULTI_CHUNK_RANDOM, MULTI_CHUNK_SEED = 37, 21


def multi_chunk_points(w, h):
    """Three placed tracks: two in chunks that are a workgroup's SECOND visit (one in the first
    such chunk of band 0, one in the last such chunk of the ragged last band), one in the last row."""
    n = w * h
    count, visit, grid = chunk_visits(n)
    second = np.flatnonzero(visit == 1)
    pts = []
    for c in (second[0], second[-1]):
        i = int(c) * 256 + 100
        pts.append((i % w, i // w))
    pts.append((w // 2, h - 1))
    return pts, visit, grid


_multi_chunk_cache = {}


def multi_chunk_case(orc, w, h, chunks, per_band, most):
    """The case and its oracle solve, computed once for the tests below (never modified)."""
    if (w, h) not in _multi_chunk_cache:
        pts, visit, grid = multi_chunk_points(w, h)
        traj, field_o, fixed_o = case_with_points(orc, w, h, MULTI_CHUNK_RANDOM, MULTI_CHUNK_SEED, pts)
        t0 = time.perf_counter()
        ref, so, rc = orc.interpolate_motion_field(field_o, fixed_o)
        t_oracle = time.perf_counter() - t0
        assert rc == 0
        print("oracle %dx%d: %.2f s, %d iterations" % (w, h, t_oracle, so.iterations))
        _multi_chunk_cache[(w, h)] = dict(
            w=w, h=h, chunks=chunks, per_band=per_band, most=most, pts=pts, visit=visit, grid=grid, traj=traj,
            field_o=field_o, fixed_o=fixed_o, ref=ref, so=so)
    return _multi_chunk_cache[(w, h)]


def assert_multi_chunk_regime(m):
    """From the restated launch shape: the case is where it claims to be."""
    w, h, visit = m["w"], m["h"], m["visit"]
    assert len(visit) == m["chunks"] and (m["chunks"] + 7) // 8 == m["per_band"]
    assert m["grid"] == 1024
    assert visit.max() + 1 == m["most"] >= 2
    # some workgroups take one chunk fewer than others, and the last band is ragged
    per_wg = [len(tvf_chunks(w * h, b, 1024)) for b in range(1024)]
    assert min(per_wg) == m["most"] - 1 and max(per_wg) == m["most"]
    assert m["chunks"] % m["per_band"] != 0 or (w * h) % 256 != 0
    fixed = {(int(x), int(y)) for x, y in m["fixed_o"]}
    assert len(m["fixed_o"]) == MULTI_CHUNK_RANDOM + 3
    for x, y in m["pts"]:
        assert (x, y) in fixed
    (x0, y0), (x1, y1), (x2, y2) = m["pts"]
    assert visit[(y0 * w + x0) >> 8] == 1 and visit[(y1 * w + x1) >> 8] == 1
    assert ((y0 * w + x0) >> 8) // m["per_band"] == 0 and ((y1 * w + x1) >> 8) // m["per_band"] == 7
    assert y2 == h - 1 and x2 < w - 1


@pytest.mark.gpu
@pytest.mark.parametrize("shape", MULTI_CHUNK, ids=lambda p: "%dx%d" % p[:2])
def test_device_field_tv_multi_chunk_matches_oracle(ebo, orc, shape):
    """More than 1024 chunks: workgroups walk 1-2 (17 x 16383) and 2-3 (40 x 16383) chunks, the
    partial sums come from all 1024 workgroups, the level-0 k_mg_up walks chunks too."""
    m = multi_chunk_case(orc, *shape)
    assert_multi_chunk_regime(m)
    t0 = time.perf_counter()
    field, fixed, out, s, cg = run_device(ebo, orc, m["w"], m["h"], m["traj"], True, False)
    print("device %dx%d: %.2f s" % (m["w"], m["h"], time.perf_counter() - t0))
    assert_matches_oracle(field, fixed, out, s, cg, m["field_o"], m["fixed_o"], m["ref"], m["so"])
    for x, y in m["fixed_o"]:
        assert np.array_equal(out[y, x], m["field_o"][y, x])


@pytest.mark.gpu
def test_device_field_tv_multi_chunk_l1_matches_oracle(ebo, orc):
    """The Huber loss over several chunks per workgroup (per-edge weights written in one chunk and
    read from the next), 6 iterations as test_device_field_tv_l1_matches_oracle, its bars."""
    m = multi_chunk_case(orc, *MULTI_CHUNK[0])  # one of the two sizes, as the oracle solves it again
    assert_multi_chunk_regime(m)
    opts, oo = l1_opts(ebo, orc, 6)
    t0 = time.perf_counter()
    ref, so, rc = orc.interpolate_motion_field(m["field_o"], m["fixed_o"], use_l1=True, opts=oo)
    t1 = time.perf_counter()
    _, _, out, s, _ = run_device(ebo, orc, m["w"], m["h"], m["traj"], True, True, opts)
    print("L1 %dx%d: oracle %.2f s, device %.2f s" % (m["w"], m["h"], t1 - t0, time.perf_counter() - t1))
    assert rc == 0 and s.iterations == so.iterations
    print("L1 final %.17g oracle %.17g" % (s.final_cost, so.final_cost))
    assert s.final_cost == pytest.approx(so.final_cost, rel=1e-8)
    assert np.abs(out.astype(np.float64) - ref).max() < 1e-5


# ------------------------------------------------------------------ 2. wide, several chunks
WIDE = (1300, 210)


@pytest.mark.gpu
def test_device_field_tv_wide_multi_chunk(ebo_ab, orc, monkeypatch):
    """1300 x 210 = 273000 pixels, 1067 chunks, 134 per band: a row is five chunks, so the stencil's
    i +- w reads land in other chunks, other workgroups' second visits and (at band borders) other
    bands.  The multigrid path, the diagonal preconditioner and scipy's sparse direct solve agree."""
    ebo = ebo_ab
    w, h = WIDE
    n = w * h
    count, visit, grid = chunk_visits(n)
    assert grid == 1024 and visit.max() + 1 >= 2 and len(count) == 1067
    i = int(np.flatnonzero(visit == 1)[0]) * 256 + 100
    pts = [(i % w, i // w), (w // 2, h - 1), (w - 1, h // 2)]
    traj, field_o, fixed_o = case_with_points(orc, w, h, 37, 22, pts)
    assert len(fixed_o) == 40
    t0 = time.perf_counter()
    field, fixed, out_mg, s_mg, cg_mg = run_device(ebo, orc, w, h, traj, True, False)
    t1 = time.perf_counter()
    monkeypatch.setenv("EBO_TVF_PRECOND", "jacobi")
    _, _, out_j, s_j, cg_j = run_device(ebo, orc, w, h, traj, True, False)
    t2 = time.perf_counter()
    monkeypatch.delenv("EBO_TVF_PRECOND")
    assert np.array_equal(field, field_o) and np.array_equal(fixed, fixed_o)
    assert cg_mg > 0 and cg_j > 0
    assert (s_mg.iterations, s_mg.termination) == (s_j.iterations, s_j.termination)
    assert s_mg.final_cost == pytest.approx(s_j.final_cost, rel=1e-10)
    diff, frac, ok = ulp_report(out_mg, out_j)
    print("multigrid %.2f s (%d cg), diagonal %.2f s (%d cg): max |diff| %.3e, differing %.3e"
          % (t1 - t0, cg_mg, t2 - t1, cg_j, diff.max(), frac))
    assert ok and frac <= 1e-3
    ref, it, c = lm_replay_scipy(field_o, fixed_o)
    print("scipy replay %.2f s, %d iterations" % (time.perf_counter() - t2, it))
    for out, s in ((out_mg, s_mg), (out_j, s_j)):
        assert s.iterations == it and s.termination == 0
        assert s.final_cost == pytest.approx(c, rel=1e-10)
        diff, frac, ok = ulp_report(out, ref)
        print("against scipy: max |diff| %.3e, differing %.3e" % (diff.max(), frac))
        assert ok and frac <= 1e-3, (diff.max(), frac)


# ------------------------------------------------------------------ 3. narrow and tiny
def corner_points(w, h):
    """Fixed points in the first and last owned row and column (owned: px <= w-2, py <= h-2)."""
    return sorted({(0, h - 2), (w - 2, 0)})


# (w, h, random tracks, seed, placed points, use_average, the multigrid levels)
SMALL = [
    (3, 400, 3, 1, "corners", True, [(3, 400), (2, 200), (1, 100)]),
    (400, 3, 3, 2, "corners", False, [(400, 3), (200, 2), (100, 1)]),
    (2, 150, 3, 3, "corners", True, [(2, 150), (1, 75)]),
    (150, 2, 3, 4, "corners", True, [(150, 2), (75, 1)]),
    (5, 300, 4, 5, "corners", False, [(5, 300), (3, 150), (2, 75)]),
    (16, 16, 3, 6, "corners", True, [(16, 16)]),
    (17, 16, 3, 7, "corners", True, [(17, 16), (9, 8)]),
    (5, 5, 2, 8, "corners", True, [(5, 5)]),
    (2, 2, 2, 8, "corners", True, [(2, 2)]),
    (3, 2, 2, 10, "corners", False, [(3, 2)]),
    # all but three pixels fixed: (5, 5) is in no residual block, (2, 2)-(3, 2) is the one free edge
    (6, 6, 0, 0, [(x, y) for y in range(6) for x in range(6) if (x, y) not in ((5, 5), (2, 2), (3, 2))], True,
     [(6, 6)]),
]
SMALL_IDS = ["%dx%d" % c[:2] for c in SMALL]


def small_case(orc, w, h, n_random, seed, points, avg):
    pts = corner_points(w, h) if points == "corners" else points
    traj, field, fixed = case_with_points(orc, w, h, n_random, seed, pts, use_average=avg)
    inside = {(int(x), int(y)) for x, y in fixed}
    assert len(fixed) == n_random + len(pts), "a random track left the image: choose another seed"
    assert len(inside) >= 2 and (w - 1, h - 1) not in inside
    for p in pts:
        assert p in inside
    return traj, field, fixed, pts


@pytest.mark.parametrize("w,h,n_random,seed,points,avg,levels", SMALL, ids=SMALL_IDS)
def test_oracle_field_tv_small_shapes_match_independent_lm_replay(orc, w, h, n_random, seed, points, avg, levels):
    """The cases of the device test below are what they claim (levels, fixed points inside the
    image, first/last owned row and column), and the oracle is right on them: the independent
    scipy replay gives the same iteration count, cost and field."""
    assert tvf_mg_dims(w, h) == levels
    _, field, fixed, pts = small_case(orc, w, h, n_random, seed, points, avg)
    if points == "corners":
        xs, ys = {p[0] for p in pts}, {p[1] for p in pts}
        assert {0, w - 2} <= xs and {0, h - 2} <= ys
    out, s, rc = orc.interpolate_motion_field(field, fixed)
    assert rc == 0 and s.termination == 0 and s.iterations >= 1
    ref, it, c = lm_replay_scipy(field, fixed)
    assert s.iterations == it
    assert s.final_cost == pytest.approx(c, rel=1e-10)
    diff, frac, ok = ulp_report(out, ref)
    assert ok and frac <= 1e-3, (diff.max(), frac)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,n_random,seed,points,avg,levels", SMALL, ids=SMALL_IDS)
def test_device_field_tv_small_shapes_match_oracle(ebo, orc, w, h, n_random, seed, points, avg, levels):
    """Coarse levels of width 2 and 1 (3 x 400 ends at 1 x 100: no horizontal edge, every node in
    the last column), owned sets of one column (2 x 150), one row (150 x 2) and one pixel (2 x 2),
    one level (<= 256 pixels: the diagonal preconditioner) and the first sizes with two (257, 272)."""
    assert tvf_mg_dims(w, h) == levels
    traj, field_o, fixed_o, _ = small_case(orc, w, h, n_random, seed, points, avg)
    field, fixed, out, s, cg = run_device(ebo, orc, w, h, traj, avg, False)
    ref, so, rc = orc.interpolate_motion_field(field_o, fixed_o)
    assert rc == 0
    assert_matches_oracle(field, fixed, out, s, cg, field_o, fixed_o, ref, so)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h,seed,avg", [(2, 2, 1, True), (3, 2, 2, False)])
def test_device_field_tv_nothing_to_solve(ebo, orc, w, h, seed, avg):
    """2 x 2 with its three usable pixels fixed: no free parameter, every residual block between
    two constants.  3 x 2 with the first row fixed and the nearest-neighbour fill: the two free
    pixels equal the fixed pixel above them, cost and gradient are zero.  The oracle stops before
    its first iteration (gradient tolerance); so does the device, without a linear solve."""
    traj, field_o, fixed_o, _ = small_case(orc, w, h, 2, seed, "corners", avg)
    ref, so, rc = orc.interpolate_motion_field(field_o, fixed_o)
    assert rc == 0 and (so.iterations, so.termination) == (0, 0)
    assert so.initial_cost == 0.0 and so.final_cost == 0.0 and np.array_equal(ref, field_o)
    field, fixed, out, s, cg = run_device(ebo, orc, w, h, traj, avg, False)
    assert np.array_equal(field, field_o) and np.array_equal(fixed, fixed_o)
    assert (s.iterations, s.termination) == (0, 0) and cg == 0
    assert s.initial_cost == 0.0 and s.final_cost == 0.0
    assert np.array_equal(out, field_o)


@pytest.mark.gpu
@pytest.mark.parametrize("w,h", [(1, 300), (300, 1)])
def test_device_field_tv_one_pixel_wide_is_refused_like_the_oracle(ebo, orc, w, h):
    """A 1 x h or w x 1 image owns no pixel (px <= w-2, py <= h-2 is empty): the reference's
    problem has no residual block and no parameter block, so marking a tracked point constant
    (feature_detector.cpp:208) is Ceres' abort, as it is for the last pixel of a larger image.
    The oracle refuses the size before it looks at the field: rc -1, summary zero (iterations 0,
    termination 0), field unchanged.  The device refuses it the same way, with EBO_ERR_ARG: no
    fault, no solver or numeric error, and the context works afterwards."""
    pts = [(0, 3), (0, 200)] if w == 1 else [(3, 0), (200, 0)]
    traj, field_o, fixed_o = case_with_points(orc, w, h, 0, 0, pts)
    assert len(fixed_o) == 2 and field_o.any()
    out_o, so, rc = orc.interpolate_motion_field(field_o, fixed_o)
    assert rc == -1 and (so.iterations, so.termination) == (0, 0) and np.array_equal(out_o, field_o)
    p = ebo.default_params()
    p.image_w, p.image_h, p.patch_w, p.patch_h = w, h, min(20, w), min(20, h)
    c = ebo.Context(p)
    try:
        field, fixed = c.init_motion_field(25000, traj)
        assert np.array_equal(field, field_o) and np.array_equal(fixed, fixed_o)
        with pytest.raises(ebo.EboError) as e:
            c.interpolate_motion_field()
        assert e.value.code == ebo.ERR_ARG
        field2, fixed2 = c.init_motion_field(25000, traj)
        assert np.array_equal(field2, field_o) and np.array_equal(fixed2, fixed_o)
    finally:
        c.close()
