"""The tracker layer (csrc/ebo_optimizer.inc, csrc/ebo_tracker.cpp) at its launch shapes, image borders and
map edges, on the inputs of tests/tracker_cases.py, which tests/test_tracker_cases_cpu.py admits on the CPU.  Seven
kernels: k_optimizer_eval, k_optimizer_cost_map, k_optimizer_solve, k_optimizer_normalize, k_optimizer_interleave,
k_estimate_num_events, k_patch_warp_image.  The bars are those of tests/test_optimizer.py:
  functor residuals 1e-12 max|r| + 1e-15, Jacobians 1e-10 max|J| + 1e-14, cost maps 1e-12 max with equal zero patterns;
  solve at <= 10 iterations: integers equal, initial cost rel 1e-11, final cost rel 1e-7 / abs 1e-13, parameters 1e-5;
  estimates: equal integers; warp images: test_warp_image.py's atol of 4e-15, scaled by the largest gradient.
"""
import numpy as np
import pytest

import tracker_cases as TC

pytestmark = pytest.mark.gpu

# k_optimizer_solve runs with 128 lanes from 512 patches up and with 256 below (launch_optimizer_solve).  First run
# (2026-10-20, MI355X, the 512 problems of tracker_cases.solve_problems and their first 511): per field, do the 511
# patches the two calls share have the same bits?
#   integers (iterations, termination, evaluation counts): yes, equal on all 511.
#   poses, flow directions, initial and final costs: no.  263 of the 511 poses differ; the largest differences are
#   7.6e-13 (pose), 3.4e-13 (flow direction), 1.1e-16 (initial cost: one ulp) and 1.1e-14 (final cost).  With 128 lanes
#   a lane sums other pixels in another order, so the sums of an evaluation differ in their last bits and the solve
#   carries that along; both calls agree with the oracle to the bars above.  test_lane_count_is_the_only_difference_
#   between_511_and_512 shows that the lane count is all there is to it ("shapes and edges").
# A test that finds otherwise, in either direction, fails: record the new finding here.  None = nothing recorded, print only.
SAME_BITS_511_512 = {"poses": False, "flow directions": False, "integers": True, "initial cost": False, "final cost": False}

# test_warp_image.py: atol 4e-15 on a scene whose largest gradient is 6.54
WARP_ATOL = 4e-15 * float(np.abs(TC.map_grid()).max()) / 6.54


def _ctx(ebo, grad):
    h, w = grad.shape[:2]
    c = ebo.Context(image_w=w, image_h=h, patch_w=min(20, w), patch_h=min(20, h))
    c.optimizer_set_grad(grad[..., 0].copy(), grad[..., 1].copy())
    return c


def _args(orc, items):
    return ([it["rect"] for it in items], [orc.normalize_nabla(it["raw"]) for it in items],
            [it["pose"] for it in items], [it["flow"] for it in items])


def _check_functor(orc, grad, items, args, res, res_v, jp, jf):
    for i, it in enumerate(items):
        ro, jpo, jfo = orc.optimizer_cost(grad, it["rect"], args[1][i], it["pose"], it["flow"])
        rv, _, _ = orc.optimizer_cost(grad, it["rect"], args[1][i], it["pose"], it["flow"], want_jac=False)
        assert len(res[i]) == len(ro) == int(it["rect"][2]) * int(it["rect"][3])
        assert np.abs(res[i] - ro).max() <= 1e-12 * np.abs(ro).max() + 1e-15, it["name"]
        assert np.abs(res_v[i] - rv).max() <= 1e-12 * np.abs(rv).max() + 1e-15, it["name"]
        assert np.abs(jp[i] - jpo).max() <= 1e-10 * np.abs(jpo).max() + 1e-14, it["name"]
        assert np.abs(jf[i] - jfo).max() <= 1e-10 * np.abs(jfo).max() + 1e-14, it["name"]


def _check_cost_maps(orc, grad, items, args, got, mw, mh):
    for i, it in enumerate(items):
        want = orc.optimizer_cost_map(grad, it["rect"], args[1][i], it["pose"], it["flow"], mw, mh)
        assert np.abs(got[i] - want).max() <= 1e-12 * want.max(), (it["name"], mw, mh)
        assert np.array_equal(got[i] == 0.0, want == 0.0), (it["name"], mw, mh)


def _functor_sets():
    sets = [(TC.gradient_grid(), TC.border_items() + TC.shape_items())]
    return sets + [(TC.tiny_grid(w, h), TC.tiny_items(w, h)) for w, h in TC.TINY_IMAGES]


# ---- 1. the functor at the borders and on tiny images ------------------------------------------------------------
@pytest.mark.parametrize("k", range(1 + len(TC.TINY_IMAGES)), ids=["64x48"] + ["%dx%d" % s for s in TC.TINY_IMAGES])
def test_functor_at_the_borders_and_on_tiny_images(ebo, orc, k):
    """optimizer_eval with and without the Jacobian, and optimizer_cost_map at a 3x3 and a 4x2 map, on the border samples
    and one patch of every shape (64x48) and on images no larger than the 4x4 neighbourhood, one call per image."""
    grad, items = _functor_sets()[k]
    args = _args(orc, items)
    zero = [np.zeros_like(a) for a in args[1]]
    with _ctx(ebo, grad) as c:
        res, jp, jf = c.optimizer_eval(*args)
        res_v, _, _ = c.optimizer_eval(*args, want_jac=False)
        pred, _, _ = c.optimizer_eval(args[0], zero, args[2], args[3], want_jac=False)
        maps = {(mw, mh): c.optimizer_cost_map(*args, mw, mh) for mw, mh in ((3, 3), (4, 2))}
    _check_functor(orc, grad, items, args, res, res_v, jp, jf)
    for (mw, mh), got in maps.items():
        _check_cost_maps(orc, grad, items, args, got, mw, mh)
    # the inside test: with a zero nabla a residual is non-zero exactly where the sample is inside the image
    stated = 0
    for i, it in enumerate(items):
        po, _, _ = orc.optimizer_cost(grad, it["rect"], zero[i], it["pose"], it["flow"], want_jac=False)
        assert np.array_equal(pred[i] != 0.0, po != 0.0), it["name"]
        if "inside" in it:
            assert int((po != 0.0).sum()) == it["inside"] == int((pred[i] != 0.0).sum()), it["name"]
            stated += 1
    assert stated == (len(TC.border_items()) if k == 0 else 0)


# ---- 2. large LDS ------------------------------------------------------------------------------------------------
def _solve_item(orc, shape):
    """the first kept solve problem of this shape and its oracle solve"""
    kept = TC.kept_problems(orc)
    i = next(i for i, it in enumerate(kept) if it["shape"] == shape)
    return kept[i], TC.oracle_solves(orc)[i]


def _solve_args(items):
    return ([it["rect"] for it in items], [it["nabla"] for it in items], [it["start"][0] for it in items],
            [it["start"][1] for it in items])


def _summary_rows(sums):
    return np.array([(s.iterations, s.termination, s.num_evals_cost, s.num_evals_jac, s.initial_cost, s.final_cost)
                     for s in sums])


def _solve_bits(got):
    """(poses, flows, summaries) of a device call -> three arrays: poses [n][4], flows [n], summary rows [n][6]"""
    return np.asarray(got[0]).copy(), np.asarray(got[1]).copy(), _summary_rows(got[2])


def _check_solves(bits, want, ids=None):
    """bits = _solve_bits of a device call, want = oracle_solves entries"""
    poses, fds, rows = bits
    assert len(rows) == len(want)
    for i, (po, fo, so) in enumerate(want):
        tag = ids[i] if ids else i
        assert tuple(int(v) for v in rows[i, :4]) == so[:4], (tag, so)
        assert rows[i, 4] == pytest.approx(so[4], rel=1e-11), tag
        assert rows[i, 5] == pytest.approx(so[5], rel=1e-7, abs=1e-13), tag
        d = max(np.abs(poses[i] - po).max(), abs(fds[i] - fo))
        assert d < 1e-5, (tag, d)


BIG_CALLS = [[s] for s in TC.BIG_SHAPES] + [TC.BIG_SHAPES + [(3, 3)]]


@pytest.mark.parametrize("shapes", BIG_CALLS, ids=["+".join("%dx%d" % s for s in call) for call in BIG_CALLS])
def test_large_lds(ebo, orc, shapes):
    """40x33 (64 KB, the largest without allow_big_lds), 37x37 (the first above), 54x55 and 60x50 (the admitted 3000
    pixels, 145 KB: one workgroup per CU) through all three entries, each alone and all in one call with a 3x3."""
    grad = TC.gradient_grid()
    items = [TC.big_item(*s) for s in shapes]
    args = _args(orc, items)
    solves = [_solve_item(orc, s) for s in shapes]
    with _ctx(ebo, grad) as c:
        res, jp, jf = c.optimizer_eval(*args)
        res_v, _, _ = c.optimizer_eval(*args, want_jac=False)
        cm = c.optimizer_cost_map(*args, 3, 3)
        got = c.optimizer_solve(*_solve_args([p for p, _ in solves]))
    _check_functor(orc, grad, items, args, res, res_v, jp, jf)
    _check_cost_maps(orc, grad, items, args, cm, 3, 3)
    _check_solves(_solve_bits(got), [w for _, w in solves], ids=shapes)
    assert max(s.iterations for s in got[2]) >= 2


def test_more_than_3000_pixels_is_refused(ebo, orc):
    """55x55: EBO_ERR_UNSUPPORTED from all three entries, alone and in a call with an admitted patch; the context goes on
    working."""
    grad = TC.gradient_grid()
    bad, ok = TC.refused_item(), TC.small_item()
    a_ok = _args(orc, [ok])
    with _ctx(ebo, grad) as c:
        for items in ([bad], [ok, bad]):
            args = _args(orc, items)
            for call in (lambda: c.optimizer_eval(*args), lambda: c.optimizer_eval(*args, want_jac=False),
                         lambda: c.optimizer_cost_map(*args, 3, 3), lambda: c.optimizer_solve(*args)):
                with pytest.raises(ebo.EboError) as ei:
                    call()
                assert ei.value.code == ebo.ERR_UNSUPPORTED
        res, jp, jf = c.optimizer_eval(*a_ok)
        res_v, _, _ = c.optimizer_eval(*a_ok, want_jac=False)
        cm = c.optimizer_cost_map(*a_ok, 3, 3)
        p, w = _solve_item(orc, (3, 3))
        got = c.optimizer_solve(*_solve_args([p]))
    _check_functor(orc, grad, [ok], a_ok, res, res_v, jp, jf)
    _check_cost_maps(orc, grad, [ok], a_ok, cm, 3, 3)
    _check_solves(_solve_bits(got), [w])


# ---- 3. alone equals in a batch ----------------------------------------------------------------------------------
def _same(a, b):
    return all(np.array_equal(x, y, equal_nan=True) for x, y in zip(a, b))


def test_optimizer_alone_equals_in_a_batch(ebo, orc):
    """A mixed call of one patch of every admitted shape -- the workgroups' LDS is sized by the call's largest patch --
    against each patch alone, the call reversed, and a second run: the same bits from optimizer_eval (both paths),
    optimizer_cost_map and optimizer_solve (parameters and summaries)."""
    grad = TC.gradient_grid()
    items = TC.shape_items()
    args = _args(orc, items)
    problems = TC.kept_problems(orc)[:len(TC.SHAPES)]
    assert {p["shape"] for p in problems} == set(TC.SHAPES)
    sargs = _solve_args(problems)
    n = len(items)

    def run(c, idx):
        a = [[col[i] for i in idx] for col in args]
        s = [[col[i] for i in idx] for col in sargs]
        res, jp, jf = c.optimizer_eval(*a)
        res_v, _, _ = c.optimizer_eval(*a, want_jac=False)
        cm = c.optimizer_cost_map(*a, 3, 3)
        sp, sf, ss = _solve_bits(c.optimizer_solve(*s))
        return [(res[k], jp[k], jf[k], res_v[k], cm[k], sp[k], sf[k], ss[k]) for k in range(len(idx))]

    with _ctx(ebo, grad) as c:
        whole = run(c, list(range(n)))
        again = run(c, list(range(n)))
        rev = run(c, list(range(n))[::-1])[::-1]
        alone = [run(c, [i])[0] for i in range(n)]
    for i in range(n):
        assert _same(whole[i], again[i]), ("second run", items[i]["name"])
        assert _same(whole[i], rev[i]), ("reversed", items[i]["name"])
        assert _same(whole[i], alone[i]), ("alone", items[i]["name"])
    _check_solves(tuple(np.array([w[k] for w in whole]) for k in (5, 6, 7)), TC.oracle_solves(orc)[:n])


def test_maps_alone_equal_in_a_batch(ebo, orc):
    """estimate_num_events and patch_warp_image on every map case: the same bits in one call, in a second run, in the
    reversed call and alone."""
    grad = TC.map_grid()
    cases = TC.map_cases()
    rects, poses, flows = ([c[k] for c in cases] for k in range(3))
    n = len(cases)
    with _ctx(ebo, grad) as c:
        est = c.estimate_num_events(rects, poses, flows)
        warp = c.patch_warp_image(rects, poses, flows)
        assert np.array_equal(est, c.estimate_num_events(rects, poses, flows))
        assert np.array_equal(est, c.estimate_num_events(rects[::-1], poses[::-1], flows[::-1])[::-1])
        warp_rev = c.patch_warp_image(rects[::-1], poses[::-1], flows[::-1])[::-1]
        warp_again = c.patch_warp_image(rects, poses, flows)
        for i in range(n):
            assert c.estimate_num_events([rects[i]], [poses[i]], [flows[i]])[0] == est[i], i
            one = c.patch_warp_image([rects[i]], [poses[i]], [flows[i]])[0]
            for other in (one, warp_rev[i], warp_again[i]):
                assert (other is None) == (warp[i] is None), i
                assert warp[i] is None or np.array_equal(other, warp[i]), i


# ---- 4. the solve at every lane count ----------------------------------------------------------------------------
@pytest.mark.parametrize("lanes", [64, 128, 192, 256])
def test_solve_at_every_lane_count(ebo_ab, orc, monkeypatch, lanes):
    """The mixed call of every admitted shape with EBO_OPT_BLOCK lanes per workgroup (the A/B build reads it): against the
    oracle, and each patch alone gives the bits it has in the call."""
    grad = TC.gradient_grid()
    problems = TC.kept_problems(orc)[:len(TC.SHAPES)]
    monkeypatch.setenv("EBO_OPT_BLOCK", str(lanes))
    with _ctx(ebo_ab, grad) as c:
        got = c.optimizer_solve(*_solve_args(problems))
        whole = _solve_bits(got)
        alone = [_solve_bits(c.optimizer_solve(*_solve_args([p]))) for p in problems]
    monkeypatch.delenv("EBO_OPT_BLOCK")
    _check_solves(whole, TC.oracle_solves(orc)[:len(problems)], ids=[p["shape"] for p in problems])
    for i, a in enumerate(alone):
        assert _same([w[i] for w in whole], [x[0] for x in a]), (lanes, problems[i]["shape"])


# ---- 5. the shipped 128-lane launch ------------------------------------------------------------------------------
FIELDS = ("poses", "flow directions", "integers", "initial cost", "final cost")


def _fields(bits):
    p, f, s = bits
    return dict(zip(FIELDS, (p, f, s[:, :4], s[:, 4], s[:, 5])))


@pytest.fixture(scope="module")
def shipped_solves(ebo, orc):
    """The kept problems (512 less the dropped ones) in one call of the shipped library -- 128 lanes -- and all but the
    last in a second call -- 256 lanes."""
    problems = TC.kept_problems(orc)
    assert len(problems) >= 512 - 10 and len(TC.DROPPED) <= 10
    with _ctx(ebo, TC.gradient_grid()) as c:
        full = c.optimizer_solve(*_solve_args(problems))
        less = c.optimizer_solve(*_solve_args(problems[:-1]))
    return problems, full, less


def test_the_128_lane_launch_matches_the_oracle(shipped_solves, orc):
    problems, full, less = shipped_solves
    want = TC.oracle_solves(orc)
    assert len(problems) == 512 and len(TC.DROPPED) == 0   # at the threshold of launch_optimizer_solve itself
    _check_solves(_solve_bits(full), want, ids=[p["shape"] for p in problems])
    _check_solves(_solve_bits(less), want[:-1], ids=[p["shape"] for p in problems])
    ends = {(s.termination, s.iterations == 10) for s in full[2]}
    assert (0, False) in ends and (1, True) in ends


def test_511_against_512_patches(shipped_solves, orc):
    """The same patch in a call of 511 (256 lanes) and of 512 (128 lanes: other pixels per lane, another order of the
    sums).  What the first run found is SAME_BITS_511_512; asserted from then on: the same bits where they were the same,
    equal integers and parameters within 1e-5 (both calls agree with the oracle to that) where not."""
    problems, full, less = shipped_solves
    a, b = _fields(_solve_bits(full)), _fields(_solve_bits(less))
    found = {k: bool(np.array_equal(a[k][:-1], b[k])) for k in FIELDS}
    worst = {k: float(np.abs(a[k][:-1] - b[k]).max()) for k in FIELDS}
    differ = int(np.any(a["poses"][:-1] != b["poses"], axis=1).sum())
    print("511 / 512 patches: same bits per field %s; largest difference %s; %d of 511 poses differ" % (found, worst, differ))
    assert np.array_equal(a["integers"][:-1], b["integers"])
    assert np.abs(a["poses"][:-1] - b["poses"]).max() <= 1e-5
    assert np.abs(a["flow directions"][:-1] - b["flow directions"]).max() <= 1e-5
    if SAME_BITS_511_512 is not None:
        assert found == SAME_BITS_511_512   # a change in either direction is news: record it


def test_lane_count_is_the_only_difference_between_511_and_512(shipped_solves, ebo_ab, orc, monkeypatch):
    """The A/B build at EBO_OPT_BLOCK=128 reproduces the shipped 512-patch call bit for bit, at 256 the 511-patch call."""
    problems, full, less = shipped_solves
    for lanes, n, ref in ((128, len(problems), full), (256, len(problems) - 1, less)):
        monkeypatch.setenv("EBO_OPT_BLOCK", str(lanes))
        with _ctx(ebo_ab, TC.gradient_grid()) as c:
            got = c.optimizer_solve(*_solve_args(problems[:n]))
        monkeypatch.delenv("EBO_OPT_BLOCK")
        assert _same(_solve_bits(got), _solve_bits(ref)), lanes
    # ... and the two lane counts on the SAME 511 patches differ exactly as the two shipped calls do
    monkeypatch.setenv("EBO_OPT_BLOCK", "128")
    with _ctx(ebo_ab, TC.gradient_grid()) as c:
        narrow = c.optimizer_solve(*_solve_args(problems[:-1]))
    monkeypatch.delenv("EBO_OPT_BLOCK")
    cut = _solve_bits(full)
    assert _same(_solve_bits(narrow), (cut[0][:-1], cut[1][:-1], cut[2][:-1]))


# ---- 6. the maps -------------------------------------------------------------------------------------------------
def test_maps_match_the_oracle(ebo, orc):
    """estimate_num_events: equal integers on every map case; patch_warp_image: the oracle's array, None exactly where the
    oracle returns None.  Non-square rects, exact quarter and half turns, rounding ties of the 10-bit map, source
    coordinates in (-1, 0) and [W - 1, W), translations to +-1e5."""
    grad = TC.map_grid()
    cases = TC.map_cases()
    rects, poses, flows = ([c[k] for c in cases] for k in range(3))
    with _ctx(ebo, grad) as c:
        est = c.estimate_num_events(rects, poses, flows)
        warp = c.patch_warp_image(rects, poses, flows)
    want = np.array([orc.estimate_num_events(grad, *case) for case in cases], dtype=np.uint64)
    assert np.array_equal(est, want), np.nonzero(est != want)[0]
    assert (want > 0).sum() > 200 and (want == 0).sum() > 0
    done = 0
    for i, case in enumerate(cases):
        w = orc.patch_warp_image(grad, *case)
        assert (w is None) == (warp[i] is None), i
        if w is not None:
            assert warp[i].shape == w.shape
            np.testing.assert_allclose(warp[i], w, rtol=0, atol=WARP_ATOL, err_msg=str(i))
            done += 1
    assert done > 150 and done < len(cases)
    # rows that are checks of their own.  Non-square rects: w and h swapped on the same corner differ
    ident = np.array([1.0, 0.0, 0.0, 0.0])
    a, b = TC.MAP_RECTS_INSIDE[0], TC.MAP_RECTS_INSIDE[1]
    with _ctx(ebo, grad) as c:
        e = c.estimate_num_events([a, b], [ident, ident], [0.3, 0.3])
        wa, wb = c.patch_warp_image([a, b], [ident, ident], [0.3, 0.3])
    assert e[0] != e[1] and wa.shape == (13, 7) and wb.shape == (7, 13)
    assert np.array_equal(wa[:7, :7], wb[:7, :7]) and wa[:7, :7].any()   # the shared corner block: rows are `w` long
    # the exact turns, the ties and the (-1, 0) rows against the direct loop
    k0 = 0
    for group, cs in (("exact", TC.exact_map_cases()), ("tie", TC.tie_cases()), ("floor", TC.floor_cases())):
        for j, case in enumerate(cs):
            rect, pose, flow = case[:3]
            shift = case[3] if len(case) > 3 else None
            i = k0 + j
            assert int(est[i]) == int(TC.direct_estimate_sum(grad, rect, pose, flow, shift)), (group, j)
            if warp[i] is not None:
                g = TC.direct_map(grad, rect, pose, shift)
                np.testing.assert_allclose(warp[i], g[..., 0] * -np.cos(flow) + g[..., 1] * -np.sin(flow), rtol=0,
                                           atol=WARP_ATOL, err_msg="%s %d" % (group, j))
                if group == "floor" and j < 8:   # the column / row that reads from (-1, 0) is outside
                    edge = warp[i][:, 0] if shift[0] else warp[i][0]
                    assert not edge.any() and warp[i].any(), j
        k0 += len(cs)


def test_map_rects_without_an_answer_are_refused(ebo, orc):
    """EBO_ERR_RANGE from both entries for a rect size that rounds outside 0..32767 or is NaN and for a corner that is
    not finite, alone and behind a good rect; the context goes on working; a size of 0 is admitted and gives 0."""
    grad = TC.map_grid()
    good = TC.MAP_RECTS_INSIDE[5]
    pose, flow = np.array([1.0, 0.0, 2.0, -1.0]), 0.4
    with _ctx(ebo, grad) as c:
        for bad in TC.BAD_MAP_RECTS:
            for rects in ([bad], [good, bad]):
                for call in (c.estimate_num_events, c.patch_warp_image):
                    with pytest.raises(ebo.EboError) as ei:
                        call(rects, [pose] * len(rects), [flow] * len(rects))
                    assert ei.value.code == ebo.ERR_RANGE, (bad, call)
        assert c.estimate_num_events([good], [pose], [flow])[0] == orc.estimate_num_events(grad, good, pose, flow) > 0
        np.testing.assert_allclose(c.patch_warp_image([good], [pose], [flow])[0],
                                   orc.patch_warp_image(grad, good, pose, flow), rtol=0, atol=WARP_ATOL)
        for empty in ((10.0, 10.0, 0.0, 5.0), (10.0, 10.0, 5.0, 0.4), (10.0, 10.0, 0.5, 0.5)):
            assert c.estimate_num_events([empty, good], [pose, pose], [flow, flow])[0] == 0
            assert orc.estimate_num_events(grad, empty, pose, flow) == 0
            assert c.patch_warp_image([empty, good], [pose, pose], [flow, flow])[0].size == 0


# ---- 7. the normalisation ----------------------------------------------------------------------------------------
def test_normalisation_at_every_reduction_shape(ebo, orc):
    """k_optimizer_normalize on raw nablas of 1, 64, 65, 256, 257 and 3000 pixels through optimizer_cost_map(normalize=
    True): the pre-normalised call's map (and the oracle's); an all-zero nabla gives the NaN map the oracle gives."""
    grad = TC.gradient_grid()
    rng = np.random.default_rng(5)
    items = []
    for i, (pw, ph) in enumerate(TC.NORMALIZE_SHAPES):
        rect = (float(min(20, TC.W - pw) if pw <= TC.W else -100), 20.0 if ph < 20 else -1.0, float(pw), float(ph))
        items.append(TC._item(rect, TC.pose_of(0.02 * (i - 2), 0.3, -0.4), 0.5 + i, 400 + i, name="%dx%d" % (pw, ph)))
        items[-1]["raw"] = items[-1]["raw"] * rng.uniform(0.5, 40.0)
    args = _args(orc, items)
    raws = [it["raw"] for it in items]
    zeros = [np.zeros_like(r) for r in raws]
    with _ctx(ebo, grad) as c:
        pre = c.optimizer_cost_map(*args, 3, 3)
        raw = c.optimizer_cost_map(args[0], raws, args[2], args[3], 3, 3, normalize=True)
        nan = c.optimizer_cost_map(args[0], zeros, args[2], args[3], 3, 3, normalize=True)
    _check_cost_maps(orc, grad, items, args, pre, 3, 3)
    _check_cost_maps(orc, grad, items, args, raw, 3, 3)
    for i, it in enumerate(items):
        assert np.abs(raw[i] - pre[i]).max() <= 1e-12 * pre[i].max(), it["name"]
        with np.errstate(all="ignore"):
            want = orc.optimizer_cost_map(grad, it["rect"], orc.normalize_nabla(zeros[i]), it["pose"], it["flow"], 3, 3)
        assert np.isnan(want).all()
        assert np.array_equal(np.isnan(nan[i]), np.isnan(want)), it["name"]
