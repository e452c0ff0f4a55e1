"""What makes the comparisons of tests/test_gpu_tracker_shapes.py fair, on the CPU: the oracle (the yardstick of the GPU
tests) against second restatements on the very inputs of tests/tracker_cases.py, and the conditions those inputs have
to meet (no estimate at the edge of its truncation, no solve problem whose own summary is at the rounding level)."""
import numpy as np
import pytest

import tracker_cases as TC
from test_optimizer import functor_np


def _grid_items():
    return TC.border_items() + TC.shape_items()


def test_case_tables_are_what_they_say():
    assert TC.gradient_grid().shape == (TC.H, TC.W, 2)
    g = np.abs(TC.gradient_grid())
    # the grid does not vanish at the border
    assert g[0].mean() > 0.5 and g[-1].mean() > 0.5 and g[:, 0].mean() > 0.5 and g[:, -1].mean() > 0.5
    px = [pw * ph for pw, ph in TC.SHAPES]
    assert {1, 9, 64, 65, 128, 129, 255, 256, 625} <= set(px) and max(px) == TC.MAX_PIXELS
    assert TC.REFUSED_SHAPE[0] * TC.REFUSED_SHAPE[1] > TC.MAX_PIXELS
    # LDS per shape: 40x33 is the largest inside 64 KB, 37x37 the first above; the maximum fits 160 KB
    assert TC.lds_bytes(40, 33) <= 64 * 1024 < TC.lds_bytes(37, 37)
    assert TC.lds_bytes(60, 50) == 145024 <= 160 * 1024 - 512
    assert [pw * ph for pw, ph in TC.NORMALIZE_SHAPES] == [1, 64, 65, 256, 257, 3000]
    for it in TC.shape_items():
        assert (int(it["rect"][2]), int(it["rect"][3])) in TC.SHAPES
    big = TC.big_item(60, 50)
    assert 0 < TC.inside_count(big) < 3000   # hangs over the border
    pw, ph = 60, 50
    c, s, tx, ty = big["pose"]
    xs = [c * X - s * Y + tx for X in (big["rect"][0], big["rect"][0] + pw - 1) for Y in (big["rect"][1], big["rect"][1] + ph - 1)]
    ys = [s * X + c * Y + ty for X in (big["rect"][0], big["rect"][0] + pw - 1) for Y in (big["rect"][1], big["rect"][1] + ph - 1)]
    assert min(xs) < 0 and max(xs) >= TC.W and min(ys) < 0 and max(ys) >= TC.H   # ... over all four


def test_stated_inside_counts(orc):
    """The border cases state how many samples are inside; exact rational arithmetic and the oracle agree (a sample inside
    has a non-zero prediction on this grid), so the inside test cannot pass trivially."""
    grad = TC.gradient_grid()
    seen = set()
    for it in TC.border_items():
        assert TC.inside_count(it) == it["inside"], it["name"]
        zero = np.zeros_like(it["raw"])
        res, _, _ = orc.optimizer_cost(grad, it["rect"], zero, it["pose"], it["flow"], want_jac=False)
        assert int((res != 0.0).sum()) == it["inside"], it["name"]
        seen.add(it["inside"])
    assert len(seen) >= 6 and min(seen) == 1 and max(seen) == 12


def test_oracle_functor_equals_numpy_on_every_case(orc):
    worst = 0.0
    sets = [(TC.gradient_grid(), _grid_items())] + [(TC.tiny_grid(w, h), TC.tiny_items(w, h)) for w, h in TC.TINY_IMAGES]
    for grad, items in sets:
        for it in items:
            nabla = orc.normalize_nabla(it["raw"])
            res, _, _ = orc.optimizer_cost(grad, it["rect"], nabla, it["pose"], it["flow"], want_jac=False)
            ref = functor_np(grad, it["rect"], nabla, it["pose"], it["flow"])
            d = float(np.abs(res - ref).max())
            worst = max(worst, d)
            assert d < 1e-13, (it["name"], d)
    print("oracle functor against numpy: max difference %.2e" % worst)


def test_tiny_images_clamp_every_tap(orc):
    """On an image no larger than the 4x4 neighbourhood every sample's taps reach a border; a constant image then
    predicts the constant wherever a sample is inside (Catmull-Rom reproduces constants)."""
    for w, h in TC.TINY_IMAGES:
        grad = np.full((h, w, 2), 2.0)
        for it in TC.tiny_items(w, h):
            zero = np.zeros_like(it["raw"])
            res, _, _ = orc.optimizer_cost(grad, it["rect"], zero, it["pose"], 0.0, want_jac=False)
            n = TC.inside_count(it, w, h)
            assert n > 0
            want = 2.0 / np.sqrt(1e-5 + 4.0 * n)
            assert int((res != 0).sum()) == n and np.abs(res[res != 0] - want).max() < 1e-15


def test_oracle_maps_equal_the_direct_loop(orc):
    grad = TC.map_grid()
    n = 0
    for rect, pose, flow in TC.exact_map_cases():
        assert orc.estimate_num_events(grad, rect, pose, flow) == int(TC.direct_estimate_sum(grad, rect, pose, flow))
        got = orc.patch_warp_image(grad, rect, pose, flow)
        if rect in TC.MAP_RECTS_OUTSIDE:
            assert got is None
        else:
            g = TC.direct_map(grad, rect, pose)
            np.testing.assert_array_equal(got, g[..., 0] * -np.cos(flow) + g[..., 1] * -np.sin(flow))
        n += 1
    assert n >= 120
    shifts = set()
    for rect, pose, flow, shift in TC.tie_cases() + TC.floor_cases():
        assert orc.estimate_num_events(grad, rect, pose, flow) == int(TC.direct_estimate_sum(grad, rect, pose, flow, shift))
        g = TC.direct_map(grad, rect, pose, shift)
        np.testing.assert_array_equal(orc.patch_warp_image(grad, rect, pose, flow),
                                      g[..., 0] * -np.cos(flow) + g[..., 1] * -np.sin(flow))
        shifts.add(shift[0] - int(np.floor(pose[2])) if pose[2] else shift[1] - int(np.floor(pose[3])))
    assert shifts == {0, 1}   # both roundings occur
    # the floor cases put a whole column or row outside: the (-1, 0) rows read nothing from column / row 0
    for rect, pose, flow, shift in TC.floor_cases()[:8]:
        g = TC.direct_map(grad, rect, pose, shift)
        edge = g[:, 0] if shift[0] else g[0]
        assert not edge.any() and g.any()
    # the non-square rects with the same corner differ
    a, b = TC.MAP_RECTS_INSIDE[0], TC.MAP_RECTS_INSIDE[1]
    assert (a[2], a[3]) == (b[3], b[2]) and a[:2] == b[:2]
    pose = np.array([1.0, 0.0, 0.0, 0.0])
    assert orc.estimate_num_events(grad, a, pose, 0.3) != orc.estimate_num_events(grad, b, pose, 0.3)


def test_no_estimate_is_at_the_edge_of_its_truncation(orc):
    """Condition (a): the estimate is a double sum truncated to an integer; the device adds in another order.  No case's
    sum lies within 1e-9 of an integer unless it is exactly 0 (nothing read).  Also: the Python restatement of the
    fixed-point map gives the oracle's integer on every case."""
    grad = TC.map_grid()
    closest, zeros, positive = 1.0, 0, 0
    for rect, pose, flow in TC.map_cases():
        s = TC.fixed_point_sum(grad, rect, pose, flow)
        assert int(s) == orc.estimate_num_events(grad, rect, pose, flow)
        if s == 0.0:
            zeros += 1
            continue
        positive += 1
        closest = min(closest, abs(s - round(s)))
    print("estimates: %d cases, %d exactly 0, smallest distance of a sum to an integer %.3e" % (zeros + positive, zeros, closest))
    assert closest >= 1e-9
    assert positive > 200 and zeros > 0


def test_solve_problems_pass_the_admission_gate(orc):
    """Condition (b), the gate of test_gpu_optimizer_branches.test_variant_is_stable_on_the_oracle: the oracle's
    (iterations, termination, cost evaluations, Jacobian evaluations) stand when the nabla moves by 1e-12 relative, eight
    seeded times.  The problems that fail are TC.DROPPED, at most 10 of 512."""
    grad = TC.gradient_grid()
    items = TC.solve_problems(orc)
    assert len(items) == TC.N_SOLVE == 512
    failed = []
    ends = set()
    for k, it in enumerate(items):
        _, _, s = orc.optimizer_solve(grad, it["rect"], it["nabla"], it["start"][0], it["start"][1])
        want = (s.iterations, s.termination, s.num_evals_cost, s.num_evals_jac)
        ends.add((s.termination, s.iterations >= 10))
        for seed in range(8):
            nabla = it["nabla"] * (1.0 + 1e-12 * np.random.default_rng([seed, k]).uniform(-1.0, 1.0, it["nabla"].shape))
            _, _, s = orc.optimizer_solve(grad, it["rect"], nabla, it["start"][0], it["start"][1])
            if (s.iterations, s.termination, s.num_evals_cost, s.num_evals_jac) != want:
                failed.append(k)
                break
    print("admission gate: %d of %d problems dropped: %s" % (len(failed), len(items), failed))
    assert tuple(failed) == tuple(TC.DROPPED) and len(failed) <= 10
    assert (0, False) in ends and (1, True) in ends   # a tolerance and the cap of 10: both exits occur
    kept = TC.kept_problems(orc)
    assert len(kept) == 512 - len(TC.DROPPED) and {it["shape"] for it in kept[:17]} == set(TC.SHAPES)


@pytest.mark.parametrize("bad", TC.BAD_MAP_RECTS)
def test_bad_map_rects_have_no_answer(bad):
    """What ebo_estimate_num_events and ebo_patch_warp_image refuse: a corner that is not finite, a size that is NaN or
    rounds outside 0..32767"""
    x, y, w, h = bad
    with np.errstate(invalid="ignore"):
        ok = np.isfinite(x) and np.isfinite(y) and 0 <= np.rint(w) <= 32767 and 0 <= np.rint(h) <= 32767
    assert not ok
