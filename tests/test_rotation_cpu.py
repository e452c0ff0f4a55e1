"""CPU: the rotational contrast maximisation's rules (include/ebo.h V1-V9, N1-N5) through tests/rotation_ref.py, the
library's host solver against the restatement's, and the device's rule functions compiled for the host
(tools/rotation_serial.cpp), also under the address and undefined-behaviour sanitizers.  No GPU."""
import os
import subprocess

import numpy as np
import pytest

import rotation_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SERIAL_SRC = os.path.join(ROOT, "event-based-odomety_amd", "tools", "rotation_serial.cpp")


def test_zero_angular_velocity_gives_the_unwarped_count():
    ev = R.random_window(11, 4000, R.W, R.H, strays=100)
    Hq, r, g, A, _ = R.eval(ev, R.ref_time(ev), R.CAM, R.W, R.H, (0.0, 0.0, 0.0))
    inside = (ev["x"] >= 0) & (ev["x"] < R.W) & (ev["y"] >= 0) & (ev["y"] < R.H)
    count = np.zeros((R.H, R.W), dtype=np.int64)
    np.add.at(count, (ev["y"][inside], ev["x"][inside]), 1)
    assert inside.sum() == 3900 and np.array_equal(Hq, count << 30)


def test_nonfinite_and_huge_angular_velocities_give_the_empty_image():
    ev = R.random_window(12, 500, R.W, R.H)
    for om in ((float("nan"), 0.0, 0.0), (1e9, 1e9, -1e9)):
        Hq, r, g, A, sb = R.eval(ev, R.ref_time(ev), R.CAM, R.W, R.H, om)
        assert not Hq.any() and r == 0.0 and not g.any() and sb == 0.0


def central_difference_error(scale, step=1e-5):
    ev = R.recovery_scene(1)
    t_ref = R.ref_time(ev)
    om = np.array([0.8, -1.5, 2.0])
    _, r, g, _, _ = R.eval(ev, t_ref, R.CAM, R.W, R.H, om, 1.0, scale)
    worst = 0.0
    for i in range(3):
        d = np.zeros(3)
        d[i] = step
        rp = R.eval(ev, t_ref, R.CAM, R.W, R.H, om + d, 1.0, scale)[1]
        rm = R.eval(ev, t_ref, R.CAM, R.W, R.H, om - d, 1.0, scale)[1]
        worst = max(worst, abs((rp - rm) / (2 * step) - g[i]) / np.abs(g).max())
    return worst


def test_the_gradient_against_central_differences():
    """V8 against central differences of the restatement's own r, relative to max |g_i|, on recovery scene 1 at
    omega = (0.8, -1.5, 2.0).  Measured with this file's restatement at step 1e-5 rad/s: 3.14e-5 with the rules' 2^30
    grid and 3.83e-5 with a 2^40 grid -- at that step one or two of the 27 000 event coordinates cross a pixel between
    the two evaluations, where the gradient of the bilinear vote has a kink, and that, not the grid, is what is left.
    At step 1e-7, where nothing crosses: 6.7e-4 with 2^30 (the grid's quantisation over a step that small), 8.9e-7 with
    2^40 and 7.3e-9 with 2^52: the formula is exact and the rest is quantisation.  The bounds are ten times the measured
    values."""
    e30 = central_difference_error(R.Q)
    e40 = central_difference_error(2.0 ** 40)
    fine52 = central_difference_error(2.0 ** 52, 1e-7)
    print("central differences: step 1e-5: 2^30 grid %.3g, 2^40 grid %.3g; step 1e-7: 2^52 grid %.3g" % (e30, e40, fine52))
    assert e30 <= 10 * 3.14e-5
    assert e40 <= 10 * 3.83e-5
    assert fine52 <= 10 * 7.3e-9


# ---- recovery ------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def recovery():
    """The restatement's solves of the 12 scenes from omega0 = 0 with the defaults: (omega, summary, requests) each."""
    return [R.solve_window(R.recovery_scene(i)) for i in range(len(R.RECOVERY_SEEDS))]


def test_the_restatement_recovers_the_twelve_scenes(recovery):
    """Seeds 1-12, omega uniform in +-5 rad/s: every scene ends within 0.10 rad/s of the truth with r at least 1.15 times
    r at zero.  Measured: worst error 0.0964 rad/s (scene 0, whose truth is the smallest), at most 52 evaluations, gain
    at least 1.245.  No seed was changed."""
    truth = R.recovery_truths()
    for i, (om, s, _) in enumerate(recovery):
        err = np.abs(np.array(om) - truth[i]).max()
        print(i, "err %.4f" % err, s)
        assert err <= 0.10, (i, err)
        assert s["r_final"] >= 1.15 * s["r_initial"], (i, s)
        assert s["status"] == R.CONVERGED_STEP


def test_without_blur_the_solve_stays_at_zero():
    """sigma_blur = 0 on scene 1 (truth (4.72, 1.15, 0.68)): at omega = 0 every event sits on an integer pixel, a strict
    optimum of the un-blurred variance, and 20 halvings of the first step do not leave it.  The same happens on 11 of
    the 12 scenes (the exception is scene 0, whose truth is (0.06, 0.65, 0.12)); it is why the default blur is 1.0."""
    om, s, _ = R.solve_window(R.recovery_scene(1), sigma_blur=0.0)
    assert om == [0.0, 0.0, 0.0] and s["status"] == R.NO_PROGRESS and s["iterations"] == 0 and s["evaluations"] == 21


# ---- libebo's host solver against the restatement's ---------------------------------------------

def drive(ebo, feeds, opts=None, omega0=None):
    """Runs the library's solver for len(feeds) windows in lock step, window i fed by feeds[i](omega) -> (r, g).
    -> (omegas, summaries, per-window request lists)"""
    n = len(feeds)
    o = ebo.rot_solver_opts(**(opts or {}))
    requests = [[] for _ in range(n)]
    with ebo.RotationSolver(n, o, omega0) as s:
        while True:
            left, om, live = s.request()
            if left == 0:
                break
            assert left == live.sum()
            r, g = np.zeros(n), np.zeros((n, 3))
            for i in range(n):
                if live[i]:
                    requests[i].append(om[i].tolist())
                    r[i], g[i] = feeds[i](om[i].tolist())
                else:
                    r[i], g[i] = np.nan, np.nan  # ignored
            s.supply(r, g)
        with pytest.raises(ebo.EboError):
            s.supply(np.zeros(n), np.zeros((n, 3)))
        om, summ = s.result()
    return om, summ, requests


def same_summary(got, want):
    return (got.status, got.iterations, got.evaluations) == (want["status"], want["iterations"], want["evaluations"]) and \
        R.same_bits(got.r_initial, want["r_initial"]) and R.same_bits(got.r_final, want["r_final"])


def test_the_host_solver_equals_the_restatement_on_the_twelve_scenes(ebo, recovery):
    """All 12 in ONE solver object, each fed the restatement's (r, g): omega, summary and the sequence of requests are
    the restatement's bit for bit."""
    def feed(i):
        ev = R.recovery_scene(i)
        t_ref = R.ref_time(ev)
        memo = {}

        def fun(om):
            key = tuple(om)
            if key not in memo:
                _, r, g, _, _ = R.eval(ev, t_ref, R.CAM, R.W, R.H, om)
                memo[key] = (r, g)
            return memo[key]
        return fun
    om, summ, requests = drive(ebo, [feed(i) for i in range(len(recovery))])
    for i, (want_om, want_s, want_req) in enumerate(recovery):
        assert R.same_bits(om[i], want_om), i
        assert same_summary(summ[i], want_s), i
        assert R.same_bits(np.array(requests[i]), np.array(want_req)), i


def quadratic(centre, curv):
    centre, curv = np.array(centre), np.array(curv)
    return lambda om: (-float(((np.array(om) - centre) ** 2 * curv).sum()), -2.0 * curv * (np.array(om) - centre))


class Script:
    """A feed that answers the k-th evaluation from a list (the last entry repeats)."""

    def __init__(self, answers):
        self.answers, self.k = answers, 0

    def __call__(self, om):
        a = self.answers[min(self.k, len(self.answers) - 1)]
        self.k += 1
        return a(om) if callable(a) else a


NAN3 = (float("nan"),) * 3
HAND_FEEDS = {
    # name: (feed factory, options, expected status)
    "nan_at_omega0": (lambda: Script([(float("nan"), (1.0, 0.0, 0.0))]), {}, R.NONFINITE),
    "nan_gradient_at_omega0": (lambda: Script([(1.0, NAN3)]), {}, R.NONFINITE),
    "nan_at_a_trial": (lambda: Script([quadratic((1, 2, 3), (1, 1, 1)), (float("nan"), (0.0, 0.0, 0.0)),
                                       quadratic((1, 2, 3), (1, 1, 1))]), {}, R.CONVERGED_STEP),
    "zero_gradient": (lambda: Script([(3.0, (0.0, 0.0, 0.0))]), {}, R.CONVERGED_GRADIENT),
    "twenty_refused_trials": (lambda: Script([(1.0, (1.0, -2.0, 0.5)), (0.5, (1.0, 1.0, 1.0))]), {}, R.NO_PROGRESS),
    # a concave direction: the gradient grows along the step, so s . y of f = -r is negative and alpha doubles
    "sy_not_positive": (lambda: quadratic((0, 0, 0), (-1, -1, -1)), {"max_iterations": 6}, R.MAX_ITERATIONS),
    "one_iteration": (lambda: quadratic((1, 2, 3), (1, 2, 3)), {"max_iterations": 1}, R.MAX_ITERATIONS),
    "converges": (lambda: quadratic((1, -2, 3), (1, 2, 3)), {}, R.CONVERGED_STEP),
    "two_backtracks_allowed": (lambda: Script([(1.0, (1.0, 0.0, 0.0)), (0.0, (1.0, 0.0, 0.0))]), {"max_backtracks": 2}, R.NO_PROGRESS),
}


@pytest.mark.parametrize("name", sorted(HAND_FEEDS))
def test_the_host_solver_equals_the_restatement_on_hand_made_feeds(ebo, name):
    make, opts, status = HAND_FEEDS[name]
    omega0 = (0.25, -0.5, 0.125)
    want_om, want_s, want_req = R.solve(make(), omega0, opts)
    assert want_s["status"] == status
    om, summ, requests = drive(ebo, [make()], opts, [omega0])
    assert R.same_bits(om[0], want_om) and same_summary(summ[0], want_s)
    assert R.same_bits(np.array(requests[0]), np.array(want_req))
    if name == "twenty_refused_trials":
        assert want_s["evaluations"] == 21 and want_om == list(omega0)
    if name == "sy_not_positive":
        steps = np.abs(np.diff(np.array(want_req)[:, 0]))
        assert np.all(steps[1:] > 1.9 * steps[:-1])


def test_solver_arguments(ebo):
    for bad in (dict(first_rate=0.0), dict(first_rate=float("nan")), dict(c1=0.0), dict(c1=1.0), dict(max_backtracks=0),
                dict(step_tol=-1.0), dict(max_iterations=0)):
        with pytest.raises(ebo.EboError):
            ebo.RotationSolver(1, ebo.rot_solver_opts(**bad))
    with pytest.raises(ebo.EboError):
        ebo.RotationSolver(0)
    o = ebo.rot_solver_opts()
    assert (o.first_rate, o.c1, o.step_tol, o.max_backtracks, o.max_iterations) == (0.5, 1e-4, 1e-4, 20, 100)
    assert ebo.RotationParams().sigma_blur == 1.0


# ---- the device's rule functions on the host ------------------------------------------------------

def build_serial(path, sanitize):
    cxx = os.environ.get("CXX", "c++")
    base = [cxx, "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas"]
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # a sanitized build that does not link fails the test: it never runs unsanitized under that name
    subprocess.check_call(base + (san if sanitize else ["-O2"]) + ["-o", path, SERIAL_SRC])
    return path


def run_serial(exe, tmp_path, ev, t_ref, cam, w, h, om):
    inside = (ev["x"] >= 0) & (ev["x"] < w) & (ev["y"] >= 0) & (ev["y"] < h)
    rows = np.stack([ev["x"][inside], ev["y"][inside], t_ref - ev["t_us"][inside]], axis=1).astype(np.float64)
    head = np.array([w, h, *cam, *om, len(rows)], dtype=np.float64)
    np.concatenate([head, rows.reshape(-1)]).tofile(tmp_path / "p.f64")
    out = subprocess.run([exe, str(tmp_path / "p.f64"), str(tmp_path / "r.f64")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    res = np.fromfile(tmp_path / "r.f64")
    return res[:w * h].reshape(h, w).astype(np.int64), int(res[w * h]), res[w * h + 1:]


@pytest.mark.parametrize("sanitize", [False, True])
def test_the_device_text_on_the_host(tmp_path, sanitize):
    """csrc/ebo_rotation.inc's rot_warp, rot_weights and rot_terms, compiled for the host and run event by event over
    every window of the GPU test's cases -- both sensors, the eight angular velocities (40 rad/s about each axis, 1e9, a
    NaN, an infinity among them), the border window (x0 = -1, x0 = w - 1, y0 = -1, y0 = h - 1, taps half outside), events
    on integers, 15 000 events on one pixel: H is the restatement's bit for bit, and the un-blurred gradient sums agree
    within V9's bound.  Once plain, once under the address and undefined-behaviour sanitizers: no report.  This covers
    the rule functions only; the kernels' tile and flush indexing is covered by tests/test_gpu_rotation.py."""
    exe = build_serial(str(tmp_path / "rotation_serial"), sanitize)
    seen_border = set()
    for name, case in R.gpu_cases().items():
        geo = case["geo"]
        w, h, cam = geo["w"], geo["h"], geo["cam"]
        for ev, om in zip(case["windows"], case["omegas"]):
            t_ref = R.ref_time(ev)
            Hq, r, g, A, _ = R.eval(ev, t_ref, cam, w, h, om, 0.0)
            got_H, voted, S = run_serial(exe, tmp_path, ev, t_ref, cam, w, h, om)
            k = R.warp(ev, t_ref, cam, w, h, om)
            assert voted == len(k["x0"]), name
            assert np.array_equal(got_H, Hq), name
            assert np.all(np.abs((2.0 / (w * h)) * S - g) <= 1e-9 * A), name
            for key, v in (("x0", -1), ("x0", w - 1), ("y0", -1), ("y0", h - 1)):
                if np.any(k[key] == v):
                    seen_border.add((geo["w"], key, v))
    assert len(seen_border) == 8, seen_border


def test_the_facade_driver_compiles(ebo, tmp_path):
    """tracker::AngularVelocityEstimator and the C ABI it is held to compile under -Wall -Wextra against the library (tests/cpp/angular_velocity_test.cpp; run on the GPU by
    tests/test_gpu_rotation_facade.py)."""
    ebo.lib()
    cpp = os.path.join(ROOT, "tests", "cpp")
    out = subprocess.run(["make", "-s", "-C", cpp, "-f", "angular_velocity.mk", "OUT=" + str(tmp_path), str(tmp_path / "angular_velocity_test")],
                         capture_output=True, text=True)
    assert out.returncode == 0 and os.path.exists(tmp_path / "angular_velocity_test"), out.stderr[-2000:]
    assert "warning" not in out.stderr


# ---- the launch shapes of tests/test_gpu_rotation_shapes.py ---------------------------------------

def test_the_tile_cases_reach_every_tile_form():
    """k_rot_vote picks its LDS tile from the unit's rect alone (rotation_ref.tile_of restates it): the cases of
    tests/test_gpu_rotation_shapes.py hold units with the grown tile, the bare tile and no tile, one at each limit, grown
    tiles clipped at each image edge, and for every form that has a tile taps inside it and taps that miss it.  The
    older cases (rotation_ref.gpu_cases) hold the grown form only."""
    assert {R.tile_form(r, g["w"], g["h"]) for g in (R.SMALL, R.LARGE, R.DAVIS346) for r in R.rects(g)} == {"grown"}
    units = [(g, r, R.tile_form(r, g["w"], g["h"])) for g in R.TILE_GEOS.values() for r in R.rects(g)]
    assert {f for _, _, f in units} == {"grown", "bare", "none"}
    assert any(f == "grown" and (r[2] + 2 * R.MARGIN) * (r[3] + 2 * R.MARGIN) == R.TILE_PX for _, r, f in units)  # the last margin
    assert any(f == "bare" and r[2] * r[3] == R.TILE_PX for _, r, f in units)                                       # the last tile
    assert any(f == "bare" and r[2] * r[3] < R.TILE_PX for _, r, f in units)           # too big for its margin, not for a tile
    above = [r[2] * r[3] for _, r, f in units if f == "none"]
    assert min(above) == R.TILE_PX + 64 and all(f != "none" or r[2] * r[3] > R.TILE_PX for _, r, f in units)  # one row of 64 more
    assert R.tile_form(R.rects(R.T150)[-1], 150, 128) == "none" and R.rects(R.T150)[-1] == (96, 48, 54, 80)  # the remainder rect
    clipped = set()
    for g, r, f in units:
        tx0, ty0, tw, th = R.tile_of(r, g["w"], g["h"])
        if f == "grown":
            edges = {e for e, hit in (("left", r[0] - R.MARGIN < 0), ("top", r[1] - R.MARGIN < 0),
                                      ("right", r[0] + r[2] + R.MARGIN > g["w"]), ("bottom", r[1] + r[3] + R.MARGIN > g["h"])) if hit}
            assert (tw * th < (r[2] + 2 * R.MARGIN) * (r[3] + 2 * R.MARGIN)) == bool(edges)
            clipped |= edges
        assert 0 <= tx0 and 0 <= ty0 and tx0 + tw <= g["w"] and ty0 + th <= g["h"] and tw * th <= R.TILE_PX
    assert clipped == {"left", "top", "right", "bottom"}
    total = {f: dict(inside=0, direct=0) for f in ("grown", "bare", "none")}
    for name, case in sorted(R.tile_cases().items()):
        census = R.tap_census(case)
        print(name, {f: (len(v["units"]), v["inside"], v["direct"]) for f, v in census.items()})
        for f, v in census.items():
            total[f]["inside"] += v["inside"]
            total[f]["direct"] += v["direct"]
        if name.endswith("_small"):  # every unit of every window accumulates taps
            n_units = len(R.rects(case["geo"]))
            assert sum(len(v["units"]) for v in census.values()) == len(case["windows"]) * n_units, name
    print("taps (in the tile, straight to H):", {f: (v["inside"], v["direct"]) for f, v in total.items()})
    assert total["grown"]["inside"] and total["grown"]["direct"] and total["bare"]["inside"] and total["bare"]["direct"]
    assert total["none"]["direct"] and not total["none"]["inside"]
    t150 = R.tap_census(R.tile_cases()["t150_x40"])  # the A/B comparison's geometry holds all of it by itself
    assert all(t150[f]["direct"] for f in t150) and t150["grown"]["inside"] and t150["bare"]["inside"]


def test_the_chunk_budgets_and_the_long_windows_are_what_they_are_meant_to_be():
    """eval_windows' slots per chunk under the budgets the GPU test sets (rotation_ref.chunk_slots restates the carve), and
    the units' dt_win of the 1.5 s windows as the loader derives them."""
    small = [R.chunk_slots(R.SMALL, mb, 70) for mb in (0, 1, None)]
    print("37 x 29: %d bytes a slot, slots at 0 MB, 1 MB, unset: %s" % (R.carve_bytes(R.SMALL), small))
    assert small[0] == 1 and 1 < small[1] < R.CHUNK_MAX and 70 % small[1] != 0 and small[2] == R.CHUNK_MAX
    large = R.chunk_slots(R.LARGE, 5, 12)
    print("240 x 180: %d bytes a slot, slots at 5 MB: %d" % (R.carve_bytes(R.LARGE), large))
    assert 1 < large <= 5 and 12 % large != 0 and R.chunk_slots(R.LARGE, None, 12) == 12
    for name, case in R.long_cases().items():
        for ev in case["windows"]:
            dt = R.unit_dt_win(ev, R.SMALL)
            span = int(ev["t_us"][-1]) - int(ev["t_us"][0])
            print(name, "span %d us, t_ref %d, dt_win %s" % (span, R.ref_time(ev), dt))
            assert span > 1400000 and R.ref_time(ev) < 2 ** 31 and len(dt) == 12
            assert max(dt.values()) > 100000 and min(dt.values()) < -100000
    assert R.ref_time(R.long_cases()["long_zero"]["windows"][1]) > 2000000000
    k = R.warp(R.long_cases()["long_slow"]["windows"][0], 750000, R.SMALL["cam"], 37, 29, R.SLOW)
    assert len(k["x0"]) > 1000 and np.any(k["al"] != 0.0)  # the events stay in view, off the integers
