"""CPU: the map-tracking rules (include/ebo.h E1-E9) through tests/maptrack_ref.py: the restatement against a brute-force
scalar loop on Python floats, its Jacobian against central differences, the recovery of a known pose on the two-depth
scene by the restatement alone, the scenes of tests/test_gpu_map_track.py taking the branches they are there for, and
the device's own text compiled for the host (tools/map_track_serial.cpp), once plain and once under the address and
undefined-behaviour sanitizers as a stand-alone program.  No GPU.

Measured here (printed by the tests):
  Jacobian against central differences at step 1e-6, 120 points, both scenes: largest |J - fd| 1.8e-9 on rows of size up
    to 24; the bound asserted is 10 x that, 1.8e-8.
  Recovery, seeds 0-7, one start displaced by 0.06 and 0.02 rad: start 1.01-1.69 px, final 0.045-0.144 px, final / start
    0.031-0.127, translation error 0.003-0.018.  13 starts (steps 0.05 and 0.015 rad) displaced by 0.10 and 0.03 rad:
    start 1.55-2.69 px, final 0.067-0.122 px, final / start 0.028-0.064, translation error 0.003-0.015."""
import math
import os
import subprocess

import numpy as np
import pytest

import bundle_ref as B
import maptrack_ref as M

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SERIAL_SRC = os.path.join(ROOT, "event-based-odomety_amd", "tools", "map_track_serial.cpp")


# ---- 1. the restatement against a scalar loop -------------------------------------------------------------------------

def py_tree(v):
    part = [0.0] * 256
    for i, x in enumerate(v):
        part[i % 256] = part[i % 256] + x
    s = 128
    while s:
        for i in range(s):
            part[i] = part[i] + part[i + s]
        s //= 2
    return part[0]


def scalar_point(cam, img, s, T, X, z_min, scale):
    """E2-E5 of one point on Python floats -> (r, J[6], visible)."""
    fx, fy, cx, cy = cam
    h, w = len(img), len(img[0])
    d = [X[0] - T[9], X[1] - T[10], X[2] - T[11]]
    q = [(T[j] * d[0] + T[3 + j] * d[1]) + T[6 + j] * d[2] for j in range(3)]
    if q[2] == 0.0 or math.isnan(q[2]):
        return 1.0, [0.0] * 6, False  # 1 / 0 and a NaN fail every test of E2
    iz = 1.0 / q[2]
    xP, yP = q[0] * iz, q[1] * iz
    u, v = fx * xP + cx, fy * yP + cy
    if not (q[2] > z_min and u >= 0.0 and u < float(w - 1) and v >= 0.0 and v < float(h - 1)):
        return 1.0, [0.0] * 6, False
    x0, y0 = math.floor(u), math.floor(v)
    al, be = u - x0, v - y0
    ial, ibe = 1.0 - al, 1.0 - be
    b00, b10, b01, b11 = img[y0][x0], img[y0][x0 + 1], img[y0 + 1][x0], img[y0 + 1][x0 + 1]
    b = ibe * (ial * b00 + al * b10) + be * (ial * b01 + al * b11)
    r = 1.0 - s * b
    Du = ibe * (b10 - b00) + be * (b11 - b01)
    Dv = ial * (b01 - b00) + al * (b11 - b10)
    au, av = Du * fx, Dv * fy
    A0, A1, A2 = -(s * (au * iz)), -(s * (av * iz)), s * ((au * xP + av * yP) * iz)
    J = [-A0, -A1, -A2, A1 * q[2] - A2 * q[1], A2 * q[0] - A0 * q[2], A0 * q[1] - A1 * q[0]]
    return r, [J[a] * scale[a] for a in range(6)], True


def test_the_restatement_against_a_scalar_loop():
    """A 9 x 7 image, five points, two poses: one point on each of u = 0 (visible), u = w - 1 and v = h - 1 (not), one
    behind the camera and a NaN point.  Under the second pose the three border points are ordinary visible points."""
    w, h = 9, 7
    cam = (4.0, 4.0, 4.0, 3.0)
    rng = np.random.default_rng(3)
    img = rng.uniform(0.0, 2.0, (h, w))

    def at(u, v, z=2.0):
        return [(u - cam[2]) / cam[0] * z, (v - cam[3]) / cam[1] * z, z]

    X = np.array([at(0.0, 2.5), at(w - 1.0, 2.5), at(3.25, h - 1.0), [0.2, 0.1, -2.0], [0.1, np.nan, 2.0]])
    second = M.pose_of(B.rot(np.array([0.02, -0.03, 0.01])), [0.02, -0.03, -0.4])  # stepping back brings the border points in
    scale = np.array([0.9, 0.8, 0.7, 0.6, 0.5, 0.4])
    s = 1.0 / M.image_max(img)
    assert s == 1.0 / max(max(row) for row in img.tolist())
    want_vis = {0: [True, False, False, False, False], 1: [True, True, True, False, False]}
    for pi, T in enumerate((M.IDENTITY, second)):
        r, J, vis = M.point_terms(cam, img, s, T, X, 0.05, scale, True)
        rows = [scalar_point(cam, img.tolist(), s, [float(t) for t in T], [float(x) for x in X[i]], 0.05, scale.tolist())
                for i in range(len(X))]
        assert [row[2] for row in rows] == want_vis[pi] == vis.tolist(), pi
        for i, (ri, Ji, _) in enumerate(rows):
            assert M.same_bits(r[i], ri) and M.same_bits(J[i], Ji), (pi, i)
        sol = M.Solver(cam, img, X, T, 0.05)
        sol.s, sol.scale = s, scale
        cost = sol.eval_jac(T)
        assert M.same_bits(cost, 0.5 * py_tree([row[0] * row[0] for row in rows]))
        for a in range(6):
            assert M.same_bits(sol.g[a], py_tree([row[1][a] * row[0] for row in rows]))
            for b in range(a + 1):
                assert M.same_bits(sol.U[a, b], py_tree([row[1][a] * row[1][b] for row in rows]))
        assert sol.vis_x == sum(want_vis[pi])
    # a 600-entry tree against bundle_ref's: the partial boundary
    v = rng.normal(size=600)
    assert M.same_bits(B.tree(v), py_tree(v.tolist()))


# ---- 2. the Jacobian ------------------------------------------------------------------------------------------------------

FD_BOUND = 1.8e-8  # 10 x the largest difference measured (module docstring)


@pytest.mark.parametrize("seed", [0, 1])
def test_the_jacobian_against_central_differences(seed):
    """dr / d(step_a) of E4 through B4's update, step 1e-6 on each of the six directions, over the points that stay at
    least 1e-3 px away from a pixel crossing (r is bilinear inside a cell and only continuous across its edge)."""
    sc = M.recovery_scene(seed)
    cam, img, X, T = sc["cam"], sc["image"], sc["points"], sc["start"]
    s = 1.0 / M.image_max(img)
    one = np.ones(6)
    r, J, vis = M.point_terms(cam, img, s, T, X, M.Z_MIN, one, True)
    uv = M.pixels_of(sc["geo"], T, X)
    frac = uv - np.floor(uv)
    away = vis & (np.minimum(frac, 1.0 - frac).min(axis=1) >= 1e-3)
    assert away.sum() >= 100
    worst = 0.0
    hstep = 1e-6
    for a in range(6):
        e = np.zeros(6)
        e[a] = hstep
        rp, _, vp = M.point_terms(cam, img, s, M.retract(T, e), X, M.Z_MIN, one, False)
        rm, _, vm = M.point_terms(cam, img, s, M.retract(T, -e), X, M.Z_MIN, one, False)
        assert vp[away].all() and vm[away].all()
        fd = (rp - rm) / (2.0 * hstep)
        worst = max(worst, float(np.abs(fd - J[:, a])[away].max()))
    print("seed %d: largest |J - fd| %.3g on rows of size up to %.3g" % (seed, worst, float(np.abs(J[away]).max())))
    assert worst <= FD_BOUND


# ---- 3. recovery ----------------------------------------------------------------------------------------------------------

def recover(seed, dt, dr, multi):
    sc = M.recovery_scene(seed, dt, dr)
    starts = M.starts13(sc["start"], 0.05, 0.015) if multi else sc["start"][None]
    pr = M.problem(sc["geo"], sc["image"][None], sc["points"], np.zeros(len(starts), int), starts)
    out = M.solve_units(pr)
    wi = M.winner([o["result"] for o in out])
    assert wi is not None
    e0 = M.reprojection_error(sc["geo"], sc["points"], sc["start"], sc["truth"])
    e1 = M.reprojection_error(sc["geo"], sc["points"], out[wi]["pose"], sc["truth"])
    terr = float(np.linalg.norm(out[wi]["pose"][9:] - sc["truth"][9:]))
    r = out[wi]["result"]
    print("seed %d starts %d: start %.2f px, final %.3f px, ratio %.3f, translation error %.4f, winner %d, termination %d, "
          "iterations %d, cost %.3f -> %.3f" % (seed, len(starts), e0, e1, e1 / e0, terr, wi, r["termination"], r["iterations"],
                                                r["initial_cost"], r["final_cost"]))
    return e0, e1, terr


@pytest.mark.parametrize("seed", range(8))
def test_recovery_from_one_start(seed):
    e0, e1, terr = recover(seed, 0.06, 0.02, False)
    assert e1 <= 0.5 and e1 <= e0 / 3.0 and terr < 0.06


@pytest.mark.parametrize("seed", range(8))
def test_recovery_from_13_starts(seed):
    """The extra starts are +- 0.05 and +- 0.015 rad, half the displacement: one of them lands about where the single
    start of the test above begins."""
    e0, e1, terr = recover(seed, 0.10, 0.03, True)
    assert e1 <= 0.5 and e1 <= e0 / 3.0 and terr < 0.10


def test_the_winner_rule():
    res = [dict(termination=2, final_cost=0.1), dict(termination=0, final_cost=3.0), dict(termination=1, final_cost=2.0),
           dict(termination=0, final_cost=2.0)]
    assert M.winner(res) == 2 and M.winner(res[:1]) is None and M.winner(res[:2]) == 1


# ---- 4. the scenes of the GPU tests take their branches -------------------------------------------------------------------

@pytest.fixture(scope="module")
def solved():
    """name -> (problem, the restatement's units); computed once, read only."""
    return {name: (pr, M.solve_units(pr)) for name, pr in M.gpu_problems().items()}


def test_the_branch_scenes_take_their_branches(solved):
    def one(name):
        pr, out = solved["branch_" + name]
        return pr, out[0], out[0]["result"], out[0]["solver"].flags

    for name in ("rej", "rej_r16", "mrd"):
        _, o, r, f = one(name)
        runs = "".join("r" if v == 0 else "." for v in f)
        assert "rrr" in runs and 1 in f, name  # a run of rejected steps, and taken ones
    assert one("rej")[2]["final_cost"] < one("rej")[2]["initial_cost"]
    _, o, r, f = one("nonmono")
    tr = o["trace"]
    taken = tr[1:len(f) + 1][np.array(f) == 1, 0]
    assert (np.diff(np.concatenate([[tr[0, 0]], taken])) > 0).any()  # a taken step that raised the cost
    assert not M.same_bits(o["trace"], one("rej_r16")[1]["trace"]) and not M.same_bits(o["trace"], one("nonmono_m2")[1]["trace"])
    for name, n in (("invalid", 5), ("invalid3", 3)):
        _, o, r, f = one(name)
        assert f == [-1] * n and r["termination"] == 2 and r["iterations"] == n and len(o["solver"].failed_pivots) == n
        assert M.same_bits(o["pose"], one(name)[0]["poses"][0])
    assert (one("it0")[2]["termination"], one("it0")[2]["iterations"]) == (1, 0)
    assert (one("it1")[2]["termination"], one("it1")[2]["iterations"]) == (1, 1)
    _, o, r, f = one("minrad")
    assert (r["termination"], r["iterations"]) == (0, 0) and o["solver"].exit_checks[-1] == (1e-33, 1e-32)
    _, o, r, f = one("gtol")
    g, tol = o["solver"].exit_checks[-1]
    assert r["termination"] == 0 and tol == 2.0 and g <= tol and f[-1] == 1
    _, o, r, f = one("ptol")
    sn, st, df, ft = o["solver"].checks[-1]
    assert r["termination"] == 0 and f[-1] == 2 and sn <= st and ft == 0.0 and df > 0.0
    for name in ("ftol", "plain"):
        _, o, r, f = one(name)
        sn, st, df, ft = o["solver"].checks[-1]
        assert r["termination"] == 0 and f[-1] == 2 and df <= ft and not sn <= st, name
    assert one("ftol")[2]["iterations"] < one("plain")[2]["iterations"]
    _, o, r, f = one("maxrad")
    assert o["trace"][:, 1].max() == 1e-2 and (o["trace"][:, 1] == 1e-2).sum() >= 2  # radius = min(max_radius, ..)
    assert not M.same_bits(one("lmclip")[1]["trace"], one("plain")[1]["trace"])
    assert not M.same_bits(one("noscale")[1]["pose"], one("plain")[1]["pose"])
    assert (one("noscale")[1]["solver"].scale == 1.0).all() and (one("plain")[1]["solver"].scale < 1.0).all()


def test_the_edge_scenes_are_what_they_say(solved):
    pr, out = solved["border"]
    X, geo = pr["points"], M.SMALL
    _, _, _, _, u, v, vis = M.project(pr["cam"], M.IDENTITY, X, pr["z_min"], geo["w"], geo["h"])
    assert u[0] == 0.0 and u[1] == geo["w"] - 1.0 and v[2] == 0.0 and v[3] == geo["h"] - 1.0 and u[5] == 0.0 and v[5] == 0.0
    assert vis.tolist() == [True, False, True, False, True, True, False, False, False, True, True, True]
    assert X[6, 2] == pr["z_min"]  # q2 exactly at z_min: not visible
    assert out[0]["result"]["visible_start"] == 7
    for u_ in (1, 2):  # a NaN and an infinite pose entry: nothing visible, the zero Jacobian converges at once
        r = out[u_]["result"]
        assert (r["termination"], r["iterations"], r["visible_start"]) == (0, 0, 0) and r["initial_cost"] == len(X) / 2.0
        assert M.same_bits(out[u_]["pose"], pr["poses"][u_])
    pr, out = solved["visibility"]
    n = len(pr["points"])
    vs = [o["result"]["visible_start"] for o in out]
    assert vs[0] == n and n // 4 <= vs[1] <= 3 * n // 4 and vs[2] == 0
    assert (out[2]["result"]["termination"], out[2]["result"]["iterations"]) == (0, 0)
    pr, out = solved["degenerate"]
    term = [o["result"]["termination"] for o in out]
    its = [o["result"]["iterations"] for o in out]
    zero, const, spike, nan_far, nan_read, inf, neg = range(7)
    for i in (zero, inf, neg):  # E1: not solved, every field 0
        assert term[i] == 2 and all(out[i]["result"][k] == 0 for k in M.RESULT_INTS[1:] + M.RESULT_DOUBLES), i
        assert M.same_bits(out[i]["pose"], pr["poses"][i]) and not out[i]["trace"].any()
    assert (term[const], its[const]) == (0, 0) and out[const]["solver"].exit_checks[-1][0] == 0.0  # zero gradient
    assert out[const]["result"]["visible_start"] == len(pr["points"])
    assert its[spike] > 0 and its[nan_far] > 0 and term[nan_far] != 2
    assert term[nan_read] == 2 and math.isnan(out[nan_read]["result"]["initial_cost"]) and its[nan_read] == 0
    assert M.same_bits(out[nan_read]["pose"], pr["poses"][nan_read])
    assert out[nan_far]["result"]["scale"] == 1.0 / np.nanmax(pr["images"][nan_far])


# ---- 5. the device's text on the host ----------------------------------------------------------------------------------------

def build_serial(path, sanitize):
    cxx = os.environ.get("CXX", "c++")
    base = [cxx, "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas"]
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # a sanitized build that does not link fails the test: it never runs unsanitized under that name
    subprocess.check_call(base + (san if sanitize else ["-O2"]) + ["-o", path, SERIAL_SRC])
    return path


@pytest.mark.parametrize("sanitize", [False, True])
def test_the_devices_text_equals_the_restatement(tmp_path, solved, sanitize):
    """csrc/ebo_maptrack.inc compiled for the host, the lanes of a sum run one after the other: every double and integer
    of every scene of tests/test_gpu_map_track.py, and of a recovery scene with 13 starts, equals the restatement.  Once
    with -O2, once as a stand-alone program under the address and undefined-behaviour sanitizers: no report."""
    exe = build_serial(str(tmp_path / "map_track_serial"), sanitize)
    sc = M.recovery_scene(0, 0.10, 0.03)
    starts = M.starts13(sc["start"], 0.05, 0.015)
    rec = M.problem(sc["geo"], sc["image"][None], sc["points"], np.zeros(13, int), starts)
    cases = dict(solved)
    cases["recovery13"] = (rec, M.solve_units(rec))
    for name, (pr, want) in cases.items():
        M.write_problem(tmp_path / "p.f64", pr)
        out = subprocess.run([exe, str(tmp_path / "p.f64"), str(tmp_path / "r.f64"), "1"], capture_output=True, text=True, timeout=300)
        assert out.returncode == 0, (name, out.stderr[-2000:])
        got = M.read_result(tmp_path / "r.f64", len(pr["unit_image"]), pr["opts"]["max_num_iterations"])
        for u, (g, w) in enumerate(zip(got, want)):
            assert M.same_unit(g, w), (name, u, g["result"], w["result"])


def test_the_facade_compiles():
    """visual_odometry::MapTracker, tools::EvaluatorParams::trackMap and track_recording --track-map compile under -Wall
    -Wextra (syntax only; tests/test_gpu_map_track_facade.py builds and runs the tool)."""
    src = os.path.join(ROOT, "event-based-odomety_amd", "tools", "track_recording.cpp")
    out = subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "warning" not in out.stderr, out.stderr[-2000:]
    text = open(src).read()
    assert "--track-map" in text and "--map-until" in text and "--track-starts" in text
    hdr = open(os.path.join(ROOT, "event-based-odomety_amd", "include", "visual_odometry", "map_tracker.h")).read()
    assert "class MapTracker" in hdr and "trackResidentWindows" in hdr


# ---- 6. the interface ---------------------------------------------------------------------------------------------------------

def test_the_defaults_and_the_bindings(ebo):
    o = ebo.default_map_track_opts()
    assert {k: getattr(o, k) for k in M.OPT_FIELDS} == M.default_opts()
    assert ebo.default_map_track_opts(max_num_iterations=7).max_num_iterations == 7
    assert all(hasattr(ebo.Context, n) for n in ("map_track", "map_track_device", "map_track_resident", "event_images",
                                                 "event_images_device"))
    assert hasattr(ebo, "map_track_starts")
    assert [f for f, _ in ebo.MapTrackResult._fields_][:6] == ["termination", "iterations", "num_evals_jac", "num_evals_cost",
                                                              "visible_start", "visible_final"]
    import ctypes
    assert ctypes.sizeof(ebo.MapTrackResult) == 64
