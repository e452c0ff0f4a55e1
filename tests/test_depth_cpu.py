"""CPU: the space-sweep depth map's rules (include/ebo.h M1-M9) through tests/depth_ref.py: the restatement against a
brute-force triple loop, the recovery of a known scene by the restatement alone, and the device's rule functions
compiled for the host (tools/dsi_serial.cpp), also under the address and undefined-behaviour sanitizers.  No GPU."""
import math
import os
import subprocess

import numpy as np
import pytest

import depth_ref as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SERIAL_SRC = os.path.join(ROOT, "event-based-odomety_amd", "tools", "dsi_serial.cpp")


# ---- 1. the restatement against brute force ------------------------------------------------------

def brute_volume(windows, poses, ref, cam, w, h, z):
    """M2-M4 event by event and plane by plane on Python floats (IEEE doubles, one rounding per operation)."""
    fx, fy, cx, cy = [float(v) for v in cam]
    H = [[[0] * w for _ in range(h)] for _ in z]
    for ev, po in zip(windows, poses):
        Rf, tf = [float(v) for v in ref[:9]], [float(v) for v in ref[9:]]
        Rw, tw = [float(v) for v in po[:9]], [float(v) for v in po[9:]]
        Rr = [[(Rf[i] * Rw[j] + Rf[3 + i] * Rw[3 + j]) + Rf[6 + i] * Rw[6 + j] for j in range(3)] for i in range(3)]
        e = [tw[i] - tf[i] for i in range(3)]
        tr = [(Rf[i] * e[0] + Rf[3 + i] * e[1]) + Rf[6 + i] * e[2] for i in range(3)]
        for rec in ev:
            x, y = int(rec["x"]), int(rec["y"])
            if not (0 <= x < w and 0 <= y < h):
                continue
            a = (float(x) - cx) / fx
            b = (float(y) - cy) / fy
            d = [(Rr[i][0] * a + Rr[i][1] * b) + Rr[i][2] for i in range(3)]
            for k, zk in enumerate(z):
                zk = float(zk)
                if d[2] == 0.0:
                    continue  # lam would be infinite or NaN: u is not finite, no vote
                lam = (zk - tr[2]) / d[2]
                if not lam > 0.0:
                    continue
                X = tr[0] + lam * d[0]
                Y = tr[1] + lam * d[1]
                u = fx * (X / zk) + cx
                v = fy * (Y / zk) + cy
                if not (u > -1.0 and u < float(w) and v > -1.0 and v < float(h)):
                    continue
                x0, y0 = math.floor(u), math.floor(v)
                al, be = u - x0, v - y0
                ial, ibe = 1.0 - al, 1.0 - be
                for dx, dy, wt in ((0, 0, ial * ibe), (1, 0, al * ibe), (0, 1, ial * be), (1, 1, al * be)):
                    q = round(wt * 1024.0)  # Python's round: ties to even
                    if 0 <= x0 + dx < w and 0 <= y0 + dy < h:
                        H[k][y0 + dy][x0 + dx] += q
    return np.array(H, dtype=np.uint32)


def brute_extract(H, z, cam, r, min_excess, m):
    nz, h, w = H.shape
    fx, fy, cx, cy = [float(v) for v in cam]
    conf = [[0] * w for _ in range(h)]
    kbest = [[0] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            for k in range(nz):
                if int(H[k, y, x]) > conf[y][x]:
                    conf[y][x], kbest[y][x] = int(H[k, y, x]), k
    off = round(min(float(min_excess), 4194304.0) * 1024.0)
    keep = [[False] * w for _ in range(h)]
    for y in range(h):
        for x in range(w):
            S = cnt = 0
            for yy in range(y - r, y + r + 1):
                for xx in range(x - r, x + r + 1):
                    if 0 <= yy < h and 0 <= xx < w:
                        S += conf[yy][xx]
                        cnt += 1
            keep[y][x] = conf[y][x] > 0 and conf[y][x] * cnt > S + off * cnt
    index = np.full((h, w), -1, dtype=np.int32)
    depth = np.zeros((h, w))
    points = []
    for y in range(h):
        for x in range(w):
            if not keep[y][x]:
                continue
            k = kbest[y][x]
            if m > 0:
                box = sorted(kbest[yy][xx] for yy in range(y - m, y + m + 1) for xx in range(x - m, x + m + 1)
                             if 0 <= yy < h and 0 <= xx < w and keep[yy][xx])
                k = box[(len(box) - 1) // 2]
            index[y, x] = k
            depth[y, x] = float(z[k])
            a = (float(x) - cx) / fx
            b = (float(y) - cy) / fy
            points.append((a * float(z[k]), b * float(z[k]), float(z[k])))
    return index, np.array(conf, dtype=np.uint32), depth, np.array(points).reshape(-1, 3)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def test_the_restatement_equals_the_brute_force_loops():
    """9 x 7 sensor, Nz = 3: four windows under a translation, a rotation, a camera beyond the near plane and a NaN
    pose, strays among the events; then the extraction at three (r, m) pairs."""
    w, h, cam = 9, 7, (7.0, 7.5, 4.0, 3.25)
    z = D.planes(3, 1.0, 4.0)
    assert z[0] == 1.0 and abs(z[2] - 4.0) < 1e-15 and z[1] == 1.0 / (1.0 + 1.0 * ((1.0 / 4.0 - 1.0) / 2.0))
    ref = D.pose(D.rot(2, 4.0), (0.02, 0.0, -0.01))
    poses = [D.pose(t=(0.3, -0.1, 0.05)), D.pose(D.rot(1, 5.0) @ D.rot(0, -3.0), (-0.2, 0.1, 0.0)), D.pose(t=(0.0, 0.0, 1.7)),
             D.pose(t=(float("nan"), 0.0, 0.0)), ref]
    wins = [D.random_window(30 + i, 60, w, h, strays=5) for i in range(len(poses))]
    Hq = D.volume(wins, poses, ref, cam, w, h, z)
    assert np.array_equal(Hq, brute_volume(wins, poses, ref, cam, w, h, z))
    assert Hq.any() and not D.volume(wins[3:4], poses[3:4], ref, cam, w, h, z).any()
    # the window at the reference pose alone: every plane is 1024 x its count image
    count = np.zeros((h, w), dtype=np.int64)
    keep = D.in_sensor(wins[4], w, h)
    np.add.at(count, (wins[4]["y"][keep], wins[4]["x"][keep]), 1)
    own = D.volume(wins[4:], poses[4:], ref, cam, w, h, z)
    assert all(np.array_equal(own[k], count * 1024) for k in range(3))
    for r, m, excess in ((0, 0, 0.0), (1, 1, 0.25), (2, 2, 0.0), (7, 7, 0.1)):
        got = D.extract(Hq, z, cam, r, excess, m)
        want = brute_extract(Hq, z, cam, r, excess, m)
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1]), (r, m)
        assert same_bits(got[2], want[2]) and same_bits(got[3], want[3]), (r, m)
        assert r == 0 or (got[0] >= 0).any()
    # r = 0: the box is the pixel itself and nothing exceeds its own mean
    assert not (D.extract(Hq, z, cam, 0, 0.0, 0)[0] >= 0).any()
    # an argmax tie goes to the nearer plane; an empty volume keeps nothing
    tie = np.zeros((3, h, w), dtype=np.uint32)
    tie[1, 3, 4] = tie[2, 3, 4] = 5000
    assert D.extract(tie, z, cam, 1, 0.0, 0)[0][3, 4] == 1
    empty = D.extract(np.zeros((3, h, w), dtype=np.uint32), z, cam)
    assert not (empty[0] >= 0).any() and not empty[1].any() and not empty[2].any() and empty[3].shape == (0, 3)
    assert D.offset(3.0) == 3072 and D.offset(1e300) == 1 << 32


# ---- 2. recovery of a known scene ----------------------------------------------------------------

@pytest.mark.parametrize("two_depths", [False, True])
@pytest.mark.parametrize("seed", D.SCENE_SEEDS)
def test_the_restatement_recovers_the_scene(seed, two_depths):
    """40 points at Z = 2 (or half of them at Z = 4) seen from nine poses along x: at least 36 points have their rounded
    reference pixel kept within one plane of the truth, and at least 95 % of the kept pixels lie within 1.5 px and one
    plane of a point.  The figures of every (seed, variant) are printed."""
    p = D.SCENE_PARAMS
    wins, poses, ref, pts = D.recovery_scene(seed, two_depths)
    z = D.planes(p["nz"], p["z_near"], p["z_far"])
    Hq = D.volume(wins, poses, ref, D.SCENE["cam"], D.SCENE["w"], D.SCENE["h"], z)
    index, conf, depth, points = D.extract(Hq, z, D.SCENE["cam"], p["box_radius"], p["min_excess"], p["median_radius"])
    kept, off, recovered = D.recovery_figures(index, pts)
    print("seed %d two_depths %d: kept %d, off %d, recovered %d of 40" % (seed, two_depths, kept, off, recovered))
    D.check_recovery(index, pts)
    assert len(points) == kept and np.array_equal(points[:, 2], depth[index >= 0])


# ---- 3. the device's rule functions on the host ----------------------------------------------------

def build_serial(path, sanitize):
    cxx = os.environ.get("CXX", "c++")
    base = [cxx, "-std=c++17", "-ffp-contract=off", "-Wno-unknown-pragmas"]
    san = ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    # a sanitized build that does not link fails the test: it never runs unsanitized under that name
    subprocess.check_call(base + (san if sanitize else ["-O2"]) + ["-o", path, SERIAL_SRC])
    return path


def run_serial(exe, tmp_path, ev, Rr, tr, cam, w, h, z):
    keep = D.in_sensor(ev, w, h)
    rows = np.stack([ev["x"][keep], ev["y"][keep]], axis=1).astype(np.float64)
    head = np.concatenate([[w, h, *cam, len(z)], z, Rr.reshape(9), tr, [len(rows)]]).astype(np.float64)
    np.concatenate([head, rows.reshape(-1)]).tofile(tmp_path / "p.f64")
    out = subprocess.run([exe, str(tmp_path / "p.f64"), str(tmp_path / "r.f64")], capture_output=True, text=True, timeout=120)
    assert out.returncode == 0, out.stderr
    res = np.fromfile(tmp_path / "r.f64")
    return res[:-1].reshape(len(z), h, w).astype(np.uint32), int(res[-1])


@pytest.mark.parametrize("sanitize", [False, True])
def test_the_device_text_on_the_host(tmp_path, sanitize):
    """csrc/ebo_depth.inc's dsi_ray, dsi_uv, dsi_tap and dsi_weights, compiled for the host and run event by event and
    plane by plane over the GPU test's cases -- both sensors, every pose of depth_ref.POSES (a NaN and two infinities
    among them), Nz 2, 5 and 32, the border window (x0 = -1, x0 = w - 1, y0 = -1, y0 = h - 1), 5000 events on one pixel:
    H is the restatement's bit for bit.  Once plain, once under the address and undefined-behaviour sanitizers: no
    report.  This covers the rule functions only; the kernel's tile and flush indexing is covered by
    tests/test_gpu_depth.py."""
    exe = build_serial(str(tmp_path / "dsi_serial"), sanitize)
    for gname, geo in D.GEOS.items():
        w, h, cam = geo["w"], geo["h"], geo["cam"]
        seen = {}
        for i, (pname, po) in enumerate(D.POSES.items()):
            nz = D.NZS[i % 3] if sanitize else 32
            z = D.planes(nz, *D.Z_RANGE)
            Rr, tr = D.relative_pose(D.REF_POSE, po)
            for ev in D.case_windows(gname)[:4]:
                want = D.volume([ev], [po], D.REF_POSE, cam, w, h, z, seen=seen)
                got, voted = run_serial(exe, tmp_path, ev, Rr, tr, cam, w, h, z)
                assert np.array_equal(got, want), (gname, pname)
                assert (voted > 0) == bool(want.any()), (gname, pname)
                assert not (pname in D.NO_VOTE and want.any()), pname
        assert {-1, w - 1} <= seen["x0"] and {-1, h - 1} <= seen["y0"], gname
    Rr, tr = D.relative_pose(D.REF_POSE, D.POSES["tz_near"])
    z = D.planes(32, *D.Z_RANGE)
    some = [bool(D.project([5], [5], Rr, tr, D.SMALL["cam"], 37, 29, zk)[0][0]) for zk in z]
    assert not some[0] and some[-1]  # lam <= 0 on the near planes only


def test_the_facade_compiles():
    """visual_odometry::DepthMapper, tools::EvaluatorParams::depthMap and track_recording --depth-map compile under
    -Wall -Wextra (syntax only: nothing is written; tests/test_gpu_depth_facade.py builds and runs the tool)."""
    src = os.path.join(ROOT, "event-based-odomety_amd", "tools", "track_recording.cpp")
    out = subprocess.run([os.environ.get("CXX", "c++"), "-std=c++17", "-Wall", "-Wextra", "-fsyntax-only", src], capture_output=True, text=True)
    assert out.returncode == 0, out.stderr[-2000:]
    assert "warning" not in out.stderr, out.stderr[-2000:]
    assert "--depth-map" in open(src).read()


def test_the_defaults_and_the_bindings(ebo):
    p = ebo.default_depth_params()
    assert (p.nz, p.z_near, p.z_far, p.box_radius, p.min_excess, p.median_radius) == (64, 0.5, 8.0, 2, 3.0, 2)
    assert {k: getattr(p, k) for k in D.DEFAULTS} == D.DEFAULTS
    assert ebo.default_depth_params(nz=5, median_radius=0).nz == 5
    with pytest.raises(AttributeError):
        ebo.default_depth_params(planes=3)
    assert all(hasattr(ebo.Context, n) for n in ("dsi_begin", "dsi_add_windows", "dsi_volume", "dsi_depth", "dsi_end"))


# ---- the launch shapes of tests/test_gpu_depth_shapes.py -------------------------------------------

def test_the_shape_cases_reach_every_tile_outcome():
    """dsi_tile has five outcomes (depth_ref.tile_of restates it).  Over (unit, plane, pose), the older cases
    (depth_ref.POSES on both sensors, 32 planes) find four of them; the cases of tests/test_gpu_depth_shapes.py find all
    five, rounds of four planes where a tile and a non-tile outcome meet, and the not-finite corner in a view that votes."""
    seen = set()
    for gname, geo in D.GEOS.items():
        c = D.tile_census(geo, 32, sorted(D.POSES))
        print("older cases", gname, c["count"], "mixed rounds", c["mixed"])
        seen |= {o for o, n in c["count"].items() if n}
    assert seen == {"tile", "lam", "off", "large"}
    total = {o: 0 for o in D.OUTCOMES}
    lists = [("small", D.SMALL, nz) for nz in D.PLANE_COUNTS] + [("medium", D.MEDIUM, 32), ("big_patch", D.BIG_PATCH, 32)]
    for gname, geo, nz in lists:
        c = D.tile_census(geo, nz, D.SHAPE_POSES)
        print(gname, nz, c["count"], "mixed rounds", c["mixed"])
        for o, n in c["count"].items():
            total[o] += n
        if gname == "small":
            # a workgroup that walks every plane, and the shipped split of a single window on 256 CUs
            split = D.planes_per_group(256, len(D.rects(geo)), nz)
            few = D.tile_census(geo, nz, D.SHAPE_POSES, split)["mixed"]
            print(gname, nz, "mixed rounds at %d planes a workgroup: %d" % (split, few))
            assert split == 3 and c["mixed"] >= 1 and few >= 1
        if gname == "medium":
            assert all(c["count"][o] for o in D.OUTCOMES) and c["mixed"] >= 1 and c["poses"]["far"] == {"ry90"}
        if gname == "big_patch":
            assert c["count"]["far"] and c["count"]["large"] > c["count"]["tile"]
            plain = D.tile_census(geo, nz, ("rz5", "ry5"))["count"]
            assert plain["large"] == 2 * len(D.rects(geo)) * nz  # these views vote by global atomics alone
    print("the shape cases:", total)
    assert all(total[o] for o in D.OUTCOMES)
    # the near-90-degree view votes: on 64 x 48 beside the not-finite corner at x == cx, on 37 x 29 with d2 changing sign
    # inside the patches of the third column
    z = D.planes_table(32)
    for gname in ("small", "medium"):
        geo = D.GEOS[gname]
        own = D.volume(D.shape_windows(gname)[5:], [D.SHAPE_POSE_TABLE["ry90"]], D.REF_POSE, geo["cam"], geo["w"], geo["h"], z)
        print(gname, "ry90 alone: %d votes of 1024" % (int(own.astype(np.int64).sum()) >> 10))
        assert own.any()
    Rr, _ = D.relative_pose(D.REF_POSE, D.SHAPE_POSE_TABLE["ry90"])
    fx, _, cx, _ = D.SMALL["cam"]
    d2 = [(Rr[2, 0] * ((float(x) - cx) / fx) + Rr[2, 1] * 0.0) + Rr[2, 2] for x in range(16, 24)]
    assert min(d2) < 0.0 < max(d2) and D.rects(D.SMALL)[2] == (16, 0, 8, 8)
    # 37 x 29 in 4 x 4 patches: 17 windows fill a 256-CU device four times over, so one workgroup walks every plane
    assert len(D.rects(D.FINE)) == 63 and [D.planes_per_group(256, 63 * 17, nz) for nz in D.PLANE_COUNTS] == list(D.PLANE_COUNTS)
    assert D.tile_census(D.FINE, 7, D.SHAPE_POSES)["mixed"] >= 1
    # the scan sensors: 255, 256, 257 and 352 workgroups of 256 pixels
    assert [(g["w"] * g["h"] + 255) // 256 for g in D.SCAN_GEOS.values()] == [255, 256, 257, 352]
    assert all(g["w"] - g["hole_x"] < 256 for g in D.SCAN_GEOS.values())
