"""GPU: ebo_dsi_begin / _add_windows / _volume / _depth / _end against tests/depth_ref.py (include/ebo.h, rules M1-M9).
Every output is bit-equal to the restatement.  Sensors 37 x 29 (remainder patches) and 64 x 48; Nz 2, 5 and 32; windows
of 1, 300 and 5000 events, 5000 events on one pixel, the four borders (x0 = -1, x0 = w - 1), strays; the poses of
depth_ref.POSES (identity, translations along each axis, tz beyond the near planes and beyond all of them, a camera
behind the volume, 5 degrees about each axis, a NaN and infinities).  With every pose the reference pose each plane is
1024 x ebo_count_image.  The volume does not depend on use masks, the split into calls and loads, the order of a batch,
the planes a workgroup walks or the vote's form (LDS tile against plain global atomics, A/B library); the 2^21 cap
refuses and leaves the volume as it was.  The extraction at r and m of 0, 2 and 7, with argmax ties, an empty volume and
max_points below the count; the recovery scene of tests/test_depth_cpu.py with the same assertions."""
import ctypes as C

import numpy as np
import pytest

import depth_ref as D

pytestmark = pytest.mark.gpu


def context(ebo, geo, n_windows=1, max_events=1 << 17):
    return ebo.Context(loss=ebo.LOSS_VARIANCE, image_w=geo["w"], image_h=geo["h"], patch_w=geo["patch_w"], patch_h=geo["patch_h"],
                       max_windows=max(n_windows, 1), max_events=max_events)


def load(c, wins):
    offsets = np.concatenate([[0], np.cumsum([len(v) for v in wins])])
    c.set_windows(np.concatenate(wins), offsets)


def params(ebo, nz, **kw):
    return ebo.default_depth_params(nz=nz, z_near=D.Z_RANGE[0], z_far=D.Z_RANGE[1], **kw)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def reference(geo, wins, poses, nz, use=None):
    return D.volume(wins, poses, D.REF_POSE, geo["cam"], geo["w"], geo["h"], D.planes(nz, *D.Z_RANGE), use)


def voted(ebo, geo, wins, poses, nz, use=None, lib=None):
    with context(lib or ebo, geo, len(wins)) as c:
        load(c, wins)
        c.dsi_begin(geo["cam"], D.REF_POSE, params(lib or ebo, nz))
        c.dsi_add_windows(poses, use)
        Hq = c.dsi_volume()
        c.dsi_end()
    return Hq


# ---- the volume ----------------------------------------------------------------------------------

@pytest.mark.parametrize("pname", sorted(D.POSES))
@pytest.mark.parametrize("nz", D.NZS)
@pytest.mark.parametrize("gname", sorted(D.GEOS))
def test_the_volume_equals_the_restatement(ebo, gname, nz, pname):
    geo, wins = D.GEOS[gname], D.case_windows(gname)
    poses = [D.POSES[pname]] * len(wins)
    want = reference(geo, wins, poses, nz)
    with context(ebo, geo, len(wins)) as c:
        load(c, wins)
        c.dsi_begin(geo["cam"], D.REF_POSE, params(ebo, nz))
        c.dsi_add_windows(poses)
        Hq = c.dsi_volume()
        count = c.count_image(ebo.COUNT_INTEGRATED)
        c.dsi_end()
    assert Hq.dtype == np.uint32 and Hq.shape == want.shape
    assert np.array_equal(Hq, want), (gname, nz, pname, np.argwhere(Hq != want)[:5])
    assert want.any() != (pname in D.NO_VOTE)
    if pname == "reference":
        # an independent pin: no warp at all, every plane is 1024 x the un-warped count image of the same windows
        total = count.sum(axis=0)
        assert total.sum() == D.counted_events(wins, geo["w"], geo["h"])
        for k in range(nz):
            assert np.array_equal(Hq[k].astype(np.float64), 1024.0 * total), k


def test_use_masks_calls_loads_and_order_do_not_change_the_volume(ebo):
    """One call against a use mask and its complement, against window-by-window calls, against two loads of half the
    windows each, and against the reversed batch."""
    geo, nz, n = D.SMALL, 5, 9
    wins, poses = D.batch(n)
    want = reference(geo, wins, poses, nz)
    mask = np.array([i % 3 != 1 for i in range(n)], dtype=np.uint8)
    with context(ebo, geo, n) as c:
        prm = params(ebo, nz)
        load(c, wins)
        c.dsi_begin(geo["cam"], D.REF_POSE, prm)
        c.dsi_add_windows(poses)
        assert np.array_equal(c.dsi_volume(), want)
        c.dsi_begin(geo["cam"], D.REF_POSE, prm)  # a begin while open starts over
        assert not c.dsi_volume().any()
        c.dsi_add_windows(poses, mask)
        assert np.array_equal(c.dsi_volume(), reference(geo, wins, poses, nz, mask))
        c.dsi_add_windows(poses, 1 - mask)
        assert np.array_equal(c.dsi_volume(), want)
        c.dsi_add_windows(poses, np.zeros(n, dtype=np.uint8))  # nothing used: nothing changes
        assert np.array_equal(c.dsi_volume(), want)
        c.dsi_begin(geo["cam"], D.REF_POSE, prm)
        for i in range(n):
            c.dsi_add_windows(poses, np.eye(n, dtype=np.uint8)[i])
        assert np.array_equal(c.dsi_volume(), want)
        c.dsi_begin(geo["cam"], D.REF_POSE, prm)
        load(c, wins[:4])
        c.dsi_add_windows(poses[:4])
        load(c, wins[4:])
        c.dsi_add_windows(poses[4:])
        assert np.array_equal(c.dsi_volume(), want)
        c.dsi_begin(geo["cam"], D.REF_POSE, prm)
        load(c, wins[::-1])
        c.dsi_add_windows(poses[::-1])
        assert np.array_equal(c.dsi_volume(), want)
        c.dsi_end()


def test_more_windows_than_a_launch_takes(ebo):
    """70 windows are more than one launch's 64; 70 x 12 (patch, window) pairs fill the device, so a workgroup walks
    every plane, where the single windows of the other tests are dealt a plane or a few each."""
    geo, nz, n = D.SMALL, 5, 70
    wins, poses = D.batch(n)
    assert np.array_equal(voted(ebo, geo, wins, poses, nz), reference(geo, wins, poses, nz))


@pytest.mark.parametrize("gname", sorted(D.GEOS))
def test_the_plain_vote_and_every_plane_split_give_the_same_bits(ebo_ab, monkeypatch, gname):
    """The A/B build's EBO_DSI_TILE=0 sends every tap to the volume through a global atomic, where the tile form
    accumulates a (patch, plane)'s surroundings in LDS first; EBO_DSI_PLANES fixes the planes a workgroup walks."""
    geo, nz = D.GEOS[gname], 32
    wins = D.case_windows(gname)
    names = ("rz5", "tz_near", "behind", "tx", "ry5")
    poses = [D.POSES[n] for n in names]
    want = reference(geo, wins, poses, nz)
    for tile, planes in (("1", "0"), ("0", "0"), ("1", "1"), ("1", "7"), ("1", "32"), ("0", "32")):
        monkeypatch.setenv("EBO_DSI_TILE", tile)
        monkeypatch.setenv("EBO_DSI_PLANES", planes)
        assert np.array_equal(voted(ebo_ab, geo, wins, poses, nz, lib=ebo_ab), want), (tile, planes)


def test_the_cap_refuses_and_leaves_the_volume_as_it_was(ebo):
    """2^20 events a call: two calls fill the volume to its 2^21 events, half of them on one pixel at the reference
    pose, whose voxels then hold 2^30; a third call is refused with EBO_ERR_RANGE and changes nothing."""
    geo, nz, n = D.SMALL, 2, 1 << 20
    w, h = geo["w"], geo["h"]
    rng = np.random.default_rng(77)
    x = np.concatenate([np.full(n // 2, 11), rng.integers(0, w, n // 2)])
    y = np.concatenate([np.full(n // 2, 7), rng.integers(0, h, n // 2)])
    wins, poses = [D.events(x, y)], [D.REF_POSE]
    one = reference(geo, wins, poses, nz).astype(np.int64)
    assert one[0, 7, 11] >= 1 << 29
    with context(ebo, geo, 1, max_events=n + 64) as c:
        load(c, wins)
        c.dsi_begin(geo["cam"], D.REF_POSE, params(ebo, nz))
        c.dsi_add_windows(poses)
        assert np.array_equal(c.dsi_volume(), one)
        c.dsi_add_windows(poses)
        full = c.dsi_volume()
        assert np.array_equal(full, 2 * one) and full[0, 7, 11] >= 1 << 30
        with pytest.raises(ebo.EboError) as e:
            c.dsi_add_windows(poses)
        assert e.value.code == ebo.ERR_RANGE
        assert np.array_equal(c.dsi_volume(), full)
        c.dsi_add_windows(poses, [0])  # a call that votes nothing is within the cap
        load(c, [D.events([3], [4])])
        with pytest.raises(ebo.EboError) as e:
            c.dsi_add_windows(poses)  # one event too many
        assert e.value.code == ebo.ERR_RANGE
        assert np.array_equal(c.dsi_volume(), full)
        c.dsi_end()


# ---- the extraction ------------------------------------------------------------------------------

def check_extraction(got, want, max_points=None):
    index, conf, depth, points, n = got
    assert index.dtype == np.int32 and conf.dtype == np.uint32
    assert np.array_equal(index, want[0]) and np.array_equal(conf, want[1])
    assert same_bits(depth, want[2])
    assert n == len(want[3])
    assert same_bits(points, want[3] if max_points is None else want[3][:max_points])


@pytest.mark.parametrize("m", [0, 2, 7])
@pytest.mark.parametrize("r", [0, 2, 7])
def test_the_extraction_equals_the_restatement(ebo, r, m):
    """A dense volume (21 windows on 37 x 29, Nz = 5, a small excess) so that boxes and medians hold many pixels."""
    geo, nz = D.SMALL, 5
    wins, poses = D.batch(21)
    z = D.planes(nz, *D.Z_RANGE)
    with context(ebo, geo, len(wins)) as c:
        load(c, wins)
        c.dsi_begin(geo["cam"], D.REF_POSE, params(ebo, nz, box_radius=r, median_radius=m, min_excess=0.125))
        c.dsi_add_windows(poses)
        Hq = c.dsi_volume()
        got = c.dsi_depth()
        few = c.dsi_depth(max_points=3)
        none = c.dsi_depth(max_points=0)
        c.dsi_end()
    want = D.extract(Hq, z, geo["cam"], r, 0.125, m)
    print("r %d m %d: kept %d" % (r, m, got[4]))
    check_extraction(got, want)
    check_extraction(few, want, 3)
    check_extraction(none, want, 0)
    assert (r == 0) == (got[4] == 0)
    assert r == 0 or got[4] > 20


def test_argmax_ties_and_an_empty_volume(ebo):
    """At the reference pose every plane holds the same votes: the nearest plane wins every pixel.  A volume nobody
    voted in keeps nothing."""
    geo, nz = D.MEDIUM, 5
    wins = D.case_windows("medium")[1:2]
    z = D.planes(nz, *D.Z_RANGE)
    with context(ebo, geo, 1) as c:
        load(c, wins)
        c.dsi_begin(geo["cam"], D.REF_POSE, params(ebo, nz, min_excess=0.0))
        index, conf, depth, points, n = c.dsi_depth()
        assert n == 0 and np.all(index == -1) and not conf.any() and not depth.any() and points.shape == (0, 3)
        c.dsi_add_windows([D.REF_POSE])
        Hq = c.dsi_volume()
        got = c.dsi_depth()
        c.dsi_end()
    check_extraction(got, D.extract(Hq, z, geo["cam"], 2, 0.0, 2))
    assert got[4] > 0 and np.all(got[0][got[0] >= 0] == 0) and np.all(got[3][:, 2] == z[0])


@pytest.mark.parametrize("two_depths", [False, True])
def test_the_recovery_scene(ebo, two_depths):
    """The scene of tests/test_depth_cpu.py, seeds 0-3: the device's maps are the restatement's and meet the same two
    conditions."""
    p = D.SCENE_PARAMS
    z = D.planes(p["nz"], p["z_near"], p["z_far"])
    for seed in D.SCENE_SEEDS:
        wins, poses, ref, pts = D.recovery_scene(seed, two_depths)
        with context(ebo, D.SCENE, len(wins)) as c:
            load(c, wins)
            c.dsi_begin(D.SCENE["cam"], ref, ebo.default_depth_params(**p))
            c.dsi_add_windows(poses)
            Hq = c.dsi_volume()
            got = c.dsi_depth()
            c.dsi_end()
        assert np.array_equal(Hq, D.volume(wins, poses, ref, D.SCENE["cam"], D.SCENE["w"], D.SCENE["h"], z))
        check_extraction(got, D.extract(Hq, z, D.SCENE["cam"], p["box_radius"], p["min_excess"], p["median_radius"]))
        print(seed, two_depths, D.check_recovery(got[0], pts))


# ---- errors --------------------------------------------------------------------------------------

def test_argument_and_state_errors(ebo):
    import torch  # device buffers for the recording check below
    geo = D.SMALL
    lib = ebo.lib()
    k = ebo.camera(geo["cam"] + (0.0,) * 5)
    ref = np.ascontiguousarray(D.REF_POSE)
    poses = np.ascontiguousarray(D.REF_POSE).reshape(1, 12)
    out = np.zeros((64, geo["h"], geo["w"]), dtype=np.uint32)
    n = C.c_int(0)
    pts = np.zeros((8, 3))

    def code(call):
        with pytest.raises(ebo.EboError) as e:
            call()
        return e.value.code

    def four_without_a_volume(c):
        return [lib.ebo_dsi_add_windows(c._h, poses.ctypes.data, None), lib.ebo_dsi_volume(c._h, out.ctypes.data),
                lib.ebo_dsi_depth(c._h, None, None, None, None, 0, C.byref(n)), lib.ebo_dsi_end(c._h)]

    with context(ebo, geo) as c:
        assert four_without_a_volume(c) == [ebo.ERR_STATE] * 4
        # begin may come before the first load; add_windows needs windows
        c.dsi_begin(geo["cam"], ref)
        assert c._dsi_prm.nz == 64
        assert lib.ebo_dsi_add_windows(c._h, poses.ctypes.data, None) == ebo.ERR_STATE
        load(c, [D.random_window(1, 50, geo["w"], geo["h"])])
        c.dsi_add_windows(poses)
        for bad in (dict(nz=1), dict(nz=257), dict(z_near=0.0), dict(z_near=-1.0), dict(z_near=float("nan")), dict(z_far=float("inf")),
                    dict(z_near=8.0), dict(z_near=9.0), dict(z_far=float("nan")), dict(box_radius=-1), dict(box_radius=8),
                    dict(median_radius=-1), dict(median_radius=8), dict(min_excess=-0.5), dict(min_excess=float("nan")),
                    dict(min_excess=float("inf"))):
            assert code(lambda: c.dsi_begin(geo["cam"], ref, ebo.default_depth_params(**bad))) == ebo.ERR_ARG, bad
        for dist in ("k1", "k2", "p1", "p2"):
            cam = ebo.camera(geo["cam"] + (0.0,) * 5)
            setattr(cam, dist, 1e-3)
            assert code(lambda: c.dsi_begin(cam, ref)) == ebo.ERR_ARG, dist
        for field, v in (("fx", 0.0), ("fy", 0.0), ("fx", float("nan")), ("fy", float("inf"))):
            cam = ebo.camera(geo["cam"] + (0.0,) * 5)
            setattr(cam, field, v)
            assert code(lambda: c.dsi_begin(cam, ref)) == ebo.ERR_RANGE, field
        assert lib.ebo_dsi_begin(c._h, None, ref.ctypes.data, None) == ebo.ERR_ARG
        assert lib.ebo_dsi_begin(c._h, C.addressof(k), None, None) == ebo.ERR_ARG
        assert lib.ebo_dsi_begin(None, C.addressof(k), ref.ctypes.data, None) == ebo.ERR_ARG
        # a refused begin leaves the open volume as it was
        assert c.dsi_volume().any()
        assert lib.ebo_dsi_add_windows(c._h, None, None) == ebo.ERR_ARG
        assert lib.ebo_dsi_volume(c._h, None) == ebo.ERR_ARG
        assert lib.ebo_dsi_depth(c._h, None, None, None, None, -1, None) == ebo.ERR_ARG
        assert lib.ebo_dsi_depth(c._h, None, None, None, None, 4, None) == ebo.ERR_ARG
        for call in (lib.ebo_dsi_end, ):
            assert call(None) == ebo.ERR_ARG
        # every output of the extraction may be null; a null params is the defaults
        assert lib.ebo_dsi_depth(c._h, None, None, None, None, 0, None) == 0
        assert lib.ebo_dsi_depth(c._h, None, None, None, pts.ctypes.data, 8, C.byref(n)) == 0
        assert lib.ebo_dsi_begin(c._h, C.addressof(k), ref.ctypes.data, None) == 0
        assert lib.ebo_dsi_volume(c._h, out.ctypes.data) == 0 and not out.any()
        # refused while a graph is being recorded, recording and context intact
        d_flows = torch.zeros((c.P, 2), dtype=torch.float64, device="cuda")
        d_out = torch.zeros(3 * c.P, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())
        c.synchronize()
        codes = []

        def body():
            codes.append(lib.ebo_dsi_begin(c._h, C.addressof(k), ref.ctypes.data, None))
            codes.extend(four_without_a_volume(c))
            c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())

        g = c.record(body)
        assert codes == [ebo.ERR_STATE] * 5
        g.launch()
        c.synchronize()
        g.close()
        c.dsi_add_windows(poses)
        assert c.dsi_volume().any()
        # units loaded by ebo_set_patches are not windows
        ev = D.random_window(2, 40, geo["w"], geo["h"])
        c.set_patches(ev, [0, len(ev)], [[0, 0, 8, 8]])
        assert code(lambda: c.dsi_add_windows(poses)) == ebo.ERR_STATE
        c.dsi_end()
        assert four_without_a_volume(c) == [ebo.ERR_STATE] * 4
