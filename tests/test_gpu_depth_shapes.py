"""GPU: the depth kernels where the LAUNCH SHAPE picks the path (tests/test_gpu_depth.py covers the data); every output
is bit-equal to tests/depth_ref.py as there.
The point list's scan (k_dsi_count, k_dsi_scan, k_dsi_points) on sensors of 255, 256, 257 and 352 workgroups of 256
pixels, max_points cut at a workgroup's seam and either side of the count; 253, 255 and 256 planes, where a workgroup's
last round of four planes has dead waves, a single window is dealt 3 planes a workgroup and the median's bisection takes
8 steps; dsi_tile's five outcomes, among them the corner that maps beyond 1e6 in a view turned by 90 degrees, and a
geometry whose patches never fit a tile (tests/test_depth_cpu.py asserts that the cases hold them)."""
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


def reference(geo, wins, poses, nz):
    return D.volume(wins, poses, D.REF_POSE, geo["cam"], geo["w"], geo["h"], D.planes_table(nz))


def voted(lib, geo, wins, poses, nz):
    with context(lib, geo, len(wins)) as c:
        load(c, wins)
        c.dsi_begin(geo["cam"], D.REF_POSE, params(lib, nz))
        c.dsi_add_windows(poses)
        Hq = c.dsi_volume()
        c.dsi_end()
    return Hq


def check_extraction(got, want, max_points=None):
    index, conf, depth, points, n = got
    assert index.dtype == np.int32 and conf.dtype == np.uint32
    assert np.array_equal(index, want[0]) and np.array_equal(conf, want[1])
    assert same_bits(depth, want[2])
    assert n == len(want[3])
    assert same_bits(points, want[3] if max_points is None else want[3][:max_points])


def shape_poses():
    return [D.SHAPE_POSE_TABLE[n] for n in D.SHAPE_POSES]


# ---- the point list's scan -------------------------------------------------------------------------

@pytest.mark.parametrize("gname", sorted(D.SCAN_GEOS))
def test_the_point_list_on_sensors_of_many_workgroups(ebo, gname):
    """k_dsi_scan is one workgroup whose lane t takes ceil(nb / 256) consecutive block counts: nb = 255 and 256 (one
    entry a lane, the last lane idle or not), 257 (two entries, lanes 129.. idle) and 352.  Every block keeps pixels and
    some keep none in their last wave, so the offsets across blocks and the ranks across waves all matter; max_points
    ends the list inside the first block, at a block's seam, one past it, and either side of the count."""
    geo, nz = D.SCAN_GEOS[gname], D.SCAN_NZ
    wins = D.scan_windows(gname)
    poses = [D.SHAPE_POSE_TABLE[n] for n in D.SCAN_POSES]
    z = D.planes_table(nz)
    want_H = reference(geo, wins, poses, nz)
    nb = (geo["w"] * geo["h"] + D.BLOCK - 1) // D.BLOCK
    with context(ebo, geo, len(wins)) as c:
        load(c, wins)
        for r in ((2,), (2, 7))[nb == 352]:
            c.dsi_begin(geo["cam"], D.REF_POSE, params(ebo, nz, box_radius=r, median_radius=r, min_excess=D.SCAN_EXCESS))
            c.dsi_add_windows(poses)
            Hq = c.dsi_volume()
            assert np.array_equal(Hq, want_H), (gname, r)
            want = D.extract(want_H, z, geo["cam"], r, D.SCAN_EXCESS, r)
            per, last, off = D.block_census(want[0])
            kept = int(per.sum())
            print(gname, "r = m = %d: %d blocks, kept %d, fewest in a block %d, blocks with an empty last wave %d"
                  % (r, nb, kept, per.min(), (last == 0).sum()))
            assert len(per) == nb and per.min() > 0 and (last == 0).any() and kept == len(want[3])
            check_extraction(c.dsi_depth(), want)
            seam = int(off[nb // 2])
            assert 1 < seam < kept - 1
            for cap in (0, 1, seam, seam + 1, kept - 1, kept, kept + 5):
                check_extraction(c.dsi_depth(max_points=cap), want, cap)
        c.dsi_end()


# ---- the plane counts ------------------------------------------------------------------------------

@pytest.mark.parametrize("nz", D.PLANE_COUNTS)
def test_plane_counts_near_the_limit(ebo, nz):
    """253, 255 and 256 planes on 37 x 29.  One window at a time: 12 (patch, window) pairs, which the shipped build deals
    3 planes a workgroup, so wave 3 is never live.  70 windows: the launches of 64 and of 6 windows walk many planes a
    workgroup, and 253 and 255 leave dead waves in a last round.  The same sensor in 4 x 4 patches, 17 windows: 1071
    pairs, at which the shipped build hands one workgroup every plane.  The extraction's median bisects over nz planes."""
    import torch
    geo = D.SMALL
    z = D.planes_table(nz)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    split = [D.planes_per_group(cus, len(D.rects(geo)) * n, nz) for n in (1, 64, 6)]
    fine_split = D.planes_per_group(cus, len(D.rects(D.FINE)) * 17, nz)
    print("nz %d on %d CUs: planes a workgroup for 1, 64 and 6 windows: %s; in 4 x 4 patches for 17 windows: %d" % (nz, cus, split, fine_split))
    if 4 * cus <= len(D.rects(D.FINE)) * 17:  # up to 267 CUs the pairs alone fill the device four times over
        assert fine_split == nz
    if cus >= 256:  # an MI355X: 4 * 256 / 12 pairs gives 86 chunks of 3 planes; a smaller device deals more planes a chunk
        assert split[0] < D.WAVES
    wins = D.shape_windows("small")
    with context(ebo, geo, 70) as c:
        # rz5 and the 90-degree view take the spread windows, tx the 5000 events on one pixel, ry5 the single event
        for i, po, pname in zip((5, 1, 2, 3, 0, 4), shape_poses(), D.SHAPE_POSES):
            load(c, [wins[i]])
            c.dsi_begin(geo["cam"], D.REF_POSE, params(ebo, nz))
            c.dsi_add_windows([po])
            want = reference(geo, [wins[i]], [po], nz)
            assert np.array_equal(c.dsi_volume(), want), (nz, pname)
            assert want.any() or pname not in ("rz5", "tx", "ry90"), pname
        many, _ = D.batch(70)
        poses = [shape_poses()[i % len(D.SHAPE_POSES)] for i in range(70)]
        load(c, many)
        c.dsi_begin(geo["cam"], D.REF_POSE, params(ebo, nz, box_radius=2, median_radius=2, min_excess=D.SCAN_EXCESS))
        c.dsi_add_windows(poses)
        want = reference(geo, many, poses, nz)
        assert np.array_equal(c.dsi_volume(), want), nz
        got = c.dsi_depth()
        c.dsi_end()
    assert np.array_equal(voted(ebo, D.FINE, many[:17], poses[:17], nz), reference(D.FINE, many[:17], poses[:17], nz))
    ext = D.extract(want, z, geo["cam"], 2, D.SCAN_EXCESS, 2)
    used = np.unique(ext[0][ext[0] >= 0])
    print("nz %d: kept %d, %d different planes from %d to %d" % (nz, got[4], len(used), used.min(), used.max()))
    check_extraction(got, ext)
    assert got[4] > 100 and len(used) > 16 and used.max() > nz // 2


def test_at_255_planes_every_split_and_the_plain_vote_give_the_same_bits(ebo_ab, monkeypatch):
    """The A/B build's EBO_DSI_PLANES of 1, 3, 5 and 256 -- one live wave; three; a second round of one; every plane in
    one workgroup, whose last round has three -- with the LDS tile and with EBO_DSI_TILE=0's plain global atomics."""
    geo, nz = D.SMALL, 255
    wins, poses = D.shape_windows("small"), shape_poses()
    want = reference(geo, wins, poses, nz)
    assert want.any()
    for planes in ("1", "3", "5", "256"):
        for tile in ("0", "1"):
            monkeypatch.setenv("EBO_DSI_TILE", tile)
            monkeypatch.setenv("EBO_DSI_PLANES", planes)
            assert np.array_equal(voted(ebo_ab, geo, wins, poses, nz), want), (tile, planes)


# ---- the tile's outcomes ---------------------------------------------------------------------------

@pytest.mark.parametrize("gname", ["medium", "big_patch"])
def test_every_tile_outcome_votes_the_same_bits(ebo, ebo_ab, monkeypatch, gname):
    """64 x 48 with 16 x 16 patches under SHAPE_POSES meets all five outcomes of dsi_tile, the corner mapped beyond 1e6
    among them (the view turned by 90 degrees, whose other rays vote); with 32 x 32 patches hardly a box fits a tile and
    the shipped build votes mostly by global atomics.  The shipped build against the restatement, then the A/B build's
    tile against its plain vote."""
    geo = D.MEDIUM if gname == "medium" else D.BIG_PATCH
    nz = 32
    wins, poses = D.shape_windows("medium"), shape_poses()
    want = reference(geo, wins, poses, nz)
    assert np.array_equal(voted(ebo, geo, wins, poses, nz), want)
    alone = reference(geo, wins[5:], poses[5:], nz)
    assert alone.any() and np.array_equal(voted(ebo, geo, wins[5:], poses[5:], nz), alone)  # the 90-degree view by itself
    for tile in ("0", "1"):
        monkeypatch.setenv("EBO_DSI_TILE", tile)
        assert np.array_equal(voted(ebo_ab, geo, wins, poses, nz), want), tile
