"""GPU: the rotation kernels where the LAUNCH SHAPE picks the path (tests/test_gpu_rotation.py covers the data), held to
tests/rotation_ref.py as there: H and F bit-equal, r and g within V9's bounds (1e-9 * sum(B^2) / Np and 1e-9 * A_i), the
value-only path the same r bits, a second run the same bits.
k_rot_vote's LDS tile in its three forms -- the rect grown by 8 pixels, the rect alone, no tile -- with one unit at each
limit ((rw + 16) * (rh + 16) == 4096, rw * rh == 4096, rw * rh == 4160) and grown tiles clipped at each image edge
(tests/test_rotation_cpu.py asserts that the cases hold them); a 346 x 260 sensor, where the folds' strided sums take
5 to 6 trips; eval_windows' chunks of 1, 38 and 64 slots under EBO_ROTATION_SCRATCH_MB, and the solver's list of live
windows cut into chunks of 5; windows of 1.5 s, whose units' own reference times lie half a second from the window's."""
import numpy as np
import pytest

import rotation_ref as R

pytestmark = pytest.mark.gpu


def context(ebo, geo, n_windows=1):
    return ebo.Context(loss=ebo.LOSS_VARIANCE, image_w=geo["w"], image_h=geo["h"], patch_w=geo["patch_w"], patch_h=geo["patch_h"],
                       max_windows=max(n_windows, 1), max_events=1 << 20)


def load(c, wins):
    offsets = np.concatenate([[0], np.cumsum([len(v) for v in wins])])
    c.set_windows(np.concatenate(wins), offsets)
    for i, ev in enumerate(wins):
        assert c.window_info(i)[0] == R.ref_time(ev)


def within_bounds(r, g, want):
    _, wr, wg, A, sb = want
    return abs(r - wr) <= 1e-9 * sb and np.all(np.abs(g - wg) <= 1e-9 * A)


def reference(case):
    geo = case["geo"]
    return [R.eval(ev, R.ref_time(ev), geo["cam"], geo["w"], geo["h"], om, case["sigma"]) for ev, om in zip(case["windows"], case["omegas"])]


def check_case(ebo, name, case, inside=None):
    """test_gpu_rotation.py's test_case_equals_the_restatement on one case; `inside` runs in the context before it closes."""
    want = reference(case)
    geo = case["geo"]
    prm = ebo.RotationParams(case["sigma"])
    n = len(case["windows"])
    with context(ebo, geo, n) as c:
        load(c, case["windows"])
        Hq, F = c.rotation_image(geo["cam"], case["omegas"])
        r, g = c.eval_rotation(geo["cam"], case["omegas"], prm)
        r_only, none = c.eval_rotation(geo["cam"], case["omegas"], prm, want_grad=False)
        Hq2, _ = c.rotation_image(geo["cam"], case["omegas"], image=False)
        r2, g2 = c.eval_rotation(geo["cam"], case["omegas"], prm)
        extra = inside(c, Hq) if inside else None
    assert none is None
    for i in range(n):
        assert Hq[i].any(), (name, i)
        assert np.array_equal(Hq[i], want[i][0]), (name, i, np.argwhere(Hq[i] != want[i][0])[:5])
        assert R.same_bits(F[i], want[i][0].astype(np.float64) * 2.0 ** -30), (name, i)
        print(name, i, "r %.17g want %.17g  |dg| %s  A %s" % (r[i], want[i][1], np.abs(g[i] - want[i][2]), want[i][3]))
        assert within_bounds(r[i], g[i], want[i]), (name, i)
    assert R.same_bits(r_only, r)
    assert np.array_equal(Hq2, Hq) and R.same_bits(r2, r) and R.same_bits(g2, g)
    return extra


# ---- the tile's three forms ------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.tile_cases()))
def test_the_tile_geometries_equal_the_restatement(ebo, name):
    check_case(ebo, name, R.tile_cases()[name])


def test_on_every_tile_form_the_vote_without_tiles_gives_the_same_bits(ebo_ab, monkeypatch):
    """150 x 128 with 48 x 48 patches holds grown tiles, bare tiles and a unit without one; at 40 rad/s taps leave every
    tile.  The A/B build's EBO_ROTATION_TILE=0 sends every tap through a global atomic: the same H, r and g bits."""
    case = R.tile_cases()["t150_x40"]
    geo = case["geo"]
    got = {}
    for tile in ("1", "0"):
        monkeypatch.setenv("EBO_ROTATION_TILE", tile)
        with context(ebo_ab, geo, len(case["windows"])) as c:
            load(c, case["windows"])
            got[tile] = (c.rotation_image(geo["cam"], case["omegas"], image=False)[0],) + c.eval_rotation(geo["cam"], case["omegas"])
    assert got["1"][0].any() and np.array_equal(got["0"][0], got["1"][0])
    assert R.same_bits(got["0"][1], got["1"][1]) and R.same_bits(got["0"][2], got["1"][2])
    assert np.array_equal(got["1"][0][0], reference(case)[0][0])


# ---- a DAVIS346 frame --------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.davis_cases()))
def test_a_346_by_260_sensor_equals_the_restatement(ebo, name):
    """352 pixel blocks and 221 patches: rot_wave_sum's strided part runs 5 to 6 trips over the blocks' folds and 3 to 4
    over the patches'.  ebo_event_images is R.blur of the vote image bit for bit."""
    case = R.davis_cases()[name]
    geo = case["geo"]
    assert (geo["w"] * geo["h"] + R.BLOCK - 1) // R.BLOCK == 352 and len(R.rects(geo)) == 221
    B = check_case(ebo, name, case, lambda c, Hq: c.event_images(geo["cam"], case["omegas"], ebo.RotationParams(case["sigma"])))
    for i, (ev, om) in enumerate(zip(case["windows"], case["omegas"])):
        Hq = R.votes(R.warp(ev, R.ref_time(ev), geo["cam"], geo["w"], geo["h"], om), geo["w"], geo["h"])
        assert R.same_bits(B[i], R.blur(Hq.astype(np.float64) * 2.0 ** -30, R.blur_weights(case["sigma"]))), (name, i)


# ---- chunks of windows -----------------------------------------------------------------------------

def test_every_chunk_size_gives_the_same_bits(ebo, monkeypatch):
    """70 windows of 37 x 29 in chunks of 1 slot (EBO_ROTATION_SCRATCH_MB=0), of 38 (1 MB: 38 + 32) and of 64 (unset:
    64 + 6): ebo_eval_rotation with and without gradient, ebo_rotation_image and ebo_event_images return the same bits,
    and they are the restatement's."""
    wins, omegas = R.batch_windows(70)
    geo = R.SMALL
    slots = {mb: R.chunk_slots(geo, mb, 70) for mb in (0, 1, None)}
    assert slots[0] == 1 and 1 < slots[1] < 64 and 70 % slots[1] != 0 and slots[None] == 64, slots
    got = {}
    with context(ebo, geo, 70) as c:
        load(c, wins)
        for mb in (None, 0, 1):
            if mb is None:
                monkeypatch.delenv("EBO_ROTATION_SCRATCH_MB", raising=False)
            else:
                monkeypatch.setenv("EBO_ROTATION_SCRATCH_MB", str(mb))
            r, g = c.eval_rotation(geo["cam"], omegas)
            r_only, _ = c.eval_rotation(geo["cam"], omegas, want_grad=False)
            Hq, F = c.rotation_image(geo["cam"], omegas)
            got[mb] = (r, g, r_only, Hq, F, c.event_images(geo["cam"], omegas))
    for mb in (0, 1):
        assert np.array_equal(got[mb][3], got[None][3]), mb
        for a, b in zip(got[mb], got[None]):
            assert R.same_bits(a, b), mb
    r, g, r_only, Hq, F, B = got[None]
    assert R.same_bits(r_only, r)
    g7 = R.blur_weights(1.0)
    for i in range(70):
        want = R.eval(wins[i], R.ref_time(wins[i]), geo["cam"], geo["w"], geo["h"], omegas[i])
        assert np.array_equal(Hq[i], want[0]) and within_bounds(r[i], g[i], want), i
        assert R.same_bits(F[i], want[0].astype(np.float64) * 2.0 ** -30), i
        assert R.same_bits(B[i], R.blur(F[i], g7)), i


def test_the_solve_in_chunks_of_five_live_windows_gives_the_same_bits(ebo, monkeypatch):
    """ebo_solve_rotation hands eval_windows the list of windows still live; at 5 MB on 240 x 180 that list of up to 12 is
    cut into chunks of 5, and it shrinks as scenes converge.  Omegas and summaries equal the default budget's bit for bit."""
    wins = [R.recovery_scene(i) for i in range(len(R.RECOVERY_SEEDS))]
    assert R.chunk_slots(R.LARGE, 5, len(wins)) == 5 and R.chunk_slots(R.LARGE, None, len(wins)) == len(wins)
    got = {}
    with context(ebo, R.LARGE, len(wins)) as c:
        load(c, wins)
        for mb in (None, 5):
            if mb is None:
                monkeypatch.delenv("EBO_ROTATION_SCRATCH_MB", raising=False)
            else:
                monkeypatch.setenv("EBO_ROTATION_SCRATCH_MB", str(mb))
            got[mb] = c.solve_rotation(R.CAM)
    (om, summ), (om5, summ5) = got[None], got[5]
    truth = R.recovery_truths()
    assert R.same_bits(om5, om)
    assert len({s.evaluations for s in summ}) > 1  # the scenes leave the list at different rounds
    for i in range(len(wins)):
        assert (summ5[i].status, summ5[i].iterations, summ5[i].evaluations) == (summ[i].status, summ[i].iterations, summ[i].evaluations), i
        assert R.same_bits(summ5[i].r_initial, summ[i].r_initial) and R.same_bits(summ5[i].r_final, summ[i].r_final), i
        assert summ[i].status == ebo.ROT_CONVERGED_STEP and np.abs(om[i] - truth[i]).max() <= 0.15, i


# ---- long windows ------------------------------------------------------------------------------------

@pytest.mark.parametrize("name", sorted(R.long_cases()))
def test_windows_of_a_second_and_a_half_equal_the_restatement(ebo, name):
    """rot_tau adds the unit's dt_win to the event's dt: here units lie +-0.5 s from their window's reference time, one
    window starting at 0 and one at 2 000 000 000 us.  dt_win is read back as window_info's time less patch_info's."""
    case = R.long_cases()[name]
    geo = case["geo"]

    def dt_wins(c, Hq):
        return [{p: c.window_info(w)[0] - c.patch_info(p, w)[2] for p in range(c.P) if c.patch_info(p, w)[0] > 0}
                for w in range(len(case["windows"]))]
    got = check_case(ebo, name, case, dt_wins)
    for w, ev in enumerate(case["windows"]):
        assert got[w] == R.unit_dt_win(ev, geo), w
        assert max(got[w].values()) > 100000 and min(got[w].values()) < -100000, got[w]
