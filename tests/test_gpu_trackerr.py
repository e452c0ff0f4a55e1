"""GPU: ebo_track_errors against tests/trackerr_ref.py, and ebo_reference_tracks against the hand-written loop over
lk_add_image / lk_track that defines it.  Every double of every result (err_mean, err_rmse, err_max) is bit-equal to the
restatement, the integers (age_us, t_first_us, n_inliers, n_comparable, first, cut, status) are equal, the per-sample
errors are bit-equal with -1 elsewhere.  The cases are trackerr_ref.gpu_cases: inlier counts 1, 63, 64, 65, 128, 129
without a cut (the lane stride's tails); one 130-sample track cut at sample 0, 1, 63, 64, 65, 129 and not at all;
e == tau exactly; samples before the ground truth's start, on its first and last time, 1 us past it and all outside;
ground-truth lengths 1, 2, 3, 64, 65, 200 with samples on and between its times; repeated estimated times; 8 thresholds
with 0 and +inf; a NaN or Inf in an estimated or ground-truth coordinate inside and outside the span with a clean
neighbour; coordinates 1e4 away at times near 2^50 us; empty tracks; a batch of 70 units mixing them, each equal to
itself alone and to a second run; the _device form; the argument errors."""
import ctypes as C

import numpy as np
import pytest

import trackerr_ref as V

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cases():
    return V.gpu_cases()


@pytest.fixture(scope="module")
def refs(cases):
    """name -> the restatement's (results, per-sample errors); computed once, read only."""
    return {name: V.track_errors(ests, gts, taus) for name, (ests, gts, taus) in cases.items()}


def check(name, got, want):
    assert len(got) == len(want), name
    for k, (g, w) in enumerate(zip(got, want)):
        for f in V.INTS:
            assert g[f] == w[f], (name, k, f, g, w)
        assert g["track"] == w["track"] and V.same_bits(g["tau"], w["tau"]), (name, k)
        for f in V.DOUBLES:
            assert V.same_bits(g[f], w[f]), (name, k, f, g[f], w[f])


def same_per_sample(a, b):
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


EXPECTED_STATUS = {"inliers": [0] * 6, "cuts": [0] * 7, "tie": [0] * 3, "span": [0, 1, 1, 1, 0], "gt_lengths": [1, 1] + [0] * 10,
                   "repeats": [0, 0], "taus8": [0] * 16, "nonfinite": [0, 0] + [2] * 10 + [0, 0], "far": [0, 0],
                   "empty": [1, 1, 1, 1, 0, 0, 1, 1]}


@pytest.mark.parametrize("name", sorted(EXPECTED_STATUS))
def test_case_equals_the_restatement(ebo, cases, refs, name):
    ests, gts, taus = cases[name]
    want, want_per = refs[name]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got, per = c.track_errors(ests, gts, taus, sample_errors=True)
        plain = c.track_errors(ests, gts, taus)
    assert [w["status"] for w in want] == EXPECTED_STATUS[name]
    check(name, got, want)
    check(name, plain, want)                                   # asking for the per-sample errors changes nothing
    assert same_per_sample(per, want_per), name
    for g in got:
        if g["status"] != 0:
            assert all(g[f] == 0 for f in V.DOUBLES + V.INTS if f != "status")
    if name == "inliers":
        assert [g["n_inliers"] for g in got] == [1, 63, 64, 65, 128, 129] and all(g["cut"] == -1 for g in got)
    if name == "cuts":
        assert [g["cut"] for g in got] == [0, 1, 63, 64, 65, 129, -1]
        assert [g["n_inliers"] for g in got] == [0, 1, 63, 64, 65, 129, 130]
    if name == "tie":
        assert [(g["n_inliers"], g["cut"]) for g in got] == [(5, -1), (0, 0), (5, -1)]
        assert all(V.same_bits(got[0][f], 5.0) for f in V.DOUBLES) and got[0]["age_us"] == 5000
    if name == "span":
        assert (got[0]["first"], got[0]["n_comparable"]) == (2, 4)
        assert list(per[:8] >= 0.0) == [False, False, True, True, True, True, False, False]
    if name == "nonfinite":
        assert V.same_result(got[0], got[12]) and V.same_result(got[1], got[13])
        n = len(ests[0][0])
        assert (per[n:6 * n] == -1.0).all() and same_per_sample(per[:n], per[6 * n:])
    if name == "taus8":
        assert got[0]["n_inliers"] == 0 and got[7]["n_inliers"] == 100 and got[6]["cut"] == -1
    if name == "far":
        assert got[1]["n_inliers"] == 66 and got[1]["t_first_us"] > 1 << 50


def test_a_batch_of_70_equals_each_unit_alone_and_the_restatement(ebo):
    ests, gts, taus = V.batch70()
    want, want_per = V.track_errors(ests, gts, taus)
    assert len(want) == 70 and {w["status"] for w in want} == {0, 1, 2}
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got, per = c.track_errors(ests, gts, taus, sample_errors=True)
        again, per_again = c.track_errors(ests, gts, taus, sample_errors=True)
        alone = [c.track_errors([e], [g], [tau])[0] for e, g in zip(ests, gts) for tau in taus]
    check("batch70", got, want)
    assert same_per_sample(per, want_per) and same_per_sample(per, per_again)
    for k in range(70):
        assert V.same_result(got[k], again[k]) and V.same_result(got[k], alone[k]), k


def test_device_form_equals_host_form(ebo):
    import torch
    ests, gts, taus = V.batch70()
    eo, et, exy = V.pack(ests)
    go, gt, gxy = V.pack(gts)
    dev = [torch.from_numpy(a).to("cuda") for a in (et, exy, gt, gxy)]
    d_per = torch.full((len(et),), 7.25, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        host, per = c.track_errors(ests, gts, taus, sample_errors=True)
        got = c.track_errors_device(eo, dev[0].data_ptr(), dev[1].data_ptr(), go, dev[2].data_ptr(), dev[3].data_ptr(), taus,
                                    d_per.data_ptr())
        none = c.track_errors_device(eo, dev[0].data_ptr(), dev[1].data_ptr(), go, dev[2].data_ptr(), dev[3].data_ptr(), taus)
    for k, (h, g, n) in enumerate(zip(host, got, none)):
        assert V.same_result(h, g) and V.same_result(h, n), k
    assert same_per_sample(d_per.cpu().numpy(), per)
    for d, a in zip(dev, (et, exy, gt, gxy)):
        assert np.array_equal(d.cpu().numpy(), a, equal_nan=True)


def test_argument_errors_and_the_recording_state(ebo, cases, synth):
    import torch
    ests, gts, _ = cases["far"]
    eo, et, exy = V.pack(ests)
    go, gt, gxy = V.pack(gts)
    res = (ebo.TrackErrorResult * 4)()
    vp = lambda a: a.ctypes.data_as(C.c_void_p)
    lib = ebo.lib()
    MARK = 7.25

    def stamp():
        for r in res:
            r.err_mean, r.err_max, r.n_inliers, r.status = MARK, MARK, -5, -6

    def untouched():
        return all(r.err_mean == MARK and r.err_max == MARK and r.n_inliers == -5 and r.status == -6 for r in res)

    def call(c, n=1, eo=eo, et=et, exy=exy, go=go, gt=gt, gxy=gxy, n_taus=2, taus=(1.0, 2.0), res=res):
        ta = np.array(taus, np.float64)
        a = lambda x, dt: None if x is None else vp(np.ascontiguousarray(x, dt))
        return lib.ebo_track_errors(c._h, n, a(eo, np.int32), a(et, np.int64), a(exy, np.float64), a(go, np.int32), a(gt, np.int64),
                                    a(gxy, np.float64), n_taus, vp(ta) if len(ta) else None,
                                    C.addressof(res) if res is not None else None, None)

    def refused(c, **kw):
        stamp()
        rc = call(c, **kw)
        return rc == ebo.ERR_ARG and untouched() and b"ebo_track_errors" in lib.ebo_last_error(c._h)

    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        for name in ("eo", "et", "exy", "go", "gt", "gxy"):
            assert refused(c, **{name: None}), name
        assert call(c, res=None) == ebo.ERR_ARG and refused(c, taus=())
        assert refused(c, n=-1) and refused(c, n=65536) and refused(c, n_taus=-1) and refused(c, n_taus=9, taus=(1.0,) * 9)
        assert refused(c, eo=[0, -1]) and refused(c, go=[1, 12]) and refused(c, eo=[3, 66])      # decreasing, not from 0
        assert refused(c, n=2, eo=[0, 40, 30], go=[0, 6, 12])
        assert refused(c, eo=[0, (1 << 24) + 1])                        # refused before any sample is read
        t = gt.copy()
        t[5] = t[4]
        assert refused(c, gt=t)                                         # ground-truth times must increase strictly
        t[5] = t[4] - 1
        assert refused(c, gt=t)
        t = et.copy()
        t[9] = t[8] - 1
        assert refused(c, et=t)                                         # estimated times must not decrease
        t[9] = t[8]
        stamp()
        assert call(c, et=t) == 0 and res[0].status == 0                # equal estimated times are allowed
        assert refused(c, taus=(1.0, np.nan)) and refused(c, taus=(-1e-300, 1.0)) and refused(c, taus=(-np.inf, 1.0))
        with pytest.raises(ebo.EboError) as err:
            c.track_errors(ests, gts, [1.0, -2.0])
        assert err.value.code == ebo.ERR_ARG
        stamp()
        assert call(c) == 0 and res[0].status == 0 and res[1].n_inliers == 66 and res[2].n_inliers == -5
        assert call(c, taus=(0.0, np.inf)) == 0 and res[1].cut == -1
        assert call(c, n_taus=8, taus=(1.0,) * 8, res=(ebo.TrackErrorResult * 8)()) == 0
        assert c.track_errors([], [], [1.0]) == [] and c.track_errors(ests, gts, []) == []
        # while a graph records: refused, and the recording survives
        ev, _ = synth.make_window(0, n_events=3000)
        c.set_window(ev)
        d_flows = torch.zeros((c.P, 2), dtype=torch.float64, device="cuda")
        d_out = torch.zeros(3 * c.P, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())
        c.synchronize()
        codes = []
        frames = np.zeros((2, c.params.image_h, c.params.image_w), np.uint8)

        def body():
            stamp()
            codes.append(call(c))
            codes.append(0 if untouched() else -1)
            for fn in (lambda: c.track_errors_device(eo, 1, 1, go, 1, 1, [1.0]),
                       lambda: c.reference_tracks(frames, [0, 1], [0], [[5.0, 5.0]])):
                try:
                    fn()
                    codes.append(0)
                except ebo.EboError as e:
                    codes.append(e.code)
            c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())

        g = c.record(body)
        assert codes == [ebo.ERR_STATE, 0, ebo.ERR_STATE, ebo.ERR_STATE]
        g.launch()
        c.synchronize()
        g.close()
        assert call(c) == 0


def test_the_timing_brackets_the_call(ebo, cases):
    ests, gts, taus = cases["inliers"]
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        c.two_view_timing(True)
        c.track_errors(ests, gts, taus)
        ms = c.two_view_timing(False)
    assert ms[0] > 0.0 and ms[4] >= ms[0] and ms[1] == ms[2] == ms[3] == 0.0


# ---- ebo_reference_tracks ------------------------------------------------------------------------------------------------
W, H, F = 96, 72, 6
SHIFT = (3, 2)                 # pixels per frame, to the right and down


@pytest.fixture(scope="module")
def frames(synth):
    """Six frames of one smooth texture moving by SHIFT per frame; a 30 x 30 region, flat in every frame, in the top
    right corner."""
    tex = synth._smooth_texture(np.random.default_rng(5), H + 40, W + 40)
    out = np.zeros((F, H, W), np.uint8)
    for f in range(F):
        y0, x0 = 20 - SHIFT[1] * f, 20 - SHIFT[0] * f
        out[f] = np.rint(tex[y0:y0 + H, x0:x0 + W]).astype(np.uint8)
        out[f, :30, W - 30:] = 128
    return out


SEED_FRAME = np.array([0, 0, 0, 2, 2, 5, 5, -1, 0, 0, 1], np.int32)
SEED_XY = np.array([[30.0, 40.0], [48.5, 30.25], [20.0, 20.0], [40.0, 36.0], [25.5, 50.5], [50.0, 40.0], [10.0, 60.0], [33.0, 33.0],
                    [89.0, 60.0],        # walks out of the image to the right
                    [81.0, 15.0],        # on the flat region: the minimum-eigenvalue test stops it
                    [44.0, 22.0]], np.float32)


def hand_written_loop(c, frames, seed_frame, seed_xy, **lk):
    """What ebo_reference_tracks is by definition."""
    n, nf = len(seed_frame), len(frames)
    first = np.where(seed_frame < 0, -1, seed_frame).astype(np.int32)
    last = first.copy()
    xy = np.zeros((n, nf, 2), np.float32)
    alive = np.zeros(n, bool)
    if nf:
        c.lk_add_image(frames[0])
    for f in range(nf):
        for k in range(n):
            if seed_frame[k] == f:
                alive[k] = True
                xy[k, f] = seed_xy[k]
        if f + 1 == nf:
            break
        c.lk_add_image(frames[f + 1])
        who = np.nonzero(alive)[0]
        if len(who) == 0:
            continue
        nxt, st, _ = c.lk_track(xy[who, f], **lk)
        for i, k in enumerate(who):
            x, y = nxt[i]
            if st[i] == 1 and 0 <= x < frames.shape[2] and 0 <= y < frames.shape[1]:
                xy[k, f + 1] = nxt[i]
                last[k] = f + 1
            else:
                alive[k] = False
    return first, last, xy


def same_tracks(got, want):
    first, last, xy = got
    return (np.array_equal(first, want[0]) and np.array_equal(last, want[1]) and xy.dtype == np.float64 and
            np.array_equal(xy.astype(np.float32).view(np.int32), want[2].view(np.int32)) and
            np.array_equal(xy, want[2].astype(np.float64)))


def test_reference_tracks_equal_the_hand_written_loop(ebo, frames):
    t = 1_000_000 + 40_000 * np.arange(F)
    with ebo.Context(image_w=W, image_h=H) as c:
        want = hand_written_loop(c, frames, SEED_FRAME, SEED_XY)
    with ebo.Context(image_w=W, image_h=H) as c:
        got = c.reference_tracks(frames, t, SEED_FRAME, SEED_XY)
        # the context's last two images are the last two frames, as after the loop
        after, st, _ = c.lk_track(SEED_XY[:3])
        c.lk_add_image(frames[F - 2])
        c.lk_add_image(frames[F - 1])
        again, st2, _ = c.lk_track(SEED_XY[:3])
    assert same_tracks(got, want)
    assert np.array_equal(after.view(np.int32), again.view(np.int32)) and np.array_equal(st, st2)
    first, last, xy = got
    assert list(first) == list(SEED_FRAME)
    assert list(last[:3]) == [5, 5, 5] and list(last[3:5]) == [5, 5]            # tracked to the end from frames 0 and 2
    assert list(last[5:8]) == [5, 5, -1]                                        # seeded on the last frame: length 1; no seed
    assert 0 <= last[8] < 5                                                     # left the image
    assert last[9] == 0                                                         # flat: stopped at once
    for k in range(len(first)):
        for f in range(F):
            inside = first[k] >= 0 and first[k] <= f <= last[k]
            assert inside or (xy[k, f] == 0.0).all(), (k, f)
        if first[k] >= 0:
            assert np.array_equal(xy[k, first[k]], SEED_XY[k].astype(np.float64))


def test_reference_tracks_with_two_frames_one_frame_and_other_parameters(ebo, frames):
    t = [5, 9]
    sf = np.array([0, 1, -1, 0], np.int32)
    lk = dict(win=(11, 9), max_level=1, max_count=7, epsilon=0.05, min_eig_threshold=1e-3)
    with ebo.Context(image_w=W, image_h=H) as c:
        want2 = hand_written_loop(c, frames[:2], sf, SEED_XY[:4])
        want_lk = hand_written_loop(c, frames[:3], sf, SEED_XY[:4], **lk)
        got2 = c.reference_tracks(frames[:2], t, sf, SEED_XY[:4])
        got_lk = c.reference_tracks(frames[:3], [5, 9, 11], sf, SEED_XY[:4], **lk)
        one = c.reference_tracks(frames[:1], [5], sf[[0, 2]], SEED_XY[:2])
        empty = c.reference_tracks(frames[:2], t, [], np.zeros((0, 2), np.float32))
        with pytest.raises(ebo.EboError) as err:
            c.reference_tracks(frames[:2], t, [2], SEED_XY[:1])                  # a seed beyond the frames
        assert err.value.code == ebo.ERR_ARG
        with pytest.raises(ebo.EboError) as err:
            c.reference_tracks(frames[:2], t, [0], SEED_XY[:1], win=(1, 1))      # what lk_track refuses
        assert err.value.code == ebo.ERR_ARG
        assert same_tracks(c.reference_tracks(frames[:2], t, sf, SEED_XY[:4]), want2)   # usable after the errors
    assert same_tracks(got2, want2) and list(got2[1]) == [1, 1, -1, 1]
    assert same_tracks(got_lk, want_lk) and not np.array_equal(got_lk[2][:, :2], got2[2])
    assert list(one[0]) == [0, -1] and list(one[1]) == [0, -1] and one[2].shape == (2, 1, 2)
    assert empty[0].shape == (0,) and empty[2].shape == (0, 2, 2)
