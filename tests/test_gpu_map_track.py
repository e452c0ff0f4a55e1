"""GPU: ebo_map_track, ebo_map_track_device, ebo_event_images and ebo_event_images_device against tests/maptrack_ref.py
and tests/rotation_ref.py (include/ebo.h, rules E1-E9 and V1-V5).  Every pose, cost, count and trace row is bit-equal to
the restatement.  The scenes are maptrack_ref.gpu_problems: images 37 x 29 and 64 x 48; 1, 5, 255, 256, 257 and 600 points
(on and around the tree's partial boundary, lanes with unequal trip counts); 1, 3 and 70 units; the whole scene in view,
half of it, none of it; points on the four visibility borders, q2 at z_min, a NaN point, a NaN and an infinite pose entry;
an all-zero, a constant, a one-pixel, an infinite and a negative image, a NaN no tap reads and one a tap reads; every
branch of B9 a scene reaches (tests/test_maptrack_cpu.py asserts that each scene takes its branch).

ebo_event_images is bit-equal to rotation_ref's blur of the vote image at sigma_blur 0, 1 and 2.5: the two passes add
their seven products in the restatement's order, one rounding each."""
import ctypes as C

import numpy as np
import pytest

import maptrack_ref as M
import rotation_ref as R

pytestmark = pytest.mark.gpu

PROBLEMS = M.gpu_problems()


@pytest.fixture(scope="module")
def refs():
    """name -> the restatement's units; computed once, read only."""
    return {name: M.solve_units(pr) for name, pr in PROBLEMS.items()}


def run(c, pr, units=None, trace=True):
    """The host form on the listed units of a problem (None: all) -> list of dicts (pose, result, trace)."""
    idx = np.arange(len(pr["unit_image"])) if units is None else np.asarray(units)
    poses, res, tr = c.map_track(pr["cam"], pr["images"], pr["points"], pr["unit_image"][idx], pr["poses"][idx], pr["z_min"],
                                 c_opts(c, pr["opts"]), trace=trace)
    return [dict(pose=poses[i], result=res[i], trace=tr[i] if trace else None) for i in range(len(idx))]


_EBO = {}


def c_opts(c, o):
    return _EBO["ebo"].default_map_track_opts(**o)


@pytest.fixture(scope="module")
def ctx(ebo):
    _EBO["ebo"] = ebo
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        yield c


@pytest.mark.parametrize("name", sorted(PROBLEMS))
def test_every_unit_equals_the_restatement(ctx, refs, name):
    pr, want = PROBLEMS[name], refs[name]
    got = run(ctx, pr)
    for u, (g, w) in enumerate(zip(got, want)):
        assert M.same_unit(g, w), (name, u, g["result"], w["result"])
    again = run(ctx, pr)
    assert all(M.same_unit(g, a) for g, a in zip(got, again))


def test_a_batch_equals_every_unit_alone_and_the_reversed_batch(ctx, refs):
    name = "size_small_40_70"
    pr, want = PROBLEMS[name], refs[name]
    n = len(pr["unit_image"])
    assert n == 70
    batch = run(ctx, pr)
    rev = run(ctx, pr, units=np.arange(n)[::-1])[::-1]
    for u in range(n):
        assert M.same_unit(batch[u], want[u]) and M.same_unit(rev[u], batch[u]), u
        assert M.same_unit(run(ctx, pr, units=[u])[0], batch[u]), u


def test_units_sharing_an_image_equal_units_on_copies_of_it(ctx):
    sc = M.recovery_scene(0, 0.10, 0.03)
    starts = M.starts13(sc["start"], 0.05, 0.015)
    o = M.default_opts(max_num_iterations=15)
    shared = M.problem(sc["geo"], sc["image"][None], sc["points"], np.zeros(13, int), starts, opts=o)
    copies = M.problem(sc["geo"], np.repeat(sc["image"][None], 13, axis=0), sc["points"], np.arange(13), starts, opts=o)
    a, b = run(ctx, shared), run(ctx, copies)
    assert all(M.same_unit(x, y) for x, y in zip(a, b))
    assert M.same_unit(a[3], M.solve_units(shared)[3])


def test_the_host_form_equals_the_device_form(ebo, ctx):
    import torch
    pr = PROBLEMS["size_mid_257_3"]
    o = c_opts(ctx, pr["opts"])
    n = len(pr["unit_image"])
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    ui = pr["unit_image"].copy()
    d_img, d_pts, d_pose = dev(pr["images"]), dev(pr["points"]), dev(pr["poses"])
    d_res = torch.zeros(n * 64, dtype=torch.uint8, device="cuda")
    d_trace = torch.full((n, o.max_num_iterations + 1, 4), -7.0, dtype=torch.float64, device="cuda")
    h, w = pr["images"].shape[1:]
    host = run(ctx, pr)

    def device(unit_image):
        d_ui = dev(np.asarray(unit_image, np.int32))
        d_pose.copy_(dev(pr["poses"]))
        torch.cuda.synchronize()
        ctx.map_track_device(pr["cam"], w, h, len(pr["images"]), d_img.data_ptr(), len(pr["points"]), d_pts.data_ptr(), n,
                             d_ui.data_ptr(), d_pose.data_ptr(), d_res.data_ptr(), pr["z_min"], o, d_trace.data_ptr())
        ctx.synchronize()
        res = ebo.Context.map_track_results(d_res.cpu().numpy())
        return [dict(pose=d_pose[u].cpu().numpy(), result=res[u], trace=d_trace[u].cpu().numpy()) for u in range(n)]

    got = device(ui)
    assert all(M.same_unit(g, hst) for g, hst in zip(got, host))
    # the device form cannot look at unit_image: a unit naming an image that is not there is not solved
    ui[1] = len(pr["images"])
    got = device(ui)
    assert M.same_unit(got[0], host[0]) and M.same_unit(got[2], host[2])
    r = got[1]["result"]
    assert r["termination"] == 2 and all(r[k] == 0 for k in M.RESULT_INTS[1:] + M.RESULT_DOUBLES)
    assert M.same_bits(got[1]["pose"], pr["poses"][1]) and not got[1]["trace"].any()


# ---- ebo_event_images -------------------------------------------------------------------------------------------------------

def rot_context(ebo, geo, n_windows=1):
    return ebo.Context(loss=ebo.LOSS_VARIANCE, image_w=geo["w"], image_h=geo["h"], patch_w=geo["patch_w"], patch_h=geo["patch_h"],
                       max_windows=max(n_windows, 1), max_events=1 << 20)


def load(c, wins):
    offsets = np.concatenate([[0], np.cumsum([len(v) for v in wins])])
    c.set_windows(np.concatenate(wins), offsets)


def event_windows(geo):
    w, h = geo["w"], geo["h"]
    return [R.random_window(5, 1, w, h), R.random_window(6, 300, w, h, strays=20), R.random_window(7, 5000, w, h, strays=100),
            R.border_window(w, h)]


@pytest.mark.parametrize("oname", ["zero", "small"])
def test_event_images_equal_the_blur_of_the_vote_image(ebo, oname):
    geo = R.SMALL  # 4 x 3 patches, the last of each axis wider
    wins = event_windows(geo)
    om = np.tile(np.array(R.OMEGAS[oname]), (len(wins), 1))
    with rot_context(ebo, geo, len(wins)) as c:
        load(c, wins)
        Hq, F = c.rotation_image(geo["cam"], om)
        B0 = c.event_images(geo["cam"], om, ebo.RotationParams(0.0))
        assert R.same_bits(B0, F)  # sigma_blur 0: F bit for bit
        if oname == "zero":
            assert R.same_bits(c.event_images(geo["cam"], None, ebo.RotationParams(0.0)), F)
            for i, ev in enumerate(wins):  # the un-warped integer count image
                keep = (ev["x"] >= 0) & (ev["x"] < geo["w"]) & (ev["y"] >= 0) & (ev["y"] < geo["h"])
                cnt = np.zeros((geo["h"], geo["w"]))
                np.add.at(cnt, (ev["y"][keep], ev["x"][keep]), 1.0)
                assert np.array_equal(F[i], cnt), i
        for sigma in (1.0, 2.5):
            got = c.event_images(geo["cam"], om, ebo.RotationParams(sigma))
            for i, ev in enumerate(wins):
                want = R.blur(Hq[i].astype(np.float64) * 2.0 ** -30, R.blur_weights(sigma))
                print(oname, sigma, i, "max |dB| %.3g of %.3g" % (np.abs(got[i] - want).max(), want.max()))
                assert R.same_bits(got[i], want), (oname, sigma, i)
        assert R.same_bits(c.event_images(geo["cam"], om), c.event_images(geo["cam"], om, ebo.RotationParams(1.0)))  # the default


def test_event_images_in_chunks_equal_the_whole_batch(ebo):
    """70 windows are more than one chunk of 64."""
    wins, omegas = R.batch_windows(70)
    geo = R.SMALL
    with rot_context(ebo, geo, 70) as c:
        load(c, wins)
        all_ = c.event_images(geo["cam"], omegas)
        load(c, wins[60:])
        assert R.same_bits(c.event_images(geo["cam"], omegas[60:]), all_[60:])
    want = R.blur(R.eval(wins[69], R.ref_time(wins[69]), geo["cam"], geo["w"], geo["h"], omegas[69])[0].astype(np.float64) * 2.0 ** -30,
                  R.blur_weights(1.0))
    assert R.same_bits(all_[69], want)


def test_the_recovery_scene_from_end_to_end_on_the_device(ebo):
    """The scene's events loaded as windows, ebo_event_images_device into ebo_map_track_device without leaving the
    device: the images are the restatement's, and so is every figure of the 13 starts of every window."""
    import torch
    geo = dict(M.MID, patch_w=16, patch_h=16)
    scenes = [M.recovery_scene(s, 0.10, 0.03) for s in (0, 1, 2)]
    wins = [R.events(sc["events"][:, 0], sc["events"][:, 1], np.arange(len(sc["events"]), dtype=np.int64) * 10) for sc in scenes]
    X = scenes[0]["points"]
    starts = np.concatenate([M.starts13(sc["start"], 0.05, 0.015) for sc in scenes])
    ui = np.repeat(np.arange(3), 13).astype(np.int32)
    o = M.default_opts(max_num_iterations=20)
    dev = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to("cuda")
    d_img = torch.zeros((3, geo["h"], geo["w"]), dtype=torch.float64, device="cuda")
    d_pts, d_pose, d_ui = dev(X), dev(starts), dev(ui)
    d_res = torch.zeros(len(ui) * 64, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    with rot_context(ebo, geo, 3) as c:
        load(c, wins)
        c.event_images_device(geo["cam"], d_img.data_ptr())
        c.map_track_device(geo["cam"], geo["w"], geo["h"], 3, d_img.data_ptr(), len(X), d_pts.data_ptr(), len(ui), d_ui.data_ptr(),
                           d_pose.data_ptr(), d_res.data_ptr(), M.Z_MIN, ebo.default_map_track_opts(**o))
        c.synchronize()
    images = d_img.cpu().numpy()
    for i, sc in enumerate(scenes):
        assert R.same_bits(images[i], sc["image"]), i
    res = ebo.Context.map_track_results(d_res.cpu().numpy())
    poses = d_pose.cpu().numpy()
    # scene 0's map under the other scenes' events is no alignment: only the bits are held to the restatement there
    want = M.solve_units(M.problem(geo, images, X, ui, starts, opts=o))
    for u, w in enumerate(want):
        assert M.same_bits(poses[u], w["pose"]), u
        assert all(res[u][k] == w["result"][k] for k in M.RESULT_INTS), u
        assert all(M.same_bits(res[u][k], w["result"][k]) for k in M.RESULT_DOUBLES), u
    wi = M.winner(res[:13])
    e0 = M.reprojection_error(geo, X, scenes[0]["start"], scenes[0]["truth"])
    e1 = M.reprojection_error(geo, X, poses[wi], scenes[0]["truth"])
    print("window 0: start %.2f px, winner %d after 20 iterations at most: %.3f px" % (e0, wi, e1))
    assert e1 <= 0.5 and e1 <= e0 / 3.0


def test_the_resident_form_and_the_starts(ebo):
    """ebo_map_track_resident is ebo_event_images + ebo_map_track with the images kept on the device between calls;
    ebo_map_track_starts is B4 on the host, the restatement's bits."""
    geo = dict(M.MID, patch_w=16, patch_h=16)
    scenes = [M.recovery_scene(s, 0.10, 0.03) for s in (0, 1)]
    wins = [R.events(sc["events"][:, 0], sc["events"][:, 1], np.arange(len(sc["events"]), dtype=np.int64) * 10) for sc in scenes]
    X = scenes[0]["points"]
    starts = ebo.map_track_starts(scenes[0]["start"], 0.05, 0.015)
    assert M.same_bits(starts, M.starts13(scenes[0]["start"], 0.05, 0.015))
    o = ebo.default_map_track_opts(max_num_iterations=12)
    ui = np.array([0] * 13 + [1], dtype=np.int32)
    poses = np.concatenate([starts, scenes[1]["start"][None]])
    with rot_context(ebo, geo, 2) as c:
        load(c, wins)
        with pytest.raises(ebo.EboError) as e:
            c.map_track_resident(geo["cam"], X, ui, poses, make_images=False, opts=o)
        assert e.value.code == ebo.ERR_STATE  # no images yet
        images = c.event_images(geo["cam"])
        want = c.map_track(geo["cam"], images, X, ui, poses, M.Z_MIN, o, trace=True)
        got = c.map_track_resident(geo["cam"], X, ui, poses, opts=o, trace=True)
        again = c.map_track_resident(geo["cam"], X, ui[13:], poses[13:], make_images=False, opts=o, trace=True)
        for a, b in ((got, want), ((again[0], again[1], again[2]), (want[0][13:], want[1][13:], want[2][13:]))):
            assert M.same_bits(a[0], b[0]) and M.same_bits(a[2], b[2])
            assert all(M.same_bits(x[k], y[k]) for x, y in zip(a[1], b[1]) for k in M.RESULT_INTS + M.RESULT_DOUBLES)
        with pytest.raises(ebo.EboError) as e:
            c.map_track_resident(geo["cam"], X, [2], poses[:1], make_images=False, opts=o)
        assert e.value.code == ebo.ERR_ARG  # no such window
        load(c, wins[:1])
        with pytest.raises(ebo.EboError) as e:
            c.map_track_resident(geo["cam"], X, [0], poses[:1], make_images=False, opts=o)
        assert e.value.code == ebo.ERR_STATE  # a loader has run since


# ---- errors ---------------------------------------------------------------------------------------------------------------------

def test_argument_and_state_errors(ebo, synth):
    import torch
    pr = PROBLEMS["size_small_5_3"]
    o = ebo.default_map_track_opts(**pr["opts"])
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        def code(cam=pr["cam"], images=pr["images"], points=pr["points"], unit_image=pr["unit_image"], poses=pr["poses"], z_min=M.Z_MIN,
                 opts=o):
            try:
                c.map_track(cam, images, points, unit_image, poses, z_min, opts)
                return 0
            except ebo.EboError as e:
                return e.code

        assert code() == 0
        assert code(unit_image=np.zeros(0, np.int32), poses=np.zeros((0, 12))) == 0
        assert code(unit_image=[0, 3, 1]) == ebo.ERR_ARG and code(unit_image=[0, -1, 1]) == ebo.ERR_ARG
        assert code(cam=(30.0, 31.0, 18.0, 14.25, 0.1, 0, 0, 0, 0)) == ebo.ERR_ARG  # distortion
        assert code(cam=(30.0, 31.0, 18.0, 14.25, 0, 0, 0, 0, 1e-3)) == ebo.ERR_ARG
        for bad in (0.0, float("nan"), float("inf")):
            assert code(cam=(bad, 31.0, 18.0, 14.25)) == ebo.ERR_RANGE and code(cam=(30.0, bad, 18.0, 14.25)) == ebo.ERR_RANGE
        for z in (float("nan"), float("inf"), -float("inf")):
            assert code(z_min=z) == ebo.ERR_ARG
        assert code(z_min=-1.0) == 0
        assert code(opts=ebo.default_map_track_opts(max_num_iterations=-1)) == ebo.ERR_ARG
        assert code(opts=ebo.default_map_track_opts(max_num_iterations=10001)) == ebo.ERR_ARG  # it sizes the trace
        assert code(opts=ebo.default_map_track_opts(max_num_iterations=2 ** 31 - 1)) == ebo.ERR_ARG
        assert code(images=np.zeros((1, 1, 9))) == ebo.ERR_ARG and code(images=np.zeros((1, 9, 1))) == ebo.ERR_ARG  # h, w < 2
        assert code(unit_image=np.zeros(65536, np.int32), poses=np.zeros((65536, 12))) == ebo.ERR_ARG
        # the raw entry: counts and null pointers
        lib = ebo.lib()
        vp = lambda a: a.ctypes.data_as(C.c_void_p)
        cam = ebo.camera(pr["cam"] + (0.0,) * 5)
        img, pts, ui, po = pr["images"].copy(), pr["points"].copy(), pr["unit_image"].copy(), pr["poses"].copy()
        res = (ebo.MapTrackResult * 3)()
        h, w = img.shape[1:]

        def raw(**kw):
            a = dict(cam=C.addressof(cam), w=w, h=h, ni=len(img), img=vp(img), np_=len(pts), pts=vp(pts), nu=3, ui=vp(ui), po=vp(po),
                     o=C.addressof(o), res=C.addressof(res))
            a.update(kw)
            return lib.ebo_map_track(c._h, a["cam"], a["w"], a["h"], a["ni"], a["img"], a["np_"], a["pts"], a["nu"], a["ui"], a["po"],
                                     C.c_double(M.Z_MIN), a["o"], a["res"], None)

        assert raw() == 0
        for k in ("cam", "img", "pts", "ui", "po", "o", "res"):
            assert raw(**{k: None}) == ebo.ERR_ARG, k
        for k in ("ni", "np_", "nu"):
            assert raw(**{k: -1}) == ebo.ERR_ARG, k
        assert raw(np_=(1 << 20) + 1) == ebo.ERR_ARG
        assert raw(np_=0, pts=None) == 0  # no points: nothing is needed of them
        assert lib.ebo_map_track(None, C.addressof(cam), w, h, 1, vp(img), 1, vp(pts), 1, vp(ui), vp(po), C.c_double(0.05), C.addressof(o),
                                 C.addressof(res), None) == ebo.ERR_ARG
        # ebo_event_images: state and argument errors as ebo_rotation_image's
        def ecode(fn):
            try:
                fn()
                return 0
            except ebo.EboError as e:
                return e.code

        k4 = (200.0, 200.0, 119.5, 89.5)
        assert ecode(lambda: c.event_images(k4)) == ebo.ERR_STATE  # no window loaded
        ev, _ = synth.make_window(0, n_events=3000)
        c.set_window(ev)
        assert ecode(lambda: c.event_images(k4)) == 0
        assert ecode(lambda: c.event_images(k4 + (0.1, 0, 0, 0, 0))) == ebo.ERR_ARG
        assert ecode(lambda: c.event_images((0.0,) + k4[1:])) == ebo.ERR_RANGE
        for s in (-1.0, float("nan"), float("inf")):
            assert ecode(lambda: c.event_images(k4, None, ebo.RotationParams(s))) == ebo.ERR_ARG
        kc = ebo.camera(k4 + (0.0,) * 5)
        assert lib.ebo_event_images(c._h, C.addressof(kc), None, None, None) == ebo.ERR_ARG
        assert lib.ebo_event_images(c._h, None, None, None, vp(np.zeros(4))) == ebo.ERR_ARG
        # while a graph records: refused, and the recording survives
        d_flows = torch.zeros((c.P, 2), dtype=torch.float64, device="cuda")
        d_out = torch.zeros(3 * c.P, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())
        c.synchronize()
        codes = []

        def body():
            codes.append(code())
            codes.append(ecode(lambda: c.map_track_device(pr["cam"], w, h, 1, 1, 1, 1, 1, 1, 1, 1)))
            codes.append(ecode(lambda: c.event_images(k4)))
            codes.append(ecode(lambda: c.event_images_device(k4, 1)))
            c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())

        g = c.record(body)
        assert codes == [ebo.ERR_STATE] * 4
        g.launch()
        c.synchronize()
        g.close()
        assert code() == 0
        # units loaded by ebo_set_patches are not windows
        ev2 = R.random_window(2, 40, 64, 48)
        c.set_patches(ev2, [0, len(ev2)], [[0, 0, 8, 8]])
        assert ecode(lambda: c.event_images(k4)) == ebo.ERR_STATE
        assert code() == 0  # the tracker itself reads no window
