"""GPU: the camera model on the device against tests/camera_ref.py -- ebo_camera_unproject, the rectification map
and table, and the rectified loaders: loading raw events with a rectification set is, bit for bit, loading
camera_ref.rectify_events(raw) on a context without one."""
import numpy as np
import pytest

import camera_ref

pytestmark = pytest.mark.gpu

CAMERAS = {"davis": camera_ref.DAVIS, "reader": camera_ref.READER, "pinhole": camera_ref.PINHOLE}
# the DAVIS lens on the 346 x 260 sensor of configuration C3 (same coefficients, the principal point near the centre)
DAVIS_346 = (287.0, 286.6, 176.3, 127.9) + camera_ref.DAVIS[4:]
# finite everywhere on 240 x 180, but the corner pixels rectify to ~4e5: beyond the 15-bit coordinate of an event
# record (found with camera_ref.rectify_map; asserted below)
OUT_OF_RANGE = (200.0, 200.0, 120.0, 90.0, -1.0, 0.0, 0.0, 0.0, 0.0)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def seeded_pixels(seed, n):
    rng = np.random.default_rng(seed)
    uv = np.stack([rng.uniform(-40, 400, n), rng.uniform(-40, 300, n)], axis=1)
    uv[:6] = [[0, 0], [239, 0], [0, 179], [239, 179], [132.192071378, 110.712660011], [120, 90]]
    return uv


@pytest.mark.parametrize("name", sorted(CAMERAS))
def test_unproject_is_bit_equal_to_camera_ref(ebo, name):
    """Bit equality holds if the device's float64 division and square root are correctly rounded: the rule uses
    only + - * / sqrt, each rounded once in numpy."""
    import torch
    cam = CAMERAS[name]
    uv = seeded_pixels(5, 100_000)
    want = camera_ref.unproject(cam, uv)
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        got = c.camera_unproject(cam, uv)
        d_uv = torch.from_numpy(uv).to("cuda")
        d_out = torch.zeros((len(uv), 3), dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        c.camera_unproject_device(cam, len(uv), d_uv.data_ptr(), d_out.data_ptr())
        c.synchronize()
        got_dev = d_out.cpu().numpy()
        few = c.camera_unproject(cam, uv[:3])
    diff = np.flatnonzero((bits(got) != bits(want)).any(axis=1))
    print("unproject %s: %d of %d points differ" % (name, len(diff), len(uv)), diff[:5], got[diff[:2]], want[diff[:2]])
    assert np.array_equal(bits(got), bits(want))
    assert np.array_equal(bits(got_dev), bits(want))
    assert np.array_equal(bits(few), bits(want[:3]))


@pytest.mark.parametrize("size", [(240, 180), (346, 260), (1280, 720)])
@pytest.mark.parametrize("name", ["davis", "pinhole"])
def test_rectification_map_is_bit_equal_to_camera_ref(ebo, size, name):
    w, h = size
    cam = CAMERAS[name]
    if name == "davis" and size != (240, 180):
        # the same lens on a larger sensor: scale the pinhole part, or the fixed point runs far outside the lens model
        cam = (cam[0] * w / 240.0, cam[1] * h / 180.0, cam[2] * w / 240.0, cam[3] * h / 180.0) + tuple(cam[4:])
    m, lut, ok = camera_ref.rectify_map(cam, w, h)
    assert ok
    with ebo.Context(image_w=w, image_h=h, patch_w=40, patch_h=20, loss=ebo.LOSS_VARIANCE) as c:
        c.set_rectification(cam)
        gm, glut = c.rectification_map()
    print("map %s %dx%d: %d map words and %d table entries differ" % (name, w, h, int((bits(gm) != bits(m)).sum()),
                                                                      int((glut != lut).sum())))
    assert np.array_equal(bits(gm), bits(m))
    assert np.array_equal(glut, lut)
    if name == "pinhole":
        ys, xs = np.mgrid[0:h, 0:w]
        assert np.array_equal(glut[..., 0], xs) and np.array_equal(glut[..., 1], ys)


def test_rectification_refusals(ebo, synth):
    m, _, ok = camera_ref.rectify_map(OUT_OF_RANGE, 240, 180)
    assert not ok and np.isfinite(m).all() and np.abs(m).max() > 16384
    import torch
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        for bad in ((0.0,) + camera_ref.DAVIS[1:], camera_ref.DAVIS[:1] + (float("inf"),) + camera_ref.DAVIS[2:],
                    camera_ref.DAVIS[:5] + (float("nan"),) + camera_ref.DAVIS[6:], OUT_OF_RANGE):
            with pytest.raises(ebo.EboError) as ei:
                c.set_rectification(bad)
            assert ei.value.code == ebo.ERR_RANGE, bad
            with pytest.raises(ebo.EboError) as ei:  # a refused call leaves none set
                c.rectification_map()
            assert ei.value.code == ebo.ERR_STATE
        # while a graph records: refused as every other entry point, and the recording survives
        ev, gt = synth.make_window(0, n_events=3000)
        c.set_window(ev)
        d_flows = torch.zeros((c.P, 2), dtype=torch.float64, device="cuda")
        d_out = torch.zeros(3 * c.P, dtype=torch.float64, device="cuda")
        torch.cuda.synchronize()
        c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())
        c.synchronize()
        codes = []

        def body():
            for call in (lambda: c.set_rectification(camera_ref.DAVIS), c.clear_rectification, c.rectification_map,
                         lambda: c.camera_unproject(camera_ref.DAVIS, [[1.0, 2.0]])):
                try:
                    call()
                    codes.append(0)
                except ebo.EboError as e:
                    codes.append(e.code)
            c.eval_device(d_flows.data_ptr(), True, d_out.data_ptr())

        g = c.record(body)
        assert codes == [ebo.ERR_STATE] * 4
        g.launch()
        c.synchronize()
        g.close()
        c.set_rectification(camera_ref.DAVIS)  # and afterwards it works


def _fixture(synth, config, n_windows, n_events, cam):
    cfg = synth.CONFIGS[config]
    w, h = cfg["image"]
    ev, offsets, gt = synth.make_stream(config, n_windows, n_events=n_events)
    ev = ev.copy()
    # raw coordinates outside the sensor (strays before and after), and the four corner pixels
    ev["x"][3] = -2
    ev["y"][11] = 15000
    ev["x"][20], ev["y"][20] = w, 5
    for i, (x, y) in enumerate(((0, 0), (w - 1, 0), (0, h - 1), (w - 1, h - 1))):
        ev["x"][30 + i], ev["y"][30 + i] = x, y
    rect = camera_ref.rectify_events(cam, w, h, ev)
    raw_out = (ev["x"] < 0) | (ev["x"] >= w) | (ev["y"] < 0) | (ev["y"] >= h)
    rect_out = (rect["x"] < 0) | (rect["x"] >= w) | (rect["y"] < 0) | (rect["y"] >= h)
    assert raw_out.sum() >= 3 and (rect_out & ~raw_out).sum() >= 4, (raw_out.sum(), (rect_out & ~raw_out).sum())
    assert np.array_equal(rect[raw_out], ev[raw_out])
    assert ((rect["x"] != ev["x"]) | (rect["y"] != ev["y"])).mean() > 0.3  # the lens moves a good part of the sensor
    return cfg, ev, rect, offsets, gt


def _snapshot(ebo, c, n_windows, gt, solves=True):
    info = [[c.patch_info(p, w) for p in range(c.P)] for w in range(n_windows)]
    wins = [c.window_info(w) for w in range(n_windows)]
    r, J = c.eval(gt * 0.5)
    out = [info, wins, r, J, c.count_image(ebo.COUNT_WARPED, gt * 0.7), c.count_image(ebo.COUNT_INTEGRATED)]
    if solves:
        out.append(c.solve(mode=ebo.SOLVE_INDEPENDENT, max_num_iterations=4)[0])
        out.append(c.solve(mode=ebo.SOLVE_GLOBAL, max_num_iterations=3)[0])
    return out


def _assert_same(got, ref, what):
    assert got[0] == ref[0], what  # unit tables: counts, active flags, reference times
    assert got[1] == ref[1], what
    for k in range(2, len(ref)):
        assert np.array_equal(bits(got[k]), bits(ref[k])), (what, k)


@pytest.mark.parametrize("loss", ["variance", "edge"])
@pytest.mark.parametrize("config,n_windows,n_events", [(2, 1, 20000), (2, 21, 8000), (3, 1, 60000), (3, 21, 12000)])
def test_rectified_load_equals_load_of_rectified_events(ebo, synth, config, n_windows, n_events, loss):
    import torch
    cam = camera_ref.DAVIS if config == 2 else DAVIS_346
    cfg, ev, rect, offsets, gt = _fixture(synth, config, n_windows, n_events, cam)
    kw = dict(image_w=cfg["image"][0], image_h=cfg["image"][1], patch_w=cfg["patch"][0], patch_h=cfg["patch"][1],
              loss=ebo.LOSS_VARIANCE if loss == "variance" else ebo.LOSS_EDGE, max_windows=n_windows, max_events=len(ev))
    t_base = np.array([int(ev["t_us"][int(offsets[w])]) - 7 * w for w in range(n_windows)], dtype=np.int64)
    ev8 = np.concatenate([ebo.pack_events8(ev[int(offsets[w]):int(offsets[w + 1])], t_base[w]) for w in range(n_windows)])
    with ebo.Context(**kw) as plain:
        plain.set_windows(rect, offsets)
        ref = _snapshot(ebo, plain, n_windows, gt)
        plain.set_windows(ev, offsets)
        raw = _snapshot(ebo, plain, n_windows, gt, solves=False)
    assert raw[0] != ref[0]  # the fixture is not trivial: rectifying moves events between patches
    with ebo.Context(**kw) as c:
        c.set_rectification(cam)
        c.set_windows(ev, offsets)
        _assert_same(_snapshot(ebo, c, n_windows, gt), ref, "ebo_set_windows")
        if n_windows == 1:
            c.set_window(ev)
            _assert_same(_snapshot(ebo, c, 1, gt, solves=False), ref[:6], "ebo_set_window")
        d24 = torch.from_numpy(np.ascontiguousarray(ev).view(np.uint8).reshape(-1, 24)).to("cuda")
        c.set_windows_device(d24.data_ptr(), offsets)
        _assert_same(_snapshot(ebo, c, n_windows, gt), ref, "ebo_set_windows_device")
        assert np.array_equal(d24.cpu().numpy().reshape(-1).view(ebo.EVENT_DTYPE), ev)  # the caller's events are untouched
        c.set_windows8(ev8, t_base, offsets)
        _assert_same(_snapshot(ebo, c, n_windows, gt), ref, "ebo_set_windows8")
        d8 = torch.from_numpy(ev8.view(np.uint8).reshape(-1, 8)).to("cuda")
        c.set_windows8(d8.data_ptr(), t_base, offsets, device=True)
        _assert_same(_snapshot(ebo, c, n_windows, gt), ref, "ebo_set_windows8_device")
        # clearing restores the un-rectified result on the same context, bit for bit
        c.clear_rectification()
        c.set_windows(ev, offsets)
        _assert_same(_snapshot(ebo, c, n_windows, gt, solves=False), raw, "after ebo_clear_rectification")


def test_rectification_affects_the_next_load_only(ebo, synth):
    cfg, ev, rect, offsets, gt = _fixture(synth, 2, 3, 9000, camera_ref.DAVIS)
    kw = dict(image_w=240, image_h=180, patch_w=30, patch_h=22, loss=ebo.LOSS_VARIANCE, max_windows=3, max_events=len(ev))
    with ebo.Context(**kw) as c:
        c.set_windows(ev, offsets)
        before = _snapshot(ebo, c, 3, gt, solves=False)
        c.set_rectification(camera_ref.DAVIS)
        _assert_same(_snapshot(ebo, c, 3, gt, solves=False), before, "resident windows keep their geometry")
        # the host-sorted shard path does not rectify and says so
        with pytest.raises(ebo.EboError) as ei:
            c.set_patches(ev[:100], [0, 100], [[0, 0, 30, 22]])
        assert ei.value.code == ebo.ERR_UNSUPPORTED
        _assert_same(_snapshot(ebo, c, 3, gt, solves=False), before, "a refused call changes nothing")
        c.set_windows(ev, offsets)
        after = _snapshot(ebo, c, 3, gt, solves=False)
        assert after[0] != before[0]
        c.clear_rectification()
        c.set_patches(ev[:100], [0, 100], [[0, 0, 30, 22]])  # allowed again
        c.set_windows(ev, offsets)
        _assert_same(_snapshot(ebo, c, 3, gt, solves=False), before, "after ebo_clear_rectification")


def test_host_counting_sort_rectifies_too(ebo_ab, synth, monkeypatch):
    """EBO_BUCKET=host (the A/B build's switch; also what a grid too fine for the device histogram takes)."""
    ebo = ebo_ab
    cfg, ev, rect, offsets, gt = _fixture(synth, 2, 2, 9000, camera_ref.DAVIS)
    kw = dict(image_w=240, image_h=180, patch_w=30, patch_h=22, loss=ebo.LOSS_VARIANCE, max_windows=2, max_events=len(ev))
    with ebo.Context(**kw) as c:
        c.set_windows(rect, offsets)
        ref = _snapshot(ebo, c, 2, gt, solves=False)
        c.set_rectification(camera_ref.DAVIS)
        monkeypatch.setenv("EBO_BUCKET", "host")
        c.set_windows(ev, offsets)
        _assert_same(_snapshot(ebo, c, 2, gt, solves=False), ref, "host counting sort")


def test_compensate_windows_rectified(ebo, synth):
    """ebo_compensate_windows (chunks of what the context holds) with a rectification set = the same call on
    host-rectified events without one, window by window."""
    cfg, ev, rect, offsets, gt = _fixture(synth, 2, 7, 9000, camera_ref.DAVIS)
    kw = dict(image_w=240, image_h=180, patch_w=30, patch_h=22, loss=ebo.LOSS_VARIANCE, max_windows=3, max_events=30000)
    opts = ebo.default_solver(mode=ebo.SOLVE_INDEPENDENT, max_num_iterations=5)
    with ebo.Context(**kw) as c:
        want = c.compensate_windows(rect, offsets, opts)
        one_want = c.compensate_events_contrast(rect[int(offsets[2]):int(offsets[3])], opts)
        c.set_rectification(camera_ref.DAVIS)
        got = c.compensate_windows(ev, offsets, opts)
        one = c.compensate_events_contrast(ev[int(offsets[2]):int(offsets[3])], opts)
    assert not want[4].any() and not got[4].any()
    for k in range(3):
        assert np.array_equal(bits(got[k]), bits(want[k])), k
    assert np.array_equal(bits(one[0]), bits(one_want[0])) and np.array_equal(bits(one[1]), bits(one_want[1]))
