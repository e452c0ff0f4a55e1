"""Batched replay: ebo_compensate_windows (R2 + R3 for many windows in lock-step chunks) against the one-window path,
window by window, and tools::EventPump with EvaluatorParams::windowBatch > 1 against the unbatched pump
(tests/cpp/replay_batch_test.cpp)."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CPP = os.path.join(HERE, "cpp")
LIBDIR = os.path.join(ROOT, "event-based-odomety_amd")
ORACLE = os.path.join(ROOT, "oracle")

LOSS_MODES = [("edge", "global"), ("variance", "global"), ("edge", "independent"), ("variance", "independent")]


def recording(ebo, synth, n_windows, seed=0):
    """Windows of different sizes, the second one a single event and the third one too small for any patch to be
    active (compensateMinNumEvents = 100 per patch)."""
    evs = []
    for w in range(n_windows):
        n = [1500, 1, 90][w] if w < 3 else 1500 + (w * 977 + seed * 131) % 4500
        e, _ = synth.make_window(0, window=w + 100 * seed, n_events=max(n, 2))
        evs.append(e[:n])
    offsets = np.zeros(n_windows + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(e) for e in evs])
    return np.ascontiguousarray(np.concatenate(evs), dtype=ebo.EVENT_DTYPE), offsets


def opts_of(ebo, mode):
    o = ebo.default_solver()
    o.mode = ebo.SOLVE_GLOBAL if mode == "global" else ebo.SOLVE_INDEPENDENT
    return o


def kw_of(ebo, loss):
    return dict(image_w=240, image_h=180, patch_w=20, patch_h=20, loss=ebo.LOSS_EDGE if loss == "edge" else ebo.LOSS_VARIANCE)


def alone(ebo, loss, mode, ev, offsets, ws, at=None):
    """The one-window path per window: ebo_compensate_events_contrast, then ebo_set_window + ebo_count_image
    (INTEGRATED) -- compensateEventsContrast + integrateEvents of the facade -- and, with `at` (flows [Wn][P][2]),
    count_image(WARPED) of the window alone at at[w]."""
    out = {}
    cap = int(max(offsets[w + 1] - offsets[w] for w in ws))
    with ebo.Context(**kw_of(ebo, loss), max_events=cap, max_windows=1) as c:
        for w in ws:
            sub = ev[int(offsets[w]):int(offsets[w + 1])]
            flows, warped, s = c.compensate_events_contrast(sub, opts_of(ebo, mode))
            c.set_window(sub)
            integrated = c.count_image(ebo.COUNT_INTEGRATED)[0]
            warped_at = c.count_image(ebo.COUNT_WARPED, at[w:w + 1])[0] if at is not None else warped
            out[w] = (flows, warped_at, integrated, s)
    return out


def summary_tuple(s):
    return (s.iterations, s.num_evals_cost, s.num_evals_jac, s.termination, s.initial_cost, s.final_cost)


def assert_window_equal(got, want, w, flow_atol=0.0):
    """Bit for bit; flow_atol > 0 (the variance loss's TV-coupled solve in a chunk of >= 1024 units): the
    flows within flow_atol with the same iteration and evaluation counts, the warped image that of the returned flows."""
    flows, warped, integrated, s = got
    wflows, wwarped, wintegrated, ws = want
    assert np.array_equal(integrated, wintegrated), "window %d: integrated image" % w
    assert np.array_equal(warped, wwarped), "window %d: warped image" % w
    if flow_atol:
        np.testing.assert_allclose(flows, wflows, rtol=0, atol=flow_atol, err_msg="window %d" % w)
        assert summary_tuple(s)[:4] == summary_tuple(ws)[:4], "window %d: %s against %s" % (w, summary_tuple(s), summary_tuple(ws))
        return
    assert np.array_equal(flows, wflows), "window %d: flows differ by up to %.3g" % (w, np.abs(flows - wflows).max())
    assert summary_tuple(s) == summary_tuple(ws), "window %d: summary %s against %s" % (w, summary_tuple(s), summary_tuple(ws))


# one chunk of 1, 3 and 21 windows; 70 windows in chunks of 16 (the last one ragged)
CASES = [(loss, mode, n, mw) for (n, mw) in [(1, 1), (3, 3), (21, 21), (70, 16)] for (loss, mode) in LOSS_MODES]


@pytest.mark.gpu
@pytest.mark.parametrize("loss,mode,n_windows,max_windows", CASES, ids=["%s-%s-%dw-chunk%d" % c for c in CASES])
def test_compensate_windows_equals_the_one_window_path(ebo, synth, loss, mode, n_windows, max_windows):
    ev, offsets = recording(ebo, synth, n_windows, seed=n_windows)
    cap = int(max(offsets[w + 1] - offsets[w] for w in range(n_windows)))
    with ebo.Context(**kw_of(ebo, loss), max_events=cap * max_windows, max_windows=max_windows) as c:
        flows, warped, integrated, summ, status = c.compensate_windows(ev, offsets, opts_of(ebo, mode))
    assert not status.any()
    want = alone(ebo, loss, mode, ev, offsets, range(n_windows), at=flows)
    # k_eval3's workgroup width follows the launch's unit count, and its f64 pixel sums are added in that lane order
    # (DESIGN.md §2): a chunk of >= 1024 units (10 windows) may part from a window alone in the last bits of a flow
    atol = 1e-7 if (loss, mode) == ("variance", "global") and min(n_windows, max_windows) * 109 >= 1024 else 0.0
    for w in range(n_windows):
        assert_window_equal((flows[w], warped[w], integrated[w], summ[w]), want[w], w, atol)
    if n_windows >= 3:
        assert not flows[2].any()  # no active patch: nothing moves


@pytest.mark.gpu
def test_warped_image_is_the_count_image_at_the_returned_flows(ebo, synth):
    ev, offsets = recording(ebo, synth, 5, seed=3)
    with ebo.Context(**kw_of(ebo, "edge"), max_events=len(ev), max_windows=5) as c:
        flows, warped, integrated, _, status = c.compensate_windows(ev, offsets)
    assert not status.any()
    with ebo.Context(**kw_of(ebo, "edge"), max_events=len(ev), max_windows=1) as c:
        for w in range(5):
            c.set_window(ev[int(offsets[w]):int(offsets[w + 1])])
            assert np.array_equal(c.count_image(ebo.COUNT_WARPED, flows[w:w + 1])[0], warped[w])
            assert np.array_equal(c.count_image(ebo.COUNT_INTEGRATED)[0], integrated[w])


@pytest.mark.gpu
def test_a_refused_window_fails_alone(ebo, synth):
    """A coordinate of 20000 (outside the packed [-16384, 16383]) in one window of a chunk: the loader's range flag
    refuses that window (EBO_ERR_RANGE, outputs untouched); its neighbours are those of a run without it, bit for bit.
    An empty window is refused as ebo_compensate_events_contrast refuses it."""
    ev, offsets = recording(ebo, synth, 9, seed=5)
    bad = 4
    ev["x"][int(offsets[bad]) + 17] = 20000
    # an empty window after the last one
    offsets = np.append(offsets, offsets[-1])
    n = len(offsets) - 1
    kw = dict(kw_of(ebo, "edge"), max_events=len(ev), max_windows=6)
    with ebo.Context(**kw) as c:
        flows, warped, integrated, summ, status = c.compensate_windows(ev, offsets)
        keep = [w for w in range(n - 1) if w != bad]
        sub = np.concatenate([ev[int(offsets[w]):int(offsets[w + 1])] for w in keep])
        sub_off = np.concatenate([[0], np.cumsum([int(offsets[w + 1] - offsets[w]) for w in keep])]).astype(np.uint64)
        f2, wa2, in2, s2, st2 = c.compensate_windows(sub, sub_off)
        # the call's return value names the first refused window
        with pytest.raises(ebo.EboError) as ei:
            c._check(ebo.lib().ebo_compensate_windows(c._h, ebo._vp(ev), ebo._vp(offsets), n, None, ebo._dp(flows),
                                                     None, None, None, None))
        assert ei.value.code == ebo.ERR_ARG  # null solver options: an error of the call itself
    assert status[bad] == ebo.ERR_RANGE and status[n - 1] == ebo.ERR_ARG
    assert [w for w in range(n) if status[w]] == [bad, n - 1] and not st2.any()
    assert not flows[bad].any() and not warped[bad].any() and not integrated[bad].any()
    for j, w in enumerate(keep):
        assert np.array_equal(flows[w], f2[j]) and np.array_equal(warped[w], wa2[j])
        assert np.array_equal(integrated[w], in2[j]) and summary_tuple(summ[w]) == summary_tuple(s2[j])
    with ebo.Context(**kw) as c:
        rc = ebo.lib().ebo_compensate_windows(c._h, ebo._vp(ev), ebo._vp(offsets), n,
                                              __import__("ctypes").byref(ebo.default_solver()), ebo._dp(flows),
                                              None, None, None, None)
        assert rc == ebo.ERR_RANGE and ("window %d" % bad) in ebo.lib().ebo_last_error(c._h).decode()


@pytest.mark.gpu
def test_events_txt_cut_and_compensated(ebo, synth, tmp_path):
    """A synthesized events.txt, read with ebo_read_events_txt, cut with the reference's rule and compensated in
    chunks: the per-window calls over the same cut give the same results."""
    ev0, _, _ = synth.make_stream(0, 8, n_events=2500)
    path = tmp_path / "events.txt"
    synth.write_events_txt(str(path), ev0)
    ev = ebo.read_events_txt(str(path), cap=len(ev0) + 8)
    begin, end, _, pending = ebo.cut_windows(ev, time_us=300000, count=3000, max_store=15000)
    assert len(begin) >= 6 and int(end[0]) == 1 and pending < len(ev)
    # consecutive windows: the events of a window start where the previous one ended (nothing truncated)
    assert np.array_equal(begin[1:], end[:-1])
    offsets = np.concatenate([begin[:1], end]).astype(np.uint64)
    with ebo.Context(**kw_of(ebo, "edge"), max_events=4 * 3000, max_windows=4) as c:
        flows, warped, integrated, summ, status = c.compensate_windows(ev, offsets)
    assert not status.any()
    want = alone(ebo, "edge", "global", ev, offsets, range(len(begin)), at=flows)
    for w in range(len(begin)):
        assert_window_equal((flows[w], warped[w], integrated[w], summ[w]), want[w], w)


def build_driver(ebo, out):
    """tests/cpp/replay_batch_test.cpp with the compiler line of tests/cpp/Makefile's facade_test."""
    ebo.lib()
    subprocess.check_call(["make", "-s", "-C", ORACLE, "liboracle.so"])
    subprocess.check_call(["g++", "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", str(out),
                           os.path.join(CPP, "replay_batch_test.cpp"),
                           "-L" + LIBDIR, "-lebo_hip", "-L" + ORACLE, "-loracle",
                           "-Wl,-rpath," + LIBDIR, "-Wl,-rpath," + ORACLE, "-Wl,-rpath,/opt/rocm/lib"])
    return str(out)


def test_replay_batch_driver_compiles(ebo, tmp_path):
    """CPU: the batched EventPump (EvaluatorParams::windowBatch, FeatureDetector::compensateWindows) compiles under
    -Wall -Wextra against the library."""
    assert os.path.exists(build_driver(ebo, tmp_path / "replay_batch_test"))


@pytest.mark.gpu
def test_batched_event_pump_equals_the_unbatched_one(ebo, synth, tmp_path):
    exe = build_driver(ebo, tmp_path / "replay_batch_test")
    ev, _, _ = synth.make_stream(0, 60, n_events=3000)
    good, bad = tmp_path / "good.bin", tmp_path / "bad.bin"
    ebo.write_events_bin(str(good), ev)
    ev = ev.copy()
    ev["x"][len(ev) // 2] = 20000  # one window the loader refuses
    ebo.write_events_bin(str(bad), ev)
    out = subprocess.run(["timeout", "-k", "10", "600", exe, "check", str(good), str(bad), "300000", "2500"],
                         capture_output=True, text=True)
    print(out.stdout[-4000:], out.stderr[-2000:])
    assert out.returncode == 0, out.stdout[-4000:]
    assert "all passed" in out.stdout
