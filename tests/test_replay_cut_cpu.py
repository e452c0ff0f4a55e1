"""CPU: ebo_cut_windows against a restatement of the reference's replay, event by event --
tools::Evaluator::eventCallback (tools/evaluator/src/evaluator.cpp:32-45) calling FeatureDetector::addEvent
(feature_detector.cpp:621-628): push, pop the front while more than maxNumEventsToStore are held, then
`ts - lastCompensation >= time || size >= count` compensates the held events and lastCompensation = ts."""
import collections

import numpy as np
import pytest


def restated(ts, time_us, count, max_store, last):
    held = collections.deque()
    windows = []
    for i, t in enumerate(ts.tolist()):
        held.append(i)  # addEvent
        while len(held) > max_store:
            held.popleft()
        if t - last >= time_us or len(held) >= count:  # eventCallback
            windows.append((held[0], held[-1] + 1))
            last = t  # compensateEventsContrast: lastCompensation = events.back().timestamp
            held.clear()  # clearEvents
    pending = held[0] if held else len(ts)
    return windows, last, pending


def stream(seed, n, t0, mean_dt, ties=0.0):
    rng = np.random.default_rng(seed)
    dt = rng.exponential(mean_dt, n).astype(np.int64)
    if ties:
        dt[rng.random(n) < ties] = 0  # runs of equal timestamps
    return t0 + np.cumsum(dt)


def events(ebo, ts):
    rng = np.random.default_rng(len(ts))
    return ebo.make_events(rng.integers(0, 240, len(ts)), rng.integers(0, 180, len(ts)), ts,
                           np.where(rng.random(len(ts)) < 0.5, -1, 1))


CASES = [
    # name, seed, n, t0, mean dt (us), ties, time_us, count, max_store, last_compensation_us
    ("default rule", 1, 60000, 1_000_000, 20, 0.0, 300000, 15000, 15000, 0),
    ("default rule, slow stream", 2, 20000, 1_000_000, 60, 0.0, 300000, 15000, 15000, 0),
    ("count only", 3, 30000, 0, 5, 0.0, 1 << 31, 1000, 15000, 0),
    ("time only", 4, 30000, 0, 37, 0.0, 50000, 1 << 31, 1 << 40, 0),
    ("count > max_store: truncation, time rule only", 5, 40000, 1_000_000, 15, 0.0, 100000, 5000, 3000, 0),
    ("count < max_store", 6, 40000, 1_000_000, 15, 0.0, 100000, 2000, 3000, 0),
    ("count == max_store", 7, 40000, 1_000_000, 15, 0.0, 100000, 3000, 3000, 0),
    ("runs of equal timestamps", 8, 50000, 0, 9, 0.7, 20000, 1500, 1200, 0),
    ("first event at 300 ms: a one-event window", 9, 5000, 300000, 30, 0.0, 300000, 15000, 15000, 0),
    ("first event just before 300 ms", 10, 5000, 299999, 30, 0.0, 300000, 15000, 15000, 0),
    ("nonzero last compensation", 11, 30000, 5_000_000, 20, 0.2, 300000, 2500, 15000, 4_900_000),
    ("last compensation after the stream's start", 12, 30000, 5_000_000, 20, 0.0, 300000, 2500, 2400, 5_100_000),
    ("count 1: every event a window", 13, 2000, 0, 3, 0.5, 300000, 1, 15000, 0),
    ("max_store 1", 14, 3000, 0, 50, 0.0, 2000, 5, 1, 0),
]


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_cut_windows_equals_the_reference_rule(ebo, case):
    _, seed, n, t0, mean_dt, ties, time_us, count, max_store, last0 = case
    ts = stream(seed, n, t0, mean_dt, ties)
    ev = events(ebo, ts)
    want, want_last, want_pending = restated(ts, time_us, count, max_store, last0)
    begin, end, last, pending = ebo.cut_windows(ev, time_us=time_us, count=min(count, 2**32 - 1),
                                                max_store=max_store, last_compensation_us=last0)
    assert len(want) > 0
    assert list(zip(begin.tolist(), end.tolist())) == want
    assert (last, pending) == (want_last, want_pending)


def test_first_event_of_a_recording_fires_alone(ebo):
    ts = stream(21, 4000, 1_000_000, 20)
    begin, end, _, _ = ebo.cut_windows(events(ebo, ts))
    assert (int(begin[0]), int(end[0])) == (0, 1)


def test_truncated_windows_hold_at_most_max_store(ebo):
    ts = stream(22, 40000, 1_000_000, 15)
    begin, end, _, _ = ebo.cut_windows(events(ebo, ts), time_us=100000, count=5000, max_store=3000)
    sizes = (end - begin).astype(np.int64)
    assert sizes.max() == 3000 and (begin[1:] > end[:-1]).any()  # events were dropped between windows


def test_streaming_continues_from_pending_begin(ebo):
    """Cutting a stream in two pieces (the held events carried over) gives the windows of one cut."""
    ts = stream(23, 50000, 1_000_000, 20, 0.1)
    ev = events(ebo, ts)
    kw = dict(time_us=300000, count=4000, max_store=3500)
    b, e, last, pending = ebo.cut_windows(ev, **kw)
    b1, e1, last1, p1 = ebo.cut_windows(ev[:21000], **kw)
    b2, e2, last2, p2 = ebo.cut_windows(ev[p1:], last_compensation_us=last1, **kw)
    # the carried events were held (and truncated) the same way: the windows agree
    assert np.array_equal(np.concatenate([b1, b2 + p1]), b) and np.array_equal(np.concatenate([e1, e2 + p1]), e)
    assert (last2, p2 + p1) == (last, pending)


def test_empty_stream(ebo):
    begin, end, last, pending = ebo.cut_windows(ebo.make_events([], [], []), last_compensation_us=77)
    assert len(begin) == 0 and len(end) == 0 and last == 77 and pending == 0


def test_cap_too_small_reports_the_count_needed(ebo):
    import ctypes as C
    ts = stream(24, 10000, 1_000_000, 20)
    ev = events(ebo, ts)
    want, _, _ = restated(ts, 300000, 1000, 15000, 0)
    begin = np.zeros(3, dtype=np.uint64)
    end = np.zeros(3, dtype=np.uint64)
    nw, last, pending = C.c_size_t(), C.c_int64(), C.c_size_t()
    rc = ebo.lib().ebo_cut_windows(ev.ctypes.data_as(C.c_void_p), C.c_size_t(len(ev)), C.c_int64(0),
                                   C.c_uint32(300000), C.c_uint32(1000), C.c_uint64(15000),
                                   begin.ctypes.data_as(C.c_void_p), end.ctypes.data_as(C.c_void_p), C.c_size_t(3),
                                   C.byref(nw), C.byref(last), C.byref(pending))
    assert rc == ebo.ERR_RANGE and nw.value == len(want) > 3
    rc = ebo.lib().ebo_cut_windows(ev.ctypes.data_as(C.c_void_p), C.c_size_t(len(ev)), C.c_int64(0),
                                   C.c_uint32(300000), C.c_uint32(1000), C.c_uint64(15000), None, None, C.c_size_t(0),
                                   C.byref(nw), C.byref(last), C.byref(pending))
    assert rc == ebo.ERR_RANGE and nw.value == len(want)


def test_max_store_zero_is_refused(ebo):
    ts = stream(25, 100, 0, 20)
    with pytest.raises(ebo.EboError) as ei:
        ebo.cut_windows(events(ebo, ts), max_store=0)
    assert ei.value.code == ebo.ERR_ARG
