"""CPU checks of csrc/launch_order.h, the table by which k_eval3 and k_solve_independent hand a batch's units to
workgroups heaviest first: tests/cpp/launch_order_test.cpp compiles the header for the host, and its tables are compared
here with numpy's stable sort -- a permutation, keys (n_ev of an active unit, 0 of any other) non-increasing, equal keys
in index order, inactive and stray units last -- for n = 0, 1, all-equal, already-sorted and mixed inputs and 40 000
random counts (the benchmark's 128 x 257 units are 32 896).  The same program's `self` mode, which needs no input, is
what a sanitizer build runs; it is run here too, under -fsanitize=address,undefined where the host compiler links it."""
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "launch_order_test.cpp")
ACTIVE, STRAY = 1, 2


@pytest.fixture(scope="module")
def exe(tmp_path_factory):
    path = str(tmp_path_factory.mktemp("launch_order") / "launch_order_test")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-Wall", "-Wextra", "-o", path, SRC])
    return path


def _table(exe, n_ev, flags, kind=0):
    text = "%d %d\n" % (kind, len(n_ev)) + "".join("%d %d\n" % (a, f) for a, f in zip(n_ev, flags))
    out = subprocess.run([exe], input=text, capture_output=True, text=True, timeout=120, check=True).stdout.split()
    return np.array([int(v) for v in out], dtype=np.int64)


def _keys(n_ev, flags):
    n_ev, flags = np.asarray(n_ev, dtype=np.int64), np.asarray(flags, dtype=np.int64)
    return np.where(flags & ACTIVE, n_ev, 0)


def _check(exe, n_ev, flags):
    n = len(n_ev)
    key = _keys(n_ev, flags)
    o = _table(exe, n_ev, flags)
    assert len(o) == n and np.array_equal(np.sort(o), np.arange(n))  # a permutation
    k = key[o]
    assert (np.diff(k) <= 0).all()  # keys non-increasing
    assert (np.diff(o)[np.diff(k) == 0] > 0).all()  # equal keys in index order
    assert np.array_equal(o, np.argsort(-key, kind="stable"))  # i.e. THE stable sort
    assert np.array_equal(_table(exe, n_ev, flags, kind=1), np.arange(n))
    assert np.array_equal(_table(exe, n_ev, flags, kind=2), np.argsort(key, kind="stable"))
    return o


def test_empty_and_single(exe):
    _check(exe, [], [])
    _check(exe, [7], [ACTIVE])
    _check(exe, [7], [0])


def test_all_equal_is_the_identity(exe):
    o = _check(exe, [64] * 300, [ACTIVE] * 300)
    assert np.array_equal(o, np.arange(300))


def test_already_sorted_stays(exe):
    n_ev = np.arange(1000, 500, -1)
    o = _check(exe, n_ev, [ACTIVE] * len(n_ev))
    assert np.array_equal(o, np.arange(len(n_ev)))
    o = _check(exe, n_ev[::-1], [ACTIVE] * len(n_ev))
    assert np.array_equal(o, np.arange(len(n_ev))[::-1])


def test_inactive_and_stray_units_come_last(exe):
    """An inactive unit keeps its (small) n_ev and a stray bucket may hold thousands of events: neither runs an
    evaluation, so both sort as 0, behind every active unit and among themselves by index."""
    n_ev = [900, 3, 40, 2000, 0, 40, 12, 5000]
    flags = [STRAY, 0, ACTIVE, ACTIVE, 0, ACTIVE, 0, STRAY]
    o = _check(exe, n_ev, flags)
    assert list(o) == [3, 2, 5, 0, 1, 4, 6, 7]


def test_40000_random_counts(exe):
    rng = np.random.default_rng(11)
    n = 40000
    n_ev = rng.integers(0, 2000, n)
    flags = np.where(n_ev > 30, ACTIVE, 0)
    flags[256::257] = STRAY  # the stray bucket of every window of 256 patches
    n_ev[::1000] = 0xFFFFFFFF  # the largest count a unit can carry
    flags[::1000] = ACTIVE
    _check(exe, n_ev, flags)


def test_counting_and_comparison_paths_agree_at_their_threshold(exe):
    """The table comes from a counting sort while the largest key is at most 8 n + 1024 and from a comparison sort of
    (key, index) words above: the same table on both sides of that threshold, and with a single huge count."""
    rng = np.random.default_rng(12)
    n = 500
    for top in (8 * n + 1023, 8 * n + 1024, 8 * n + 1025, 1 << 20):
        n_ev = rng.integers(0, 40, n)  # many ties
        n_ev[7] = top
        flags = np.where(n_ev > 10, ACTIVE, 0)
        _check(exe, n_ev, flags)


def test_self_check_under_the_sanitizers(tmp_path):
    """The stand-alone form: the same edge cases and 40 000 counts checked inside the program, built with the address and
    undefined-behaviour sanitizers where the host compiler can link them (else plain)."""
    cxx = os.environ.get("CXX", "c++")
    path = str(tmp_path / "launch_order_self")
    san = ["-fsanitize=address,undefined", "-fno-sanitize-recover=all"]
    if subprocess.run([cxx, "-std=c++17", "-O1", "-g"] + san + ["-o", path, SRC], capture_output=True).returncode != 0:
        subprocess.check_call([cxx, "-std=c++17", "-O1", "-o", path, SRC])
    res = subprocess.run([path, "self"], capture_output=True, text=True, timeout=120)
    assert res.returncode == 0 and res.stdout.strip() == "ok", res.stdout + res.stderr
