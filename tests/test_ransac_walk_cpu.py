"""CPU: the serial stopping rule both RANSAC paths share (csrc/ransac_walk.h, free of HIP) against its two numpy
restatements: twoview_ref.ransac_walk (rule 6, sample size 8) and abspose_ref.ransac_walk (A5, sample size 4).
tests/cpp/ransac_walk_test.cpp reads the cases from stdin and prints (best, winner, iterations) per case; the integers
must be equal.  The rule decides `winner`, `iterations` and `found` of every RANSAC call, so the cases sit where it can
go wrong: one hypothesis, no inliers at all, the maximum first, equal maxima (the first wins), every point an inlier
(w = 1: the lower clamp binds), one inlier of 65535 (the upper clamp binds), three probabilities, and random count
vectors up to the 4096 hypotheses a call admits.  Plain and under AddressSanitizer + UBSan."""
import os
import subprocess

import numpy as np
import pytest

import abspose_ref
import twoview_ref

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")
RESTATEMENT = {8: twoview_ref.ransac_walk, 4: abspose_ref.ransac_walk}
PROBABILITIES = (0.5, 0.99, 1.0 - 1e-12)


def _cases():
    """-> [(n, counts)]: the named edge cases, then 300 random count vectors."""
    rng = np.random.default_rng(20240607)
    out = [
        (200, [57]),                                   # H = 1
        (200, [0]),
        (200, [0] * 50),                               # all counts zero: hypothesis 0 wins with best = 0
        (200, [150] + [10] * 99),                      # the maximum at h = 0
        (200, [3, 90, 12, 90, 90, 7] + [5] * 500),     # equal maxima: the first must win
        (200, [10, 20, 200] + [0] * 30),               # best == n: w = 1, the lower clamp binds
        (8, [8] * 4),
        (4, [4] * 4),
        (65535, [1] * 4096),                           # best = 1 of n = 65535: the upper clamp binds
        (65535, [0, 1, 0, 2] + [1] * 1000),
        (200, list(range(1, 101))),                    # a new best at every step
    ]
    for i in range(300):
        n = int(rng.integers(8, 65536)) if i % 3 else int(rng.integers(8, 600))
        H = int(rng.integers(1, 4097)) if i % 4 == 0 else int(rng.integers(1, 300))
        top = int(rng.integers(0, n + 1))
        shape = i % 5
        if shape == 0:
            c = rng.integers(0, top + 1, H)
        elif shape == 1:    # mostly failures, a few good hypotheses
            c = np.where(rng.random(H) < 0.05, rng.integers(0, top + 1, H), rng.integers(0, 9, H))
        elif shape == 2:    # slowly rising: many updates of the bound
            c = np.sort(rng.integers(0, top + 1, H))
        elif shape == 3:    # ties everywhere
            c = rng.choice(np.array([0, top // 2, top]), H)
        else:               # low inlier shares, where k stays near the cap
            c = rng.integers(0, max(1, n // 3) + 1, H)
        out.append((n, [int(v) for v in c]))
    return out


@pytest.fixture(scope="module")
def cases():
    """[(sampleSize, n, probability, counts)] and what the restatements say: [(best, winner, iterations)]."""
    rows, want = [], []
    for n, counts in _cases():
        for sample, walk in RESTATEMENT.items():
            for p in PROBABILITIES:
                found, winner, iterations, best = walk(np.array(counts), n, p, len(counts))
                assert found == (best >= sample)
                rows.append((sample, n, p, counts))
                want.append((best, winner, iterations))
    return rows, want


@pytest.mark.parametrize("binary", ["ransac_walk_test", "ransac_walk_test_asan"])
def test_walk_equals_both_restatements(binary, cases):
    rows, want = cases
    subprocess.check_call(["make", "-s", "-C", CPP, binary])
    text = "".join("%d %d %d %r\n%s\n" % (s, n, len(c), p, " ".join(map(str, c))) for s, n, p, c in rows)
    out = subprocess.run([os.path.join(CPP, binary)], input=text, capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    for bad in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert bad not in out.stderr, out.stderr[-4000:]
    got = [tuple(int(v) for v in line.split()) for line in out.stdout.splitlines()]
    assert len(got) == len(want)
    wrong = [(rows[i][:3], len(rows[i][3]), got[i], want[i]) for i in range(len(want)) if got[i] != want[i]]
    assert not wrong, wrong[:10]
    # the cases do reach both clamps and both ways of stopping
    its = np.array([w[2] for w in want])
    lens = np.array([len(r[3]) for r in rows])
    assert (its < lens).any() and (its == lens).any() and (its == 1).any()
