"""CPU: the two encodings of a value tap's fixed-point word are the same integer (DESIGN.md 4.1 item 14,
csrc/fix_form.h), and the host's rule for choosing between them.

  biased     bits(fma(a, b, 1.5 * 2^k)) - bits(1.5 * 2^k)                    (libm's fma: one rounding)
  subnormal  bits((a * 2^-511) * (b * 2^-(511 + k)))                         (IEEE multiply into the subnormal range)

Both are RNE(a b / 2^(k - 52)); the bias is an even multiple of the grid step, so ties break alike.  Every comparison
is exact.  numpy's float64 multiply is the host's IEEE multiply (no flush to zero)."""
import ctypes
import ctypes.util
import math
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
KS = [-6, -3, 0, 2, 5]
N_RANDOM = 75_000   # per k; with N_TIES forced ties: >= 1e5 triples, at least a quarter of them ties
N_TIES = 30_000


def _libm_fma():
    libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
    libm.fma.restype = ctypes.c_double
    libm.fma.argtypes = [ctypes.c_double] * 3
    return libm.fma


def _bits(x):
    return np.asarray(x, dtype=np.float64).view(np.int64)


def biased(fma, a, b, k):
    bias = math.ldexp(1.5, k)
    s = np.array([fma(float(x), float(y), bias) for x, y in zip(a, b)], dtype=np.float64)
    return _bits(s) - _bits(np.float64(bias))


def subnormal(a, b, k):
    pa = np.asarray(a, dtype=np.float64) * math.ldexp(1.0, -511)
    pb = np.asarray(b, dtype=np.float64) * math.ldexp(1.0, -(511 + k))
    # the rule's premise: scaling by a power of two is exact while the result is normal (or the weight is 0)
    tiny = math.ldexp(1.0, -1022)
    assert (((pa >= tiny) | (pa == 0)) & (pb >= tiny)).all()
    return _bits(pa * pb)


def random_triples(rng, k, n):
    """Weights as the kernels see them: b an outer-to-centre axis weight in (2^-8, 1], a b log-uniform from 2^-8 of a
    grid step up to the largest tap the grid admits, 2^(k-1)."""
    b = np.exp2(-rng.uniform(0.0, 8.0, n))
    t = np.exp2(rng.uniform(k - 60.0, k - 1.0, n))
    a = t / b
    a[a * b >= math.ldexp(1.0, k - 1)] *= 0.5
    return a, b


def tie_triples(rng, k, n):
    """a b EXACTLY an odd multiple of half a grid step, 2^(k-53): a = o1 2^e1, b = o2 2^e2 with odd o1, o2 < 2^26 (the
    product of the mantissas is exact and odd) and e1 + e2 = k - 53."""
    o1 = rng.integers(0, 1 << 25, n) * 2 + 1
    o2 = rng.integers(0, 1 << 25, n) * 2 + 1
    # half of them small: ties between 0 and a few steps (1 x 1: half a step itself, which rounds to the even 0)
    small = rng.random(n) < 0.5
    o1[small] = rng.integers(0, 4, small.sum()) * 2 + 1
    o2[small] = rng.integers(0, 4, small.sum()) * 2 + 1
    e2 = -rng.integers(26, 34, n)             # b = o2 2^e2 in (2^-34, 1)
    e1 = (k - 53) - e2
    a = np.ldexp(o1.astype(np.float64), e1)
    b = np.ldexp(o2.astype(np.float64), e2)
    q2 = o1.astype(object) * o2.astype(object)  # a b in units of half a step
    assert all(int(v) % 2 == 1 and int(v) < (1 << 53) for v in q2[:64])
    return a, b, q2


@pytest.fixture(scope="module")
def fma():
    f = _libm_fma()
    # a fused fma: (1 + 2^-30)^2 - (1 + 2^-29) = 2^-60 exactly, lost by a multiply that rounds first
    x = 1.0 + math.ldexp(1.0, -30)
    assert f(x, x, -(1.0 + math.ldexp(1.0, -29))) == math.ldexp(1.0, -60)
    return f


@pytest.mark.parametrize("k", KS)
def test_random_and_tie_triples(fma, k):
    rng = np.random.default_rng(1000 + k)
    a, b = random_triples(rng, k, N_RANDOM)
    at, bt, q2 = tie_triples(rng, k, N_TIES)
    assert N_TIES * 4 >= N_RANDOM + N_TIES and N_RANDOM + N_TIES >= 100_000
    assert np.array_equal(biased(fma, a, b, k), subnormal(a, b, k))
    wb, ws = biased(fma, at, bt, k), subnormal(at, bt, k)
    assert np.array_equal(wb, ws)
    # and the ties went to the even neighbour: q2 = 2 q + 1 half steps -> q if q is even, q + 1 if odd
    q = np.array([int(v) // 2 for v in q2], dtype=np.int64)
    assert np.array_equal(ws, q + (q & 1))


@pytest.mark.parametrize("k", KS)
def test_edges_of_the_grid(fma, k):
    step = math.ldexp(1.0, k - 52)
    top = math.ldexp(1.0, k - 1)  # the grid admits taps below 2^(k-1)
    a, b, want = [], [], []
    # below half a step: 0; exactly half a step: the tie goes to the even 0; just above: 1
    for p, w in ((step * 0.25, 0), (step * 0.4999999, 0), (math.ldexp(1.0, k - 300), 0), (step * 0.5, 0),
                 (math.nextafter(step * 0.5, 1.0), 1), (step * 1.5, 2), (step * 2.5, 2)):
        for bb in (1.0, 0.25, math.ldexp(1.0, -8)):
            a.append(p / bb), b.append(bb), want.append(w)
    # a = 0
    for bb in (1.0, 0.3, math.ldexp(1.0, -8)):
        a.append(0.0), b.append(bb), want.append(0)
    # just under the largest tap: the last words of the grid, and products that round up onto 2^(k-1) itself
    for m in (1, 2, 3, 1000):
        a.append(top - m * step), b.append(1.0), want.append((1 << 51) - m)
    for p in (math.nextafter(top, 0.0), top * (1.0 - math.ldexp(1.0, -53))):
        a.append(p * 2.0), b.append(0.5), want.append(1 << 51)
    a, b = np.array(a), np.array(b)
    wb, ws = biased(fma, a, b, k), subnormal(a, b, k)
    assert np.array_equal(wb, ws)
    assert np.array_equal(ws, np.array(want, dtype=np.int64))


def test_host_rule(tmp_path):
    """csrc/fix_form.h as the host compiles it: the subnormal form where 2^-400 <= norm <= 2^400 and |k| <= 400, and the
    prefactors norm 2^-511 and 2^-(511 + k).  Every sigma ebo_create admits (0.25 ... 1e3) passes, with the smallest
    scaled weights of the sigma >= 1 path (e^-8 of the prefactors, on a grid raised by 32) far above 2^-1022."""
    exe = str(tmp_path / "fix_form_test")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-o", exe,
                           os.path.join(HERE, "cpp", "fix_form_test.cpp")])
    cases = []
    for sigma in (0.25, 0.5, 1.0, 3.0, 1e3):
        norm = 1.0 / ((2 * math.pi) * (sigma * sigma))
        k = 0
        while norm >= math.ldexp(0.5, k):
            k += 1
        cases.append((norm, k, 400))
    cases += [(math.ldexp(1.0, -400), 0, 400), (math.nextafter(math.ldexp(1.0, -400), 0.0), 0, 400),
              (math.ldexp(1.0, 400), 0, 400), (math.nextafter(math.ldexp(1.0, 400), math.inf), 0, 400),
              (0.159, 400, 400), (0.159, 401, 400), (0.159, -400, 400), (0.159, -401, 400),
              (0.0, 0, 400), (math.inf, 0, 400), (math.nan, 0, 400), (5e-324, 0, 400),
              (0.159, 0, 1), (0.5, 0, 1), (0.5, 2, 1)]
    args = []
    for norm, k, g in cases:
        args += [float(norm).hex() if math.isfinite(norm) else repr(norm), str(k), str(g)]
    out = subprocess.run([exe] + args, capture_output=True, text=True, timeout=60, check=True).stdout.split("\n")
    for (norm, k, g), line in zip(cases, out):
        ok, bx, by = line.split()
        want = math.isfinite(norm) and math.ldexp(1.0, -g) <= norm <= math.ldexp(1.0, g) and abs(k) <= g
        assert int(ok) == int(want), (norm, k, g, line)
        if want:
            px = np.array([int(bx, 16)], dtype=np.uint64).view(np.float64)[0]
            py = np.array([int(by, 16)], dtype=np.uint64).view(np.float64)[0]
            assert px == norm * math.ldexp(1.0, -511) and py == math.ldexp(1.0, -(511 + k))
            assert math.frexp(px)[0] == math.frexp(norm)[0]  # the mantissa is norm's
            if g == 400:
                assert min(px, py * math.ldexp(1.0, -32)) * math.exp(-8.0) > math.ldexp(1.0, -1022 + 60)
    assert all(int(line.split()[0]) == 1 for line in out[:5])  # the admitted sigmas
