"""CPU: the sigma >= 1 path's exponentials (csrc/exp_taps.h) against expl.

The yardstick is the polynomial they replace -- exp_small, degree-12 Taylor on x / 4 and two squarings -- restated in
tests/cpp/exp_taps_test.cpp and measured on the same points (about 7.6e-16 on [-1, 1], 5.0e-16 on [-0.5, 0]).

  exp_pair   exp(a) and exp(-a) from a shared cosh / sinh: at most 2 x the yardstick.  C - S amplifies the parts'
             errors by (C + S) / (C - S) <= e^0.5 = 1.65 at |t| <= 0.25, and one rounding of the extra add comes on top.
  exp_gauss  exp(hs f^2), argument in [-0.5, 0]: not above the yardstick on that interval.
"""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
POINTS = 1 << 20   # >= 1e6, plus +-1 and +-0 inside the program


@pytest.fixture(scope="module")
def figures(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("exp_taps") / "exp_taps_test")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O2", "-ffp-contract=off", "-o", exe,
                           os.path.join(HERE, "cpp", "exp_taps_test.cpp")])
    out = subprocess.run([exe, "20261019", str(POINTS)], capture_output=True, text=True, timeout=120, check=True).stdout
    fig = {}
    for line in out.strip().split("\n"):
        name, *vals = line.split()
        fig[name] = [float(v) for v in vals]
    print(out)
    return fig


def test_yardstick_is_the_polynomial_measured_before(figures):
    yard, yard_half = figures["yard"]
    # one to two ulp: a yardstick far from the recorded figures would mean the restatement is not exp_small
    assert 4e-16 < yard < 1e-15
    assert 3e-16 < yard_half <= yard


def test_pair_within_twice_the_yardstick(figures):
    yard, _ = figures["yard"]
    pair, prod = figures["pair"]
    assert pair <= 2.0 * yard
    assert prod <= 4.0 * yard   # p q = exp(a) exp(-a): both errors and one rounding


def test_gauss_not_above_the_yardstick(figures):
    _, yard_half = figures["yard"]
    assert figures["gauss"][0] <= yard_half


def test_zero_arguments_are_exact(figures):
    assert figures["edge"] == [1.0] * 6
