"""CPU: the moment forms of the Jacobian sums (csrc/tap_moments.h) and the quarter-argument
exponentials (csrc/exp_taps.h), as tests/cpp/tap_moments_test.cpp measures them on 2^20 seeded events: the header's D1 and
D2 forms and the statements they replace (restated in the program) against a long-double evaluation, fx, fy in [0, 1) and
in (-1, 0], |g| <= 20, 7 x 7 values with zeros and large entries mixed.  Built once plainly and once under
AddressSanitizer + UBSan, a stand-alone program either way.

The bound of a new form is the OLD form's own maximum error on the same points times 4: g (A - f B) rounds once more than a
sum of weight x factor products, and the moment's differences (w6 - w0, ...) once each; a numpy model without FMAs saw a
factor 2.  Both maxima are printed.  The sum of the weights and the exponentials keep their bits: zero mismatches."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "tap_moments_test.cpp")
POINTS = 1 << 20
MARGIN = 4.0


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_moment_forms_within_four_times_the_old_forms_error(tmp_path, flags):
    exe = str(tmp_path / "tap_moments_test")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", *flags,
                           "-o", exe, SRC])
    out = subprocess.run([exe, "20261021", str(POINTS)], capture_output=True, text=True, timeout=300)
    print(out.stdout)
    fig = {}
    for line in out.stdout.strip().split("\n"):
        name, *vals = line.split()
        fig[name] = [float(v) for v in vals]
    for name in ("d1x", "d1y", "d2a", "d2b"):
        old, new = fig[name]
        # a few ulp of the scale: an old figure far from that would mean the restatement or the reference is broken
        assert 1e-16 < old < 5e-14, (name, old)
        assert new <= MARGIN * old, (name, old, new)
    assert fig["sumw"] == [0.0]
    assert fig["bits"] == [0.0]
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
