"""CPU: k_eval3's all-interior rule (csrc/eval_interior.h) is free of HIP; tests/cpp/eval_interior_test.cpp holds it against a
brute-force loop that mirrors warp_event, the sub-band's row test and the interior test event by event, over a seeded sweep
of a few thousand unit x flow x capacity cases (built once plainly and once under AddressSanitizer + UBSan, a stand-alone
program either way).  Wherever the rule admits a unit the brute force finds no rejected, skipped or clipped event; the share
of clean cases the rule refuses is printed, with no threshold on it."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "eval_interior_test.cpp")
HDR = os.path.join(os.path.dirname(HERE), "event-based-odomety_amd", "csrc", "eval_interior.h")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_rule_against_brute_force(tmp_path, flags):
    assert os.path.exists(HDR)
    exe = str(tmp_path / "eval_interior_test")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-Wall", "-Wextra", "-ffp-contract=off", *flags, "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    print(out.stdout[-2000:])
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "all passed" in out.stdout and "the rule refuses" in out.stdout
