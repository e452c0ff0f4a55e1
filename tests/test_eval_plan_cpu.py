"""CPU: the launch plan of the variance evaluation (csrc/eval_plan.h) is free of HIP; tests/cpp/eval_plan_test.cpp sweeps
it over every patch geometry a context admits, both wave caps and both sides of 1024 flow slots, and pins the shapes the
batched evaluation runs at.  Built once plainly and once under AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "eval_plan_test.cpp")
HDR = os.path.join(os.path.dirname(HERE), "event-based-odomety_amd", "csrc", "eval_plan.h")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_plan_invariants_and_pinned_shapes(tmp_path, flags):
    assert os.path.exists(HDR)
    exe = str(tmp_path / "eval_plan_test")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-Wall", "-Wextra", *flags, "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "all passed" in out.stdout
