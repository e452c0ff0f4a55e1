"""CPU: the arithmetic that takes k_eval3's bounding box from a unit's per-column / per-row time extents
(csrc/box_extents.h) is free of HIP; tests/cpp/box_extents_test.cpp compares it, over random units and flows from zero
to NaN, with a brute-force loop over the events: equal whenever the rule admits the table, and refused whenever an
event is rejected.  Built with -ffp-contract=off, as the kernels are, and once more under AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "box_extents_test.cpp")
HDR = os.path.join(os.path.dirname(HERE), "event-based-odomety_amd", "csrc", "box_extents.h")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_table_box_equals_the_event_loop(tmp_path, flags):
    assert os.path.exists(HDR)
    exe = str(tmp_path / "box_extents_test")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-ffp-contract=off", "-Wall", "-Wextra", *flags,
                           "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "all passed" in out.stdout
