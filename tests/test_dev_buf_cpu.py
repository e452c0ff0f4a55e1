"""CPU: the owner type of the context's device and pinned buffers (csrc/dev_buf.h, the one grow rule of the host
sources) is free of HIP; tests/cpp/dev_buf_test.cpp drives it with a memory policy that counts allocations and
releases and fails the k-th allocation on request: a buffer that fits keeps its pointer, growth releases one
allocation and makes one, a failed growth leaves an empty buffer, "allocation not allowed" refuses without touching
anything, move and swap transfer ownership once, the three blocks of the evaluation staging are all there or all
gone, and nothing is live at the end of any scenario.  Plain and under AddressSanitizer + UBSan."""
import os
import subprocess

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")


@pytest.mark.parametrize("binary", ["dev_buf_test", "dev_buf_test_asan"])
def test_dev_buf_owner_type(binary):
    subprocess.check_call(["make", "-s", "-C", CPP, binary])
    out = subprocess.run([os.path.join(CPP, binary)], capture_output=True, text=True, timeout=300)
    text = out.stdout + out.stderr
    assert out.returncode == 0, text[-4000:]
    assert "all passed" in out.stdout
    for bad in ("AddressSanitizer", "runtime error", "LeakSanitizer"):
        assert bad not in text, text[-4000:]
