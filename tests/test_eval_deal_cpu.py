"""CPU: the index arithmetic of k_eval3's bank deal (csrc/eval_deal.h) is free of HIP; tests/cpp/eval_deal_test.cpp holds
its maps against a brute-force walk for workgroups of 128, 256 and 512 lanes at unit sizes 1, 2, 127, 128, 129,
8 x block +- 1 and the admission bounds +- 1 (built once plainly and once under AddressSanitizer + UBSan), and the numpy
restatement the GPU test compares the device with (tools/ab/lds_conflict_model.py) is held against the same header."""
import importlib.util
import os
import subprocess

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
SRC = os.path.join(HERE, "cpp", "eval_deal_test.cpp")
PKG = os.path.join(os.path.dirname(HERE), "event-based-odomety_amd")
HDR = os.path.join(PKG, "csrc", "eval_deal.h")


@pytest.mark.parametrize("flags", [["-O2"], ["-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all"]],
                         ids=["plain", "asan-ubsan"])
def test_maps_against_brute_force(tmp_path, flags):
    assert os.path.exists(HDR)
    exe = str(tmp_path / "eval_deal_test")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-Wall", "-Wextra", *flags, "-o", exe, SRC])
    out = subprocess.run([exe], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "all passed" in out.stdout


def _model():
    spec = importlib.util.spec_from_file_location("lds_conflict_model", os.path.join(PKG, "tools", "ab", "lds_conflict_model.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_restatement_follows_the_header(tmp_path):
    """deal_positions (a cumulative sum over the slots) against the header's closed form, printed by a small program"""
    prog = tmp_path / "dump.cpp"
    prog.write_text('#include "%s"\n#include <cstdio>\n#include <cstdlib>\n'
                    'int main(int c, char** v) { unsigned n = std::atoi(v[1]); int b = std::atoi(v[2]);\n'
                    '  for (unsigned q = 0; q < n; ++q) std::printf("%%u\\n", ebo::deal_sorted_index(q, n, b)); return c < 3; }\n' % HDR)
    exe = str(tmp_path / "dump")
    subprocess.check_call([os.environ.get("CXX", "c++"), "-std=c++17", "-O1", "-o", exe, str(prog)])
    m = _model()
    for block in (128, 256):
        for n in (1, 129, 2 * block, 2 * block + 1, 781, 8 * block - 1, 12 * block):
            out = subprocess.run([exe, str(n), str(block)], capture_output=True, text=True, timeout=60)
            got = np.array(out.stdout.split(), dtype=np.int64)
            assert np.array_equal(got, m.deal_positions(n, block, 16)), (n, block)
    # the sort: by key (a negative word's residue is the two's-complement one; rejected events last), then canonical lane,
    # then round -- on a list whose layout is the identity (one event per lane of a 16-lane block)
    base = np.array([5, 21, m.REJECT, 37, 3, -1, 5, 0, 16, 1, 2, 4, 6, 7, 8, 9], dtype=np.int64)
    assert m.dealt_order(base, 16, 16).tolist() == [7, 8, 9, 10, 4, 11, 0, 1, 3, 6, 12, 13, 14, 15, 5, 2]
    assert m.deal_admitted(256, 128, 1, 2542, 41, 40) and not m.deal_admitted(255, 128, 1, 2542, 41, 40)
    assert not m.deal_admitted(1024, 512, 1, 4960, 41, 40) and not m.deal_admitted(300, 128, 2, 2542, 41, 40)
    assert m.deal_admitted(781, 128, 1, 2542, 51, 46) and not m.deal_admitted(781, 128, 1, 2542, 51, 47)
