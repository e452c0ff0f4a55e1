"""CPU: the count-image launch plan (csrc/count_plan.h, the choice launch_count_image launches) is free of HIP;
tests/cpp/count_plan_test.cpp compares the plan of the shapes the GPU tests and bench.py use with a table, checks that
over a grid of modes, sensors, batch sizes and window sizes the default plan reaches exactly the kernels the launch
can launch (so libebo_hip.so holds none it cannot reach), and that every plan fits the device's LDS and block limits."""
import os
import subprocess

HERE = os.path.dirname(os.path.abspath(__file__))
CPP = os.path.join(HERE, "cpp")


def test_count_plan_table_reachability_and_limits():
    subprocess.check_call(["make", "-s", "-C", CPP, "count_plan_test"])
    out = subprocess.run([os.path.join(CPP, "count_plan_test")], capture_output=True, text=True, timeout=300)
    assert out.returncode == 0, (out.stdout + out.stderr)[-4000:]
    assert "all passed" in out.stdout
