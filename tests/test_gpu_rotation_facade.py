"""GPU: the facade's angular-velocity side end to end.  tests/cpp/angular_velocity_test.cpp holds
tracker::AngularVelocityEstimator to the C ABI on one scene; tools/track_recording --rectify --angular-velocity runs
tools::Evaluator over a synth.make_recording directory whose scene rotates at (0.4, -0.6, 1.0) rad/s and every window
lands within the recorded bound of the truth, unbatched and batched with the same bits; a distorted recording without
--rectify is refused; the translating default recording writes the same trajectory.txt and final_cost.txt with the flag
as without."""
import json
import os
import subprocess

import numpy as np
import pytest

import rotation_ref as R

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
CPP = os.path.join(HERE, "cpp")
CSRC = os.path.join(ROOT, "event-based-odomety_amd", "csrc")
TOOL = os.path.join(ROOT, "event-based-odomety_amd", "tools", "track_recording")

TRUTH = (0.4, -0.6, 1.0)
# The restatement alone (rotation_ref.solve_window with calib.txt's camera) on the seven whole windows of 15 000 events
# of the recording below ends 0.0108, 0.0282, 0.0091, 0.0147, 0.0253, 0.0341 and 0.0599 rad/s from the truth (largest
# component); the bound is the worst of them plus half as much again.
RESTATEMENT_WORST = 0.0599
BOUND = 1.5 * RESTATEMENT_WORST


def run_tool(d, out, flags, expect=0):
    out.mkdir()
    r = subprocess.run(["timeout", "-k", "10", "600", TOOL, "--dataset", d, "--out", str(out), "--tracker-experiment"] + flags,
                       capture_output=True, text=True)
    assert (r.returncode == 0) == (expect == 0), r.stdout[-2000:] + r.stderr[-2000:]
    return r


@pytest.fixture(scope="module")
def tool(ebo):
    ebo.lib()
    subprocess.check_call(["make", "-s", "-C", CSRC, "track_recording"])
    return TOOL


@pytest.fixture(scope="module")
def rotating(synth, tmp_path_factory):
    """threshold 0.7: 15 000 events span about 50 ms, over which the scene moves by several pixels."""
    d = tmp_path_factory.mktemp("rotating") / "rec"
    info = synth.make_recording(str(d), seed=1, duration_s=0.4, threshold=0.7, angular_velocity=TRUTH)
    assert info["angular_velocity"] == TRUTH
    return str(d), info


def test_the_estimator_equals_the_c_abi(ebo, tmp_path):
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "angular_velocity.mk", "OUT=" + str(tmp_path),
                           str(tmp_path / "angular_velocity_test")])
    ev = R.recovery_scene(2)
    ebo.write_events_bin(str(tmp_path / "ev.bin"), ev)
    r = subprocess.run(["timeout", "-k", "10", "120", str(tmp_path / "angular_velocity_test"), str(tmp_path / "ev.bin"), str(R.W), str(R.H)] +
                       [repr(v) for v in R.CAM], capture_output=True, text=True)
    assert r.returncode == 0 and "all passed" in r.stdout, r.stdout[-2000:] + r.stderr[-2000:]
    line = [ln for ln in r.stdout.splitlines() if ln.startswith("omega ")][0].split()
    with ebo.Context(loss=ebo.LOSS_VARIANCE) as c:
        c.set_window(ev)
        om, summ = c.solve_rotation(R.CAM)
    assert R.same_bits(np.array([float(v) for v in line[1:4]]), om[0])
    assert [int(v) for v in line[4:]] == [summ[0].status, summ[0].iterations, summ[0].evaluations]
    assert np.abs(om[0] - R.recovery_truths()[2]).max() <= 0.15


def test_every_window_of_the_rotating_recording_lands_near_the_truth(ebo, tool, rotating, tmp_path):
    d, info = rotating
    ev = ebo.read_events_txt(os.path.join(d, "events.txt"), cap=info["events"] + 16)
    whole = len(ev) // 15000
    assert whole >= 6
    t_refs = [R.ref_time(ev[k * 15000:(k + 1) * 15000]) for k in range(whole)]
    rows = {}
    for name, flags in (("one", []), ("batch", ["--window-batch", "4"])):
        out = tmp_path / name
        r = run_tool(d, out, ["--rectify", "--angular-velocity"] + flags)
        js = json.loads(r.stdout.strip().splitlines()[-1])
        rows[name] = np.loadtxt(out / "angular_velocity.txt", ndmin=2)
        assert rows[name].shape[1] == 8 and len(rows[name]) >= js["windows"] >= 1
        assert os.path.exists(out / "trajectory.txt")
    got = rows["one"]
    # the windows are the whole 15 000-event chunks of the stream up to the last frame
    n = len(got)
    assert 5 <= n <= whole
    assert np.array_equal(np.rint(got[:, 0] * 1e6).astype(np.int64), np.array(t_refs[:n]))
    for row in got:
        err = np.abs(row[1:4] - TRUTH).max()
        print("t_ref %.6f omega %s err %.4f r %.4f -> %.4f iterations %d status %d" % (row[0], row[1:4], err, row[4], row[5], row[6], row[7]))
        assert err <= BOUND, row
        assert row[7] == ebo.ROT_CONVERGED_STEP and row[5] > row[4]
    # batched under --window-batch: the same bits, window for window
    assert rows["batch"][:n].tobytes() == got.tobytes() and len(rows["batch"]) >= n


def test_a_distorted_recording_needs_rectify(ebo, tool, synth, tmp_path):
    d = tmp_path / "lens"
    synth.make_recording(str(d), seed=2, duration_s=0.1, distortion=(-0.368, 0.151, 0.0, 0.0))
    r = run_tool(str(d), tmp_path / "refused", ["--angular-velocity"], expect=1)
    assert "--rectify" in r.stderr + r.stdout
    assert not os.path.exists(tmp_path / "refused" / "angular_velocity.txt")
    run_tool(str(d), tmp_path / "rectified", ["--rectify", "--angular-velocity"])
    assert os.path.exists(tmp_path / "rectified" / "angular_velocity.txt")


def test_the_translating_recording_writes_what_it_wrote(ebo, tool, synth, tmp_path):
    d = tmp_path / "plain"
    synth.make_recording(str(d), seed=1, duration_s=0.25)
    run_tool(str(d), tmp_path / "without", [])
    run_tool(str(d), tmp_path / "with", ["--angular-velocity"])
    for name in ("trajectory.txt", "final_cost.txt"):
        a, b = (tmp_path / "without" / name).read_bytes(), (tmp_path / "with" / name).read_bytes()
        assert a == b, name
    assert len((tmp_path / "with" / "trajectory.txt").read_bytes()) > 0
    assert not os.path.exists(tmp_path / "without" / "angular_velocity.txt")
    assert len(np.loadtxt(tmp_path / "with" / "angular_velocity.txt", ndmin=2)) >= 1
