"""GPU: the two-view facade's device refinement end to end (tests/cpp/two_view_refine_test.cpp): twoview_ref's facade
scene through TwoViewInitializer::initCameras with and without useDeviceRefinement(), alone and through
VisualOdometryFrontEnd::twoView().  With the refinement: the model against tests/relpose_ref.py's (RANSAC -> refine
over its inliers -> unit t -> re-selection) within 10 x the scene's delta, the re-selected inliers exactly
(tests/test_relpose_refine_cpu.py checks that the refined model keeps every score clear of the threshold).  Without it:
bit-equal to the existing driver's answer, which never heard of the refinement."""
import json
import os
import subprocess

import numpy as np
import pytest

import camera_ref
import relpose_ref as R
import twoview_ref as tv

pytestmark = pytest.mark.gpu

CPP = os.path.join(os.path.dirname(os.path.abspath(__file__)), "cpp")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


@pytest.fixture(scope="module")
def driver(ebo, tmp_path_factory):
    ebo.lib()
    out = tmp_path_factory.mktemp("twoview_refine")
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "twoview_refine.mk", "OUT=" + str(out), str(out / "two_view_refine_test")])
    subprocess.check_call(["make", "-s", "-C", CPP, "-f", "twoview.mk", "OUT=" + str(out), str(out / "two_view_lines_test")])
    fs = tv.make_facade_scene()
    fs["x1"].tofile(str(out / "x1.f64"))
    fs["x2"].tofile(str(out / "x2.f64"))

    def run(refine, front_end=False, old=False):
        cmd = ["timeout", "-k", "10", "300", str(out / ("two_view_lines_test" if old else "two_view_refine_test")), "init"]
        cmd += [repr(float(v)) for v in camera_ref.DAVIS] + [str(out / "x1.f64"), str(out / "x2.f64"), "55", str(tv.RANSAC_SEED)]
        if not old:
            cmd += ["1" if refine else "0", "1" if front_end else "0"]
        r = subprocess.run(cmd, capture_output=True, text=True)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-2000:]
        return json.loads(r.stdout.strip().splitlines()[-1])

    return fs, run


@pytest.fixture(scope="module")
def restated(driver):
    """The restatement's chain on the facade's bearing vectors; computed once, read only."""
    fs, _ = driver
    f1, f2 = tv.facade_bearings(fs)
    ransac = tv.ransac(f1, f2, seed=tv.RANSAC_SEED, pair=0)
    pair = dict(model=ransac["model"], f1=f1, f2=f2, idx=ransac["inliers"])
    fwd, rev = R.solve(pair), R.solve(pair, reverse_sums=True)
    return f1, f2, ransac, fwd, R.result_difference(fwd, rev)


def unit_translation(model):
    out = np.array(model, dtype=np.float64).reshape(3, 4).copy()
    t = out[:, 3]
    s = t[0] * t[0] + t[1] * t[1]
    s = s + t[2] * t[2]
    out[:, 3] = t / np.sqrt(s)
    return out


@pytest.mark.parametrize("front_end", [False, True])
def test_without_the_refinement_nothing_changes(driver, front_end):
    _, run = driver
    today = run(False, old=True)
    got = run(False, front_end)
    assert got["initialised"] is True and today["initialised"] is True
    for k in ("found", "winner", "iterations", "ransac_inliers", "inliers"):
        assert got[k] == today[k], k
    for k in ("ransac_model", "Tw2c", "pose"):
        assert np.array_equal(bits(got[k]), bits(today[k])), k
    assert got["refinement"] == dict(iterations=0, num_evals_cost=0, num_evals_jac=0, termination=0, initial_cost=0.0, final_cost=0.0)


@pytest.mark.parametrize("front_end", [False, True])
def test_with_the_refinement_the_model_is_the_restatements(driver, restated, front_end):
    fs, run = driver
    f1, f2, ransac, want, delta = restated
    got = run(True, front_end)
    tracks = 3 * np.arange(len(fs["x1"])) + 5
    assert got["initialised"] is True
    assert (got["winner"], got["iterations"], got["ransac_inliers"]) == (ransac["winner"], ransac["iterations"], ransac["n_inliers"])
    for k in ("iterations", "num_evals_cost", "num_evals_jac", "termination"):
        assert got["refinement"][k] == want["summary"][k], k
    Tw2c = np.array(got["Tw2c"]).reshape(3, 4)
    worst = max(R.difference(Tw2c, unit_translation(want["model"])),
                R.difference(got["refinement"]["final_cost"], want["summary"]["final_cost"]),
                R.difference(got["refinement"]["initial_cost"], want["summary"]["initial_cost"]))
    same_start = np.array_equal(bits(got["ransac_model"]), bits(ransac["model"]))
    print("refined model: largest difference %.3g, delta %.3g, cost %.3g -> %.3g in %d iterations; RANSAC models bit-equal: %s" % (
        worst, delta, want["summary"]["initial_cost"], want["summary"]["final_cost"], want["summary"]["iterations"], same_start))
    assert worst <= 10 * delta
    assert abs(np.linalg.norm(Tw2c[:, 3]) - 1.0) <= 1e-14
    flags = tv.inliers(tv.scores(want["model"], f1, f2))
    assert np.array_equal(got["inliers"], tracks[flags])
    assert len(got["inliers"]) >= ransac["n_inliers"]
    assert np.array_equal(np.array(got["pose"]).reshape(3, 4), Tw2c)     # start.pose (identity) * Tw2c
    assert want["summary"]["final_cost"] < want["summary"]["initial_cost"]
