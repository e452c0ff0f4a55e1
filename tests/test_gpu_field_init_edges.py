"""k_field_fixed / k_field_fill (FeatureDetector::initMotionField: one serial walk over the patches, then one lane per
pixel) on the hand-built scenes of tests/plumbing_cases.py, with the average and with the nearest fill: the field
equals the oracle's as float32 bits, the fixed list as integers.  Where both sides hold a NaN (dt = 0 gives 0/0 and
inf - inf) its sign and payload are free: x86 and the GPU produce different ones.  The image is 37 x 29 = 1073 pixels,
no multiple of 256, so the last workgroup of k_field_fill is partly idle.  tests/test_plumbing_cases_cpu.py shows on
the CPU that each scene reaches the edge it is named after."""
import numpy as np
import pytest

import plumbing_cases as K

pytestmark = pytest.mark.gpu

SCENES = K.field_scenes()


@pytest.fixture(scope="module")
def ctx(ebo):
    with ebo.Context(image_w=K.FIELD_W, image_h=K.FIELD_H) as c:
        yield c


@pytest.fixture(scope="module")
def oracle(orc):
    """The oracle's answers, computed once per (scene, fill)."""
    memo = {}

    def get(name, ts, trajectories, use_average):
        key = (name, use_average)
        if key not in memo:
            memo[key] = orc.init_motion_field(K.FIELD_W, K.FIELD_H, ts, trajectories, use_average)
        return memo[key]
    return get


def assert_field(ctx, oracle, name, ts, trajectories, use_average):
    field, fixed = ctx.init_motion_field(ts, trajectories, use_average)
    want, wfixed = oracle(name, ts, trajectories, use_average)
    assert fixed.dtype == wfixed.dtype and np.array_equal(fixed, wfixed), name
    assert K.same_floats(field, want), name
    return field, fixed


@pytest.mark.parametrize("use_average", [True, False], ids=["average", "nearest"])
@pytest.mark.parametrize("name,ts,trajectories", SCENES, ids=[s[0] for s in SCENES])
def test_initial_field_matches_the_oracle(ctx, oracle, name, ts, trajectories, use_average):
    assert_field(ctx, oracle, name, ts, trajectories, use_average)


@pytest.mark.parametrize("use_average", [True, False], ids=["average", "nearest"])
def test_a_call_that_fixes_nothing_after_one_that_fixed_points(ctx, oracle, use_average):
    by_name = {s[0]: s for s in SCENES}
    _, fixed = assert_field(ctx, oracle, *by_name["many"], use_average)
    assert len(fixed) == 300
    for quiet in ("only_short", "lower_bound_0", "no_patches"):
        field, fixed = assert_field(ctx, oracle, *by_name[quiet], use_average)
        assert len(fixed) == 0 and not field.any()
