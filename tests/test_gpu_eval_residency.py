"""GPU: the workgroups of a variance evaluation one CU keeps resident are the ones the launch plan intends.

csrc/eval_plan.h divides a CU's LDS among as many workgroups as fill the wave slots k_eval3 is compiled for; whether the
runtime places that many is a property of the chip (the LDS allocation granule, the registers of the code object), so it
is asked: ebo_eval_resident_workgroups returns the plan's count beside hipOccupancyMaxActiveBlocksPerMultiprocessor's
for the instantiation, the block and the dynamic LDS the launch would use.  The events do not matter here: a few hundred
per window."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

N_EVENTS = 600


def _resident(lib, synth, config, windows, sigma=None):
    cfg = synth.CONFIGS[config]
    evs = [synth.make_window(config, window=w, n_events=N_EVENTS)[0] for w in range(windows)]
    offsets = np.zeros(windows + 1, dtype=np.uint64)
    offsets[1:] = np.cumsum([len(e) for e in evs])
    p = lib.default_params(image_w=cfg["image"][0], image_h=cfg["image"][1], patch_w=cfg["patch"][0], patch_h=cfg["patch"][1],
                           loss=lib.LOSS_VARIANCE, max_events=int(offsets[-1]), max_windows=windows)
    if sigma is not None:
        p.k.sigma_compensate = sigma
    with lib.Context(p) as c:
        c.set_windows(np.concatenate(evs), offsets)
        slots = windows * c.P
        return slots, c.eval_launch_shape(True)[1], c.eval_resident_workgroups(True), c.eval_resident_workgroups(False)


def test_small_canvas_many_units_keeps_eight(ebo, synth):
    """ten windows of 20 x 20 patches, and C3's 21 x 16: 128 lanes, 8 x 20 480 B"""
    for config, windows in ((0, 10), (3, 4)):
        slots, block, jac, val = _resident(ebo, synth, config, windows)
        assert slots >= 1024 and block == 128
        assert jac == (8, 8), jac
        assert val == (8, 8), val


def test_large_canvas_many_units_keeps_four(ebo, synth):
    """sixteen windows of C2's 30 x 22 patches: 256 lanes, 4 x 40 960 B"""
    slots, block, jac, val = _resident(ebo, synth, 2, 16)
    assert slots >= 1024 and block == 256
    assert jac == (4, 4), jac
    assert val == (4, 4), val


def test_below_1024_slots(ebo, synth):
    """one window: 512 lanes and 40 KB, two workgroups fill the sixteen wave slots"""
    slots, block, jac, val = _resident(ebo, synth, 0, 1)
    assert slots < 1024 and block == 512
    assert jac[1] == jac[0] == 2, jac
    assert val[1] == val[0] == 2, val


def test_sigma_below_one_instantiation(ebo, synth):
    """k_eval3<false> is compiled for twelve waves per CU: six workgroups of 26 880 B, three of 53 760 B"""
    for config, windows, want in ((0, 10, 6), (2, 16, 3)):
        slots, _, jac, val = _resident(ebo, synth, config, windows, sigma=0.5)
        assert slots >= 1024
        assert jac == (want, want), jac
        assert val == (want, want), val
