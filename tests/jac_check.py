"""Tolerance of edge-loss Jacobians against the oracle (test helper).

A Jacobian entry is a sum over events and taps with cancellation, so its absolute error scales with the
magnitude of the patch's Jacobian, not with the entry itself: an entry may be 1e-3 of its neighbour.  The bound is
therefore RELATIVE TO THE PATCH -- |dJ| <= rtol * |J_oracle| + patch_rel * max|J_oracle of the patch| -- and not an
absolute 1e-7 (which was 1e-3 relative on entries like the probe's 7.7e-5).

Measured on the round-5 kernels over tests/test_gpu_{fullsize,random,edge}.py (EBO_JAC_RECORD=file collects the
ratios): every ordinary comparison stays below 1.2e-9 of the patch's largest entry, so patch_rel = 1e-8.  The
zero-flow TIE patches re-evaluated in reference-order mode (tests/test_gpu_random.py) reproduce the oracle's argmax
choice but not its last bits -- up to 5.7e-6 of the largest entry -- and are held to patch_rel = 1e-5 there, with an
absolute floor of 5e-8 (half the 1e-7 of rounds 1-4): over 6000 campaign seeds (tests/diag_random_campaign.py, round 5)
35 tie patches with Jacobians of 1e-7 ... 7e-4 keep a second, smaller tie and differ by up to 1.5e-8 absolute there,
while no ORDINARY comparison -- any patch at any non-zero flow -- exceeded the 1e-8 bound."""
import os

import numpy as np


def assert_jac_close(J, Jo, rtol=1e-8, patch_rel=1e-8, floor=1e-13):
    J = np.asarray(J, dtype=np.float64).reshape(-1, 2)
    Jo = np.asarray(Jo, dtype=np.float64).reshape(-1, 2)
    assert J.shape == Jo.shape
    scale = np.abs(Jo).max(axis=1, keepdims=True)
    bound = rtol * np.abs(Jo) + patch_rel * scale + floor
    err = np.abs(J - Jo)
    rec = os.environ.get("EBO_JAC_RECORD")  # diagnostics: the largest error in units of the patch's largest entry
    if rec and len(J):
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.nanmax(np.where(scale > 0, (err - rtol * np.abs(Jo)) / scale, 0.0))
        with open(rec, "a") as f:
            f.write("%.3e %d\n" % (ratio, len(J)))
    bad = ~(err <= bound)  # also catches NaN on one side only
    bad &= ~(np.isnan(J) & np.isnan(Jo))
    if bad.any():
        q = int(np.flatnonzero(bad.any(axis=1))[0])
        raise AssertionError("Jacobian of patch %d: got %r, oracle %r, |diff| %r > bound %r (%d of %d patches)"
                             % (q, J[q], Jo[q], err[q], bound[q], int(bad.any(axis=1).sum()), len(J)))
