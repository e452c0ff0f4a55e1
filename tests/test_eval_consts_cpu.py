"""CPU checks behind the objective sweep (tests/test_gpu_eval_sweep.py):
  * ebo_create admits only functor constants the kernels are built for (it validates before it looks for a device);
  * the oracle's variance objective agrees with a second, naive restatement of calculateVarianceLoss
    (contrast_functor.h:38-150) at constants away from the reference's defaults -- the sweep trusts the oracle
    there, so the oracle is checked there;
  * a closed-form known answer: N events on one integer pixel at zero flow make the image N x the 7 x 7 stencil."""
import ctypes as C
import math

import numpy as np
import pytest

import eval_cases as EC


# ---- admission ---------------------------------------------------------------------------------------------
def _create(ebo, p):
    h = C.c_void_p()
    rc = ebo.lib().ebo_create(C.byref(p), C.byref(h))
    if rc == 0:
        ebo.lib().ebo_destroy(h)
    return rc, ebo.lib().ebo_last_error(None).decode()


BAD = [float("nan"), float("inf"), -float("inf"), 0.0, -1.0]


@pytest.mark.parametrize("field", ["sigma_compensate", "sigma_st", "max_possible_residual"])
@pytest.mark.parametrize("value", BAD)
def test_create_refuses_bad_functor_constants(ebo, field, value):
    p = ebo.default_params()
    setattr(p.k, field, value)
    rc, msg = _create(ebo, p)
    assert rc == ebo.ERR_ARG and field in msg


@pytest.mark.parametrize("value", BAD)
def test_create_refuses_a_bad_central_difference_step(ebo, value):
    p = ebo.default_params(grad=ebo.GRAD_CENTRAL, fd_step=value)
    rc, msg = _create(ebo, p)
    assert rc == ebo.ERR_ARG and "fd_step" in msg
    # the step is not read with Jet derivatives
    p = ebo.default_params(grad=ebo.GRAD_JET, fd_step=value)
    assert _create(ebo, p)[0] != ebo.ERR_ARG


@pytest.mark.parametrize("value", [float("nan"), float("inf"), -float("inf")])
def test_create_refuses_a_non_finite_scale(ebo, value):
    rc, msg = _create(ebo, ebo.default_params(scale=value))
    assert rc == ebo.ERR_ARG and "scale" in msg


@pytest.mark.parametrize("sigma", [math.nextafter(EC.SIGMA_MIN, 0.0), 0.01, math.nextafter(EC.SIGMA_MAX, 2e9), 1e4])
def test_create_refuses_sigma_outside_the_built_range(ebo, sigma):
    p = ebo.default_params()
    p.k.sigma_compensate = sigma
    rc, msg = _create(ebo, p)
    assert rc == ebo.ERR_UNSUPPORTED and "sigma_compensate" in msg


@pytest.mark.parametrize("sigma", [EC.SIGMA_MIN, 1.0, EC.SIGMA_MAX])
def test_create_admits_sigma_inside_the_built_range(ebo, sigma):
    p = ebo.default_params()
    p.k.sigma_compensate = sigma
    rc, _ = _create(ebo, p)
    assert rc in (0, ebo.ERR_NO_DEVICE)  # arguments accepted: only the device can refuse


@pytest.mark.parametrize("sigma_st", [0.3, math.nextafter(EC.SIGMA_ST_MIN, 0.0), math.nextafter(EC.SIGMA_ST_MAX, 20.0)])
def test_create_refuses_sigma_st_outside_the_built_range(ebo, sigma_st):
    p = ebo.default_params()
    p.k.sigma_st = sigma_st
    rc, msg = _create(ebo, p)
    assert rc == ebo.ERR_UNSUPPORTED and "sigma_st" in msg


@pytest.mark.parametrize("sigma_st", [EC.SIGMA_ST_MIN, EC.SIGMA_ST_MAX])
def test_create_admits_sigma_st_inside_the_built_range(ebo, sigma_st):
    p = ebo.default_params()
    p.k.sigma_st = sigma_st
    assert _create(ebo, p)[0] in (0, ebo.ERR_NO_DEVICE)


# ---- a second restatement of the variance objective ---------------------------------------------------------
def naive_variance(ev, rect, motion, scale, sigma, max_res, h=1e-30):
    """contrast_functor.h:38-150 with the loss switched to calculateVarianceLoss, in float64, one event and one
    tap at a time; the Jacobian by complex steps (every operation on the motion is analytic; the truncation
    int(compEventX) and the tests v > 0 read the real part, as the Jet's .a)."""
    rx, ry, rw, rh = rect
    t = ev["t_us"].astype(np.int64)
    t_ref = int(np.int32((float(t[0] + t[-1])) * 0.5))
    out = []
    for d in (None, 0, 1):
        m = np.array(motion, dtype=np.complex128)
        if d is not None:
            m[d] += 1j * h
        img = np.zeros((3 * rh, 3 * rw), dtype=np.complex128)
        for e in range(len(ev)):
            tau = float(t_ref - t[e]) * scale
            cx = float(ev["x"][e]) + tau * m[0]
            cy = float(ev["y"][e]) + tau * m[1]
            bx, by = int(cx.real), int(cy.real)
            for i in range(-3, 4):
                for j in range(-3, 4):
                    px, py = bx + i - rx + rw, by + j - ry + rh
                    if 0 <= px < 3 * rw and 0 <= py < 3 * rh:
                        ssq = sigma * sigma
                        dx, dy = (bx + i) - cx, (by + j) - cy
                        img[py, px] += 1.0 / (2 * math.pi * ssq) * np.exp(-0.5 / ssq * (dx * dx + dy * dy))
        mean, cnt = 0.0, 1
        for v in img.ravel():
            if v.real > 0.0:
                mean += v
                cnt += 1
        mean = mean / cnt
        if mean.real > 0.0:
            std = 0.0
            for v in img.ravel():
                if v.real > 0.0:
                    std += (v - mean) * (v - mean)
            r = max_res - std / cnt
        else:
            r = max_res * (1 + m[0] * m[0] + m[1] * m[1])
        out.append(r)
    return out[0].real, np.array([out[1].imag / h, out[2].imag / h])


def _tiny(orc, seed, n=40, rect=(3, 4, 5, 6)):
    rng = np.random.default_rng(seed)
    x, y, w, h = rect
    t = np.sort(rng.integers(0, 4000, n))
    t[rng.choice(n, 6, replace=False)] = 1000  # 1 ms before the reference time 2000 ...
    t = np.sort(t)
    t[0], t[-1] = 0, 4000
    return orc.make_events(rng.integers(x - 1, x + w + 1, n), rng.integers(y - 1, y + h + 1, n), t)


RESTATED = [dict(sigma=s) for s in (0.05, 0.065, 0.25, EC._RSQRT_PI, math.nextafter(1.0, 0.0), 1.5, 30.0, 1e3)]
RESTATED += [dict(max_res=1.0), dict(max_res=1e6), dict(scale=1e-6), dict(scale=0.1)]


@pytest.mark.parametrize("kw", RESTATED, ids=[",".join("%s=%r" % i for i in k.items()) for k in RESTATED])
def test_oracle_variance_equals_a_naive_restatement(orc, kw):
    sigma, max_res, scale = kw.get("sigma", 1.0), kw.get("max_res", 1e3), kw.get("scale", 1e-3)
    case = EC.Case("x", sigma=sigma, max_res=max_res, scale=scale)
    k = case.consts(orc)
    rect = (3, 4, 5, 6)
    one = (1.0 - 1e-7) / (1000.0 * scale)  # ... which this flow moves by a pixel minus 1e-7: fractions near 1
    for seed, motion in enumerate([(0.37, -0.61), (one, -one), (-one, one), (1e-3, 2e-3), (-3.1, 0.4)]):
        ev = _tiny(orc, seed)
        r, J = orc.contrast_eval(ev, rect, motion, 1, scale=scale, consts=k)
        rn, Jn = naive_variance(ev, rect, motion, scale, sigma, max_res)
        assert abs(r - rn) <= 1e-12 * max(abs(rn), 1e-300), (motion, r, rn)
        np.testing.assert_allclose(J, Jn, rtol=1e-12, atol=1e-12 * max(np.abs(Jn).max(), 1e-300))


# ---- closed-form known answer: a pure pile-up at zero flow ----------------------------------------------------
@pytest.mark.parametrize("sigma", [0.25, 0.5, 1.0, 4.0])
@pytest.mark.parametrize("n", [1, 7, 25736])
def test_pile_up_at_zero_flow_is_n_times_the_stencil(orc, sigma, n):
    rect = (10, 10, 20, 20)
    ev = orc.make_events(np.full(n, 17), np.full(n, 22), np.full(n, 5000))
    k = EC.Case("x", sigma=sigma).consts(orc)
    img = orc.contrast_image(ev, rect, (0.0, 0.0), 3, consts=k)
    d = np.arange(-3, 4, dtype=np.float64)
    stencil = np.exp(-0.5 / sigma ** 2 * (d[:, None] ** 2 + d[None, :] ** 2)) / (2 * math.pi * sigma ** 2)
    want = np.zeros((60, 60))
    want[22 - 10 + 20 - 3:22 - 10 + 20 + 4, 17 - 10 + 20 - 3:17 - 10 + 20 + 4] = stencil * n
    np.testing.assert_allclose(img[0], want, rtol=1e-12, atol=0)
    assert not img[1].any() and not img[2].any()  # all events at the reference time: tau = 0
    # the variance objective of that image: 49 equal-count pixels in sum_nonzero / (49 + 1)
    mean = want.sum() / 50
    var = ((stencil * n - mean) ** 2).sum() / 50
    r, J = orc.contrast_eval(ev, rect, (0.0, 0.0), 1, consts=k)
    assert abs(r - (1e3 - var)) <= 1e-12 * var * math.sqrt(n)  # n sequential additions per pixel in the oracle
    assert np.all(J == 0.0)
