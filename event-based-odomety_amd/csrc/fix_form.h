// fix_form.h — how a value tap becomes its 64-bit fixed-point word (free of HIP: tests/cpp/fix_form_test.cpp).
//
// The value image is summed in fixed point on the grid 2^(k-52) (EvalConsts::fix_scale).  Two encodings of a tap
// wx * wy give the same word, RNE(wx wy / 2^(k-52)):
//   biased     bits(fma(wx, wy, 1.5 * 2^k)) - bits(1.5 * 2^k): the sum's ulp is the grid step, the bias is an even
//              multiple of it, and taking its bits off leaves the integer           (v_fma_f64 + a 32-bit subtract)
//   subnormal  bits((wx * 2^-511) * (wy * 2^-(511 + k))): the product lies below 2^-1022, where a double's bit pattern
//              IS value / 2^-1074 = wx wy / 2^(k-52), rounded once, to nearest even, by the multiply itself (v_mul_f64)
// The powers of two ride in the prefactor that an axis' weights are multiplied by anyway; scaling a normal number by a
// power of two is exact as long as the result is normal, so every weight keeps its mantissa.  That is the condition
// the subnormal form rests on: the smallest scaled weights, norm e^-8 2^-511 and e^-8 2^-(511 + k) (the sigma >= 1 path:
// outer taps at most e^-4.5 of the centre, the factors of exp_taps.h within e^+-1), have to stay far above 2^-1022.
// With |log2 norm| and |k| below kFixGuardExp = 400 they are above 2^-923; every sigma ebo_create admits gives
// norm in [1.6e-7, 2.6] and k in [0, 3 + 32].  A context outside the rule evaluates with the biased form.
#pragma once

#include <cmath>

namespace ebo
{
constexpr int kFixSubnormal = 0;    // k_eval3<true> / the edge loss's value scatter: subnormal products
constexpr int kFixBiasedGuard = 1;  // the rule below failed: the launch takes the <false> instantiation (biased taps)
constexpr int kFixBiasedAb = 2;     // libebo_hip_ab.so with EBO_FIX_FORM=bias: the <true> instantiation with biased taps
constexpr int kFixGuardExp = 400;

// True where the subnormal form is exact for a grid exponent up to kexp + 32 (unit_fix_grid raises it by less than
// log2 of a unit's event count).
inline bool fix_subnormal_ok(double norm, int kexp, int guardExp = kFixGuardExp)
{
	return std::isfinite(norm) && norm >= std::ldexp(1.0, -guardExp) && norm <= std::ldexp(1.0, guardExp) &&
		   kexp >= -guardExp && kexp <= guardExp;
}

inline double fix_pre_x(double norm) { return norm * std::ldexp(1.0, -511); }
inline double fix_pre_y(int kexp) { return std::ldexp(1.0, -(511 + kexp)); }
}  // namespace ebo
