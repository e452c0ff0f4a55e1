// exp_taps.h — the exponentials behind an axis' seven Gaussian taps at sigma >= 1 (axis_taps3<true> in ebo_eval3.inc;
// free of HIP: tests/cpp/exp_taps_test.cpp).
//
//   exp(hs (k - f)^2) = exp(hs k^2) exp(hs f^2) exp(f / s^2)^k,  k = -3 .. 3:
// one exponential of hs f^2 in [-0.5, 0] and the pair exp(a), exp(-a) with |a| = |f| / s^2 <= 1.  No range reduction:
// Taylor polynomials (the pair's on a / 4, squared twice).  Every fma is explicit (the library is built with
// -ffp-contract=off).
//
// exp_pair: exp(+-a) = cosh a +- sinh a share their even and odd parts.  With t = a / 4 and u = t^2, C = cosh t to t^12
// (degree 6 in u) and S = sinh t to t^11 (t times degree 5 in u): 20 operations for both instead of 2 x 15.  C - S
// cancels by (C + S) / (C - S) <= e^0.5 at |t| <= 0.25, so the pair's relative error may reach about twice that of
// the single polynomial; measured against expl on 2^20 points of [-1, 1]: 1.2e-15 where the degree-12 polynomial it
// replaces has 7.6e-16.
//
// exp_gauss: the bound is the degree-12 polynomial's own error on [-0.5, 0], 4.8e-16.  On x / 4 with two squarings
// degree 9 has 1.6e-15 and degree 10 4.9e-16 (a hair above: its truncation, 3e-18 of the value, is a tenth of an ulp
// after the squarings), so it is degree 11: 14 operations, ONE fewer than before, and every coefficient is one the
// pair uses too.  The plain degree-14 polynomial on x itself costs the same 14 and is more accurate (1.8e-16, no
// squaring doubles its rounding errors), but its two further constants cost k_eval3 ten more spilled scalar registers
// and 1.5-2 % on launches of small units (measured); not used.
#pragma once

#if defined(__HIPCC__)
#define EBO_EXP_FN __host__ __device__ __forceinline__
#else
#define EBO_EXP_FN inline
#endif

namespace ebo
{
// p = exp(4 t), q = exp(-4 t) for |t| <= 0.25: exp_pair behind its first multiply.  A caller whose argument is a
// product with a constant folds the quarter into the constant: f * (k / 4) has the bits of (f * k) / 4, a division by
// four being exact short of underflow (and there both are below every term the polynomials keep).
EBO_EXP_FN void exp_pair_quarter(double t, double& p, double& q)
{
	const double u = t * t;
	double c = 1.0 / 479001600.0;                // 1/12!
	c = __builtin_fma(c, u, 1.0 / 3628800.0);    // 1/10!
	c = __builtin_fma(c, u, 1.0 / 40320.0);
	c = __builtin_fma(c, u, 1.0 / 720.0);
	c = __builtin_fma(c, u, 1.0 / 24.0);
	c = __builtin_fma(c, u, 0.5);
	c = __builtin_fma(c, u, 1.0);
	double s = 1.0 / 39916800.0;                 // 1/11!
	s = __builtin_fma(s, u, 1.0 / 362880.0);     // 1/9!
	s = __builtin_fma(s, u, 1.0 / 5040.0);
	s = __builtin_fma(s, u, 1.0 / 120.0);
	s = __builtin_fma(s, u, 1.0 / 6.0);
	s = __builtin_fma(s, u, 1.0);
	s = s * t;
	p = c + s;
	q = c - s;
	p = p * p;
	q = q * q;
	p = p * p;
	q = q * q;
}

// p = exp(a), q = exp(-a) for |a| <= 1.
EBO_EXP_FN void exp_pair(double a, double& p, double& q)
{
	exp_pair_quarter(a * 0.25, p, q);
}

// exp(4 t) for -0.125 <= t <= 0: exp_gauss behind its first multiply (as exp_pair_quarter).
EBO_EXP_FN double exp_gauss_quarter(double t)
{
	double p = 1.0 / 39916800.0;                 // 1/11!
	p = __builtin_fma(p, t, 1.0 / 3628800.0);
	p = __builtin_fma(p, t, 1.0 / 362880.0);
	p = __builtin_fma(p, t, 1.0 / 40320.0);
	p = __builtin_fma(p, t, 1.0 / 5040.0);
	p = __builtin_fma(p, t, 1.0 / 720.0);
	p = __builtin_fma(p, t, 1.0 / 120.0);
	p = __builtin_fma(p, t, 1.0 / 24.0);
	p = __builtin_fma(p, t, 1.0 / 6.0);
	p = __builtin_fma(p, t, 0.5);
	p = __builtin_fma(p, t, 1.0);
	p = __builtin_fma(p, t, 1.0);
	p = p * p;
	return p * p;
}

// exp(x) for -0.5 <= x <= 0.
EBO_EXP_FN double exp_gauss(double x)
{
	return exp_gauss_quarter(x * 0.25);
}
}  // namespace ebo
