// tap_moments.h — the Jacobian sums of an interior event as MOMENTS of its tap weights (eval_unit3 in ebo_eval3.inc;
// free of HIP: tests/cpp/tap_moments_test.cpp executes the same text).
//
// A tap's derivative factor is c_i = g ((i - 3) - f), with g = tau / sigma^2 and the fractional part f constant per
// event.  So every sum of weight x factor products is g times a first moment of the weights about the centre tap, less
// f times their plain sum -- no factor per tap, no table of derivative weights:
//
//   D1 (image-free):  sum_i w_i c_i = g (M1 - f W),   M1 = 3 (w6 - w0) + 2 (w5 - w1) + (w4 - w2),  W = sum_i w_i
//   D2 (gather):      d2a = sum_j wy_j sum_i wx_i cx_i v_ij = g (A - fx B),   d2b = sum_j wy_j cy_j sum_i wx_i v_ij = g (C - fy B)
//        A = sum_j wy_j rc_j,  B = sum_j wy_j rb_j,  C = sum_{j != 3} wy_j ((j - 3) rb_j)
//        rb_j = sum_i wx_i v_ij  (7 operations),  rc_j = sum_{i != 3} (i - 3) wx_i v_ij  (6 operations)
//
// The centre tap has moment 0, the +-1 taps need no product (a negation is an operand modifier), so the x axis' table
// is four products (-3 w0, -2 w1, 2 w5, 3 w6); the y axis has none: (j - 3) rb_j is formed per row (a y table costs the
// kernel its fourth wave).  W keeps its sequential adds, so it keeps its bits; the moments are
// linear in the weights, so exact power-of-two prefactors on them come off the sums as before.  Every fma is explicit
// (the library is built with -ffp-contract=off).
#pragma once

#if defined(__HIPCC__)
#define EBO_MOM_FN __host__ __device__ __forceinline__
#else
#define EBO_MOM_FN inline
#endif

namespace ebo
{
// W = sum_i w_i (in tap order, from 0.0) and sum_i w_i c_i = g (M1 - f W) of one axis.
EBO_MOM_FN void axis_d1(const double (&w)[7], double g, double f, double& sumW, double& sumA)
{
	double s = 0.0;
	s += w[0];
	s += w[1];
	s += w[2];
	s += w[3];
	s += w[4];
	s += w[5];
	s += w[6];
	const double m1 = __builtin_fma(3.0, w[6] - w[0], __builtin_fma(2.0, w[5] - w[1], w[4] - w[2]));
	sumW = s;
	sumA = g * __builtin_fma(-f, s, m1);
}

// The x axis' moment weights of the outer taps: (i - 3) w_i for i = 0, 1, 5, 6.
EBO_MOM_FN void moment_table(const double (&w)[7], double (&k)[4])
{
	k[0] = -3.0 * w[0];
	k[1] = -2.0 * w[1];
	k[2] = 2.0 * w[5];
	k[3] = 3.0 * w[6];
}

// One image row v of the 7 x 7 footprint: rb = sum_i w_i v_i and rc = sum_{i != 3} (i - 3) w_i v_i.
EBO_MOM_FN void moment_row(const double (&w)[7], const double (&k)[4], const double (&v)[7], double& rb, double& rc)
{
	double b = w[0] * v[0];
	b = __builtin_fma(w[1], v[1], b);
	b = __builtin_fma(w[2], v[2], b);
	b = __builtin_fma(w[3], v[3], b);
	b = __builtin_fma(w[4], v[4], b);
	b = __builtin_fma(w[5], v[5], b);
	b = __builtin_fma(w[6], v[6], b);
	double m = k[0] * v[0];
	m = __builtin_fma(k[1], v[1], m);
	m = __builtin_fma(-w[2], v[2], m);
	m = __builtin_fma(w[4], v[4], m);
	m = __builtin_fma(k[2], v[5], m);
	m = __builtin_fma(k[3], v[6], m);
	rb = b;
	rc = m;
}

// Row j's share of A, B and C (J: the row's index 0 .. 6, a constant of the caller's unrolled loop).
template <int J>
EBO_MOM_FN void moment_acc(double wy, double rb, double rc, double& A, double& B, double& C)
{
	A = __builtin_fma(wy, rc, A);
	B = __builtin_fma(wy, rb, B);
	if (J == 2)
	{
		C = __builtin_fma(wy, -rb, C);
	}
	else if (J == 4)
	{
		C = __builtin_fma(wy, rb, C);
	}
	else if (J != 3)
	{
		C = __builtin_fma(wy, static_cast<double>(J - 3) * rb, C);
	}
}

// d2a = g (A - fx B), d2b = g (C - fy B).
EBO_MOM_FN void moment_d2(double g, double fx, double fy, double A, double B, double C, double& d2a, double& d2b)
{
	d2a = g * __builtin_fma(-fx, B, A);
	d2b = g * __builtin_fma(-fy, B, C);
}
}  // namespace ebo
