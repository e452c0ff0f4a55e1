// The moment forms of csrc/tap_moments.h as the host compiles them (free of HIP; the kernels execute the same text),
// against the statements they replace and a long-double evaluation, and the quarter-argument entry points of
// csrc/exp_taps.h against exp_pair / exp_gauss bit for bit.
//   tap_moments_test <seed> <points>
// Every point is one event: fractional parts fx, fy (even points in [0, 1), odd points in (-1, 0]), g = tau / sigma^2
// in [-20, 20], the two axes' seven weights as axis_taps3<true> forms them (sigma 1, 1.5, 2 or 1000 in turn) and a
// 7 x 7 image patch with a quarter of its entries 0, a quarter up to 1000 and the others below 1.  Points 0 .. 7 take
// f = +-0 and |g| = 20.
//
// Errors are absolute, against the long-double sum over the SAME double weights and values, divided by a scale that
// belongs to neither form: |g| max_i w_i for an axis' D1 sum, |g| max_ij wx_i wy_j |v_ij| for D2.  (The factor
// (i - 3) - f reaches 4 and vanishes only on single taps, so this is the event's largest term up to that factor; J's
// parity bounds are relative to J's largest entry, which is a sum of such scales.)
//   d1x <old> <new>     sum_i wx_i cx_i: the scatter's fma chain against axis_d1
//   d1y <old> <new>     sum_j wy_j cy_j: product and add per tap against axis_d1
//   d2a <old> <new>     sum_j wy_j sum_i ax_i v_ij against g (A - fx B)
//   d2b <old> <new>     sum_j ay_j sum_i wx_i v_ij against g (C - fy B)
//   sumw <mismatches>   axis_d1's W against the sequential sum, bit for bit
//   bits <mismatches>   exp_pair_quarter / exp_gauss_quarter against exp_pair / exp_gauss, direct and with the quarter
//                       folded into the constant as axis_taps3<true> does
// Exit status 1 if a new form exceeds 4 x the old form's maximum or any bit differs (tests/test_tap_moments_cpu.py
// asserts the same from the printed figures).
#include "../../event-based-odomety_amd/csrc/exp_taps.h"
#include "../../event-based-odomety_amd/csrc/tap_moments.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

static uint64_t splitmix64(uint64_t& s)
{
	uint64_t z = (s += 0x9e3779b97f4a7c15ull);
	z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
	z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
	return z ^ (z >> 31);
}

static double unit(uint64_t& s)  // [0, 1)
{
	return static_cast<double>(splitmix64(s) >> 11) * (1.0 / 9007199254740992.0);
}

static uint64_t bits(double x)
{
	uint64_t u;
	std::memcpy(&u, &x, 8);
	return u;
}

struct Consts
{
	double norm, hs, inv_sigsq, ck1, ck2, ck3;
};

static Consts consts_of(double sig)
{
	Consts c;
	c.norm = 1.0 / ((2 * M_PI) * (sig * sig));
	c.hs = -0.5 / (sig * sig);
	c.inv_sigsq = 1.0 / (sig * sig);
	c.ck1 = std::exp(c.hs * 1.0);
	c.ck2 = std::exp(c.hs * 4.0);
	c.ck3 = std::exp(c.hs * 9.0);
	return c;
}

// axis_taps3<true> (ebo_eval3.inc) with the parent's entry points; returns the number of results whose bits differ
// from the quarter-argument entry points', direct or folded
static int axis_taps(double f, double pre, const Consts& c, double (&w)[7])
{
	const double a = f * c.inv_sigsq;
	const double x = c.hs * (f * f);
	const double eg = ebo::exp_gauss(x);
	double p, q;
	ebo::exp_pair(a, p, q);
	int bad = 0;
	{
		double p1, q1, p2, q2;
		ebo::exp_pair_quarter(a * 0.25, p1, q1);
		ebo::exp_pair_quarter(f * (c.inv_sigsq * 0.25), p2, q2);
		bad += bits(p1) != bits(p) || bits(q1) != bits(q);
		bad += bits(p2) != bits(p) || bits(q2) != bits(q);
		bad += bits(ebo::exp_gauss_quarter(x * 0.25)) != bits(eg);
		bad += bits(ebo::exp_gauss_quarter((c.hs * 0.25) * (f * f))) != bits(eg);
	}
	const double e0 = pre * eg;
	const double p2 = p * p, q2 = q * q;
	const double e1 = c.ck1 * e0, e2 = c.ck2 * e0, e3 = c.ck3 * e0;
	w[3] = e0;
	w[4] = e1 * p;
	w[5] = e2 * p2;
	w[6] = e3 * (p2 * p);
	w[2] = e1 * q;
	w[1] = e2 * q2;
	w[0] = e3 * (q2 * q);
	return bad;
}

int main(int argc, char** argv)
{
	if (argc < 3)
	{
		return 2;
	}
	uint64_t state = std::strtoull(argv[1], nullptr, 10);
	const long n = std::atol(argv[2]);
	const double sigmas[4] = {1.0, 1.5, 2.0, 1000.0};
	Consts cs[4];
	for (int k = 0; k < 4; ++k)
	{
		cs[k] = consts_of(sigmas[k]);
	}
	double d1xOld = 0, d1xNew = 0, d1yOld = 0, d1yNew = 0, d2aOld = 0, d2aNew = 0, d2bOld = 0, d2bNew = 0;
	long badBits = 0, badSum = 0;
	for (long k = 0; k < n; ++k)
	{
		const Consts& c = cs[k & 3];
		double fx = unit(state), fy = unit(state);
		double g = 40.0 * unit(state) - 20.0;
		if (k & 1)
		{
			fx = -fx;
			fy = -fy;
		}
		if (k < 8)
		{
			fx = (k & 1) ? -0.0 : 0.0;
			fy = (k & 2) ? -0.0 : 0.0;
			g = (k & 4) ? -20.0 : 20.0;
		}
		double wx[7], wy[7], v[7][7];
		badBits += axis_taps(fx, c.norm, c, wx);
		badBits += axis_taps(fy, 1.0, c, wy);
		for (int j = 0; j < 7; ++j)
		{
			for (int i = 0; i < 7; ++i)
			{
				const uint64_t kind = splitmix64(state) & 3;
				const double u = unit(state);
				v[j][i] = kind == 0 ? 0.0 : kind == 1 ? 1000.0 * u : u;
			}
		}

		// ---- the parent's statements (eval_unit3's interior branches before the moment forms) ----
		const double gfx = g * fx, gfy = g * fy;
		double sumW = 0.0, sumA = 0.0, sumWy = 0.0, sumAy = 0.0;
		for (int i = 0; i < 7; ++i)
		{
			sumW += wx[i];
			sumA = __builtin_fma(wx[i], __builtin_fma(g, static_cast<double>(i - 3), -gfx), sumA);
		}
		for (int j = 0; j < 7; ++j)
		{
			const double ay = wy[j] * __builtin_fma(g, static_cast<double>(j - 3), -gfy);
			sumWy += wy[j];
			sumAy += ay;
		}
		double ax[7];
		for (int i = 0; i < 7; ++i)
		{
			ax[i] = wx[i] * __builtin_fma(g, static_cast<double>(i - 3), -gfx);
		}
		double d2a = 0.0, d2b = 0.0;
		for (int j = 0; j < 7; ++j)
		{
			double rb = wx[0] * v[j][0], ra = ax[0] * v[j][0];
			for (int i = 1; i < 7; ++i)
			{
				rb = __builtin_fma(wx[i], v[j][i], rb);
				ra = __builtin_fma(ax[i], v[j][i], ra);
			}
			const double ay = wy[j] * __builtin_fma(g, static_cast<double>(j - 3), -gfy);
			d2a = __builtin_fma(wy[j], ra, d2a);
			d2b = __builtin_fma(ay, rb, d2b);
		}

		// ---- the moment forms, as eval_unit3 calls them ----
		double mW, mA, mWy, mAy;
		ebo::axis_d1(wx, g, fx, mW, mA);
		ebo::axis_d1(wy, g, fy, mWy, mAy);
		badSum += bits(mW) != bits(sumW) || bits(mWy) != bits(sumWy);
		double kx[4];
		ebo::moment_table(wx, kx);
		double A = 0.0, B = 0.0, C = 0.0, rb, rc;
		ebo::moment_row(wx, kx, v[0], rb, rc);
		ebo::moment_acc<0>(wy[0], rb, rc, A, B, C);
		ebo::moment_row(wx, kx, v[1], rb, rc);
		ebo::moment_acc<1>(wy[1], rb, rc, A, B, C);
		ebo::moment_row(wx, kx, v[2], rb, rc);
		ebo::moment_acc<2>(wy[2], rb, rc, A, B, C);
		ebo::moment_row(wx, kx, v[3], rb, rc);
		ebo::moment_acc<3>(wy[3], rb, rc, A, B, C);
		ebo::moment_row(wx, kx, v[4], rb, rc);
		ebo::moment_acc<4>(wy[4], rb, rc, A, B, C);
		ebo::moment_row(wx, kx, v[5], rb, rc);
		ebo::moment_acc<5>(wy[5], rb, rc, A, B, C);
		ebo::moment_row(wx, kx, v[6], rb, rc);
		ebo::moment_acc<6>(wy[6], rb, rc, A, B, C);
		double m2a, m2b;
		ebo::moment_d2(g, fx, fy, A, B, C, m2a, m2b);

		// ---- long double, on the same doubles ----
		const long double G = g, FX = fx, FY = fy;
		long double tx = 0, ty = 0, ta = 0, tb = 0;
		double wxMax = 0, wyMax = 0, tapMax = 0;
		for (int i = 0; i < 7; ++i)
		{
			tx += static_cast<long double>(wx[i]) * (G * (static_cast<long double>(i - 3) - FX));
			ty += static_cast<long double>(wy[i]) * (G * (static_cast<long double>(i - 3) - FY));
			wxMax = std::fmax(wxMax, wx[i]);
			wyMax = std::fmax(wyMax, wy[i]);
		}
		for (int j = 0; j < 7; ++j)
		{
			for (int i = 0; i < 7; ++i)
			{
				const long double t = static_cast<long double>(wx[i]) * wy[j] * v[j][i];
				ta += t * (G * (static_cast<long double>(i - 3) - FX));
				tb += t * (G * (static_cast<long double>(j - 3) - FY));
				tapMax = std::fmax(tapMax, static_cast<double>(t));
			}
		}
		const long double ag = fabsl(G);
		auto err = [](double got, long double want, long double scale) {
			return scale > 0 ? static_cast<double>(fabsl(static_cast<long double>(got) - want) / scale) : 0.0;
		};
		d1xOld = std::fmax(d1xOld, err(sumA, tx, ag * wxMax));
		d1xNew = std::fmax(d1xNew, err(mA, tx, ag * wxMax));
		d1yOld = std::fmax(d1yOld, err(sumAy, ty, ag * wyMax));
		d1yNew = std::fmax(d1yNew, err(mAy, ty, ag * wyMax));
		d2aOld = std::fmax(d2aOld, err(d2a, ta, ag * tapMax));
		d2aNew = std::fmax(d2aNew, err(m2a, ta, ag * tapMax));
		d2bOld = std::fmax(d2bOld, err(d2b, tb, ag * tapMax));
		d2bNew = std::fmax(d2bNew, err(m2b, tb, ag * tapMax));
	}
	std::printf("d1x %.6g %.6g\n", d1xOld, d1xNew);
	std::printf("d1y %.6g %.6g\n", d1yOld, d1yNew);
	std::printf("d2a %.6g %.6g\n", d2aOld, d2aNew);
	std::printf("d2b %.6g %.6g\n", d2bOld, d2bNew);
	std::printf("sumw %ld\n", badSum);
	std::printf("bits %ld\n", badBits);
	const bool ok = d1xNew <= 4.0 * d1xOld && d1yNew <= 4.0 * d1yOld && d2aNew <= 4.0 * d2aOld && d2bNew <= 4.0 * d2bOld &&
					badSum == 0 && badBits == 0;
	return ok ? 0 : 1;
}
