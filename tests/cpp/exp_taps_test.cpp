// The exponentials of csrc/exp_taps.h as the host compiles them (free of HIP), against expl.
//   exp_taps_test <seed> <points>
// draws <points> arguments of [-1, 1] from a 64-bit generator written out here (the same points on every platform),
// adds +-1 and +-0, and prints the largest relative errors:
//   yard  <exp_small on [-1, 1]>  <exp_small on [-0.5, 0]>      the degree-12 polynomial the kernels used before
//   pair  <exp_pair's p and q on [-1, 1]>  <largest |p q - 1|>
//   gauss <exp_gauss on [-0.5, 0]>                               (arguments -|x| / 2 of the same points)
//   edge  <p(0) q(0) p(-0) q(-0) gauss(0) gauss(-0)>             (each must be exactly 1)
// tests/test_exp_taps_cpu.py compiles this, runs it and asserts the bounds.
#include "../../event-based-odomety_amd/csrc/exp_taps.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>

// exp(x) for |x| <= 1 as ebo_eval3.inc had it: degree-12 Taylor on x / 4, two squarings.
static double exp_small(double x)
{
	const double t = x * 0.25;
	double p = 1.0 / 479001600.0;
	p = __builtin_fma(p, t, 1.0 / 39916800.0);
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

static uint64_t splitmix64(uint64_t& s)
{
	uint64_t z = (s += 0x9e3779b97f4a7c15ull);
	z = (z ^ (z >> 30)) * 0xbf58476d1ce4e5b9ull;
	z = (z ^ (z >> 27)) * 0x94d049bb133111ebull;
	return z ^ (z >> 31);
}

static double rel(double got, long double x)
{
	const long double want = expl(x);
	return static_cast<double>(fabsl((static_cast<long double>(got) - want) / want));
}

int main(int argc, char** argv)
{
	if (argc < 3)
	{
		return 2;
	}
	uint64_t state = std::strtoull(argv[1], nullptr, 10);
	const long n = std::atol(argv[2]);
	double yard = 0.0, yardHalf = 0.0, pair = 0.0, prod = 0.0, gauss = 0.0;
	for (long k = -4; k < n; ++k)
	{
		double x;
		if (k < 0)
		{
			x = (k == -4) ? 1.0 : (k == -3) ? -1.0 : (k == -2) ? 0.0 : -0.0;
		}
		else
		{
			// 53 random bits in [0, 1), then onto [-1, 1)
			x = static_cast<double>(splitmix64(state) >> 11) * (1.0 / 9007199254740992.0) * 2.0 - 1.0;
		}
		double p, q;
		ebo::exp_pair(x, p, q);
		yard = std::fmax(yard, rel(exp_small(x), x));
		pair = std::fmax(pair, std::fmax(rel(p, x), rel(q, -static_cast<long double>(x))));
		prod = std::fmax(prod, std::fabs(p * q - 1.0));
		const double h = -0.5 * std::fabs(x);
		yardHalf = std::fmax(yardHalf, rel(exp_small(h), h));
		gauss = std::fmax(gauss, rel(ebo::exp_gauss(h), h));
	}
	double p0, q0, p1, q1;
	ebo::exp_pair(0.0, p0, q0);
	ebo::exp_pair(-0.0, p1, q1);
	std::printf("yard %.17g %.17g\n", yard, yardHalf);
	std::printf("pair %.17g %.17g\n", pair, prod);
	std::printf("gauss %.17g\n", gauss);
	std::printf("edge %.17g %.17g %.17g %.17g %.17g %.17g\n", p0, q0, p1, q1, ebo::exp_gauss(0.0), ebo::exp_gauss(-0.0));
	return 0;
}
