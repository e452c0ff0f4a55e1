// rotation_serial.cpp — the rotational warp's rule functions (csrc/ebo_rotation.inc: rot_warp, rot_weights, rot_terms;
// rules V1-V3 and V8 of include/ebo.h) compiled for the host and run the way a CPU runs them, one event after the other,
// with the kernels' own in-image tests around every access of the vote image.  The CPU check of that text
// (tests/test_rotation_cpu.py) and, built with -fsanitize=address,undefined, the check that no border case reads or
// writes outside the image.  Not part of the library and not a fallback.
//
//   g++ -std=c++17 -O2 -ffp-contract=off -o rotation_serial rotation_serial.cpp
//   rotation_serial <problem.f64> <result.f64>
//       problem.f64, raw float64: w, h, fx, fy, cx, cy, wx, wy, wz, n, then n x (x, y, dt_us).
//       result.f64: H [h][w] as doubles (exact below 2^53), then voted (the number of events that voted), then
//         S [3] = the sum over the voting events, in their order, of V8's terms with C = H * 2^-30 - mu (sigma_blur = 0;
//         mu from the exact integer sum of H).
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/ebo.h"

#define __device__
#define __forceinline__ inline
#define __restrict__
#define __dadd_rn(a, b) ((a) + (b))
#define __dsub_rn(a, b) ((a) - (b))
#define __dmul_rn(a, b) ((a) * (b))
#define __ddiv_rn(a, b) ((a) / (b))
#define EBO_ROTATION_RULES_ONLY
#include "../csrc/ebo_rotation.h"
namespace ebo
{
using std::floor;
using std::rint;
#include "../csrc/ebo_rotation.inc"
}  // namespace ebo
using namespace ebo;

int main(int argc, char** argv)
{
	if (argc != 3)
	{
		std::fprintf(stderr, "usage: rotation_serial <problem.f64> <result.f64>\n");
		return 2;
	}
	std::vector<double> in;
	FILE* f = std::fopen(argv[1], "rb");
	if (!f)
	{
		std::fprintf(stderr, "cannot open %s\n", argv[1]);
		return 2;
	}
	double buf[1024];
	size_t got;
	while ((got = std::fread(buf, sizeof(double), 1024, f)) > 0)
	{
		in.insert(in.end(), buf, buf + got);
	}
	std::fclose(f);
	if (in.size() < 10 || in.size() != 10 + 3 * static_cast<size_t>(in[9]))
	{
		std::fprintf(stderr, "malformed problem\n");
		return 2;
	}
	RotConsts k{};
	k.w = static_cast<int>(in[0]);
	k.h = static_cast<int>(in[1]);
	k.fx = in[2];
	k.fy = in[3];
	k.cx = in[4];
	k.cy = in[5];
	const double wx = in[6], wy = in[7], wz = in[8];
	const size_t n = static_cast<size_t>(in[9]);
	std::vector<long long> H(static_cast<size_t>(k.w) * k.h, 0);
	auto inside = [&](int px, int py) { return px >= 0 && px < k.w && py >= 0 && py < k.h; };
	auto tau = [&](size_t e) { return in[10 + 3 * e + 2] * 1e-6; };
	auto warp = [&](size_t e, RotEvent& r) {
		return rot_warp(k, static_cast<int>(in[10 + 3 * e]), static_cast<int>(in[10 + 3 * e + 1]), tau(e), wx, wy, wz, r);
	};
	double voted = 0.0;
	for (size_t e = 0; e < n; ++e)
	{
		RotEvent r;
		if (!warp(e, r))
		{
			continue;
		}
		voted += 1.0;
		long long q[4];
		rot_weights(r, q);
		for (int t = 0; t < 4; ++t)
		{
			const int px = r.x0 + (t & 1), py = r.y0 + (t >> 1);
			if (inside(px, py))
			{
				H[static_cast<size_t>(py) * k.w + px] += q[t];
			}
		}
	}
	long long total = 0;
	for (const long long v : H)
	{
		total += v;
	}
	const double mu = static_cast<double>(total) * 0x1p-30 / (static_cast<double>(k.w) * static_cast<double>(k.h));
	double S[3] = {0.0, 0.0, 0.0};
	for (size_t e = 0; e < n; ++e)
	{
		RotEvent r;
		if (!warp(e, r))
		{
			continue;
		}
		double c[4];
		for (int t = 0; t < 4; ++t)
		{
			const int px = r.x0 + (t & 1), py = r.y0 + (t >> 1);
			c[t] = inside(px, py) ? static_cast<double>(H[static_cast<size_t>(py) * k.w + px]) * 0x1p-30 - mu : 0.0;
		}
		double t3[3];
		rot_terms(k, r, tau(e), c[0], c[1], c[2], c[3], t3);
		for (int i = 0; i < 3; ++i)
		{
			S[i] = S[i] + t3[i];
		}
	}
	FILE* o = std::fopen(argv[2], "wb");
	if (!o)
	{
		std::fprintf(stderr, "cannot write %s\n", argv[2]);
		return 2;
	}
	std::vector<double> out(H.begin(), H.end());
	out.push_back(voted);
	out.insert(out.end(), S, S + 3);
	std::fwrite(out.data(), sizeof(double), out.size(), o);
	std::fclose(o);
	return 0;
}
