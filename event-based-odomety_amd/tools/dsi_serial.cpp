// dsi_serial.cpp — the space-sweep vote's rule functions (csrc/ebo_depth.inc: dsi_ray, dsi_uv, dsi_tap, dsi_weights;
// rules M2-M4 of include/ebo.h) compiled for the host and run the way a CPU runs them, one event and one plane after
// the other, with the kernel's own in-image tests around every access of the volume.  The CPU check of that text
// (tests/test_depth_cpu.py) and, built with -fsanitize=address,undefined, the check that no border case reads or writes
// outside the volume.  Not part of the library and not a fallback.
//
//   g++ -std=c++17 -O2 -ffp-contract=off -o dsi_serial dsi_serial.cpp
//   dsi_serial <problem.f64> <result.f64>
//       problem.f64, raw float64: w, h, fx, fy, cx, cy, nz, z [nz], Rr [9], tr [3] (M2's relative pose), n, then
//         n x (x, y).
//       result.f64: H [nz][h][w] as doubles (exact), then the number of (event, plane) pairs that voted.
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
#define EBO_DEPTH_RULES_ONLY
#include "../csrc/ebo_depth.h"
namespace ebo
{
using std::floor;
using std::rint;
#include "../csrc/ebo_depth.inc"
}  // namespace ebo
using namespace ebo;

int main(int argc, char** argv)
{
	if (argc != 3)
	{
		std::fprintf(stderr, "usage: dsi_serial <problem.f64> <result.f64>\n");
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
	const size_t nz = in.size() > 6 ? static_cast<size_t>(in[6]) : 0;
	const size_t head = 7 + nz + 12 + 1;
	if (nz < 2 || nz > static_cast<size_t>(kDsiMaxPlanes) || in.size() < head || in.size() != head + 2 * static_cast<size_t>(in[head - 1]))
	{
		std::fprintf(stderr, "malformed problem\n");
		return 2;
	}
	DsiConsts k{};
	k.w = static_cast<int>(in[0]);
	k.h = static_cast<int>(in[1]);
	k.fx = in[2];
	k.fy = in[3];
	k.cx = in[4];
	k.cy = in[5];
	k.nz = static_cast<int>(nz);
	const double* z = &in[7];
	DsiPose p;
	for (int i = 0; i < 9; ++i)
	{
		p.Rr[i] = in[7 + nz + i];
	}
	for (int i = 0; i < 3; ++i)
	{
		p.tr[i] = in[7 + nz + 9 + i];
	}
	const size_t n = static_cast<size_t>(in[head - 1]);
	const size_t np = static_cast<size_t>(k.w) * k.h;
	std::vector<uint32_t> H(nz * np, 0u);
	double voted = 0.0;
	for (size_t e = 0; e < n; ++e)
	{
		DsiRay r;
		dsi_ray(k, p, static_cast<int>(in[head + 2 * e]), static_cast<int>(in[head + 2 * e + 1]), r);
		for (size_t kp = 0; kp < nz; ++kp)
		{
			double u, v;
			DsiTap t;
			if (!dsi_uv(k, p, r, z[kp], u, v) || !dsi_tap(k, u, v, t))
			{
				continue;
			}
			voted += 1.0;
			unsigned int q[4];
			dsi_weights(t, q);
			for (int i = 0; i < 4; ++i)
			{
				const int px = t.x0 + (i & 1), py = t.y0 + (i >> 1);
				if (px >= 0 && px < k.w && py >= 0 && py < k.h)
				{
					H[kp * np + static_cast<size_t>(py) * k.w + px] += q[i];
				}
			}
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
	std::fwrite(out.data(), sizeof(double), out.size(), o);
	std::fclose(o);
	return 0;
}
