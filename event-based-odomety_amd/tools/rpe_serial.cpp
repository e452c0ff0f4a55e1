// rpe_serial.cpp — the relative-pose-error rules of include/ebo.h (T1-T7) compiled for the host: the device's own text
// (csrc/ebo_rpe.inc) with the 64 lanes of a sum run one after the other on one thread.  The serial timing baseline of
// tools/time_rpe.py and the CPU check of that text (tests/test_rpe_cpu.py).  Not part of the library and not a
// fallback.
//
//   g++ -std=c++17 -O2 -ffp-contract=off -I include -o rpe_serial rpe_serial.cpp
//   rpe_serial <problem.f64> <result.f64> <repeats>
//       problem.f64, raw float64: n_poses, n_segments, n_deltas, has_scale (0 or 1), seg_begin [n_segments],
//         seg_end [n_segments], seg_scale [n_segments] (only with has_scale), deltas [n_deltas], gt [n_poses][12],
//         est [n_poses][12].
//       result.f64: per (segment, delta) the translation's rmse, mean, min, max, the rotation's rmse, mean, min, max,
//         count, status (10 doubles).
//       Prints one JSON line with the median milliseconds of `repeats` evaluations of ALL units.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/ebo.h"
#include "../csrc/ebo_relpose.h"
#include "../csrc/ebo_rpe.h"

using namespace ebo;
using std::fabs;
using std::sqrt;
#define EBO_RELPOSE_RULES_ONLY
#include "../csrc/ebo_relpose.inc"
#include "../csrc/ebo_rpe.inc"

namespace
{
std::vector<double> readAll(const char* path)
{
	std::vector<double> v;
	FILE* f = std::fopen(path, "rb");
	if (!f)
	{
		std::fprintf(stderr, "cannot open %s\n", path);
		std::exit(2);
	}
	double buf[1024];
	size_t n;
	while ((n = std::fread(buf, sizeof(double), 1024, f)) > 0)
	{
		v.insert(v.end(), buf, buf + n);
	}
	std::fclose(f);
	return v;
}
}  // namespace

int main(int argc, char** argv)
{
	if (argc != 4)
	{
		std::fprintf(stderr, "usage: %s <problem.f64> <result.f64> <repeats>\n", argv[0]);
		return 2;
	}
	const std::vector<double> in = readAll(argv[1]);
	const int repeats = std::atoi(argv[3]);
	constexpr size_t kHead = 4;
	if (in.size() < kHead || repeats < 1)
	{
		std::fprintf(stderr, "short problem file or no repeats\n");
		return 2;
	}
	const long long N = static_cast<long long>(in[0]), G = static_cast<long long>(in[1]), D = static_cast<long long>(in[2]);
	const bool hasScale = in[3] != 0.0;
	if (N < 0 || G < 0 || G > kRpeMaxSegments || D < 0 || D > kRpeMaxDeltas ||
		in.size() != kHead + static_cast<size_t>(G) * (hasScale ? 3 : 2) + static_cast<size_t>(D) +
						 2 * kRpePoseDoubles * static_cast<size_t>(N))
	{
		std::fprintf(stderr, "a negative pose count, a segment or delta count out of range or sizes that are not those of the file\n");
		return 2;
	}
	std::vector<int> begin(G), end(G), deltas(D);
	std::vector<double> scale(G, 1.0);
	const double* at = in.data() + kHead;
	for (long long g = 0; g < G; ++g)
	{
		const double b = at[g], e = at[G + g];
		if (!(b >= 0.0 && e >= b && e <= static_cast<double>(N) && e - b <= kRpeMaxSegmentPoses))
		{
			std::fprintf(stderr, "a segment outside [0, n_poses] or beyond 2^24 poses\n");
			return 2;
		}
		begin[g] = static_cast<int>(b);
		end[g] = static_cast<int>(e);
	}
	at += 2 * G;
	if (hasScale)
	{
		std::copy(at, at + G, scale.begin());
		at += G;
	}
	for (long long k = 0; k < D; ++k)
	{
		if (!(at[k] >= 1.0 && at[k] <= 2147483647.0))
		{
			std::fprintf(stderr, "a delta below 1\n");
			return 2;
		}
		deltas[k] = static_cast<int>(at[k]);
	}
	at += D;
	const double* gt = at;
	const double* est = gt + kRpePoseDoubles * N;
	std::vector<ebo_rpe_result> res(static_cast<size_t>(G * D));
	std::vector<double> ms;
	for (int rep = 0; rep < repeats; ++rep)
	{
		const auto t0 = std::chrono::steady_clock::now();
		for (long long g = 0; g < G; ++g)
		{
			for (long long k = 0; k < D; ++k)
			{
				RpeView v;
				v.n = end[g] - begin[g];
				v.delta = deltas[k];
				v.s = scale[g];
				v.gt = gt + kRpePoseDoubles * static_cast<size_t>(begin[g]);
				v.est = est + kRpePoseDoubles * static_cast<size_t>(begin[g]);
				rpe_unit(v, &res[static_cast<size_t>(g * D + k)]);
			}
		}
		ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
	}
	std::vector<double> out;
	size_t pairs = 0;
	for (const ebo_rpe_result& r : res)
	{
		const double row[10] = {r.trans_rmse, r.trans_mean, r.trans_min, r.trans_max, r.rot_rmse,
								r.rot_mean,   r.rot_min,    r.rot_max,   static_cast<double>(r.count), static_cast<double>(r.status)};
		out.insert(out.end(), row, row + 10);
		pairs += static_cast<size_t>(r.count);
	}
	FILE* fo = std::fopen(argv[2], "wb");
	if (!fo || std::fwrite(out.data(), sizeof(double), out.size(), fo) != out.size())
	{
		std::fprintf(stderr, "cannot write %s\n", argv[2]);
		return 2;
	}
	std::fclose(fo);
	std::sort(ms.begin(), ms.end());
	std::printf("{\"units\": %zu, \"pairs\": %zu, \"ms_median\": %.4f, \"repeats\": %d}\n", res.size(), pairs, ms[ms.size() / 2], repeats);
	return 0;
}
