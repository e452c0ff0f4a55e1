// align_sim3_serial.cpp — the trajectory-alignment rules of include/ebo.h (S1-S7) compiled for the host: the device's
// own text (csrc/ebo_align.inc) with the 64 lanes of a sum run one after the other on one thread.  The serial timing
// baseline of tools/time_align.py and the CPU check of that text (tests/test_align_cpu.py).  Not part of the library
// and not a fallback.
//
//   g++ -std=c++17 -O2 -ffp-contract=off -I include -o align_sim3_serial align_sim3_serial.cpp
//   align_sim3_serial <problem.f64> <result.f64> <repeats>
//       problem.f64, raw float64: n_points, n_segments, fix_scale, seg_begin [n_segments], seg_end [n_segments],
//         data [n_points][3], model [n_points][3].
//       result.f64: per segment scale, R [9], t [3], rmse, mean, min, max, count, status (19 doubles).
//       Prints one JSON line with the median milliseconds of `repeats` alignments of ALL segments.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../csrc/ebo_bundle.h"
#include "../csrc/ebo_relpose.h"
#include "../csrc/ebo_align.h"

using namespace ebo;
using std::fabs;
using std::sqrt;
#define EBO_RELPOSE_RULES_ONLY
#include "../csrc/ebo_relpose.inc"
#include "../csrc/ebo_align.inc"

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
	constexpr size_t kHead = 3;
	if (in.size() < kHead || repeats < 1)
	{
		std::fprintf(stderr, "short problem file or no repeats\n");
		return 2;
	}
	const long long N = static_cast<long long>(in[0]), G = static_cast<long long>(in[1]);
	const int fixScale = in[2] != 0.0 ? 1 : 0;
	if (N < 0 || G < 0 || G > kAlMaxSegments || in.size() != kHead + 2 * static_cast<size_t>(G) + 6 * static_cast<size_t>(N))
	{
		std::fprintf(stderr, "a negative point count, a segment count outside [0, 65535] or sizes that are not those of the file\n");
		return 2;
	}
	std::vector<int> begin(G), end(G);
	for (long long g = 0; g < G; ++g)
	{
		const double b = in[kHead + g], e = in[kHead + G + g];
		if (!(b >= 0.0 && e >= b && e <= static_cast<double>(N) && e - b <= kAlMaxSegmentPoints))
		{
			std::fprintf(stderr, "a segment outside [0, n_points] or beyond 2^24 points\n");
			return 2;
		}
		begin[g] = static_cast<int>(b);
		end[g] = static_cast<int>(e);
	}
	const double* data = in.data() + kHead + 2 * G;
	const double* model = data + 3 * N;
	std::vector<ebo_align_result> res(G);
	std::vector<double> ms;
	for (int rep = 0; rep < repeats; ++rep)
	{
		const auto t0 = std::chrono::steady_clock::now();
		for (long long g = 0; g < G; ++g)
		{
			AlView v;
			v.n = end[g] - begin[g];
			v.d = data + 3 * static_cast<size_t>(begin[g]);
			v.m = model + 3 * static_cast<size_t>(begin[g]);
			al_solve(v, fixScale, &res[g]);
		}
		ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
	}
	std::vector<double> out;
	size_t points = 0;
	for (long long g = 0; g < G; ++g)
	{
		const ebo_align_result& r = res[g];
		out.push_back(r.scale);
		out.insert(out.end(), r.R, r.R + 9);
		out.insert(out.end(), r.t, r.t + 3);
		const double tail[6] = {r.rmse, r.mean, r.min, r.max, static_cast<double>(r.count), static_cast<double>(r.status)};
		out.insert(out.end(), tail, tail + 6);
		points += static_cast<size_t>(r.count);
	}
	FILE* fo = std::fopen(argv[2], "wb");
	if (!fo || std::fwrite(out.data(), sizeof(double), out.size(), fo) != out.size())
	{
		std::fprintf(stderr, "cannot write %s\n", argv[2]);
		return 2;
	}
	std::fclose(fo);
	std::sort(ms.begin(), ms.end());
	std::printf("{\"segments\": %lld, \"points\": %zu, \"ms_median\": %.4f, \"repeats\": %d}\n", G, points, ms[ms.size() / 2], repeats);
	return 0;
}
