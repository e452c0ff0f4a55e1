// abs_pose_serial.cpp — the absolute-pose rules of include/ebo.h (A1-A5) compiled for the host and run the way a CPU
// runs RANSAC: one thread, one hypothesis after the other, each scored against every point, stopping by A5 as soon as
// it allows.  A throw-away yardstick for tools/time_abs_pose.py: what the device's "all hypotheses at once" is
// honestly compared with.  Not part of the library and not a fallback.
//
//   g++ -std=c++17 -O2 -ffp-contract=off -o abs_pose_serial abs_pose_serial.cpp
//   abs_pose_serial <f.f64> <points.f64> <seed> <frame> <max_iterations> <repeats> <threshold> [models_out.f64]
//       f / points: raw float64 [n][3].  Prints one JSON line: winner, iterations, inliers, median milliseconds.
//       With models_out every hypothesis is solved (no early stop, nothing timed) and written as raw float64
//       [max_iterations][13]: the [3][4] pose (zeros without a model) and 1.0 / 0.0 for "has a model".
//
// The closed forms are the device's own text: the rules parts of csrc/ebo_twoview.inc and csrc/ebo_abspose.inc
// compiled with the rounding intrinsics spelled as plain operators.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>

#define __device__
#define __forceinline__ inline
#define __restrict__
#define __dadd_rn(a, b) ((a) + (b))
#define __dsub_rn(a, b) ((a) - (b))
#define __dmul_rn(a, b) ((a) * (b))
#define __ddiv_rn(a, b) ((a) / (b))
#define __dsqrt_rn(a) std::sqrt(a)
#define EBO_TWOVIEW_RULES_ONLY
#define EBO_ABSPOSE_RULES_ONLY
using std::fabs;
#include "../csrc/ebo_twoview.inc"
#include "../csrc/ebo_abspose.inc"

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

// A2-A4 for one hypothesis: false when it has no model
bool solve(const double* f, const double* pts, int n, unsigned long long seed, int frame, int h, TvPoseRT& out)
{
	int smp[4];
	ransac_sample<4>(seed, frame, h, n, smp);
	double sf[4][3], sp[4][3];
	for (int i = 0; i < 4; ++i)
	{
		for (int k = 0; k < 3; ++k)
		{
			sf[i][k] = f[3 * smp[i] + k];
			sp[i][k] = pts[3 * smp[i] + k];
		}
	}
	return ap_solve(sf, sp, out);
}
}  // namespace

int main(int argc, char** argv)
{
	if (argc != 8 && argc != 9)
	{
		std::fprintf(stderr, "usage: %s <f.f64> <points.f64> <seed> <frame> <max_iterations> <repeats> <threshold> [models_out.f64]\n",
					 argv[0]);
		return 2;
	}
	const std::vector<double> f = readAll(argv[1]), pts = readAll(argv[2]);
	const unsigned long long seed = std::strtoull(argv[3], nullptr, 10);
	const int frame = std::atoi(argv[4]), H = std::atoi(argv[5]), repeats = std::atoi(argv[6]);
	const double threshold = std::atof(argv[7]), probability = 0.99;
	const int n = static_cast<int>(f.size() / 3);
	if (n < 4 || pts.size() != f.size() || H < 1 || repeats < 1 || !(threshold > 0.0))
	{
		std::fprintf(stderr, "need two equal lists of at least 4 vectors and a positive threshold\n");
		return 2;
	}
	if (argc == 9)
	{
		std::vector<double> out(static_cast<size_t>(H) * 13, 0.0);
		for (int h = 0; h < H; ++h)
		{
			TvPoseRT T;
			if (solve(f.data(), pts.data(), n, seed, frame, h, T))
			{
				double* o = out.data() + 13 * static_cast<size_t>(h);
				for (int i = 0; i < 3; ++i)
				{
					for (int j = 0; j < 3; ++j)
					{
						o[4 * i + j] = T.R[i][j];
					}
					o[4 * i + 3] = T.t[i];
				}
				o[12] = 1.0;
			}
		}
		FILE* fo = std::fopen(argv[8], "wb");
		if (!fo || std::fwrite(out.data(), sizeof(double), out.size(), fo) != out.size())
		{
			std::fprintf(stderr, "cannot write %s\n", argv[8]);
			return 2;
		}
		std::fclose(fo);
	}
	std::vector<double> ms;
	int best = -1, winner = -1, iterations = 0;
	for (int rep = 0; rep < repeats; ++rep)
	{
		const auto t0 = std::chrono::steady_clock::now();
		best = -1;
		winner = -1;
		double k = static_cast<double>(H);
		int h = 0;
		for (;; ++h)
		{
			TvPoseRT T;
			int count = 0;
			if (solve(f.data(), pts.data(), n, seed, frame, h, T))
			{
				for (int i = 0; i < n; ++i)
				{
					const double a[3] = {f[3 * i], f[3 * i + 1], f[3 * i + 2]};
					const double b[3] = {pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]};
					count += ap_score(T, a, b) < threshold ? 1 : 0;
				}
			}
			if (count > best)
			{
				best = count;
				winner = h;
				const double w = static_cast<double>(best) / n;
				const double w2 = w * w, w4 = w2 * w2;
				k = std::log(1.0 - probability) / std::log(std::min(std::max(1.0 - w4, 1e-15), 1.0 - 1e-15));
			}
			if (h + 1 >= k || h + 1 == H)
			{
				break;
			}
		}
		iterations = h + 1;
		ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
	}
	std::sort(ms.begin(), ms.end());
	std::printf("{\"n\": %d, \"winner\": %d, \"iterations\": %d, \"inliers\": %d, \"found\": %s, \"ms_median\": %.4f, \"repeats\": %d}\n", n,
				winner, iterations, best, best >= 4 ? "true" : "false", ms[ms.size() / 2], repeats);
	return 0;
}
