// two_view_serial.cpp — the two-view rules of include/ebo.h (rules 1-6) compiled for the host and run the way a CPU
// runs RANSAC: one thread, one hypothesis after the other, each scored against every correspondence, stopping by
// rule 6 as soon as it allows.  A throw-away yardstick for tools/time_two_view.py: what the device's "all hypotheses
// at once" is honestly compared with.  Not part of the library and not a fallback.
//
//   g++ -std=c++17 -O2 -ffp-contract=off -o two_view_serial two_view_serial.cpp
//   two_view_serial <f1.f64> <f2.f64> <seed> <pair> <max_iterations> <repeats>
//       f1 / f2: raw float64 [n][3].  Prints one JSON line: winner, iterations, inliers, median milliseconds.
//
// The closed forms (triangulation, score, sampler, rotation, 3 x 3 Jacobi) are the device's own text: the rules part
// of csrc/ebo_twoview.inc compiled with the rounding intrinsics spelled as plain operators.
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
using std::fabs;
#include "../csrc/ebo_twoview.inc"

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

// rules 3-5 for one hypothesis: false when it has no model
bool solve(const double* f1, const double* f2, int n, unsigned long long seed, int pair, int h, TvPoseRT& out)
{
	int smp[8];
	ransac_sample<8>(seed, pair, h, n, smp);
	double S1[8][3], S2[8][3], A[8][9], V[9][9];
	for (int i = 0; i < 8; ++i)
	{
		for (int k = 0; k < 3; ++k)
		{
			S1[i][k] = f1[3 * smp[i] + k];
			S2[i][k] = f2[3 * smp[i] + k];
		}
		for (int j = 0; j < 9; ++j)
		{
			A[i][j] = S2[i][j / 3] * S1[i][j % 3];
		}
	}
	for (int i = 0; i < 9; ++i)
	{
		for (int j = 0; j < 9; ++j)
		{
			V[i][j] = i == j ? 1.0 : 0.0;
		}
	}
	auto col = [&](int p, int q) {
		double acc = A[0][p] * A[0][q];
		for (int i = 1; i < 8; ++i)
		{
			acc = acc + A[i][p] * A[i][q];
		}
		return acc;
	};
	for (int sweep = 0; sweep < kTvSweeps9; ++sweep)
	{
		for (int p = 0; p < 8; ++p)
		{
			for (int q = p + 1; q < 9; ++q)
			{
				const double app = col(p, p), aqq = col(q, q), apq = col(p, q);
				if (apq != 0.0)
				{
					double t, c, s;
					tv_rotation(app, aqq, apq, t, c, s);
					for (int i = 0; i < 8; ++i)
					{
						const double x = A[i][p], y = A[i][q];
						A[i][p] = c * x - s * y;
						A[i][q] = s * x + c * y;
					}
					for (int i = 0; i < 9; ++i)
					{
						const double x = V[i][p], y = V[i][q];
						V[i][p] = c * x - s * y;
						V[i][q] = s * x + c * y;
					}
				}
			}
		}
	}
	int jmin = 0;
	double dmin = col(0, 0);
	for (int j = 1; j < 9; ++j)
	{
		const double dj = col(j, j);
		if (dj < dmin)
		{
			dmin = dj;
			jmin = j;
		}
	}
	double F[3][3];
	for (int a = 0; a < 3; ++a)
	{
		for (int b = 0; b < 3; ++b)
		{
			F[b][a] = V[3 * a + b][jmin];
		}
	}
	double G3[3][3], V3[3][3];
	for (int j = 0; j < 3; ++j)
	{
		for (int c = 0; c < 3; ++c)
		{
			G3[j][c] = tv_dot3(F[0][j], F[1][j], F[2][j], F[0][c], F[1][c], F[2][c]);
			V3[j][c] = j == c ? 1.0 : 0.0;
		}
	}
	for (int sweep = 0; sweep < kTvSweeps3; ++sweep)
	{
		tv_rot3<0, 1>(G3, V3);
		tv_rot3<0, 2>(G3, V3);
		tv_rot3<1, 2>(G3, V3);
	}
	double dd[3] = {G3[0][0], G3[1][1], G3[2][2]};
	double vc[3][3];
	for (int c = 0; c < 3; ++c)
	{
		for (int r = 0; r < 3; ++r)
		{
			vc[c][r] = V3[r][c];
		}
	}
	const int order[3][2] = {{0, 1}, {1, 2}, {0, 1}};
	for (const auto& ab : order)
	{
		if (dd[ab[0]] < dd[ab[1]])
		{
			std::swap(dd[ab[0]], dd[ab[1]]);
			std::swap(vc[ab[0]], vc[ab[1]]);
		}
	}
	const double s0 = std::sqrt(dd[0]), s1 = std::sqrt(dd[1]);
	if (!(s0 > 0.0) || !(s1 > 0.0))
	{
		return false;
	}
	double u0[3], u1[3], u2[3], v2[3];
	for (int i = 0; i < 3; ++i)
	{
		u0[i] = tv_dot3(F[i][0], F[i][1], F[i][2], vc[0][0], vc[0][1], vc[0][2]) / s0;
		u1[i] = tv_dot3(F[i][0], F[i][1], F[i][2], vc[1][0], vc[1][1], vc[1][2]) / s1;
	}
	const double n0 = std::sqrt(tv_dot3(u0[0], u0[1], u0[2], u0[0], u0[1], u0[2]));
	for (double& x : u0)
	{
		x = x / n0;
	}
	const double hh = tv_dot3(u0[0], u0[1], u0[2], u1[0], u1[1], u1[2]);
	for (int i = 0; i < 3; ++i)
	{
		u1[i] = u1[i] - hh * u0[i];
	}
	const double n1 = std::sqrt(tv_dot3(u1[0], u1[1], u1[2], u1[0], u1[1], u1[2]));
	for (double& x : u1)
	{
		x = x / n1;
	}
	tv_cross(u0, u1, u2);
	tv_cross(vc[0], vc[1], v2);
	TvPoseRT cand[4];
	for (int i = 0; i < 3; ++i)
	{
		for (int j = 0; j < 3; ++j)
		{
			const double a = u1[i] * vc[0][j], b = u0[i] * vc[1][j], c = u2[i] * v2[j];
			cand[0].R[i][j] = (a - b) + c;
			cand[2].R[i][j] = (b - a) + c;
		}
	}
	for (int k = 0; k < 4; k += 2)
	{
		if (tv_det3(cand[k].R) < 0.0)
		{
			for (auto& row : cand[k].R)
			{
				for (double& x : row)
				{
					x = -x;
				}
			}
		}
		cand[k + 1] = cand[k];
		for (int i = 0; i < 3; ++i)
		{
			cand[k].t[i] = u2[i];
			cand[k + 1].t[i] = -u2[i];
		}
	}
	double best = HUGE_VAL;
	int bc = -1;
	for (int k = 0; k < 4; ++k)
	{
		double tot = tv_score(cand[k], S1[0], S2[0]);
		for (int i = 1; i < 8; ++i)
		{
			tot = tot + tv_score(cand[k], S1[i], S2[i]);
		}
		if (std::isfinite(tot) && tot < best)
		{
			best = tot;
			bc = k;
		}
	}
	if (bc < 0)
	{
		return false;
	}
	out = cand[bc];
	return true;
}
}  // namespace

int main(int argc, char** argv)
{
	if (argc != 7)
	{
		std::fprintf(stderr, "usage: %s <f1.f64> <f2.f64> <seed> <pair> <max_iterations> <repeats>\n", argv[0]);
		return 2;
	}
	const std::vector<double> f1 = readAll(argv[1]), f2 = readAll(argv[2]);
	const unsigned long long seed = std::strtoull(argv[3], nullptr, 10);
	const int pair = std::atoi(argv[4]), H = std::atoi(argv[5]), repeats = std::atoi(argv[6]);
	const int n = static_cast<int>(f1.size() / 3);
	if (n < 8 || f2.size() != f1.size() || H < 1 || repeats < 1)
	{
		std::fprintf(stderr, "need two equal lists of at least 8 bearing vectors\n");
		return 2;
	}
	const double threshold = 5e-5, probability = 0.99;
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
			if (solve(f1.data(), f2.data(), n, seed, pair, h, T))
			{
				for (int i = 0; i < n; ++i)
				{
					const double a1[3] = {f1[3 * i], f1[3 * i + 1], f1[3 * i + 2]};
					const double a2[3] = {f2[3 * i], f2[3 * i + 1], f2[3 * i + 2]};
					count += tv_score(T, a1, a2) < threshold ? 1 : 0;
				}
			}
			if (count > best)
			{
				best = count;
				winner = h;
				const double w = static_cast<double>(best) / n;
				const double w2 = w * w, w4 = w2 * w2, w8 = w4 * w4;
				k = std::log(1.0 - probability) / std::log(std::min(std::max(1.0 - w8, 1e-15), 1.0 - 1e-15));
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
				winner, iterations, best, best >= 8 ? "true" : "false", ms[ms.size() / 2], repeats);
	return 0;
}
