// landmark_serial.cpp — the landmark-maintenance rules of include/ebo.h (L1-L7) compiled for the host: the device's own
// rule functions (csrc/ebo_landmark.inc, with the parts of csrc/ebo_twoview.inc and csrc/ebo_abspose.inc they use) run
// the way a CPU runs them, one thread, one landmark after the other, one hypothesis after the other.  The serial
// timing baseline of tools/time_triangulate_tracks.py and the CPU check of that text (tests/test_landmark_cpu.py).
// Not part of the library and not a fallback.
//
//   g++ -std=c++17 -O2 -ffp-contract=off -o landmark_serial landmark_serial.cpp
//   landmark_serial <problem.f64> <result.f64> <repeats>
//       problem.f64, raw float64: audit (0: triangulate, 1: audit), n_poses, n_landmarks, threshold, min_parallax,
//         min_inliers, max_hypotheses, seed, obs_offsets [n_landmarks + 1], obs_pose [n_obs], poses [n_poses][12],
//         obs_f [n_obs][3], points [n_landmarks][3] (only with audit).
//       result.f64: per landmark point [3], parallax, score_max, status, n_obs, n_inliers, winner, hypotheses
//         (10 doubles); then scores [n_obs] and flags [n_obs] (as doubles).
//       Prints one JSON line with the median milliseconds of `repeats` evaluations of ALL landmarks.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "../../include/ebo.h"
#include "../csrc/ebo_landmark.h"

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
#define EBO_LANDMARK_RULES_ONLY
using namespace ebo;
using std::fabs;
#include "../csrc/ebo_twoview.inc"
#include "../csrc/ebo_abspose.inc"
#include "../csrc/ebo_landmark.inc"

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

struct Problem
{
	bool audit;
	int nPoses, n;
	ebo_landmark_params prm;
	std::vector<int> offsets, obsPose;
	const double* poses;
	const double* obsF;
	const double* points;
};

// L2's sums over the observations with in[o], the sixteen partials and their tree as the rule writes them
void treeSums(const std::vector<double>& rays, const std::vector<char>& in, int m, double (&S)[kLmTerms])
{
	double part[kLmPartials][kLmTerms] = {};
	for (int o = 0; o < m; ++o)
	{
		if (in[o])
		{
			double r[6], t[kLmTerms];
			std::copy(rays.begin() + 6 * o, rays.begin() + 6 * o + 6, r);
			lm_terms(r, t);
			for (int k = 0; k < kLmTerms; ++k)
			{
				part[o % kLmPartials][k] = part[o % kLmPartials][k] + t[k];
			}
		}
	}
	for (int s = kLmPartials / 2; s > 0; s /= 2)
	{
		for (int i = 0; i < s; ++i)
		{
			for (int k = 0; k < kLmTerms; ++k)
			{
				part[i][k] = part[i][k] + part[i + s][k];
			}
		}
	}
	std::copy(part[0], part[0] + kLmTerms, S);
}

void landmark(const Problem& p, int l, ebo_landmark_result& out, double* scores, double* flags)
{
	const int base = p.offsets[l], m = p.offsets[l + 1] - base;
	out = ebo_landmark_result{};
	out.n_obs = m;
	out.winner = -1;
	std::fill(scores + base, scores + base + m, 0.0);
	std::fill(flags + base, flags + base + m, 0.0);
	auto pose = [&](int o) { return p.poses + kLmPoseDoubles * static_cast<size_t>(p.obsPose[base + o]); };
	auto bearing = [&](int o) { return p.obsF + 3 * static_cast<size_t>(base + o); };
	// L6's scan
	bool bad = false;
	for (int o = 0; o < m && !bad; ++o)
	{
		const int k = p.obsPose[base + o];
		bad = k < 0 || k >= p.nPoses;
		for (int i = 0; i < 3 && !bad; ++i)
		{
			bad = !lm_finite(bearing(o)[i]);
		}
		for (int i = 0; i < kLmPoseDoubles && !bad; ++i)
		{
			bad = !lm_finite(pose(o)[i]);
		}
	}
	double X[3] = {0.0, 0.0, 0.0};
	if (p.audit)
	{
		for (int i = 0; i < 3; ++i)
		{
			X[i] = p.points[3 * static_cast<size_t>(l) + i];
			bad = bad || !lm_finite(X[i]);
		}
	}
	if (bad)
	{
		out.status = 2;
		return;
	}
	if (m < (p.audit ? 1 : 2))
	{
		out.status = 1;
		return;
	}
	// L1
	const double cref[3] = {pose(0)[3], pose(0)[7], pose(0)[11]};
	std::vector<double> rays(6 * static_cast<size_t>(m));
	for (int o = 0; o < m; ++o)
	{
		const double f[3] = {bearing(o)[0], bearing(o)[1], bearing(o)[2]};
		double r[6];
		lm_ray(pose(o), f, cref, r);
		std::copy(r, r + 6, rays.begin() + 6 * o);
	}
	std::vector<char> in(static_cast<size_t>(m));
	double S[kLmTerms];
	if (!p.audit)
	{
		// L4
		const long long nPairs = static_cast<long long>(m) * (m - 1) / 2;
		const bool exhaustive = nPairs <= p.prm.max_hypotheses;
		const int H = exhaustive ? static_cast<int>(nPairs) : p.prm.max_hypotheses;
		out.hypotheses = H;
		int bestCount = -1, bestH = -1;
		auto hypothesis = [&](int h, double (&Xh)[3]) {
			int a, b;
			lm_hypothesis(exhaustive, p.prm.seed, h, m, a, b);
			double ra[6], rb[6], Sh[kLmTerms];
			std::copy(rays.begin() + 6 * a, rays.begin() + 6 * a + 6, ra);
			std::copy(rays.begin() + 6 * b, rays.begin() + 6 * b + 6, rb);
			if (!lm_gate(ra, rb, p.prm.min_parallax))
			{
				return false;
			}
			lm_pair_sums(ra, rb, Sh);
			return lm_solve(Sh, cref, Xh);
		};
		for (int h = 0; h < H; ++h)
		{
			double Xh[3];
			if (!hypothesis(h, Xh))
			{
				continue;
			}
			int count = 0;
			for (int o = 0; o < m; ++o)
			{
				count += lm_score(pose(o), bearing(o), Xh) < p.prm.threshold ? 1 : 0;
			}
			if (count > bestCount)
			{
				bestCount = count;
				bestH = h;
			}
		}
		if (bestCount < 2)
		{
			out.status = 3;
			return;
		}
		// L5
		out.winner = bestH;
		double Xh[3];
		(void)hypothesis(bestH, Xh);
		for (int o = 0; o < m; ++o)
		{
			in[o] = lm_score(pose(o), bearing(o), Xh) < p.prm.threshold;
		}
		treeSums(rays, in, m, S);
		const bool havePoint = lm_solve(S, cref, X);
		out.parallax = lm_parallax(S, static_cast<double>(bestCount));
		if (!havePoint || !(out.parallax >= p.prm.min_parallax))
		{
			out.status = 4;
			return;
		}
	}
	// L5's re-selection (L7: the selection)
	bool haveMax = false;
	for (int o = 0; o < m; ++o)
	{
		const double sc = lm_score(pose(o), bearing(o), X);
		in[o] = sc < p.prm.threshold;
		out.n_inliers += in[o] ? 1 : 0;
		if (lm_finite(sc) && (!haveMax || sc > out.score_max))
		{
			out.score_max = sc;
			haveMax = true;
		}
		scores[base + o] = sc;
		flags[base + o] = in[o] ? 1.0 : 0.0;
	}
	if (p.audit)
	{
		treeSums(rays, in, m, S);
		out.parallax = out.n_inliers > 0 ? lm_parallax(S, static_cast<double>(out.n_inliers)) : 0.0;
		if (!(out.parallax >= p.prm.min_parallax))
		{
			out.status = 4;
			return;
		}
	}
	if (out.n_inliers < p.prm.min_inliers)
	{
		out.status = 5;
		return;
	}
	std::copy(X, X + 3, out.point);
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
	constexpr size_t kHead = 8;
	if (in.size() < kHead || repeats < 1)
	{
		std::fprintf(stderr, "short problem file or no repeats\n");
		return 2;
	}
	Problem p;
	p.audit = in[0] != 0.0;
	const long long N = static_cast<long long>(in[1]), L = static_cast<long long>(in[2]);
	p.prm.threshold = in[3];
	p.prm.min_parallax = in[4];
	p.prm.min_inliers = static_cast<int>(in[5]);
	p.prm.max_hypotheses = static_cast<int>(in[6]);
	p.prm.seed = static_cast<uint64_t>(in[7]);
	if (N < 0 || L < 0 || L > kLmMaxLandmarks || in.size() < kHead + static_cast<size_t>(L) + 1 || !(p.prm.threshold > 0.0 && p.prm.threshold < 1.0) ||
		!(p.prm.min_parallax >= 0.0) || p.prm.min_inliers < 2 || p.prm.max_hypotheses < 1 || p.prm.max_hypotheses > kLmMaxHypotheses)
	{
		std::fprintf(stderr, "counts or parameters out of range\n");
		return 2;
	}
	p.nPoses = static_cast<int>(N);
	p.n = static_cast<int>(L);
	const double* at = in.data() + kHead;
	p.offsets.resize(static_cast<size_t>(L) + 1);
	for (long long l = 0; l <= L; ++l)
	{
		p.offsets[l] = static_cast<int>(at[l]);
		if ((l == 0 && p.offsets[0] != 0) || (l > 0 && (p.offsets[l] < p.offsets[l - 1] || p.offsets[l] - p.offsets[l - 1] > kLmMaxObs)))
		{
			std::fprintf(stderr, "offsets that do not start at 0, decrease or give a landmark more than 512 observations\n");
			return 2;
		}
	}
	at += L + 1;
	const size_t total = static_cast<size_t>(p.offsets[L]);
	if (in.size() != kHead + static_cast<size_t>(L) + 1 + total + kLmPoseDoubles * static_cast<size_t>(N) + 3 * total + (p.audit ? 3 * static_cast<size_t>(L) : 0))
	{
		std::fprintf(stderr, "sizes that are not those of the file\n");
		return 2;
	}
	p.obsPose.resize(total);
	for (size_t o = 0; o < total; ++o)
	{
		p.obsPose[o] = static_cast<int>(at[o]);
	}
	at += total;
	p.poses = at;
	p.obsF = at + kLmPoseDoubles * N;
	p.points = p.obsF + 3 * total;
	std::vector<ebo_landmark_result> res(static_cast<size_t>(L));
	std::vector<double> scores(total), flags(total), ms;
	for (int rep = 0; rep < repeats; ++rep)
	{
		const auto t0 = std::chrono::steady_clock::now();
		for (int l = 0; l < p.n; ++l)
		{
			landmark(p, l, res[static_cast<size_t>(l)], scores.data(), flags.data());
		}
		ms.push_back(std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
	}
	std::vector<double> out;
	for (const ebo_landmark_result& r : res)
	{
		const double row[10] = {r.point[0],
								r.point[1],
								r.point[2],
								r.parallax,
								r.score_max,
								static_cast<double>(r.status),
								static_cast<double>(r.n_obs),
								static_cast<double>(r.n_inliers),
								static_cast<double>(r.winner),
								static_cast<double>(r.hypotheses)};
		out.insert(out.end(), row, row + 10);
	}
	out.insert(out.end(), scores.begin(), scores.end());
	out.insert(out.end(), flags.begin(), flags.end());
	FILE* fo = std::fopen(argv[2], "wb");
	if (!fo || std::fwrite(out.data(), sizeof(double), out.size(), fo) != out.size())
	{
		std::fprintf(stderr, "cannot write %s\n", argv[2]);
		return 2;
	}
	std::fclose(fo);
	std::sort(ms.begin(), ms.end());
	std::printf("{\"landmarks\": %d, \"observations\": %zu, \"ms_median\": %.4f, \"repeats\": %d}\n", p.n, total, ms[ms.size() / 2], repeats);
	return 0;
}
