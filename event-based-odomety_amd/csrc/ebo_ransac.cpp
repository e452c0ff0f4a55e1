// ebo_ransac.cpp — the host side both RANSAC paths share: the driver behind ebo_relative_pose_ransac* (eight points,
// VisualOdometryFrontEnd::findInliersRansac) and ebo_absolute_pose_ransac* (three points and a fourth,
// VisualOdometryFrontEnd::localizeCamera), and the one behind their *_scores entries.  The device solves and scores
// every hypothesis (the paths' own hypothesis kernels, then ebo_ransac.inc); the serial stopping rule (ransac_walk.h)
// runs here afterwards.  A path is a RansacProblem (ebo_ctx.h); ebo_twoview.cpp and ebo_abspose.cpp hold the two.
#include "ebo_ctx.h"
#include "ransac_walk.h"

#include <chrono>

using namespace ebo;

namespace ebo_host
{
int ransac(ebo_ctx* c, const RansacProblem& P, int n_groups, const int* offsets, const double* a, const double* b, bool hostArrays,
		   const ebo_two_view_params* prm, ebo_two_view_result* result, int* inlier_idx, int* hyp_counts, double* hyp_models,
		   int* hyp_samples)
{
	int rc = enter(c, "", true);
	if (rc)
	{
		return rc;
	}
	auto bad = [&](const std::string& what) { return c->fail(EBO_ERR_ARG, std::string(P.entry) + ": " + what); };
	if (!prm)
	{
		return bad("null parameters");
	}
	if (prm->max_iterations < 1 || prm->max_iterations > 4096)
	{
		return bad("max_iterations outside [1, 4096]");
	}
	if (!(prm->probability > 0.0 && prm->probability < 1.0))
	{
		return bad("probability outside (0, 1)");
	}
	if (!(prm->threshold > 0.0))
	{
		return bad("threshold must be positive");
	}
	if (n_groups < 0 || n_groups > 65535 || (n_groups > 0 && (!offsets || !result)))
	{
		return bad(std::string("null offsets or result, or a ") + P.group + " count outside [0, 65535]");
	}
	if (n_groups == 0)
	{
		return EBO_OK;
	}
	int maxN = 0;
	if (offsets[0] != 0)
	{
		return bad("offsets[0] must be 0");
	}
	for (int p = 0; p < n_groups; ++p)
	{
		const long long n = static_cast<long long>(offsets[p + 1]) - offsets[p];
		if (n < 0 || n > 65535)
		{
			return bad(std::string("offsets must not decrease, and a ") + P.group + " holds at most 65535 " + P.points);
		}
		maxN = std::max(maxN, static_cast<int>(n));
	}
	const int total = offsets[n_groups];
	if (total > 0 && (!a || !b || !inlier_idx))
	{
		return bad(std::string("null ") + P.arrays + " or inlier list");
	}
	const int H = prm->max_iterations;
	const size_t nh = static_cast<size_t>(n_groups) * H;
	const auto wall0 = std::chrono::steady_clock::now();

	ScratchCarve cv;
	const size_t bA = static_cast<size_t>(total) * 3 * sizeof(double);
	const size_t oA = hostArrays ? cv.take(bA) : 0, oB = hostArrays ? cv.take(bA) : 0;
	const size_t oOff = cv.take((static_cast<size_t>(n_groups) + 1) * sizeof(int));
	const size_t oModels = cv.take(nh * 12 * sizeof(double));
	const size_t oValid = cv.take(nh * sizeof(int));
	const size_t oCounts = cv.take(nh * sizeof(int));
	const size_t oSamples = hyp_samples ? cv.take(nh * P.sample * sizeof(int)) : 0;
	const size_t oWinner = cv.take(static_cast<size_t>(n_groups) * sizeof(int));
	const size_t oFlags = cv.take(static_cast<size_t>(total) + 1);
	const size_t oWinModels = cv.take(static_cast<size_t>(n_groups) * 12 * sizeof(double));
	rc = c->grow(c->d_scratch, cv.at, "hipMalloc scratch");
	if (rc)
	{
		return rc;
	}
	const double* d_a = a;
	const double* d_b = b;
	hipError_t e = hipSuccess;
	if (hostArrays && total > 0)
	{
		e = hipMemcpyAsync(c->scratch<double>(oA), a, bA, hipMemcpyHostToDevice, c->stream);
		if (e == hipSuccess)
		{
			e = hipMemcpyAsync(c->scratch<double>(oB), b, bA, hipMemcpyHostToDevice, c->stream);
		}
		d_a = c->scratch<double>(oA);
		d_b = c->scratch<double>(oB);
	}
	if (e == hipSuccess)
	{
		e = hipMemcpyAsync(c->scratch<int>(oOff), offsets, (static_cast<size_t>(n_groups) + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream);
	}
	if (e == hipSuccess)
	{
		e = hipMemsetAsync(c->scratch<int>(oCounts), 0, nh * sizeof(int), c->stream);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, (std::string(P.label) + " uploads").c_str());
	}
	int* d_samples = hyp_samples ? c->scratch<int>(oSamples) : nullptr;
	if (hyp_samples)
	{
		// hypotheses of a group with fewer than P.sample points draw no sample: their entries read 0
		e = hipMemsetAsync(d_samples, 0, nh * P.sample * sizeof(int), c->stream);
		if (e != hipSuccess)
		{
			return c->hip(e, (std::string(P.label) + " sample table").c_str());
		}
	}
	mark(c, 0);
	if (P.hypotheses(n_groups, H, c->scratch<int>(oOff), d_a, d_b, prm->seed, c->scratch<double>(oModels), c->scratch<int>(oValid),
					 d_samples, c->stream))
	{
		return c->hip(hipGetLastError(), "hypothesis kernel launch");
	}
	mark(c, 1);
	if (launch_ransac_count(P.kind, n_groups, H, maxN, c->scratch<int>(oOff), d_a, d_b, c->scratch<double>(oModels),
							c->scratch<int>(oValid), prm->threshold, c->scratch<int>(oCounts), c->stream))
	{
		return c->hip(hipGetLastError(), "counting kernel launch");
	}
	mark(c, 2);
	std::vector<int> counts(nh);
	e = hipMemcpyAsync(counts.data(), c->scratch<int>(oCounts), nh * sizeof(int), hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "D2H inlier counts");
	}
	const auto walk0 = std::chrono::steady_clock::now();
	std::vector<int> winner(n_groups, -1);
	for (int p = 0; p < n_groups; ++p)
	{
		ebo_two_view_result& r = result[p];
		r = ebo_two_view_result{};
		r.winner = -1;
		r.inlier_offset = offsets[p];
		const int n = offsets[p + 1] - offsets[p];
		if (n < P.sample)
		{
			continue;
		}
		int best = 0;
		ransac_walk(counts.data() + static_cast<size_t>(p) * H, n, H, prm->probability, P.sample, best, r.winner, r.iterations);
		r.found = best >= P.sample ? 1 : 0;
		winner[p] = r.winner;
	}
	const auto walk1 = std::chrono::steady_clock::now();
	mark(c, 3);
	e = hipMemcpyAsync(c->scratch<int>(oWinner), winner.data(), static_cast<size_t>(n_groups) * sizeof(int), hipMemcpyHostToDevice, c->stream);
	if (e != hipSuccess)
	{
		return c->hip(e, "H2D winners");
	}
	if (launch_ransac_winner_flags(P.kind, n_groups, H, maxN, c->scratch<int>(oOff), d_a, d_b, c->scratch<double>(oModels),
								   c->scratch<int>(oValid), c->scratch<int>(oWinner), prm->threshold,
								   c->scratch<unsigned char>(oFlags), c->scratch<double>(oWinModels), c->stream))
	{
		return c->hip(hipGetLastError(), "inlier list launch");
	}
	mark(c, 4);
	std::vector<unsigned char> flags(static_cast<size_t>(total) + 1);
	std::vector<double> winModels(static_cast<size_t>(n_groups) * 12);
	e = hipSuccess;
	if (total > 0)
	{
		e = hipMemcpyAsync(flags.data(), c->scratch<unsigned char>(oFlags), static_cast<size_t>(total), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess)
	{
		e = hipMemcpyAsync(winModels.data(), c->scratch<double>(oWinModels), winModels.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess && hyp_counts)
	{
		std::copy(counts.begin(), counts.end(), hyp_counts);
	}
	if (e == hipSuccess && hyp_models)
	{
		e = hipMemcpyAsync(hyp_models, c->scratch<double>(oModels), nh * 12 * sizeof(double), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess && hyp_samples)
	{
		e = hipMemcpyAsync(hyp_samples, d_samples, nh * P.sample * sizeof(int), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, (std::string("D2H ") + P.label + " results").c_str());
	}
	if (c->tv_timing)
	{
		(void)hipEventElapsedTime(&c->tv_ms[0], c->tv_ev[0], c->tv_ev[1]);
		(void)hipEventElapsedTime(&c->tv_ms[1], c->tv_ev[1], c->tv_ev[2]);
		c->tv_ms[2] = std::chrono::duration<float, std::milli>(walk1 - walk0).count();
		(void)hipEventElapsedTime(&c->tv_ms[3], c->tv_ev[3], c->tv_ev[4]);
		c->tv_ms[4] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - wall0).count();
	}
	for (int p = 0; p < n_groups; ++p)
	{
		ebo_two_view_result& r = result[p];
		const int n = offsets[p + 1] - offsets[p];
		std::copy(winModels.begin() + 12 * static_cast<size_t>(p), winModels.begin() + 12 * (static_cast<size_t>(p) + 1), &r.model[0][0]);
		int m = 0;
		for (int i = 0; i < n; ++i)
		{
			if (flags[static_cast<size_t>(offsets[p]) + i])
			{
				inlier_idx[offsets[p] + m++] = i;
			}
		}
		r.n_inliers = m;
	}
	return EBO_OK;
}

int ransac_scores(ebo_ctx* c, const RansacProblem& P, const double* model, int n, const double* a, const double* b, bool hostArrays,
				  double threshold, double* scores, uint8_t* flags)
{
	int rc = enter(c, P.scoresArgs, model && n >= 0 && (n == 0 || (a && b)));
	if (rc || (hostArrays && n == 0))
	{
		return rc;
	}
	if (!hostArrays)
	{
		if (launch_ransac_scores(P.kind, model, n, a, b, threshold, scores, flags, c->stream))
		{
			return c->hip(hipGetLastError(), "scores launch");
		}
		return EBO_OK;
	}
	ScratchCarve cv;
	const size_t bA = static_cast<size_t>(n) * 3 * sizeof(double);
	const size_t oA = cv.take(bA), oB = cv.take(bA), oS = cv.take(static_cast<size_t>(n) * sizeof(double)), oFl = cv.take(n);
	rc = c->grow(c->d_scratch, cv.at, "hipMalloc scratch");
	if (rc)
	{
		return rc;
	}
	hipError_t e = hipMemcpyAsync(c->scratch<double>(oA), a, bA, hipMemcpyHostToDevice, c->stream);
	if (e == hipSuccess)
	{
		e = hipMemcpyAsync(c->scratch<double>(oB), b, bA, hipMemcpyHostToDevice, c->stream);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, P.scoresUpload);
	}
	if (launch_ransac_scores(P.kind, model, n, c->scratch<double>(oA), c->scratch<double>(oB), threshold, c->scratch<double>(oS),
							 c->scratch<unsigned char>(oFl), c->stream))
	{
		return c->hip(hipGetLastError(), "scores launch");
	}
	if (scores)
	{
		e = hipMemcpyAsync(scores, c->scratch<double>(oS), static_cast<size_t>(n) * sizeof(double), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess && flags)
	{
		e = hipMemcpyAsync(flags, c->scratch<unsigned char>(oFl), static_cast<size_t>(n), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	return c->hip(e, "D2H scores");
}
}  // namespace ebo_host
