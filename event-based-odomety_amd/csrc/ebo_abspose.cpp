// ebo_abspose.cpp — the absolute-pose entry points of include/ebo.h: three-point RANSAC over the (bearing vector,
// landmark) pairs of many keyframes (VisualOdometryFrontEnd::localizeCamera, visual_odometry.cpp:212-286) and the
// scores for a given pose; the kernels are in ebo_abspose.inc.  The device solves and scores every hypothesis; the
// serial stopping rule (A5) runs here afterwards.  The shape is ebo_twoview.cpp's, entry for entry.
#include "ebo_ctx.h"

#include <chrono>
#include <cmath>

using namespace ebo;

namespace
{
size_t align256(size_t v)
{
	return (v + 255) & ~static_cast<size_t>(255);
}

// a bump allocator over the context's scratch buffer
struct Carve
{
	size_t at = 0;
	size_t take(size_t bytes)
	{
		const size_t o = at;
		at = align256(at + bytes);
		return o;
	}
};

template <class T>
T* at(ebo_ctx* c, size_t off)
{
	return reinterpret_cast<T*>(static_cast<char*>(c->d_scratch.get()) + off);
}

int check_params(ebo_ctx* c, const ebo_two_view_params* p)
{
	if (!p)
	{
		return c->fail(EBO_ERR_ARG, "ebo_absolute_pose_ransac: null parameters");
	}
	if (p->max_iterations < 1 || p->max_iterations > 4096)
	{
		return c->fail(EBO_ERR_ARG, "ebo_absolute_pose_ransac: max_iterations outside [1, 4096]");
	}
	if (!(p->probability > 0.0 && p->probability < 1.0))
	{
		return c->fail(EBO_ERR_ARG, "ebo_absolute_pose_ransac: probability outside (0, 1)");
	}
	if (!(p->threshold > 0.0))
	{
		return c->fail(EBO_ERR_ARG, "ebo_absolute_pose_ransac: threshold must be positive");
	}
	return EBO_OK;
}

// A5 (rule 6 with w^4): the serial loop's answer from the inlier counts of all hypotheses
void walk(const int* count, int n, int maxIterations, double probability, int& best, int& winner, int& iterations)
{
	best = -1;
	winner = -1;
	double k = static_cast<double>(maxIterations);
	int h = 0;
	for (;; ++h)
	{
		if (count[h] > best)
		{
			best = count[h];
			winner = h;
			const double w = static_cast<double>(best) / static_cast<double>(n);
			const double w2 = w * w;
			const double w4 = w2 * w2;
			const double x = std::min(std::max(1.0 - w4, 1e-15), 1.0 - 1e-15);
			k = std::log(1.0 - probability) / std::log(x);
		}
		if (static_cast<double>(h + 1) >= k || h + 1 == maxIterations)
		{
			break;
		}
	}
	iterations = h + 1;
}

// phase marks of ebo_two_view_timing, which brackets these calls too: nothing is recorded unless the caller asked for timing
void mark(ebo_ctx* c, int i)
{
	if (c->tv_timing)
	{
		(void)hipEventRecord(c->tv_ev[i], c->stream);
	}
}

// hostArrays: f (bearing vectors) and pts (landmarks) are host arrays and are staged in scratch; otherwise device pointers used in place
int ransac(ebo_ctx* c, int n_frames, const int* offsets, const double* f, const double* pts, bool hostArrays,
		   const ebo_two_view_params* prm, ebo_two_view_result* result, int* inlier_idx, int* hyp_counts, double* hyp_models,
		   int* hyp_samples)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	if (c->capturing)
	{
		return c->fail(EBO_ERR_STATE, kNotWhileRecording);
	}
	int rc = check_params(c, prm);
	if (rc)
	{
		return rc;
	}
	if (n_frames < 0 || n_frames > 65535 || (n_frames > 0 && (!offsets || !result)))
	{
		return c->fail(EBO_ERR_ARG, "ebo_absolute_pose_ransac: null offsets or result, or a frame count outside [0, 65535]");
	}
	if (n_frames == 0)
	{
		return EBO_OK;
	}
	int maxN = 0;
	if (offsets[0] != 0)
	{
		return c->fail(EBO_ERR_ARG, "ebo_absolute_pose_ransac: offsets[0] must be 0");
	}
	for (int p = 0; p < n_frames; ++p)
	{
		const long long n = static_cast<long long>(offsets[p + 1]) - offsets[p];
		if (n < 0 || n > 65535)
		{
			return c->fail(EBO_ERR_ARG, "ebo_absolute_pose_ransac: offsets must not decrease, and a frame holds at most 65535 points");
		}
		maxN = std::max(maxN, static_cast<int>(n));
	}
	const int total = offsets[n_frames];
	if (total > 0 && (!f || !pts || !inlier_idx))
	{
		return c->fail(EBO_ERR_ARG, "ebo_absolute_pose_ransac: null bearing vectors, landmarks or inlier list");
	}
	const int H = prm->max_iterations;
	const size_t nh = static_cast<size_t>(n_frames) * H;
	(void)hipSetDevice(c->prm.device);
	const auto wall0 = std::chrono::steady_clock::now();

	Carve cv;
	const size_t bF = static_cast<size_t>(total) * 3 * sizeof(double);
	const size_t oF = hostArrays ? cv.take(bF) : 0, oP = hostArrays ? cv.take(bF) : 0;
	const size_t oOff = cv.take((static_cast<size_t>(n_frames) + 1) * sizeof(int));
	const size_t oModels = cv.take(nh * 12 * sizeof(double));
	const size_t oValid = cv.take(nh * sizeof(int));
	const size_t oCounts = cv.take(nh * sizeof(int));
	const size_t oSamples = hyp_samples ? cv.take(nh * 4 * sizeof(int)) : 0;
	const size_t oWinner = cv.take(static_cast<size_t>(n_frames) * sizeof(int));
	const size_t oFlags = cv.take(static_cast<size_t>(total) + 1);
	const size_t oWinModels = cv.take(static_cast<size_t>(n_frames) * 12 * sizeof(double));
	rc = c->grow(c->d_scratch, cv.at, "hipMalloc scratch");
	if (rc)
	{
		return rc;
	}
	const double* d_f = f;
	const double* d_points = pts;
	hipError_t e = hipSuccess;
	if (hostArrays && total > 0)
	{
		e = hipMemcpyAsync(at<double>(c, oF), f, bF, hipMemcpyHostToDevice, c->stream);
		if (e == hipSuccess)
		{
			e = hipMemcpyAsync(at<double>(c, oP), pts, bF, hipMemcpyHostToDevice, c->stream);
		}
		d_f = at<double>(c, oF);
		d_points = at<double>(c, oP);
	}
	if (e == hipSuccess)
	{
		e = hipMemcpyAsync(at<int>(c, oOff), offsets, (static_cast<size_t>(n_frames) + 1) * sizeof(int), hipMemcpyHostToDevice, c->stream);
	}
	if (e == hipSuccess)
	{
		e = hipMemsetAsync(at<int>(c, oCounts), 0, nh * sizeof(int), c->stream);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "absolute-pose uploads");
	}
	int* d_samples = hyp_samples ? at<int>(c, oSamples) : nullptr;
	if (hyp_samples)
	{
		// hypotheses of a frame with fewer than 4 points draw no sample: their entries read 0
		e = hipMemsetAsync(d_samples, 0, nh * 4 * sizeof(int), c->stream);
		if (e != hipSuccess)
		{
			return c->hip(e, "absolute-pose sample table");
		}
	}
	mark(c, 0);
	if (launch_ap_hypotheses(n_frames, H, at<int>(c, oOff), d_f, d_points, prm->seed, at<double>(c, oModels), at<int>(c, oValid),
							 d_samples, c->stream))
	{
		return c->hip(hipGetLastError(), "hypothesis kernel launch");
	}
	mark(c, 1);
	if (launch_ap_count(n_frames, H, maxN, at<int>(c, oOff), d_f, d_points, at<double>(c, oModels), at<int>(c, oValid), prm->threshold,
						at<int>(c, oCounts), c->stream))
	{
		return c->hip(hipGetLastError(), "counting kernel launch");
	}
	mark(c, 2);
	std::vector<int> counts(nh);
	e = hipMemcpyAsync(counts.data(), at<int>(c, oCounts), nh * sizeof(int), hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "D2H inlier counts");
	}
	const auto walk0 = std::chrono::steady_clock::now();
	std::vector<int> winner(n_frames, -1);
	for (int p = 0; p < n_frames; ++p)
	{
		ebo_two_view_result& r = result[p];
		r = ebo_two_view_result{};
		r.winner = -1;
		r.inlier_offset = offsets[p];
		const int n = offsets[p + 1] - offsets[p];
		if (n < 4)
		{
			continue;
		}
		int best = 0;
		walk(counts.data() + static_cast<size_t>(p) * H, n, H, prm->probability, best, r.winner, r.iterations);
		r.found = best >= 4 ? 1 : 0;
		winner[p] = r.winner;
	}
	const auto walk1 = std::chrono::steady_clock::now();
	mark(c, 3);
	e = hipMemcpyAsync(at<int>(c, oWinner), winner.data(), static_cast<size_t>(n_frames) * sizeof(int), hipMemcpyHostToDevice, c->stream);
	if (e != hipSuccess)
	{
		return c->hip(e, "H2D winners");
	}
	if (launch_ap_winner_flags(n_frames, H, maxN, at<int>(c, oOff), d_f, d_points, at<double>(c, oModels), at<int>(c, oValid),
							   at<int>(c, oWinner), prm->threshold, at<unsigned char>(c, oFlags), at<double>(c, oWinModels), c->stream))
	{
		return c->hip(hipGetLastError(), "inlier list launch");
	}
	mark(c, 4);
	std::vector<unsigned char> flags(static_cast<size_t>(total) + 1);
	std::vector<double> winModels(static_cast<size_t>(n_frames) * 12);
	e = hipSuccess;
	if (total > 0)
	{
		e = hipMemcpyAsync(flags.data(), at<unsigned char>(c, oFlags), static_cast<size_t>(total), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess)
	{
		e = hipMemcpyAsync(winModels.data(), at<double>(c, oWinModels), winModels.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess && hyp_counts)
	{
		std::copy(counts.begin(), counts.end(), hyp_counts);
	}
	if (e == hipSuccess && hyp_models)
	{
		e = hipMemcpyAsync(hyp_models, at<double>(c, oModels), nh * 12 * sizeof(double), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess && hyp_samples)
	{
		e = hipMemcpyAsync(hyp_samples, d_samples, nh * 4 * sizeof(int), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "D2H absolute-pose results");
	}
	if (c->tv_timing)
	{
		(void)hipEventElapsedTime(&c->tv_ms[0], c->tv_ev[0], c->tv_ev[1]);
		(void)hipEventElapsedTime(&c->tv_ms[1], c->tv_ev[1], c->tv_ev[2]);
		c->tv_ms[2] = std::chrono::duration<float, std::milli>(walk1 - walk0).count();
		(void)hipEventElapsedTime(&c->tv_ms[3], c->tv_ev[3], c->tv_ev[4]);
		c->tv_ms[4] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - wall0).count();
	}
	for (int p = 0; p < n_frames; ++p)
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

int enter(ebo_ctx* c, const char* what, bool argsOk)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	if (c->capturing)
	{
		return c->fail(EBO_ERR_STATE, kNotWhileRecording);
	}
	if (!argsOk)
	{
		return c->fail(EBO_ERR_ARG, what);
	}
	(void)hipSetDevice(c->prm.device);
	return EBO_OK;
}
}  // namespace

extern "C" {

int ebo_absolute_pose_ransac(ebo_ctx* c, int n_frames, const int* offsets, const double* f, const double* pts,
							 const ebo_two_view_params* params, ebo_two_view_result* result, int* inlier_idx, int* hyp_counts,
							 double* hyp_models, int* hyp_samples)
{
	return ransac(c, n_frames, offsets, f, pts, true, params, result, inlier_idx, hyp_counts, hyp_models, hyp_samples);
}

int ebo_absolute_pose_ransac_device(ebo_ctx* c, int n_frames, const int* offsets, const double* d_f, const double* d_points,
									const ebo_two_view_params* params, ebo_two_view_result* result, int* inlier_idx,
									int* hyp_counts, double* hyp_models, int* hyp_samples)
{
	return ransac(c, n_frames, offsets, d_f, d_points, false, params, result, inlier_idx, hyp_counts, hyp_models, hyp_samples);
}

int ebo_absolute_pose_scores_device(ebo_ctx* c, const double* pose, int n, const double* d_f, const double* d_points, double threshold,
									double* d_scores, uint8_t* d_flags)
{
	int rc = enter(c, "ebo_absolute_pose_scores: null pose, bearing vectors or landmarks, or a negative count",
				   pose && n >= 0 && (n == 0 || (d_f && d_points)));
	if (rc)
	{
		return rc;
	}
	if (launch_ap_scores(pose, n, d_f, d_points, threshold, d_scores, d_flags, c->stream))
	{
		return c->hip(hipGetLastError(), "scores launch");
	}
	return EBO_OK;
}

int ebo_absolute_pose_scores(ebo_ctx* c, const double* pose, int n, const double* f, const double* pts, double threshold,
							 double* scores, uint8_t* flags)
{
	int rc = enter(c, "ebo_absolute_pose_scores: null pose, bearing vectors or landmarks, or a negative count",
				   pose && n >= 0 && (n == 0 || (f && pts)));
	if (rc || n == 0)
	{
		return rc;
	}
	Carve cv;
	const size_t bF = static_cast<size_t>(n) * 3 * sizeof(double);
	const size_t oF = cv.take(bF), oP = cv.take(bF), oS = cv.take(static_cast<size_t>(n) * sizeof(double)), oFl = cv.take(n);
	rc = c->grow(c->d_scratch, cv.at, "hipMalloc scratch");
	if (rc)
	{
		return rc;
	}
	hipError_t e = hipMemcpyAsync(at<double>(c, oF), f, bF, hipMemcpyHostToDevice, c->stream);
	if (e == hipSuccess)
	{
		e = hipMemcpyAsync(at<double>(c, oP), pts, bF, hipMemcpyHostToDevice, c->stream);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "H2D bearing vectors and landmarks");
	}
	if (launch_ap_scores(pose, n, at<double>(c, oF), at<double>(c, oP), threshold, at<double>(c, oS), at<unsigned char>(c, oFl),
						 c->stream))
	{
		return c->hip(hipGetLastError(), "scores launch");
	}
	if (scores)
	{
		e = hipMemcpyAsync(scores, at<double>(c, oS), static_cast<size_t>(n) * sizeof(double), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess && flags)
	{
		e = hipMemcpyAsync(flags, at<unsigned char>(c, oFl), static_cast<size_t>(n), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	return c->hip(e, "D2H scores");
}

}  // extern "C"
