// ebo_relpose.cpp — the relative-pose refinement entry points of include/ebo.h: the models of many keyframe pairs
// refined over their RANSAC inliers by a five-variable Levenberg-Marquardt in one launch, one wave per pair (what the
// reference does through relative_pose::optimize_nonlinear, visual_odometry.cpp:316-330); the kernel is in
// ebo_relpose.inc.  The arrays are laid out as ebo_relative_pose_ransac leaves them, so the call chains straight off it.
#include "ebo_ctx.h"

#include <chrono>

using namespace ebo;

namespace
{
int refine(ebo_ctx* c, int n, const int* offsets, const double* f1, const double* f2, double* models, const int* nInliers, const int* idx,
		   bool hostArrays, const ebo_solver_opts* opts, ebo_summary* summaries, double* trace)
{
	int rc = enter(c, "ebo_relative_pose_refine: a pair count outside [0, 65535]", n >= 0 && n <= kRpMaxPairs);
	if (rc)
	{
		return rc;
	}
	auto bad = [&](const char* what) { return c->fail(EBO_ERR_ARG, std::string("ebo_relative_pose_refine: ") + what); };
	if (!opts || opts->max_num_iterations < 0)
	{
		return bad("null options or a negative iteration count");
	}
	if (n == 0)
	{
		return EBO_OK;
	}
	if (!offsets || !models || !nInliers || !summaries)
	{
		return bad("null offsets, models, inlier counts or summaries");
	}
	if (offsets[0] != 0)
	{
		return bad("offsets[0] must be 0");
	}
	for (int p = 0; p < n; ++p)
	{
		const long long size = static_cast<long long>(offsets[p + 1]) - offsets[p];
		if (size < 0 || size > kRpMaxPoints)
		{
			return bad("offsets must not decrease, and a pair holds at most 65535 correspondences");
		}
		if (nInliers[p] < 0 || nInliers[p] > size)
		{
			return bad("an inlier count that is negative or beyond its pair's size");
		}
	}
	const size_t total = static_cast<size_t>(offsets[n]);
	if (total > 0 && (!f1 || !f2 || !idx))
	{
		return bad("null bearing vectors or inlier list");
	}
	if (hostArrays)
	{
		for (int p = 0; p < n; ++p)
		{
			const int size = offsets[p + 1] - offsets[p];
			for (int i = 0; i < nInliers[p]; ++i)
			{
				const int k = idx[offsets[p] + i];
				if (k < 0 || k >= size)
				{
					return bad("an inlier index outside its pair");
				}
			}
		}
	}
	const auto wall0 = std::chrono::steady_clock::now();
	const size_t traceDoubles = static_cast<size_t>(n) * (static_cast<size_t>(opts->max_num_iterations) + 1) * 4;
	const size_t bF = 3 * total * sizeof(double), bModels = 12 * static_cast<size_t>(n) * sizeof(double);
	ScratchCarve cv;
	const size_t oOff = cv.take((static_cast<size_t>(n) + 1) * sizeof(int)), oCount = cv.take(n * sizeof(int));
	const size_t oSum = cv.take(n * sizeof(ebo_summary));
	const size_t oWork = cv.take(rp_work_doubles(total) * sizeof(double));
	size_t oF1 = 0, oF2 = 0, oIdx = 0, oModels = 0, oTrace = 0;
	if (hostArrays)
	{
		oF1 = cv.take(bF);
		oF2 = cv.take(bF);
		oIdx = cv.take(total * sizeof(int));
		oModels = cv.take(bModels);
		oTrace = trace ? cv.take(traceDoubles * sizeof(double)) : 0;
	}
	rc = c->grow(c->d_scratch, cv.at, "hipMalloc scratch");
	if (rc)
	{
		return rc;
	}
	hipError_t e = hipSuccess;
	auto up = [&](size_t off, const void* src, size_t bytes) {
		if (e == hipSuccess && bytes)
		{
			e = hipMemcpyAsync(c->scratch<char>(off), src, bytes, hipMemcpyHostToDevice, c->stream);
		}
	};
	up(oOff, offsets, (static_cast<size_t>(n) + 1) * sizeof(int));
	up(oCount, nInliers, n * sizeof(int));
	const double* dF1 = f1;
	const double* dF2 = f2;
	const int* dIdx = idx;
	double* dModels = models;
	double* dTrace = trace;
	if (hostArrays)
	{
		up(oF1, f1, bF);
		up(oF2, f2, bF);
		up(oIdx, idx, total * sizeof(int));
		up(oModels, models, bModels);
		dF1 = c->scratch<double>(oF1);
		dF2 = c->scratch<double>(oF2);
		dIdx = c->scratch<int>(oIdx);
		dModels = c->scratch<double>(oModels);
		dTrace = trace ? c->scratch<double>(oTrace) : nullptr;
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "relative-pose refinement uploads");
	}
	mark(c, 0);
	if (launch_relpose_refine(n, c->scratch<int>(oOff), c->scratch<int>(oCount), dF1, dF2, dIdx, dModels, c->scratch<double>(oWork), *opts,
							  c->scratch<ebo_summary>(oSum), dTrace, c->stream))
	{
		return c->hip(hipGetLastError(), "relative-pose refinement kernel launch");
	}
	mark(c, 1);
	auto down = [&](void* dst, size_t off, size_t bytes) {
		if (e == hipSuccess && bytes)
		{
			e = hipMemcpyAsync(dst, c->scratch<char>(off), bytes, hipMemcpyDeviceToHost, c->stream);
		}
	};
	down(summaries, oSum, n * sizeof(ebo_summary));
	if (hostArrays)
	{
		down(models, oModels, bModels);
		if (trace)
		{
			down(trace, oTrace, traceDoubles * sizeof(double));
		}
	}
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "relative-pose refinement results");
	}
	if (c->tv_timing)
	{
		// slot 0: the kernel; slot 4: the whole call (wall clock); the others do not apply
		(void)hipEventElapsedTime(&c->tv_ms[0], c->tv_ev[0], c->tv_ev[1]);
		c->tv_ms[1] = c->tv_ms[2] = c->tv_ms[3] = 0.0f;
		c->tv_ms[4] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - wall0).count();
	}
	return EBO_OK;
}
}  // namespace

extern "C" {

int ebo_relative_pose_refine(ebo_ctx* c, int n_pairs, const int* offsets, const double* f1, const double* f2, double* models,
							 const int* n_inliers, const int* inlier_idx, const ebo_solver_opts* opts, ebo_summary* summaries,
							 double* trace)
{
	return refine(c, n_pairs, offsets, f1, f2, models, n_inliers, inlier_idx, true, opts, summaries, trace);
}

int ebo_relative_pose_refine_device(ebo_ctx* c, int n_pairs, const int* offsets, const double* d_f1, const double* d_f2, double* d_models,
									const int* n_inliers, const int* d_inlier_idx, const ebo_solver_opts* opts, ebo_summary* summaries,
									double* d_trace)
{
	return refine(c, n_pairs, offsets, d_f1, d_f2, d_models, n_inliers, d_inlier_idx, false, opts, summaries, d_trace);
}

}  // extern "C"
