// ebo_rpe.cpp — the relative-pose-error entry points of include/ebo.h: many (segment, delta) units of a pair of pose
// arrays (ground truth and estimate) evaluated in one launch, one wave per unit, beside the absolute trajectory error
// of ebo_align.cpp; the kernel is in ebo_rpe.inc.
#include "ebo_ctx.h"

#include <chrono>

using namespace ebo;

namespace
{
int rpe(ebo_ctx* c, int nPoses, const double* gt, const double* est, int n, const int* segBegin, const int* segEnd, const double* segScale,
		int nDeltas, const int* deltas, bool hostArrays, ebo_rpe_result* results)
{
	int rc = enter(c, "ebo_trajectory_rpe: a negative pose count, a segment count outside [0, 65535] or a delta count outside [0, 16]",
				   nPoses >= 0 && n >= 0 && n <= kRpeMaxSegments && nDeltas >= 0 && nDeltas <= kRpeMaxDeltas);
	if (rc)
	{
		return rc;
	}
	auto bad = [&](const char* what) { return c->fail(EBO_ERR_ARG, std::string("ebo_trajectory_rpe: ") + what); };
	if (n > 0 && (!segBegin || !segEnd))
	{
		return bad("null segment bounds");
	}
	if (nDeltas > 0 && !deltas)
	{
		return bad("null deltas");
	}
	for (int g = 0; g < n; ++g)
	{
		if (segBegin[g] < 0 || segEnd[g] < segBegin[g] || segEnd[g] > nPoses)
		{
			return bad("a segment that ends before it begins or lies outside [0, n_poses]");
		}
		if (segEnd[g] - segBegin[g] > kRpeMaxSegmentPoses)
		{
			return bad("a segment holds at most 2^24 poses");
		}
	}
	for (int k = 0; k < nDeltas; ++k)
	{
		if (deltas[k] < 1)
		{
			return bad("a delta below 1");
		}
	}
	if (n == 0 || nDeltas == 0)
	{
		return EBO_OK;
	}
	if (!results)
	{
		return bad("null results");
	}
	if (nPoses > 0 && (!gt || !est))
	{
		return bad("null gt or est");
	}
	const auto wall0 = std::chrono::steady_clock::now();
	const size_t units = static_cast<size_t>(n) * static_cast<size_t>(nDeltas);
	const size_t bPoses = kRpePoseDoubles * static_cast<size_t>(nPoses) * sizeof(double), bSeg = static_cast<size_t>(n) * sizeof(int);
	const size_t bScale = segScale ? static_cast<size_t>(n) * sizeof(double) : 0, bDeltas = static_cast<size_t>(nDeltas) * sizeof(int);
	ScratchCarve cv;
	const size_t oBegin = cv.take(bSeg), oEnd = cv.take(bSeg), oScale = cv.take(bScale), oDeltas = cv.take(bDeltas);
	const size_t oRes = cv.take(units * sizeof(ebo_rpe_result));
	size_t oGt = 0, oEst = 0;
	if (hostArrays)
	{
		oGt = cv.take(bPoses);
		oEst = cv.take(bPoses);
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
	up(oBegin, segBegin, bSeg);
	up(oEnd, segEnd, bSeg);
	up(oScale, segScale, bScale);
	up(oDeltas, deltas, bDeltas);
	const double* dGt = gt;
	const double* dEst = est;
	if (hostArrays)
	{
		up(oGt, gt, bPoses);
		up(oEst, est, bPoses);
		dGt = c->scratch<double>(oGt);
		dEst = c->scratch<double>(oEst);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "relative pose error uploads");
	}
	mark(c, 0);
	if (launch_trajectory_rpe(nPoses, dGt, dEst, n, c->scratch<int>(oBegin), c->scratch<int>(oEnd),
							  segScale ? c->scratch<double>(oScale) : nullptr, nDeltas, c->scratch<int>(oDeltas),
							  c->scratch<ebo_rpe_result>(oRes), c->stream))
	{
		return c->hip(hipGetLastError(), "relative pose error kernel launch");
	}
	mark(c, 1);
	e = hipMemcpyAsync(results, c->scratch<char>(oRes), units * sizeof(ebo_rpe_result), hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "relative pose error results");
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

int ebo_trajectory_rpe(ebo_ctx* c, int n_poses, const double* gt, const double* est, int n_segments, const int* seg_begin,
					   const int* seg_end, const double* seg_scale_or_null, int n_deltas, const int* deltas, ebo_rpe_result* results)
{
	return rpe(c, n_poses, gt, est, n_segments, seg_begin, seg_end, seg_scale_or_null, n_deltas, deltas, true, results);
}

int ebo_trajectory_rpe_device(ebo_ctx* c, int n_poses, const double* d_gt, const double* d_est, int n_segments, const int* seg_begin,
							  const int* seg_end, const double* seg_scale_or_null, int n_deltas, const int* deltas,
							  ebo_rpe_result* results)
{
	return rpe(c, n_poses, d_gt, d_est, n_segments, seg_begin, seg_end, seg_scale_or_null, n_deltas, deltas, false, results);
}

}  // extern "C"
