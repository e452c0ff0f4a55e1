// ebo_align.cpp — the trajectory-alignment entry points of include/ebo.h: many segments of a pair of point arrays
// (ground-truth and estimated camera centres) aligned by a similarity or rigid transform in one launch, one wave per
// segment, with the absolute trajectory error each alignment leaves (what the reference does through
// align_points_sim3, aligner.cpp:27-88, once per new keyframe); the kernel is in ebo_align.inc.
#include "ebo_ctx.h"

#include <chrono>

using namespace ebo;

namespace
{
int align(ebo_ctx* c, int nPoints, const double* data, const double* model, int n, const int* segBegin, const int* segEnd, int fixScale,
		  bool hostArrays, ebo_align_result* results)
{
	int rc = enter(c, "ebo_align_sim3: a negative point count or a segment count outside [0, 65535]",
				   nPoints >= 0 && n >= 0 && n <= kAlMaxSegments);
	if (rc)
	{
		return rc;
	}
	auto bad = [&](const char* what) { return c->fail(EBO_ERR_ARG, std::string("ebo_align_sim3: ") + what); };
	if (n == 0)
	{
		return EBO_OK;
	}
	if (!segBegin || !segEnd || !results)
	{
		return bad("null segment bounds or results");
	}
	for (int g = 0; g < n; ++g)
	{
		if (segBegin[g] < 0 || segEnd[g] < segBegin[g] || segEnd[g] > nPoints)
		{
			return bad("a segment that ends before it begins or lies outside [0, n_points]");
		}
		if (segEnd[g] - segBegin[g] > kAlMaxSegmentPoints)
		{
			return bad("a segment holds at most 2^24 points");
		}
	}
	if (nPoints > 0 && (!data || !model))
	{
		return bad("null data or model");
	}
	const auto wall0 = std::chrono::steady_clock::now();
	const size_t bPts = 3 * static_cast<size_t>(nPoints) * sizeof(double), bSeg = static_cast<size_t>(n) * sizeof(int);
	ScratchCarve cv;
	const size_t oBegin = cv.take(bSeg), oEnd = cv.take(bSeg), oRes = cv.take(n * sizeof(ebo_align_result));
	size_t oData = 0, oModel = 0;
	if (hostArrays)
	{
		oData = cv.take(bPts);
		oModel = cv.take(bPts);
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
	const double* dData = data;
	const double* dModel = model;
	if (hostArrays)
	{
		up(oData, data, bPts);
		up(oModel, model, bPts);
		dData = c->scratch<double>(oData);
		dModel = c->scratch<double>(oModel);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "trajectory alignment uploads");
	}
	mark(c, 0);
	if (launch_align_sim3(nPoints, dData, dModel, n, c->scratch<int>(oBegin), c->scratch<int>(oEnd), fixScale ? 1 : 0,
						  c->scratch<ebo_align_result>(oRes), c->stream))
	{
		return c->hip(hipGetLastError(), "trajectory alignment kernel launch");
	}
	mark(c, 1);
	e = hipMemcpyAsync(results, c->scratch<char>(oRes), n * sizeof(ebo_align_result), hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "trajectory alignment results");
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

int ebo_align_sim3(ebo_ctx* c, int n_points, const double* data, const double* model, int n_segments, const int* seg_begin,
				   const int* seg_end, int fix_scale, ebo_align_result* results)
{
	return align(c, n_points, data, model, n_segments, seg_begin, seg_end, fix_scale, true, results);
}

int ebo_align_sim3_device(ebo_ctx* c, int n_points, const double* d_data, const double* d_model, int n_segments, const int* seg_begin,
						  const int* seg_end, int fix_scale, ebo_align_result* results)
{
	return align(c, n_points, d_data, d_model, n_segments, seg_begin, seg_end, fix_scale, false, results);
}

}  // extern "C"
