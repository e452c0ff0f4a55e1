// ebo_bundle.cpp — the bundle-adjustment entry points of include/ebo.h: many windowed problems (camera poses,
// landmarks, observations) refined by a Schur-complement Levenberg-Marquardt in one launch, one workgroup per problem
// (VisualOdometryFrontEnd::optimize, visual_odometry.cpp:416-497; with fix_points the refinement after localizeCamera's
// RANSAC, :262); the kernel is in ebo_bundle.inc.  The host form checks the indices and sorts every problem's
// observations by (point, frame), which is the order the rules' sums are taken in.
#include "ebo_ctx.h"

#include <algorithm>
#include <chrono>
#include <numeric>

using namespace ebo;

namespace
{
int check_offsets(ebo_ctx* c, const int* off, int n, int cap, const char* what)
{
	if (!off || off[0] != 0)
	{
		return c->fail(EBO_ERR_ARG, std::string("ebo_bundle_adjust: ") + what + " offsets are null or do not start at 0");
	}
	for (int p = 0; p < n; ++p)
	{
		const long long d = static_cast<long long>(off[p + 1]) - off[p];
		if (d < 0 || d > cap)
		{
			return c->fail(EBO_ERR_ARG, std::string("ebo_bundle_adjust: ") + what + " offsets decrease, or a problem is over its limit (24 frames, 4096 points, 65535 observations)");
		}
	}
	return EBO_OK;
}

int adjust(ebo_ctx* c, int n, const int* fo, const int* po, const int* oo, double* poses, const uint8_t* fixed, double* points,
		   const int* of, const int* op, const double* uv, bool hostArrays, const ebo_camera* cam, double huber, int fixPoints,
		   const ebo_solver_opts* opts, ebo_summary* summaries, double* trace)
{
	int rc = enter(c, "ebo_bundle_adjust: a problem count outside [0, 65535]", n >= 0 && n <= kBaMaxProblems);
	if (rc)
	{
		return rc;
	}
	if (!cam || !opts || !(huber > 0.0) || opts->max_num_iterations < 0)
	{
		return c->fail(EBO_ERR_ARG, "ebo_bundle_adjust: null camera or options, a Huber width that is not positive, or a negative iteration count");
	}
	if (n == 0)
	{
		return EBO_OK;
	}
	if (!summaries)
	{
		return c->fail(EBO_ERR_ARG, "ebo_bundle_adjust: null summaries");
	}
	rc = check_offsets(c, fo, n, kBaMaxFrames, "frame");
	rc = rc ? rc : check_offsets(c, po, n, kBaMaxPoints, "point");
	rc = rc ? rc : check_offsets(c, oo, n, kBaMaxObs, "observation");
	if (rc)
	{
		return rc;
	}
	const size_t tF = fo[n], tP = po[n], tN = oo[n];
	if ((tF && (!poses || !fixed)) || (tP && !points) || (tN && (!of || !op || !uv)))
	{
		return c->fail(EBO_ERR_ARG, "ebo_bundle_adjust: a needed array is null");
	}
	std::vector<long long> tableOff(static_cast<size_t>(n) + 1, 0);
	int maxF = 0;
	for (int p = 0; p < n; ++p)
	{
		const int F = fo[p + 1] - fo[p], P = po[p + 1] - po[p];
		tableOff[p + 1] = tableOff[p] + static_cast<long long>(F) * P;
		maxF = std::max(maxF, F);
	}
	// the host form: indices in range, observations in (point, frame) order, no pair twice
	std::vector<int> sf, sp;
	std::vector<double> suv;
	if (hostArrays && tN)
	{
		sf.resize(tN);
		sp.resize(tN);
		suv.resize(2 * tN);
		std::vector<int> order;
		for (int p = 0; p < n; ++p)
		{
			const int F = fo[p + 1] - fo[p], P = po[p + 1] - po[p], N = oo[p + 1] - oo[p], base = oo[p];
			for (int i = 0; i < N; ++i)
			{
				if (of[base + i] < 0 || of[base + i] >= F || op[base + i] < 0 || op[base + i] >= P)
				{
					return c->fail(EBO_ERR_ARG, "ebo_bundle_adjust: an observation's frame or point index is outside its problem");
				}
			}
			order.resize(N);
			std::iota(order.begin(), order.end(), 0);
			auto key = [&](int i) { return op[base + i] * F + of[base + i]; };
			std::sort(order.begin(), order.end(), [&](int a, int b) { return key(a) < key(b); });
			for (int i = 0; i < N; ++i)
			{
				if (i > 0 && key(order[i]) == key(order[i - 1]))
				{
					return c->fail(EBO_ERR_ARG, "ebo_bundle_adjust: a (frame, point) pair is observed twice");
				}
				sf[base + i] = of[base + order[i]];
				sp[base + i] = op[base + order[i]];
				suv[2 * (static_cast<size_t>(base) + i)] = uv[2 * (static_cast<size_t>(base) + order[i])];
				suv[2 * (static_cast<size_t>(base) + i) + 1] = uv[2 * (static_cast<size_t>(base) + order[i]) + 1];
			}
		}
	}
	const auto wall0 = std::chrono::steady_clock::now();
	const size_t traceDoubles = static_cast<size_t>(n) * (static_cast<size_t>(opts->max_num_iterations) + 1) * 4;
	ScratchCarve cv;
	const size_t oFo = cv.take((n + 1) * sizeof(int)), oPo = cv.take((n + 1) * sizeof(int)), oOo = cv.take((n + 1) * sizeof(int));
	const size_t oTo = cv.take((n + 1) * sizeof(long long));
	const size_t oSum = cv.take(n * sizeof(ebo_summary));
	const size_t oWork = cv.take(ba_work_doubles(tF, tP, tN) * sizeof(double));
	const size_t oIwork = cv.take(ba_work_ints(tF, tP, static_cast<size_t>(tableOff[n]), n) * sizeof(int));
	size_t oPoses = 0, oFixed = 0, oPoints = 0, oOf = 0, oOp = 0, oUv = 0, oTrace = 0;
	if (hostArrays)
	{
		oPoses = cv.take(12 * tF * sizeof(double));
		oFixed = cv.take(tF);
		oPoints = cv.take(3 * tP * sizeof(double));
		oOf = cv.take(tN * sizeof(int));
		oOp = cv.take(tN * sizeof(int));
		oUv = cv.take(2 * tN * sizeof(double));
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
	up(oFo, fo, (n + 1) * sizeof(int));
	up(oPo, po, (n + 1) * sizeof(int));
	up(oOo, oo, (n + 1) * sizeof(int));
	up(oTo, tableOff.data(), (n + 1) * sizeof(long long));
	BaTables t{};
	t.frameOff = c->scratch<int>(oFo);
	t.pointOff = c->scratch<int>(oPo);
	t.obsOff = c->scratch<int>(oOo);
	t.tableOff = c->scratch<long long>(oTo);
	t.work = c->scratch<double>(oWork);
	t.iwork = c->scratch<int>(oIwork);
	t.totalF = tF;
	t.totalP = tP;
	t.totalN = tN;
	t.totalTable = static_cast<size_t>(tableOff[n]);
	double* dTrace = trace;
	if (hostArrays)
	{
		up(oPoses, poses, 12 * tF * sizeof(double));
		up(oFixed, fixed, tF);
		up(oPoints, points, 3 * tP * sizeof(double));
		up(oOf, sf.data(), tN * sizeof(int));
		up(oOp, sp.data(), tN * sizeof(int));
		up(oUv, suv.data(), 2 * tN * sizeof(double));
		t.poses = c->scratch<double>(oPoses);
		t.fixed = c->scratch<unsigned char>(oFixed);
		t.points = c->scratch<double>(oPoints);
		t.of = c->scratch<int>(oOf);
		t.op = c->scratch<int>(oOp);
		t.uv = c->scratch<double>(oUv);
		dTrace = trace ? c->scratch<double>(oTrace) : nullptr;
	}
	else
	{
		t.poses = poses;
		t.fixed = fixed;
		t.points = points;
		t.of = of;
		t.op = op;
		t.uv = uv;
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "bundle-adjustment uploads");
	}
	mark(c, 0);
	if (launch_bundle_adjust(n, maxF, t, *cam, huber, fixPoints ? 1 : 0, *opts, c->scratch<ebo_summary>(oSum), dTrace, c->stream))
	{
		return c->hip(hipGetLastError(), "bundle-adjustment kernel launch");
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
		down(poses, oPoses, 12 * tF * sizeof(double));
		down(points, oPoints, 3 * tP * sizeof(double));
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
		return c->hip(e, "bundle-adjustment results");
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

void ebo_default_ba_opts(ebo_solver_opts* o)
{
	if (!o)
	{
		return;
	}
	ba_default_opts(*o);
}

int ebo_bundle_adjust(ebo_ctx* c, int n_problems, const int* frame_offsets, const int* point_offsets, const int* obs_offsets,
					  double* poses, const uint8_t* pose_fixed, double* points, const int* obs_frame, const int* obs_point,
					  const double* obs_uv, const ebo_camera* cam, double huber, int fix_points, const ebo_solver_opts* opts,
					  ebo_summary* summaries, double* trace)
{
	return adjust(c, n_problems, frame_offsets, point_offsets, obs_offsets, poses, pose_fixed, points, obs_frame, obs_point, obs_uv, true,
				  cam, huber, fix_points, opts, summaries, trace);
}

int ebo_bundle_adjust_device(ebo_ctx* c, int n_problems, const int* frame_offsets, const int* point_offsets, const int* obs_offsets,
							 double* d_poses, const uint8_t* d_pose_fixed, double* d_points, const int* d_obs_frame,
							 const int* d_obs_point, const double* d_obs_uv, const ebo_camera* cam, double huber, int fix_points,
							 const ebo_solver_opts* opts, ebo_summary* summaries, double* d_trace)
{
	return adjust(c, n_problems, frame_offsets, point_offsets, obs_offsets, d_poses, d_pose_fixed, d_points, d_obs_frame, d_obs_point,
				  d_obs_uv, false, cam, huber, fix_points, opts, summaries, d_trace);
}

}  // extern "C"
