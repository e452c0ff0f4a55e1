// ebo_landmark.cpp — the landmark-maintenance entry points of include/ebo.h: robust N-view triangulation of every
// landmark of a call from its whole observation list (ebo_triangulate_tracks) and the audit of given points against
// their observations (ebo_landmark_scores), one launch each; the kernel is in ebo_landmark.inc.
#include "ebo_ctx.h"

#include <chrono>

using namespace ebo;

namespace
{
// Lanes per landmark when every landmark of the call fits a quarter of a wave's staging area: four landmarks share a
// wave.  DESIGN.md 4.20 has the measurement behind the choice; the results do not depend on it.
constexpr size_t kLmSmallLanes = 16;

int landmarks(ebo_ctx* c, const char* entry, bool solve, bool hostArrays, int nPoses, const double* poses, int n, const int* offsets,
			  const int* obsPose, const double* obsF, const double* points, const ebo_landmark_params* prm, ebo_landmark_result* results,
			  double* scores, uint8_t* flags)
{
	auto bad = [&](const char* what) { return c->fail(EBO_ERR_ARG, std::string(entry) + ": " + what); };
	int rc = enter(c, "landmark maintenance: a negative pose count or a landmark count outside [0, 2^20]",
				   nPoses >= 0 && n >= 0 && n <= kLmMaxLandmarks);
	if (rc)
	{
		return rc;
	}
	if (!prm)
	{
		return bad("null params");
	}
	if (!(prm->threshold > 0.0 && prm->threshold < 1.0))
	{
		return bad("threshold outside (0, 1)");
	}
	if (!(prm->min_parallax >= 0.0))
	{
		return bad("a negative (or NaN) min_parallax");
	}
	if (prm->min_inliers < 2 || prm->max_hypotheses < 1 || prm->max_hypotheses > kLmMaxHypotheses)
	{
		return bad("min_inliers below 2 or max_hypotheses outside [1, 4096]");
	}
	if (!offsets)
	{
		return bad("null obs_offsets");
	}
	if (offsets[0] != 0)
	{
		return bad("obs_offsets do not start at 0");
	}
	int maxObs = 0;
	for (int l = 0; l < n; ++l)
	{
		if (offsets[l + 1] < offsets[l])
		{
			return bad("obs_offsets decrease");
		}
		if (offsets[l + 1] - offsets[l] > kLmMaxObs)
		{
			return bad("a landmark holds at most 512 observations");
		}
		maxObs = std::max(maxObs, offsets[l + 1] - offsets[l]);
	}
	if (n == 0)
	{
		return EBO_OK;
	}
	const size_t total = static_cast<size_t>(offsets[n]);
	if (!results || (!solve && !points))
	{
		return bad(solve ? "null results" : "null results or points");
	}
	if (total > 0 && (!obsPose || !obsF))
	{
		return bad("null obs_pose or obs_f");
	}
	if (nPoses > 0 && !poses)
	{
		return bad("null poses");
	}
	if (hostArrays)
	{
		for (size_t o = 0; o < total; ++o)
		{
			if (obsPose[o] < 0 || obsPose[o] >= nPoses)
			{
				return bad("a pose index outside [0, n_poses)");
			}
		}
	}
	const auto wall0 = std::chrono::steady_clock::now();
	const size_t bOff = (static_cast<size_t>(n) + 1) * sizeof(int), bRes = static_cast<size_t>(n) * sizeof(ebo_landmark_result);
	const size_t bPoses = kLmPoseDoubles * static_cast<size_t>(nPoses) * sizeof(double), bIdx = total * sizeof(int);
	const size_t bF = 3 * total * sizeof(double), bPts = solve ? 0 : 3 * static_cast<size_t>(n) * sizeof(double);
	const size_t bScores = scores ? total * sizeof(double) : 0, bFlags = flags ? total : 0;
	ScratchCarve cv;
	const size_t oOff = cv.take(bOff);
	size_t oRes = 0, oPoses = 0, oIdx = 0, oF = 0, oPts = 0, oScores = 0, oFlags = 0;
	if (hostArrays)
	{
		oRes = cv.take(bRes);
		oPoses = cv.take(bPoses);
		oIdx = cv.take(bIdx);
		oF = cv.take(bF);
		oPts = cv.take(bPts);
		oScores = cv.take(bScores);
		oFlags = cv.take(bFlags);
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
	up(oOff, offsets, bOff);
	const double* dPoses = poses;
	const int* dIdx = obsPose;
	const double* dF = obsF;
	const double* dPts = points;
	ebo_landmark_result* dRes = results;
	double* dScores = scores;
	uint8_t* dFlags = flags;
	if (hostArrays)
	{
		up(oPoses, poses, bPoses);
		up(oIdx, obsPose, bIdx);
		up(oF, obsF, bF);
		up(oPts, points, bPts);
		dPoses = c->scratch<double>(oPoses);
		dIdx = c->scratch<int>(oIdx);
		dF = c->scratch<double>(oF);
		dPts = solve ? nullptr : c->scratch<double>(oPts);
		dRes = c->scratch<ebo_landmark_result>(oRes);
		dScores = scores ? c->scratch<double>(oScores) : nullptr;
		dFlags = flags ? c->scratch<uint8_t>(oFlags) : nullptr;
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "landmark maintenance uploads");
	}
	int lanes = 64;
	if (maxObs <= kLmGroupMaxObs)
	{
		lanes = ab_size("EBO_LANDMARK_LANES", kLmSmallLanes) == 64 ? 64 : 16;
	}
	mark(c, 0);
	if (launch_landmarks(solve ? 1 : 0, lanes, nPoses, dPoses, n, c->scratch<int>(oOff), dIdx, dF, dPts, prm, dRes, dScores, dFlags, c->stream))
	{
		return c->hip(hipGetLastError(), "landmark maintenance kernel launch");
	}
	mark(c, 1);
	if (!hostArrays)
	{
		return EBO_OK;
	}
	auto down = [&](void* dst, size_t off, size_t bytes) {
		if (e == hipSuccess && bytes)
		{
			e = hipMemcpyAsync(dst, c->scratch<char>(off), bytes, hipMemcpyDeviceToHost, c->stream);
		}
	};
	down(results, oRes, bRes);
	down(scores, oScores, bScores);
	down(flags, oFlags, bFlags);
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "landmark maintenance results");
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

void ebo_default_landmark_params(ebo_landmark_params* p)
{
	if (!p)
	{
		return;
	}
	p->threshold = 0x1.a36622p-15;          // (double)(float)(1 - cos(atan2(2, 200))) = 4.99962516e-05: localizeCamera's
	p->min_parallax = 0x1.3f680a5076p-13;   // 1 - cos(1 degree) = 1.5230484360873042e-04
	p->min_inliers = 2;
	p->max_hypotheses = 300;  // every landmark of up to 25 observations is exhaustive
	p->seed = 0;
}

int ebo_triangulate_tracks(ebo_ctx* c, int n_poses, const double* poses, int n_landmarks, const int* obs_offsets, const int* obs_pose,
						   const double* obs_f, const ebo_landmark_params* params, ebo_landmark_result* results, double* scores_or_null,
						   uint8_t* inlier_flags_or_null)
{
	return landmarks(c, "ebo_triangulate_tracks", true, true, n_poses, poses, n_landmarks, obs_offsets, obs_pose, obs_f, nullptr, params,
					 results, scores_or_null, inlier_flags_or_null);
}

int ebo_triangulate_tracks_device(ebo_ctx* c, int n_poses, const double* d_poses, int n_landmarks, const int* obs_offsets,
								  const int* d_obs_pose, const double* d_obs_f, const ebo_landmark_params* params,
								  ebo_landmark_result* d_results, double* d_scores_or_null, uint8_t* d_inlier_flags_or_null)
{
	return landmarks(c, "ebo_triangulate_tracks_device", true, false, n_poses, d_poses, n_landmarks, obs_offsets, d_obs_pose, d_obs_f,
					 nullptr, params, d_results, d_scores_or_null, d_inlier_flags_or_null);
}

int ebo_landmark_scores(ebo_ctx* c, int n_poses, const double* poses, int n_landmarks, const int* obs_offsets, const int* obs_pose,
						const double* obs_f, const double* points, const ebo_landmark_params* params, ebo_landmark_result* results,
						double* scores_or_null, uint8_t* inlier_flags_or_null)
{
	return landmarks(c, "ebo_landmark_scores", false, true, n_poses, poses, n_landmarks, obs_offsets, obs_pose, obs_f, points, params,
					 results, scores_or_null, inlier_flags_or_null);
}

int ebo_landmark_scores_device(ebo_ctx* c, int n_poses, const double* d_poses, int n_landmarks, const int* obs_offsets,
							   const int* d_obs_pose, const double* d_obs_f, const double* d_points, const ebo_landmark_params* params,
							   ebo_landmark_result* d_results, double* d_scores_or_null, uint8_t* d_inlier_flags_or_null)
{
	return landmarks(c, "ebo_landmark_scores_device", false, false, n_poses, d_poses, n_landmarks, obs_offsets, d_obs_pose, d_obs_f,
					 d_points, params, d_results, d_scores_or_null, d_inlier_flags_or_null);
}

}  // extern "C"
