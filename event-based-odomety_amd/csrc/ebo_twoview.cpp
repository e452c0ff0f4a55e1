// ebo_twoview.cpp — the two-view entry points of include/ebo.h: eight-point RANSAC over many keyframe pairs
// (VisualOdometryFrontEnd::findInliersRansac, visual_odometry.cpp:288-341), scores for a given model, midpoint
// triangulation (triangulation.cpp:7-29) and the epipolar test (triangulation.cpp:31-63); the kernels are in
// ebo_twoview.inc.  The RANSAC and score entries are ebo_ransac.cpp's drivers with this path's description.
#include "ebo_ctx.h"

using namespace ebo;

namespace
{
const RansacProblem kTwoView = {RansacKind::kTwoView,
								8,
								launch_tv_hypotheses,
								"ebo_relative_pose_ransac",
								"pair",
								"correspondences",
								"bearing vectors",
								"two-view",
								"ebo_relative_pose_scores: null model or bearing vectors, or a negative count",
								"H2D bearing vectors"};
}  // namespace

extern "C" {

void ebo_default_two_view_params(ebo_two_view_params* p)
{
	if (p)
	{
		p->threshold = 5e-5;     // VisualOdometryParams::ransacThreshold
		p->probability = 0.99;   // OpenGV's sac::Ransac default
		p->max_iterations = 1000;
		p->reserved = 0;
		p->seed = 0;
	}
}

int ebo_two_view_timing(ebo_ctx* c, int enable, float* ms5)
{
	int rc = enter(c, "", true);
	if (rc)
	{
		return rc;
	}
	if (enable)
	{
		for (hipEvent_t& e : c->tv_ev)
		{
			// a call that failed half way left the later events null: create what is missing
			rc = e ? EBO_OK : c->hip(hipEventCreate(&e), "hipEventCreate");
			if (rc)
			{
				e = nullptr;
				c->tv_timing = false;
				return rc;
			}
		}
	}
	if (ms5)
	{
		std::copy(c->tv_ms, c->tv_ms + 5, ms5);
	}
	c->tv_timing = enable != 0;
	return EBO_OK;
}

int ebo_relative_pose_ransac(ebo_ctx* c, int n_pairs, const int* offsets, const double* f1, const double* f2,
							 const ebo_two_view_params* params, ebo_two_view_result* result, int* inlier_idx, int* hyp_counts,
							 double* hyp_models, int* hyp_samples)
{
	return ransac(c, kTwoView, n_pairs, offsets, f1, f2, true, params, result, inlier_idx, hyp_counts, hyp_models, hyp_samples);
}

int ebo_relative_pose_ransac_device(ebo_ctx* c, int n_pairs, const int* offsets, const double* d_f1, const double* d_f2,
									const ebo_two_view_params* params, ebo_two_view_result* result, int* inlier_idx,
									int* hyp_counts, double* hyp_models, int* hyp_samples)
{
	return ransac(c, kTwoView, n_pairs, offsets, d_f1, d_f2, false, params, result, inlier_idx, hyp_counts, hyp_models, hyp_samples);
}

int ebo_relative_pose_scores_device(ebo_ctx* c, const double* model, int n, const double* d_f1, const double* d_f2, double threshold,
									double* d_scores, uint8_t* d_flags)
{
	return ransac_scores(c, kTwoView, model, n, d_f1, d_f2, false, threshold, d_scores, d_flags);
}

int ebo_relative_pose_scores(ebo_ctx* c, const double* model, int n, const double* f1, const double* f2, double threshold,
							 double* scores, uint8_t* flags)
{
	return ransac_scores(c, kTwoView, model, n, f1, f2, true, threshold, scores, flags);
}

int ebo_triangulate_device(ebo_ctx* c, int n_poses, const double* d_poses, int n, const int* d_pose_pair, const double* d_f1,
						   const double* d_f2, double* d_points)
{
	int rc = enter(c, "ebo_triangulate: null poses, pairs, bearing vectors or output, or a negative count",
				   n_poses >= 0 && n >= 0 && (n == 0 || (d_poses && d_pose_pair && d_f1 && d_f2 && d_points)));
	if (rc)
	{
		return rc;
	}
	if (launch_tv_triangulate(n_poses, d_poses, n, d_pose_pair, d_f1, d_f2, d_points, c->stream))
	{
		return c->hip(hipGetLastError(), "triangulation launch");
	}
	return EBO_OK;
}

int ebo_triangulate(ebo_ctx* c, int n_poses, const double* poses, int n, const int* pose_pair, const double* f1, const double* f2,
					double* points)
{
	int rc = enter(c, "ebo_triangulate: null poses, pairs, bearing vectors or output, or a negative count",
				   n_poses >= 0 && n >= 0 && (n == 0 || (poses && pose_pair && f1 && f2 && points)));
	if (rc || n == 0)
	{
		return rc;
	}
	for (int i = 0; i < 2 * n; ++i)
	{
		if (pose_pair[i] < 0 || pose_pair[i] >= n_poses)
		{
			return c->fail(EBO_ERR_ARG, "ebo_triangulate: a pose index outside [0, n_poses)");
		}
	}
	ScratchCarve cv;
	const size_t bF = static_cast<size_t>(n) * 3 * sizeof(double), bP = static_cast<size_t>(n_poses) * 12 * sizeof(double);
	const size_t oP = cv.take(bP), oPair = cv.take(static_cast<size_t>(n) * 2 * sizeof(int));
	const size_t oF1 = cv.take(bF), oF2 = cv.take(bF), oOut = cv.take(bF);
	rc = c->grow(c->d_scratch, cv.at, "hipMalloc scratch");
	if (rc)
	{
		return rc;
	}
	hipError_t e = hipMemcpyAsync(c->scratch<double>(oP), poses, bP, hipMemcpyHostToDevice, c->stream);
	if (e == hipSuccess)
	{
		e = hipMemcpyAsync(c->scratch<int>(oPair), pose_pair, static_cast<size_t>(n) * 2 * sizeof(int), hipMemcpyHostToDevice, c->stream);
	}
	if (e == hipSuccess)
	{
		e = hipMemcpyAsync(c->scratch<double>(oF1), f1, bF, hipMemcpyHostToDevice, c->stream);
	}
	if (e == hipSuccess)
	{
		e = hipMemcpyAsync(c->scratch<double>(oF2), f2, bF, hipMemcpyHostToDevice, c->stream);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "H2D triangulation inputs");
	}
	if (launch_tv_triangulate(n_poses, c->scratch<double>(oP), n, c->scratch<int>(oPair), c->scratch<double>(oF1), c->scratch<double>(oF2),
							  c->scratch<double>(oOut), c->stream))
	{
		return c->hip(hipGetLastError(), "triangulation launch");
	}
	e = hipMemcpyAsync(points, c->scratch<double>(oOut), bF, hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	return c->hip(e, "D2H points");
}

int ebo_epipolar_inliers(ebo_ctx* c, const double* model, int n, const double* f1, const double* f2, double threshold, uint8_t* flags)
{
	int rc = enter(c, "ebo_epipolar_inliers: null model, bearing vectors or flags, or a negative count",
				   model && n >= 0 && (n == 0 || (f1 && f2 && flags)));
	if (rc || n == 0)
	{
		return rc;
	}
	ScratchCarve cv;
	const size_t bF = static_cast<size_t>(n) * 3 * sizeof(double);
	const size_t oF1 = cv.take(bF), oF2 = cv.take(bF), oFl = cv.take(n);
	rc = c->grow(c->d_scratch, cv.at, "hipMalloc scratch");
	if (rc)
	{
		return rc;
	}
	hipError_t e = hipMemcpyAsync(c->scratch<double>(oF1), f1, bF, hipMemcpyHostToDevice, c->stream);
	if (e == hipSuccess)
	{
		e = hipMemcpyAsync(c->scratch<double>(oF2), f2, bF, hipMemcpyHostToDevice, c->stream);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "H2D bearing vectors");
	}
	if (launch_tv_epipolar(model, n, c->scratch<double>(oF1), c->scratch<double>(oF2), threshold, c->scratch<unsigned char>(oFl), c->stream))
	{
		return c->hip(hipGetLastError(), "epipolar launch");
	}
	e = hipMemcpyAsync(flags, c->scratch<unsigned char>(oFl), static_cast<size_t>(n), hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	return c->hip(e, "D2H flags");
}

}  // extern "C"
