// ebo_abspose.cpp — the absolute-pose entry points of include/ebo.h: three-point RANSAC over the (bearing vector,
// landmark) pairs of many keyframes (VisualOdometryFrontEnd::localizeCamera, visual_odometry.cpp:212-286) and the
// scores for a given pose; the hypothesis kernel is in ebo_abspose.inc.  All of them are ebo_ransac.cpp's drivers with
// this path's description.
#include "ebo_ctx.h"

using namespace ebo;

namespace
{
const RansacProblem kAbsPose = {RansacKind::kAbsPose,
								4,
								launch_ap_hypotheses,
								"ebo_absolute_pose_ransac",
								"frame",
								"points",
								"bearing vectors, landmarks",
								"absolute-pose",
								"ebo_absolute_pose_scores: null pose, bearing vectors or landmarks, or a negative count",
								"H2D bearing vectors and landmarks"};
}  // namespace

extern "C" {

int ebo_absolute_pose_ransac(ebo_ctx* c, int n_frames, const int* offsets, const double* f, const double* pts,
							 const ebo_two_view_params* params, ebo_two_view_result* result, int* inlier_idx, int* hyp_counts,
							 double* hyp_models, int* hyp_samples)
{
	return ransac(c, kAbsPose, n_frames, offsets, f, pts, true, params, result, inlier_idx, hyp_counts, hyp_models, hyp_samples);
}

int ebo_absolute_pose_ransac_device(ebo_ctx* c, int n_frames, const int* offsets, const double* d_f, const double* d_points,
									const ebo_two_view_params* params, ebo_two_view_result* result, int* inlier_idx,
									int* hyp_counts, double* hyp_models, int* hyp_samples)
{
	return ransac(c, kAbsPose, n_frames, offsets, d_f, d_points, false, params, result, inlier_idx, hyp_counts, hyp_models, hyp_samples);
}

int ebo_absolute_pose_scores_device(ebo_ctx* c, const double* pose, int n, const double* d_f, const double* d_points, double threshold,
									double* d_scores, uint8_t* d_flags)
{
	return ransac_scores(c, kAbsPose, pose, n, d_f, d_points, false, threshold, d_scores, d_flags);
}

int ebo_absolute_pose_scores(ebo_ctx* c, const double* pose, int n, const double* f, const double* pts, double threshold,
							 double* scores, uint8_t* flags)
{
	return ransac_scores(c, kAbsPose, pose, n, f, pts, true, threshold, scores, flags);
}

}  // extern "C"
