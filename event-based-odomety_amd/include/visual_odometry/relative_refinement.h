// visual_odometry/relative_refinement.h — the hook of TwoViewInitializer filled in by ebo_relative_pose_refine
// (include/ebo.h, "relative-pose refinement", rules R1-R8: this project's own statement; parity with OpenGV is not
// claimed, INTEGRATION.md §7 lists the differences).
//
//   refineRelativePose: the non-linear refinement after findInliersRansac's RANSAC (visual_odometry.cpp:316-330) -- five
//     variables (the translation's direction on the unit sphere, the rotation), the chords of the two-view score over
//     the RANSAC inliers, no loss function, ebo_default_ba_opts with maxNumIterations.  It minimises the very quantity
//     the re-selection that follows thresholds; the model that comes back has a unit translation.
#pragma once

#include <algorithm>
#include <stdexcept>
#include <vector>

#include "triangulation.h"

namespace visual_odometry
{
// the signature of TwoViewInitializer::Refinement plus the context and the iteration count
inline common::Pose3d refineRelativePose(ebo_ctx* ctx, size_t maxNumIterations, const common::Pose3d& model,
										 const bearingVectors_t& bearingVectors1, const bearingVectors_t& bearingVectors2,
										 const std::vector<int>& inliers, ebo_summary* summaryOut = nullptr)
{
	double m[12];
	model.toArray(m);
	const int n = static_cast<int>(bearingVectors1.size());
	if (bearingVectors2.size() != bearingVectors1.size() || inliers.size() > bearingVectors1.size())
	{
		throw std::invalid_argument("refineRelativePose: bearing vectors differ in length, or more inliers than correspondences");
	}
	const int offsets[2] = {0, n}, count = static_cast<int>(inliers.size());
	std::vector<int> idx(static_cast<size_t>(n) + 1);  // never empty: the entry wants a pointer
	std::copy(inliers.begin(), inliers.end(), idx.begin());
	ebo_solver_opts opts;
	ebo_default_ba_opts(&opts);
	opts.max_num_iterations = static_cast<int>(maxNumIterations);
	ebo_summary summary{};
	detail::check(ctx,
				  ebo_relative_pose_refine(ctx, 1, offsets, detail::packed(bearingVectors1), detail::packed(bearingVectors2), m, &count,
										   idx.data(), &opts, &summary, nullptr),
				  "refineRelativePose");
	if (summaryOut)
	{
		*summaryOut = summary;
	}
	return common::Pose3d(m);
}
}  // namespace visual_odometry
