// visual_odometry/triangulation.h — triangulateLandmarks, computeEssential and findInliersEssential with the
// reference's parameter lists (visual_odometry/include/visual_odometry/triangulation.h:11-21, src/triangulation.cpp:7-63)
// plus the context handle, over the stand-in vector types (no Eigen, Sophus or OpenGV).  The point loops run on the
// device (include/ebo.h "two-view geometry": ebo_triangulate, ebo_epipolar_inliers); computeEssential is rule 7 of
// that section on the host.
#pragma once

#include <stdexcept>
#include <string>
#include <vector>

#include "keyframe.h"

namespace visual_odometry
{
// opengv::bearingVectors_t stand-in: unit vectors, packed as double [n][3]
using bearingVectors_t = std::vector<common::Vector3d>;

namespace detail
{
inline void check(ebo_ctx* ctx, int rc, const char* who)
{
	if (rc != EBO_OK)
	{
		throw std::runtime_error(std::string(who) + ": " + ebo_last_error(ctx));
	}
}
inline const double* packed(const bearingVectors_t& v)
{
	static_assert(sizeof(common::Vector3d) == 3 * sizeof(double), "packed bearing vectors");
	return v.empty() ? nullptr : v[0].data();
}
}  // namespace detail

// world points of correspondences seen along bearingVectors1[i] from cam1Pose and bearingVectors2[i] from cam2Pose
// (camera-to-world poses): cam1Pose * triangulate2(cam1Pose^-1 * cam2Pose, ..), the midpoint method
inline std::vector<common::Vector3d> triangulateLandmarks(ebo_ctx* ctx, const common::Pose3d& cam1Pose,
														   const common::Pose3d& cam2Pose,
														   const bearingVectors_t& bearingVectors1,
														   const bearingVectors_t& bearingVectors2)
{
	if (bearingVectors1.size() != bearingVectors2.size())
	{
		throw std::invalid_argument("triangulateLandmarks: the two lists of bearing vectors differ in length");
	}
	const int n = static_cast<int>(bearingVectors1.size());
	std::vector<common::Vector3d> points(bearingVectors1.size());
	if (n == 0)
	{
		return points;
	}
	double poses[2][12];
	cam1Pose.toArray(poses[0]);
	cam2Pose.toArray(poses[1]);
	std::vector<int> pairs(2 * static_cast<size_t>(n));
	for (int i = 0; i < n; ++i)
	{
		pairs[2 * i] = 0;
		pairs[2 * i + 1] = 1;
	}
	detail::check(ctx,
				  ebo_triangulate(ctx, 2, &poses[0][0], n, pairs.data(), detail::packed(bearingVectors1),
								  detail::packed(bearingVectors2), points[0].data()),
				  "triangulateLandmarks");
	return points;
}

// hat(t / |t|) * R of the relative pose T_0_1, entry by entry as rule 7 writes it
inline common::Matrix3d computeEssential(const common::Pose3d& T_0_1)
{
	const common::Vector3d& t = T_0_1.translation();
	const common::Matrix3d& R = T_0_1.rotationMatrix();
	const double len = std::sqrt((t[0] * t[0] + t[1] * t[1]) + t[2] * t[2]);
	const double ux = t[0] / len, uy = t[1] / len, uz = t[2] / len;
	common::Matrix3d E;
	for (int j = 0; j < 3; ++j)
	{
		E(0, j) = uy * R(2, j) - uz * R(1, j);
		E(1, j) = uz * R(0, j) - ux * R(2, j);
		E(2, j) = ux * R(1, j) - uy * R(0, j);
	}
	return E;
}

// match.inliers = the tracks whose |f1^T E f2| lies below the threshold, E from keyframe1.pose^-1 * keyframe2.pose
inline void findInliersEssential(ebo_ctx* ctx, const bearingVectors_t& bearingVectors1, const bearingVectors_t& bearingVectors2,
								 const Keyframe& keyframe1, const Keyframe& keyframe2,
								 const std::vector<tracker::TrackId>& tracks, Match& match, double epipolarErrorThreshold)
{
	if (bearingVectors1.size() != bearingVectors2.size() || tracks.size() != bearingVectors1.size())
	{
		throw std::invalid_argument("findInliersEssential: bearing vectors and tracks differ in length");
	}
	match.inliers.clear();
	const int n = static_cast<int>(bearingVectors1.size());
	if (n == 0)
	{
		return;
	}
	double model[12];
	(keyframe1.pose.inverse() * keyframe2.pose).toArray(model);
	std::vector<uint8_t> flags(bearingVectors1.size());
	detail::check(ctx,
				  ebo_epipolar_inliers(ctx, model, n, detail::packed(bearingVectors1), detail::packed(bearingVectors2),
									   epipolarErrorThreshold, flags.data()),
				  "findInliersEssential");
	for (int j = 0; j < n; ++j)
	{
		if (flags[j])
		{
			match.inliers.push_back(tracks[j]);
		}
	}
}
}  // namespace visual_odometry
