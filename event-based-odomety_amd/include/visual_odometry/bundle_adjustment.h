// visual_odometry/bundle_adjustment.h — the two hooks of VisualOdometryFrontEnd filled in by ebo_bundle_adjust
// (include/ebo.h, "bundle adjustment", rules B1-B9: this project's own statement; parity with Ceres, Sophus or OpenGV
// is not claimed, INTEGRATION.md §7 lists the differences).
//
//   bundleAdjust: VisualOdometryFrontEnd::optimize (visual_odometry.cpp:416-497) -- the active frames in map order, the
//     first two constant, the camera constant, HuberLoss(huberLoss), maxNumIterations, one residual per observation
//     that passes the filter of :445-474; landmarks are taken in ASCENDING TRACK ID (the reference walks an
//     unordered_map).  Poses and landmarks are written back.
//   refinePose: the non-linear refinement after localizeCamera's RANSAC (:262) -- the same entry with fix_points on
//     the identity camera and uv = (f_x / f_z, f_y / f_z) of the inliers' bearing vectors; an inlier with f_z <= 0 is
//     left out.  It minimises the reprojection error on the normalised plane, where OpenGV's optimize_nonlinear
//     minimises a bearing-vector error.
#pragma once

#include <algorithm>
#include <map>
#include <vector>

#include "keyframe.h"
#include "triangulation.h"
#include "../common/camera_model.h"

namespace visual_odometry
{
// -> the problem's summary (iterations 0 and nothing touched when there is no frame to adjust)
inline ebo_summary bundleAdjust(ebo_ctx* ctx, const common::CameraModelParams<double>& calibration, double huberLoss,
								size_t maxNumIterations, std::map<size_t, Keyframe>& activeFrames, MapLandmarks& map)
{
	ebo_summary summary{};
	if (activeFrames.empty())
	{
		return summary;
	}
	std::map<size_t, int> frameIndex;
	std::vector<double> poses;
	std::vector<uint8_t> fixed;
	for (const auto& frame : activeFrames)
	{
		const int i = static_cast<int>(frameIndex.size());
		frameIndex[frame.first] = i;
		double m[12];
		frame.second.pose.toArray(m);
		poses.insert(poses.end(), m, m + 12);
		fixed.push_back(i < 2 ? 1 : 0);
	}
	std::vector<tracker::TrackId> tracks;
	for (const auto& landmark : map.landmarks)
	{
		tracks.push_back(landmark.first);
	}
	std::sort(tracks.begin(), tracks.end());
	std::vector<double> points;
	std::vector<int> obsFrame, obsPoint;
	std::vector<double> uv;
	for (size_t l = 0; l < tracks.size(); ++l)
	{
		const common::Vector3d& p = map.landmarks.at(tracks[l]);
		points.insert(points.end(), {p[0], p[1], p[2]});
		const auto observations = map.observations.find(tracks[l]);
		if (observations == map.observations.end() || observations->second.size() < 2)
		{
			continue;
		}
		for (const size_t frameId : observations->second)
		{
			const auto frameIt = activeFrames.find(frameId);
			if (frameIt == activeFrames.end())
			{
				continue;
			}
			const auto cornerIt = frameIt->second.getLandmarks().find(tracks[l]);
			if (cornerIt == frameIt->second.getLandmarks().end())
			{
				continue;
			}
			obsFrame.push_back(frameIndex.at(frameId));
			obsPoint.push_back(static_cast<int>(l));
			uv.push_back(cornerIt->second[0]);
			uv.push_back(cornerIt->second[1]);
		}
	}
	const int frameOffsets[2] = {0, static_cast<int>(fixed.size())};
	const int pointOffsets[2] = {0, static_cast<int>(tracks.size())};
	const int obsOffsets[2] = {0, static_cast<int>(obsFrame.size())};
	const ebo_camera cam = common::toEboCamera(calibration);
	ebo_solver_opts opts;
	ebo_default_ba_opts(&opts);
	opts.max_num_iterations = static_cast<int>(maxNumIterations);
	detail::check(ctx,
				  ebo_bundle_adjust(ctx, 1, frameOffsets, pointOffsets, obsOffsets, poses.data(), fixed.data(), points.data(), obsFrame.data(),
									obsPoint.data(), uv.data(), &cam, huberLoss, 0, &opts, &summary, nullptr),
				  "bundleAdjust");
	for (auto& frame : activeFrames)
	{
		frame.second.pose = common::Pose3d(poses.data() + 12 * frameIndex.at(frame.first));
	}
	for (size_t l = 0; l < tracks.size(); ++l)
	{
		map.landmarks.at(tracks[l]) = common::Vector3d(points[3 * l], points[3 * l + 1], points[3 * l + 2]);
	}
	return summary;
}

// the signature of VisualOdometryFrontEnd::LocalizeRefinement plus the context and the options' sources
inline common::Pose3d refinePose(ebo_ctx* ctx, double huberLoss, size_t maxNumIterations, const common::Pose3d& pose,
								 const bearingVectors_t& bearingVectors, const std::vector<common::Vector3d>& points,
								 const std::vector<int>& inliers, ebo_summary* summaryOut = nullptr)
{
	std::vector<double> pts, uv;
	std::vector<int> obsFrame, obsPoint;
	for (const int i : inliers)
	{
		const common::Vector3d& f = bearingVectors[static_cast<size_t>(i)];
		if (!(f[2] > 0.0))
		{
			continue;
		}
		const common::Vector3d& p = points[static_cast<size_t>(i)];
		obsPoint.push_back(static_cast<int>(obsFrame.size()));
		obsFrame.push_back(0);
		pts.insert(pts.end(), {p[0], p[1], p[2]});
		uv.push_back(f[0] / f[2]);
		uv.push_back(f[1] / f[2]);
	}
	double m[12];
	pose.toArray(m);
	const uint8_t fixed = 0;
	const int n = static_cast<int>(obsFrame.size());
	const int frameOffsets[2] = {0, 1}, pointOffsets[2] = {0, n}, obsOffsets[2] = {0, n};
	const ebo_camera identity{1.0, 1.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
	ebo_solver_opts opts;
	ebo_default_ba_opts(&opts);
	opts.max_num_iterations = static_cast<int>(maxNumIterations);
	ebo_summary summary{};
	detail::check(ctx,
				  ebo_bundle_adjust(ctx, 1, frameOffsets, pointOffsets, obsOffsets, m, &fixed, pts.data(), obsFrame.data(), obsPoint.data(),
									uv.data(), &identity, huberLoss, 1, &opts, &summary, nullptr),
				  "refinePose");
	if (summaryOut)
	{
		*summaryOut = summary;
	}
	return common::Pose3d(m);
}
}  // namespace visual_odometry
