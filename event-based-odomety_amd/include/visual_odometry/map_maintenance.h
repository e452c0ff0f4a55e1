// visual_odometry/map_maintenance.h — the map cleaned between keyframes, which the reference leaves as TODOs
// (visual_odometry/src/visual_odometry.cpp:169, :407): every landmark the active keyframes observe at least twice is
// audited against ALL its observations under the current poses (ebo_landmark_scores); the ones that fail, and the
// tracks that have no landmark yet, are triangulated from their whole observation list (ebo_triangulate_tracks); what
// still has no point leaves the map.  include/ebo.h "landmark maintenance" (L1-L7) has the rules;
// tests/landmark_ref.py restates this policy as `maintain`.
//
//   visual_odometry::MapMaintenanceSummary s = visual_odometry::maintainMap(ctx, calibration, params, activeFrames, mapLandmarks);
//
// mapLandmarks.observations is never touched, so the reference's own bookkeeping (addNewLandmarks' size() == 2 trigger,
// deleteLandmarks) works on unchanged.
#pragma once

#include <algorithm>
#include <cmath>
#include <map>

#include "../common/camera_model.h"
#include "triangulation.h"

namespace visual_odometry
{
struct MapMaintenanceParams
{
	double reprojectionError = 2.0;   // pixels at f = 200: the inlier threshold by localizeCamera's formula
	double minParallaxDegrees = 1.0;  // a policy default in the range ORB-SLAM and COLMAP use
	int minInliers = 2;
	int maxHypotheses = 300;
	uint64_t seed = 0;

	// visual_odometry.cpp:240-241: the reference keeps the threshold in a float
	double threshold() const
	{
		const float t = static_cast<float>(1.0 - std::cos(std::atan2(reprojectionError, 200.)));
		return static_cast<double>(t);
	}
	double minParallax() const { return 1.0 - std::cos(minParallaxDegrees * (3.14159265358979323846 / 180.0)); }
	ebo_landmark_params toEbo() const
	{
		ebo_landmark_params p;
		ebo_default_landmark_params(&p);
		p.threshold = threshold();
		p.min_parallax = minParallax();
		p.min_inliers = minInliers;
		p.max_hypotheses = maxHypotheses;
		p.seed = seed;
		return p;
	}
};

struct MapMaintenanceSummary
{
	size_t candidates = 0;      // tracks with at least two listed keyframes that are active and hold their corner
	size_t audited = 0;         // candidates that had a landmark
	size_t kept = 0;            // audited, status 0: untouched
	size_t retriangulated = 0;  // failed the audit, triangulated again with status 0: replaced
	size_t added = 0;           // had no landmark, triangulated with status 0
	size_t culled = 0;          // failed the audit and the triangulation: erased
};

// Candidates in ascending track id, their observations in ascending keyframe id, all corners unprojected in one launch.
inline MapMaintenanceSummary maintainMap(ebo_ctx* ctx, const common::CameraModelParams<double>& calibration,
										 const MapMaintenanceParams& params, const std::map<size_t, Keyframe>& activeFrames,
										 MapLandmarks& mapLandmarks)
{
	MapMaintenanceSummary summary;
	std::map<size_t, int> poseIndex;
	std::vector<double> poses(12 * activeFrames.size());
	for (const auto& kf : activeFrames)
	{
		const int idx = static_cast<int>(poseIndex.size());
		poseIndex[kf.first] = idx;
		kf.second.pose.toArray(poses.data() + 12 * static_cast<size_t>(idx));
	}
	std::vector<tracker::TrackId> tracks;
	for (const auto& obs : mapLandmarks.observations)
	{
		tracks.push_back(obs.first);
	}
	std::sort(tracks.begin(), tracks.end());
	struct Candidate
	{
		tracker::TrackId track;
		size_t first, count;  // its observations in obsPose / corners
	};
	std::vector<Candidate> candidates;
	std::vector<int> obsPose;
	std::vector<common::Vector2d> corners;
	for (const tracker::TrackId track : tracks)
	{
		std::vector<size_t> seen(mapLandmarks.observations.at(track).begin(), mapLandmarks.observations.at(track).end());
		std::sort(seen.begin(), seen.end());
		seen.erase(std::unique(seen.begin(), seen.end()), seen.end());
		const size_t first = obsPose.size();
		for (const size_t kId : seen)
		{
			const auto kf = activeFrames.find(kId);
			if (kf == activeFrames.end())
			{
				continue;
			}
			const auto corner = kf->second.getLandmarks().find(track);
			if (corner == kf->second.getLandmarks().end())
			{
				continue;
			}
			obsPose.push_back(poseIndex.at(kId));
			corners.push_back(corner->second);
		}
		if (obsPose.size() - first >= 2)
		{
			candidates.push_back({track, first, obsPose.size() - first});
		}
		else
		{
			obsPose.resize(first);
			corners.resize(first);
		}
	}
	summary.candidates = candidates.size();
	if (candidates.empty())
	{
		return summary;
	}
	const common::CameraModel<double> cameraModel(calibration);
	const bearingVectors_t vectors = cameraModel.unprojectBatch(ctx, corners);
	const ebo_landmark_params prm = params.toEbo();
	const int nPoses = static_cast<int>(poseIndex.size());

	// one call over a subset of the candidates: their observations gathered in order
	struct Subset
	{
		std::vector<size_t> which;
		std::vector<int> offsets{0}, pose;
		bearingVectors_t f;
	};
	const auto add = [&](Subset& s, size_t c) {
		s.which.push_back(c);
		for (size_t o = candidates[c].first; o < candidates[c].first + candidates[c].count; ++o)
		{
			s.pose.push_back(obsPose[o]);
			s.f.push_back(vectors[o]);
		}
		s.offsets.push_back(static_cast<int>(s.pose.size()));
	};
	Subset audit, solve;
	for (size_t c = 0; c < candidates.size(); ++c)
	{
		if (mapLandmarks.landmarks.count(candidates[c].track) != 0)
		{
			add(audit, c);
		}
	}
	summary.audited = audit.which.size();
	std::vector<char> failed(candidates.size(), 0);
	if (!audit.which.empty())
	{
		std::vector<common::Vector3d> points;
		for (const size_t c : audit.which)
		{
			points.push_back(mapLandmarks.landmarks.at(candidates[c].track));
		}
		std::vector<ebo_landmark_result> results(audit.which.size());
		detail::check(ctx,
					  ebo_landmark_scores(ctx, nPoses, poses.data(), static_cast<int>(audit.which.size()), audit.offsets.data(),
										  audit.pose.data(), detail::packed(audit.f), points[0].data(), &prm, results.data(), nullptr, nullptr),
					  "maintainMap");
		for (size_t i = 0; i < audit.which.size(); ++i)
		{
			if (results[i].status == 0)
			{
				summary.kept++;
			}
			else
			{
				failed[audit.which[i]] = 1;
			}
		}
	}
	for (size_t c = 0; c < candidates.size(); ++c)
	{
		if (failed[c] || mapLandmarks.landmarks.count(candidates[c].track) == 0)
		{
			add(solve, c);
		}
	}
	if (!solve.which.empty())
	{
		std::vector<ebo_landmark_result> results(solve.which.size());
		detail::check(ctx,
					  ebo_triangulate_tracks(ctx, nPoses, poses.data(), static_cast<int>(solve.which.size()), solve.offsets.data(),
											 solve.pose.data(), detail::packed(solve.f), &prm, results.data(), nullptr, nullptr),
					  "maintainMap");
		for (size_t i = 0; i < solve.which.size(); ++i)
		{
			const tracker::TrackId track = candidates[solve.which[i]].track;
			const bool existed = failed[solve.which[i]] != 0;
			if (results[i].status == 0)
			{
				mapLandmarks.landmarks[track] = common::Vector3d(results[i].point[0], results[i].point[1], results[i].point[2]);
				(existed ? summary.retriangulated : summary.added)++;
			}
			else if (existed)
			{
				mapLandmarks.landmarks.erase(track);
				summary.culled++;
			}
		}
	}
	return summary;
}
}  // namespace visual_odometry
