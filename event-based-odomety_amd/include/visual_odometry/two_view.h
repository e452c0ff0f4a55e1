// visual_odometry/two_view.h — the two-view initialisation of the reference's visual odometry front end on the device:
// VisualOdometryFrontEnd::initCameras + findInliersRansac + getCommonBearingVectors and the `observations.size() == 2`
// branch of addNewLandmarks (visual_odometry/src/visual_odometry.cpp:176-210, 288-341, 343-377, 499-520), without
// OpenGV, Ceres, Sophus or Eigen.
//
//   visual_odometry::TwoViewInitializer init(ctx, recording.getCalibration(), visual_odometry::VisualOdometryParams());
//   tools::Evaluator evaluator(params, [&](const tracker::Patches& patches, const common::timestamp_t& t) {
//       visual_odometry::Keyframe keyframe(patches, t);
//       init.newKeyframeCandidate(keyframe);
//   });
//
// Differences from the reference, all stated in INTEGRATION.md §7:
//   * the shared tracks are SORTED BY TRACK ID before they are unprojected (the reference walks an unordered_map,
//     whose order is not defined), so that a run is reproducible and correspondence i means the same everywhere;
//   * the relative pose comes from ebo_relative_pose_ransac (include/ebo.h "two-view geometry", rules 1-6), this
//     project's own statement of eight-point RANSAC: parity with OpenGV is not claimed;
//   * where the reference calls opengv::relative_pose::optimize_nonlinear the caller may plug a refinement in
//     (setRefinement); there is none by default and the RANSAC model is used as it is; useDeviceRefinement() installs
//     ebo_relative_pose_refine over the RANSAC inliers (relative_refinement.h);
//   * absolute pose, bundle adjustment and the ground-truth alignment are not here: they are
//     VisualOdometryFrontEnd's (visual_odometry.h, bundle_adjustment.h, aligner.h).
#pragma once

#include <algorithm>
#include <cmath>
#include <cstdint>
#include <functional>
#include <memory>
#include <vector>

#include "../common/camera_model.h"
#include "relative_refinement.h"
#include "triangulation.h"

namespace visual_odometry
{
// visual_odometry.h:27-38, the reference's fields and defaults
struct VisualOdometryParams
{
	size_t numOfActiveFrames = 20;
	size_t numOfInliers = 55;
	size_t numOfEssentialInliers = 10;
	size_t ransacMinInliers = 15;
	size_t maxNumIterations = 50;
	size_t maxNumWithoutAdd = 4;
	double ransacThreshold = 5e-5;
	double reprojectionError = 3;
	double huberLoss = 0.8;
};

class TwoViewInitializer
{
   public:
	// (the RANSAC model, both lists of bearing vectors, the RANSAC inliers as indices into them) -> the refined model
	using Refinement = std::function<common::Pose3d(const common::Pose3d&, const bearingVectors_t&, const bearingVectors_t&,
													const std::vector<int>&)>;

	TwoViewInitializer(ebo_ctx* ctx, const common::CameraModelParams<double>& calibration, const VisualOdometryParams& params,
					   uint64_t seed = 0)
		: ctx_(ctx), cameraModel_(calibration), params_(params)
	{
		ebo_default_two_view_params(&ransac_);
		ransac_.threshold = params.ransacThreshold;
		ransac_.seed = seed;
	}

	void setRefinement(Refinement refinement) { refinement_ = std::move(refinement); }
	// the refinement after the RANSAC (visual_odometry.cpp:316-330) on the device, over the RANSAC inliers, with
	// params.maxNumIterations; lastRefinement() is its summary
	void useDeviceRefinement()
	{
		// the hook holds what it needs by value, so the initializer stays copyable; a copy shares the summary
		ebo_ctx* ctx = ctx_;
		const size_t maxNumIterations = params_.maxNumIterations;
		std::shared_ptr<ebo_summary> summary = lastRefinement_;
		refinement_ = [ctx, maxNumIterations, summary](const common::Pose3d& model, const bearingVectors_t& f1, const bearingVectors_t& f2,
													   const std::vector<int>& inliers) {
			return refineRelativePose(ctx, maxNumIterations, model, f1, f2, inliers, summary.get());
		};
	}
	const ebo_summary& lastRefinement() const { return *lastRefinement_; }
	// max_iterations, probability and seed of the RANSAC; the threshold follows VisualOdometryParams::ransacThreshold
	ebo_two_view_params& ransacParams() { return ransac_; }
	const ebo_two_view_result& lastRansac() const { return last_; }

	// visual_odometry.cpp:499-520, the tracks in ascending id order, all corners unprojected in two launches
	void getCommonBearingVectors(const Keyframe& keyframe1, const Keyframe& keyframe2, std::vector<tracker::TrackId>& trackIds,
								 bearingVectors_t& bearingVectors1, bearingVectors_t& bearingVectors2) const
	{
		std::vector<tracker::TrackId> shared = keyframe1.getSharedTracks(keyframe2);
		std::sort(shared.begin(), shared.end());
		std::vector<common::Vector2d> corners1, corners2;
		corners1.reserve(shared.size());
		corners2.reserve(shared.size());
		for (const tracker::TrackId track : shared)
		{
			trackIds.push_back(track);
			corners1.push_back(keyframe1.getLandmarks().at(track));
			corners2.push_back(keyframe2.getLandmarks().at(track));
		}
		const bearingVectors_t b1 = cameraModel_.unprojectBatch(ctx_, corners1);
		const bearingVectors_t b2 = cameraModel_.unprojectBatch(ctx_, corners2);
		bearingVectors1.insert(bearingVectors1.end(), b1.begin(), b1.end());
		bearingVectors2.insert(bearingVectors2.end(), b2.begin(), b2.end());
	}

	// visual_odometry.cpp:288-341: RANSAC, used only when found with >= ransacMinInliers inliers; then the optional
	// refinement, match.Tw2c with a unit translation, and the inliers RE-SELECTED under the refined model
	size_t findInliersRansac(const bearingVectors_t& bearingVectors1, const bearingVectors_t& bearingVectors2,
							 const std::vector<tracker::TrackId>& trackIds, Keyframe& /*keyframe*/, Match& match)
	{
		match.inliers.clear();
		last_ = ebo_two_view_result{};
		const int n = static_cast<int>(bearingVectors1.size());
		if (bearingVectors2.size() != bearingVectors1.size() || trackIds.size() != bearingVectors1.size())
		{
			throw std::invalid_argument("findInliersRansac: bearing vectors and tracks differ in length");
		}
		const int offsets[2] = {0, n};
		std::vector<int> inlierIdx(static_cast<size_t>(n) + 1);
		ransac_.threshold = params_.ransacThreshold;
		detail::check(ctx_,
					  ebo_relative_pose_ransac(ctx_, 1, offsets, detail::packed(bearingVectors1), detail::packed(bearingVectors2),
											   &ransac_, &last_, inlierIdx.data(), nullptr, nullptr, nullptr),
					  "findInliersRansac");
		if (!last_.found || static_cast<size_t>(last_.n_inliers) < params_.ransacMinInliers)
		{
			return 0;
		}
		inlierIdx.resize(static_cast<size_t>(last_.n_inliers));
		common::Pose3d model(&last_.model[0][0]);
		if (refinement_)
		{
			model = refinement_(model, bearingVectors1, bearingVectors2, inlierIdx);
		}
		// a refinement that returns no direction of translation (zero or not finite) leaves the match untouched
		const common::Vector3d& tm = model.translation();
		const double len = std::sqrt((tm[0] * tm[0] + tm[1] * tm[1]) + tm[2] * tm[2]);
		if (!(len > 0.0) || !std::isfinite(len))
		{
			return 0;
		}
		match.Tw2c = model;
		match.Tw2c.translation() = common::Vector3d(tm[0] / len, tm[1] / len, tm[2] / len);
		double m[12];
		model.toArray(m);
		std::vector<uint8_t> flags(static_cast<size_t>(n));
		detail::check(ctx_,
					  ebo_relative_pose_scores(ctx_, m, n, detail::packed(bearingVectors1), detail::packed(bearingVectors2),
											   params_.ransacThreshold, nullptr, flags.data()),
					  "findInliersRansac");
		for (int i = 0; i < n; ++i)
		{
			if (flags[i])
			{
				match.inliers.push_back(trackIds[i]);
			}
		}
		return match.inliers.size();
	}

	// visual_odometry.cpp:176-210 with the start keyframe passed in: true when the re-selected inliers number at
	// least numOfInliers; then keyframe.pose = startKeyframe.pose * match.Tw2c
	bool initCameras(const Keyframe& startKeyframe, Keyframe& keyframe, Match& match)
	{
		bearingVectors_t bearingVectors1, bearingVectors2;
		std::vector<tracker::TrackId> trackIds;
		getCommonBearingVectors(startKeyframe, keyframe, trackIds, bearingVectors1, bearingVectors2);
		const size_t inliers = findInliersRansac(bearingVectors1, bearingVectors2, trackIds, keyframe, match);
		if (inliers < params_.numOfInliers)
		{
			return false;
		}
		keyframe.pose = startKeyframe.pose * match.Tw2c;
		return true;
	}

	// the `observations.size() == 2` branch of addNewLandmarks (visual_odometry.cpp:343-377) for every inlier of the
	// match at once: both keyframes are recorded as observers and the track is triangulated from their poses
	void addNewLandmarks(const Keyframe& startKeyframe, const Keyframe& keyframe, const Match& match)
	{
		std::vector<common::Vector2d> corners1, corners2;
		for (const tracker::TrackId track : match.inliers)
		{
			corners1.push_back(startKeyframe.getLandmarks().at(track));
			corners2.push_back(keyframe.getLandmarks().at(track));
		}
		const bearingVectors_t b1 = cameraModel_.unprojectBatch(ctx_, corners1);
		const bearingVectors_t b2 = cameraModel_.unprojectBatch(ctx_, corners2);
		const std::vector<common::Vector3d> points = triangulateLandmarks(ctx_, startKeyframe.pose, keyframe.pose, b1, b2);
		for (size_t i = 0; i < match.inliers.size(); ++i)
		{
			std::list<size_t>& seen = mapLandmarks_.observations[match.inliers[i]];
			seen.clear();
			seen.push_back(static_cast<size_t>(startKeyframe.timestamp.count()));
			seen.push_back(static_cast<size_t>(keyframe.timestamp.count()));
			mapLandmarks_.landmarks[match.inliers[i]] = points[i];
		}
	}

	// The body of a tools::Evaluator KeyframeHook.  The first candidate becomes the start keyframe (identity pose);
	// every later one is tried against it until one initialises: its pose is set, the landmarks are triangulated,
	// and true is returned.  Candidates after that are ignored (tracking them needs the absolute-pose layer).
	bool newKeyframeCandidate(Keyframe& keyframe)
	{
		if (initialised_)
		{
			return false;
		}
		if (!haveStart_)
		{
			keyframe.pose = common::Pose3d();
			start_ = keyframe;
			haveStart_ = true;
			return false;
		}
		Match match;
		if (!initCameras(start_, keyframe, match))
		{
			return false;
		}
		addNewLandmarks(start_, keyframe, match);
		second_ = keyframe;
		match_ = match;
		initialised_ = true;
		return true;
	}

	bool initialised() const { return initialised_; }
	const Keyframe& startKeyframe() const { return start_; }
	const Keyframe& secondKeyframe() const { return second_; }
	const Match& match() const { return match_; }
	MapLandmarks const& getMapLandmarks() const { return mapLandmarks_; }

   private:
	ebo_ctx* ctx_;
	common::CameraModel<double> cameraModel_;
	VisualOdometryParams params_;
	ebo_two_view_params ransac_;
	ebo_two_view_result last_{};
	std::shared_ptr<ebo_summary> lastRefinement_ = std::make_shared<ebo_summary>();
	Refinement refinement_;
	MapLandmarks mapLandmarks_;
	Keyframe start_, second_;
	Match match_;
	bool haveStart_ = false, initialised_ = false;
};
}  // namespace visual_odometry
