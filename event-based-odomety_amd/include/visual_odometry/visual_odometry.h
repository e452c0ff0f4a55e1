// visual_odometry/visual_odometry.h — the keyframe front end of the reference's visual odometry on the device:
// VisualOdometryFrontEnd with the reference's member names (visual_odometry/include/visual_odometry/visual_odometry.h:40-100),
// each member a restatement of visual_odometry/src/visual_odometry.cpp:52-174, 212-286, 343-414, without OpenGV, Ceres,
// Sophus or Eigen.  Two-view initialisation is visual_odometry::TwoViewInitializer's (two_view.h), composed here.
//
//   visual_odometry::VisualOdometryFrontEnd frontEnd(ctx, recording.getCalibration(), visual_odometry::VisualOdometryParams());
//   tools::Evaluator evaluator(params, [&](const tracker::Patches& patches, const common::timestamp_t& t) {
//       visual_odometry::Keyframe keyframe(patches, t);
//       frontEnd.newKeyframeCandidate(keyframe);
//   });
//
// Differences from the reference, all stated in INTEGRATION.md §7:
//   * localizeCamera takes the keyframe's tracks that are in the map in ASCENDING TRACK ID (the reference walks an
//     unordered_map), unprojects their corners in one launch, and gets the pose from ebo_absolute_pose_ransac
//     (include/ebo.h "absolute pose", A1-A5), this project's own statement of three-point RANSAC: parity with OpenGV
//     is not claimed;
//   * where the reference calls opengv::absolute_pose::optimize_nonlinear the caller may plug a refinement in
//     (setLocalizeRefinement); there is none by default and the RANSAC pose is used as it is;
//     useDeviceLocalizeRefinement() installs ebo_bundle_adjust with the points held constant (bundle_adjustment.h);
//   * optimize() is a hook (setOptimizer), called where the reference calls it; there is none by default;
//     useDeviceBundleAdjustment() installs ebo_bundle_adjust (include/ebo.h "bundle adjustment", B1-B9), this
//     project's own statement of the windowed problem: parity with Ceres is not claimed;
//   * addNewLandmarks triangulates all tracks whose observation list has just reached two in ONE ebo_triangulate
//     call, after the loop over the inliers (nothing in that loop reads a landmark);
//   * deleteLandmarks moves the landmarks whose last observation went to storedLandmarks_ in ascending track id (the
//     reference walks an unordered_map);
//   * withoutAdd_, which the reference leaves uninitialised, starts at 0;
//   * the ground truth is opt-in: with setGroundTruthSamples the gt_ bookkeeping of :62-71 runs, and with
//     useDeviceAlignment() the alignment of :83-97 through ebo_align_sim3 (aligner.h; include/ebo.h "trajectory
//     alignment", S1-S7, this project's own statement: parity with Eigen's JacobiSVD is not claimed).  The reference
//     indexes gt_[i] by keyframe position even when a keyframe had no ground truth, which reads out of range; here a
//     keyframe without a synced pose is left out of the pairing.  Without the two calls nothing of it runs;
//   * useDeviceRelativeErrors(deltas) adds what the reference does not have: after every added keyframe the relative
//     pose error (ebo_trajectory_rpe, include/ebo.h T1-T7) of the same paired keyframes, poses instead of centres.
//     Without the call nothing of it runs;
//   * useDeviceMapMaintenance(params) adds what the reference leaves as TODOs (:169, :407): after the optimizer hook of
//     every added keyframe the map is audited and repaired (map_maintenance.h): landmarks can be replaced and erased
//     between keyframes, observations never.  Without the call nothing of it runs;
//   * the log lines are not here.
#pragma once

#include <list>
#include <map>
#include <utility>

#include "aligner.h"
#include "bundle_adjustment.h"
#include "map_maintenance.h"
#include "two_view.h"

namespace visual_odometry
{
class VisualOdometryFrontEnd
{
   public:
	// (the RANSAC pose, the bearing vectors, their landmarks, the RANSAC inliers as indices into them) -> the refined pose
	using LocalizeRefinement = std::function<common::Pose3d(const common::Pose3d&, const bearingVectors_t&,
															const std::vector<common::Vector3d>&, const std::vector<int>&)>;
	// what the reference's optimize() works on: the active keyframes and the map
	using Optimizer = std::function<void(std::map<size_t, Keyframe>&, MapLandmarks&)>;

	VisualOdometryFrontEnd(ebo_ctx* ctx, const common::CameraModelParams<double>& calibration, const VisualOdometryParams& params,
						   uint64_t seed = 0)
		: ctx_(ctx), calibration_(calibration), cameraModel_(calibration), params_(params), twoView_(ctx, calibration, params, seed)
	{
		ebo_default_two_view_params(&ransac_);
		ransac_.threshold = localizeThreshold();
		ransac_.seed = seed;
	}

	// the hooks that the two use... members install hold this object's address: it is neither copied nor moved
	VisualOdometryFrontEnd(const VisualOdometryFrontEnd&) = delete;
	VisualOdometryFrontEnd& operator=(const VisualOdometryFrontEnd&) = delete;

	void setLocalizeRefinement(LocalizeRefinement refinement) { localizeRefinement_ = std::move(refinement); }
	void setOptimizer(Optimizer optimizer) { optimizer_ = std::move(optimizer); }
	// optimize() (visual_odometry.cpp:416-497) on the device: HuberLoss(params.huberLoss), params.maxNumIterations, the
	// first two active frames constant; lastBundleAdjustment() is its summary
	void useDeviceBundleAdjustment()
	{
		optimizer_ = [this](std::map<size_t, Keyframe>& active, MapLandmarks& map) {
			lastBundle_ = bundleAdjust(ctx_, calibration_, params_.huberLoss, params_.maxNumIterations, active, map);
		};
	}
	// the refinement after localizeCamera's RANSAC (:262) on the device, over the RANSAC inliers
	void useDeviceLocalizeRefinement()
	{
		localizeRefinement_ = [this](const common::Pose3d& pose, const bearingVectors_t& f, const std::vector<common::Vector3d>& points,
									 const std::vector<int>& inliers) {
			return refinePose(ctx_, params_.huberLoss, params_.maxNumIterations, pose, f, points, inliers, &lastRefinement_);
		};
	}
	// visual_odometry.cpp:563-567; from here on every added keyframe is synced against the samples (:62-71)
	void setGroundTruthSamples(const common::GroundTruth& groundTruthSamples)
	{
		groundTruthSamples_ = groundTruthSamples;
		useGroundTruth_ = true;
	}
	// visual_odometry.cpp:522-561
	std::optional<common::Pose3d> syncGtAndImage(const common::timestamp_t& timestamp) const
	{
		return syncGroundTruth(groundTruthSamples_, timestamp);
	}
	// the alignment after the optimizer (:83-97) on the device, once more than 5 keyframes exist
	void useDeviceAlignment() { deviceAlignment_ = true; }
	// of the last candidate that was aligned; status 1 and the identity before that
	const Alignment& lastAlignment() const { return lastAlignment_; }
	// the relative pose error at every one of `deltas` (steps in paired keyframes) after every added keyframe, once
	// ground-truth samples are set: over the keyframes alignToGroundTruth pairs, in its order.  The estimate's
	// translations are multiplied by lastAlignment()'s scale when that alignment has status 0, else by 1
	void useDeviceRelativeErrors(std::vector<int> deltas) { relativeDeltas_ = std::move(deltas); }
	// of the last added keyframe: one entry per delta; empty before the first evaluation
	const std::vector<RelativeErrors>& lastRelativeErrors() const { return lastRelativeErrors_; }
	// the scale they were evaluated with, and whether it is an alignment's (false: no alignment with status 0, scale 1)
	double lastRelativeErrorsScale() const { return relativeScale_; }
	bool lastRelativeErrorsAligned() const { return relativeAligned_; }
	// maintainMap (map_maintenance.h) after the optimizer hook of every added keyframe and before the alignment
	void useDeviceMapMaintenance(const MapMaintenanceParams& params)
	{
		mapMaintenance_ = params;
		deviceMapMaintenance_ = true;
	}
	// of the last added keyframe; zeros before the first
	const MapMaintenanceSummary& lastMapMaintenance() const { return lastMapMaintenance_; }
	// the reference's getGtPoses(): the synced poses relative to the first, in keyframe order; after an alignment
	// sim.inverse() * each of them
	std::vector<common::Pose3d> const& alignedGroundTruth() const { return gtAligned_; }
	const ebo_summary& lastBundleAdjustment() const { return lastBundle_; }
	const ebo_summary& lastRefinement() const { return lastRefinement_; }
	// the two-view layer that initCameras goes through (its refinement and RANSAC parameters are set there)
	TwoViewInitializer& twoView() { return twoView_; }
	// max_iterations, probability and seed of localizeCamera's RANSAC; the threshold follows reprojectionError
	ebo_two_view_params& ransacParams() { return ransac_; }
	const ebo_two_view_result& lastLocalize() const { return last_; }
	// the match of the last candidate, as isNewKeyframeNeeded left it
	const Match& lastMatch() const { return match_; }

	// visual_odometry.cpp:240-241: the reference keeps the threshold in a float
	double localizeThreshold() const
	{
		const float threshold = static_cast<float>(1.0 - std::cos(std::atan2(params_.reprojectionError, 200.)));
		return static_cast<double>(threshold);
	}

	// visual_odometry.cpp:52-104 without the log; the ground truth only when it was asked for
	void newKeyframeCandidate(Keyframe& keyframe)
	{
		Match match;
		const bool needed = isNewKeyframeNeeded(keyframe, match);
		match_ = match;
		if (!needed)
		{
			withoutAdd_++;
			return;
		}
		if (useGroundTruth_)
		{
			const auto poseGt = syncGtAndImage(keyframe.timestamp);
			if (poseGt.has_value())
			{
				if (gt_.empty())
				{
					zeroGt_ = poseGt.value();
				}
				gt_[static_cast<size_t>(keyframe.timestamp.count())] = zeroGt_.inverse() * poseGt.value();
				gtAligned_.push_back(zeroGt_.inverse() * poseGt.value());
			}
		}
		deleteKeyframe();
		addKeyframe(keyframe, match);
		if (optimizer_)
		{
			optimizer_(activeFrames_, mapLandmarks_);
		}
		if (deviceMapMaintenance_)
		{
			lastMapMaintenance_ = maintainMap(ctx_, calibration_, mapMaintenance_, activeFrames_, mapLandmarks_);
		}
		if (deviceAlignment_)
		{
			alignToGroundTruth();
		}
		if (!relativeDeltas_.empty())
		{
			evaluateRelativeErrors();
		}
	}

	// stored and active keyframes against their synced ground-truth poses, pose by pose, in alignToGroundTruth's order
	void evaluateRelativeErrors()
	{
		if (gt_.empty())
		{
			return;
		}
		std::vector<common::Pose3d> reference, cameras;
		const auto pair = [&](const Keyframe& kf) {
			const auto it = gt_.find(static_cast<size_t>(kf.timestamp.count()));
			if (it != gt_.end())
			{
				reference.push_back(it->second);
				cameras.push_back(kf.pose);
			}
		};
		for (const auto& kf : storedFrames_)
		{
			pair(kf);
		}
		for (const auto& kf : activeFrames_)
		{
			pair(kf.second);
		}
		relativeAligned_ = lastAlignment_.status == 0;
		relativeScale_ = relativeAligned_ ? lastAlignment_.sim.scale : 1.0;
		lastRelativeErrors_ = relativePoseErrors(ctx_, reference, cameras, relativeDeltas_, relativeScale_);
	}

	// visual_odometry.cpp:78-97: stored and active keyframes against their synced ground-truth poses, by their centres
	void alignToGroundTruth()
	{
		if (storedFrames_.size() + activeFrames_.size() <= 5 || gt_.empty())
		{
			return;
		}
		std::vector<common::Vector3d> reference, cameras;
		const auto pair = [&](const Keyframe& kf) {
			const auto it = gt_.find(static_cast<size_t>(kf.timestamp.count()));
			if (it != gt_.end())
			{
				reference.push_back(it->second.translation());
				cameras.push_back(kf.pose.translation());
			}
		};
		for (const auto& kf : storedFrames_)
		{
			pair(kf);
		}
		for (const auto& kf : activeFrames_)
		{
			pair(kf.second);
		}
		lastAlignment_ = alignPoints(ctx_, reference, cameras);
		const common::Sim3 back = lastAlignment_.sim.inverse();
		gtAligned_.clear();
		for (const auto& kf : gt_)
		{
			gtAligned_.push_back(back * kf.second);
		}
	}

	MapLandmarks const& getMapLandmarks() { return mapLandmarks_; }
	std::map<size_t, Keyframe> const& getActiveFrames() const { return activeFrames_; }
	std::list<Keyframe> const& getStoredFrames() const { return storedFrames_; }
	std::vector<std::pair<tracker::TrackId, common::Vector3d>> const& getStoredLandmarks() const { return storedLandmarks_; }

	// visual_odometry.cpp:106-154, branch for branch: it returns true on every path after the second keyframe, the
	// fall-back branch appends to match.inliers without clearing them, and initCameras is tried against the LAST
	// active frame
	bool isNewKeyframeNeeded(Keyframe& keyframe, Match& match)
	{
		if (activeFrames_.empty())
		{
			keyframe.pose = common::Pose3d();
			for (const auto& lm : keyframe.getLandmarks())
			{
				match.inliers.emplace_back(lm.first);
			}
			return true;
		}
		if (activeFrames_.size() == 1)
		{
			if (initCameras(keyframe, match))
			{
				return true;
			}
			return false;
		}
		localizeCamera(keyframe, match);
		keyframe.pose = match.Tw2c;
		if (match.inliers.size() > params_.numOfInliers)
		{
			return true;
		}
		else if (initCameras(keyframe, match))
		{
			return true;
		}
		else if (params_.maxNumWithoutAdd > withoutAdd_)
		{
			match.Tw2c = activeFrames_.rbegin()->second.pose;
			for (const auto& lm : keyframe.getLandmarks())
			{
				match.inliers.emplace_back(lm.first);
			}
			return true;
		}
		return true;
	}

	// visual_odometry.cpp:176-210: two-view RANSAC against the last active frame
	bool initCameras(Keyframe& keyframe, Match& match)
	{
		const Keyframe startKeyframe = activeFrames_.rbegin()->second;
		return twoView_.initCameras(startKeyframe, keyframe, match);
	}

	// visual_odometry.cpp:212-286.  A RANSAC that finds nothing leaves match with no inliers and Tw2c untouched.
	void localizeCamera(const Keyframe& keyframe, Match& match)
	{
		match.inliers.clear();
		last_ = ebo_two_view_result{};
		std::vector<tracker::TrackId> trackIds;
		for (const auto& landmark : keyframe.getLandmarks())
		{
			if (mapLandmarks_.landmarks.find(landmark.first) != mapLandmarks_.landmarks.end())
			{
				trackIds.push_back(landmark.first);
			}
		}
		std::sort(trackIds.begin(), trackIds.end());
		std::vector<common::Vector2d> corners;
		std::vector<common::Vector3d> points;
		corners.reserve(trackIds.size());
		points.reserve(trackIds.size());
		for (const tracker::TrackId track : trackIds)
		{
			corners.push_back(keyframe.getLandmarks().at(track));
			points.push_back(mapLandmarks_.landmarks.at(track));
		}
		const bearingVectors_t bearingVectors = cameraModel_.unprojectBatch(ctx_, corners);
		const int n = static_cast<int>(trackIds.size());
		const int offsets[2] = {0, n};
		std::vector<int> inlierIdx(static_cast<size_t>(n) + 1);
		const double threshold = localizeThreshold();
		ransac_.threshold = threshold;
		detail::check(ctx_,
					  ebo_absolute_pose_ransac(ctx_, 1, offsets, detail::packed(bearingVectors), detail::packed(points), &ransac_, &last_,
											   inlierIdx.data(), nullptr, nullptr, nullptr),
					  "localizeCamera");
		if (!last_.found)
		{
			return;
		}
		inlierIdx.resize(static_cast<size_t>(last_.n_inliers));
		common::Pose3d model(&last_.model[0][0]);
		if (localizeRefinement_)
		{
			model = localizeRefinement_(model, bearingVectors, points, inlierIdx);
		}
		match.Tw2c = model;
		double m[12];
		model.toArray(m);
		std::vector<uint8_t> flags(static_cast<size_t>(n));
		detail::check(ctx_,
					  ebo_absolute_pose_scores(ctx_, m, n, detail::packed(bearingVectors), detail::packed(points), threshold, nullptr,
											   flags.data()),
					  "localizeCamera");
		for (int i = 0; i < n; ++i)
		{
			if (flags[i])
			{
				match.inliers.emplace_back(trackIds[i]);
			}
		}
	}

	// visual_odometry.cpp:156-163
	void addKeyframe(const Keyframe& keyframe, const Match& match)
	{
		withoutAdd_ = 0;
		activeFrames_[static_cast<size_t>(keyframe.timestamp.count())] = keyframe;
		addNewLandmarks(keyframe, match);
	}

	// visual_odometry.cpp:165-174
	void deleteKeyframe()
	{
		if (activeFrames_.size() > params_.numOfActiveFrames)
		{
			storedFrames_.push_back(activeFrames_.begin()->second);
			deleteLandmarks(activeFrames_.begin()->second);
			activeFrames_.erase(activeFrames_.begin());
		}
	}

	// visual_odometry.cpp:343-377: every inlier gains this keyframe as an observer; a track whose list has just reached
	// two is triangulated from its two observers' poses and corners, all such tracks in one call with a pose pair each
	void addNewLandmarks(const Keyframe& keyframe, const Match& match)
	{
		std::vector<tracker::TrackId> fresh;
		std::vector<int> posePair;
		std::vector<common::Vector2d> corners1, corners2;
		std::map<size_t, int> poseIndex;
		std::vector<double> poses;
		const auto indexOf = [&](size_t kId) {
			const auto it = poseIndex.find(kId);
			if (it != poseIndex.end())
			{
				return it->second;
			}
			const int idx = static_cast<int>(poseIndex.size());
			poseIndex[kId] = idx;
			poses.resize(poses.size() + 12);
			activeFrames_.at(kId).pose.toArray(poses.data() + 12 * static_cast<size_t>(idx));
			return idx;
		};
		for (const tracker::TrackId landmark : match.inliers)
		{
			std::list<size_t>& seen = mapLandmarks_.observations[landmark];
			seen.push_back(static_cast<size_t>(keyframe.timestamp.count()));
			if (seen.size() == 2)
			{
				const size_t kId1 = seen.front(), kId2 = seen.back();
				posePair.push_back(indexOf(kId1));
				posePair.push_back(indexOf(kId2));
				corners1.push_back(activeFrames_.at(kId1).getLandmarks().at(landmark));
				corners2.push_back(activeFrames_.at(kId2).getLandmarks().at(landmark));
				fresh.push_back(landmark);
			}
		}
		if (fresh.empty())
		{
			return;
		}
		const bearingVectors_t vectors1 = cameraModel_.unprojectBatch(ctx_, corners1);
		const bearingVectors_t vectors2 = cameraModel_.unprojectBatch(ctx_, corners2);
		std::vector<common::Vector3d> positions(fresh.size());
		detail::check(ctx_,
					  ebo_triangulate(ctx_, static_cast<int>(poseIndex.size()), poses.data(), static_cast<int>(fresh.size()), posePair.data(),
									  detail::packed(vectors1), detail::packed(vectors2), positions[0].data()),
					  "addNewLandmarks");
		for (size_t i = 0; i < fresh.size(); ++i)
		{
			mapLandmarks_.landmarks[fresh[i]] = positions[i];
		}
	}

	// visual_odometry.cpp:379-414: the keyframe leaves every observation list; a track nobody observes any more leaves
	// the map, its landmark (if it had one) going to the stored ones
	void deleteLandmarks(const Keyframe& keyframe)
	{
		for (const auto& landmarks : keyframe.getLandmarks())
		{
			const auto it = mapLandmarks_.observations.find(landmarks.first);
			if (it != mapLandmarks_.observations.end())
			{
				const auto obsIt = std::find(it->second.begin(), it->second.end(), static_cast<size_t>(keyframe.timestamp.count()));
				if (obsIt != it->second.end())
				{
					it->second.erase(obsIt);
				}
			}
		}
		std::vector<tracker::TrackId> unseen;
		for (const auto& obs : mapLandmarks_.observations)
		{
			if (obs.second.size() == 0)
			{
				unseen.push_back(obs.first);
			}
		}
		std::sort(unseen.begin(), unseen.end());
		for (const tracker::TrackId track : unseen)
		{
			const auto lmIt = mapLandmarks_.landmarks.find(track);
			if (lmIt != mapLandmarks_.landmarks.end())
			{
				storedLandmarks_.emplace_back(*lmIt);
				mapLandmarks_.landmarks.erase(lmIt);
			}
			mapLandmarks_.observations.erase(track);
		}
	}

   private:
	ebo_ctx* ctx_;
	common::CameraModelParams<double> calibration_;
	common::CameraModel<double> cameraModel_;
	VisualOdometryParams params_;
	TwoViewInitializer twoView_;
	ebo_two_view_params ransac_;
	ebo_two_view_result last_{};
	LocalizeRefinement localizeRefinement_;
	Optimizer optimizer_;
	ebo_summary lastBundle_{};
	ebo_summary lastRefinement_{};

	std::map<size_t, Keyframe> activeFrames_;
	std::list<Keyframe> storedFrames_;
	MapLandmarks mapLandmarks_;
	std::vector<std::pair<tracker::TrackId, common::Vector3d>> storedLandmarks_;
	size_t withoutAdd_ = 0;
	Match match_;

	bool useGroundTruth_ = false;
	bool deviceAlignment_ = false;
	common::GroundTruth groundTruthSamples_;
	std::map<size_t, common::Pose3d> gt_;  // by keyframe timestamp, relative to the first synced pose
	std::vector<common::Pose3d> gtAligned_;
	common::Pose3d zeroGt_;
	Alignment lastAlignment_;
	std::vector<int> relativeDeltas_;
	std::vector<RelativeErrors> lastRelativeErrors_;
	double relativeScale_ = 1.0;
	bool relativeAligned_ = false;
	bool deviceMapMaintenance_ = false;
	MapMaintenanceParams mapMaintenance_;
	MapMaintenanceSummary lastMapMaintenance_;
};
}  // namespace visual_odometry
