// tools/recording_evaluator.h — tools::Evaluator, the tracker side of the reference's evaluator
// (tools/evaluator/src/evaluator.cpp:10-124,125-150,209-225): a DAVIS recording goes in through tools::Replayer,
// trajectory.txt and final_cost.txt come out.
//
//   tools::EvaluatorParams p;  p.outputDir = out;  p.trackerExperiment = true;
//   tools::Evaluator evaluator(p);
//   tools::Replayer replayer(std::make_shared<tools::Davis240cRecording>(dir));
//   replayer.addEventCallback([&](const common::EventSample& s) { evaluator.eventCallback(s); });
//   replayer.addImageCallback([&](const common::ImageSample& s) { evaluator.imageCallback(s); });
//   while (!replayer.finished()) replayer.next();      // or evaluator.replay(replayer): the same files
//   // ~Evaluator: preExit, <outputDir>/trajectory.txt and <outputDir>/final_cost.txt
//
// The detector is ONE tracker::FeatureDetector built from imageSize / drawImages with the device front end installed
// (useDeviceFrontEnd: ebo_good_features, ebo_image_gradients, ebo_lk_*).  eventCallback is addEvent -> updatePatches ->
// the window rule of tools::EventPump (compensateEventsContrast + integrateEvents + clearEvents, or, with windowBatch
// > 1, queued and compensated in batches; queued windows are flushed before an image is handled, so every call runs in
// the unbatched order).  The visual odometry is not owned here (it stays the user's front end): where the reference
// calls visualOdometry_->newKeyframeCandidate, the keyframe hook receives the patches and the image's timestamp, and
// savePoses / setGroundTruthSamples belong to the VO's owner.  EvaluatorParams has the reference's fields, plus
// windowBatch, rectifyEvents (the events of every window are undistorted with cameraModelParams as they are loaded) and
// rectifyFrames / rectifiedCamera (frames are remapped too, so tracks and corners are in rectified pixels).
#pragma once

#include <cstdio>
#include <fstream>
#include <functional>
#include <iomanip>
#include <memory>
#include <optional>
#include <string>
#include <unordered_map>
#include <vector>

#include "../feature_tracker/feature_detector.h"
#include "evaluator.h"
#include "event_pump.h"
#include "replayer.h"

namespace tools
{
class Evaluator
{
   public:
	// where the reference builds a visual_odometry::Keyframe and calls newKeyframeCandidate (evaluator.cpp:79-103)
	using KeyframeHook = std::function<void(const tracker::Patches&, const common::timestamp_t&)>;

	explicit Evaluator(const EvaluatorParams& params, KeyframeHook onKeyframe = nullptr)
		: params_(params), onKeyframe_(std::move(onKeyframe))
	{
		reset();
	}

	// evaluator.cpp:15-21 without savePoses: the archived patches and the final costs of the oldest optimizer in use.
	// A failure here is reported on stderr (a destructor does not throw); call finish() to have it thrown.
	~Evaluator()
	{
		if (finished_)
		{
			return;
		}
		try
		{
			finish();
		}
		catch (const std::exception& e)
		{
			std::fprintf(stderr, "tools::Evaluator: %s\n", e.what());
		}
	}
	Evaluator(const Evaluator&) = delete;
	Evaluator& operator=(const Evaluator&) = delete;

	// what the destructor does, once: queued windows compensated, preExit, the two files written
	void finish()
	{
		if (finished_)
		{
			return;
		}
		finished_ = true;
		pump_->flush();
		tracker_->preExit();
		saveFeaturesTrajectory(tracker_->getArchivedPatches());
		saveFinalCosts(tracker_->getOptimizedFinalCosts());
		if (params_.estimateAngularVelocity)
		{
			saveAngularVelocities(pump_->angularVelocities());
		}
		if (params_.depthMap)
		{
			depthMap_ = pump_->finishDepthMap();
			saveDepthMap(depthMap_, pump_->depthWindows());
			if (params_.trackMap)
			{
				saveTrackedPoses(pump_->trackedWindows());
			}
		}
	}

	// evaluator.cpp:32-45
	void eventCallback(const common::EventSample& sample)
	{
		++events_;
		tracker_->addEvent(sample);
		tracker_->updatePatches(sample);
		pump_->closeWindowIfDue(sample);
	}

	void groundTruthCallback(const common::GroundTruthSample& /*sample*/) {}

	// evaluator.cpp:51-104
	void imageCallback(const common::ImageSample& sample)
	{
		pump_->flush();
		imageNum_++;
		if (params_.trackerExperiment && imageNum_ > 2)
		{
			return;
		}
		if (!params_.visOdometryExperiment)
		{
			tracker_->newImage(sample);
			corners_ = tracker_->getFeatures();
		}
		else
		{
			const auto it = keyframes_.find(sample.timestamp.count());
			if (it != keyframes_.end())
			{
				patches_ = it->second;
			}
		}
		if (imageNum_ > 2 && onKeyframe_)
		{
			if (!params_.visOdometryExperiment)
			{
				onKeyframe_(tracker_->getPatches(), sample.timestamp);
			}
			else
			{
				const auto it = keyframes_.find(sample.timestamp.count());
				if (it != keyframes_.end())
				{
					onKeyframe_(it->second, sample.timestamp);
				}
			}
		}
	}

	// Not in the reference: the whole recording.  The replayer hands over the events up to each frame as one chunk
	// (Replayer::nextChunk: no callback per event, each frame decoded once) and every event goes through eventCallback.
	// The tracker itself already advances all patches in lock-step rounds over DetectorParams::eventBatch events at a
	// time (updatePatches(event) queues; tracked_patches.h).  Those rounds are deliberately NOT widened to the whole
	// frame interval here: a round appends the final costs of its patches in patch order, so a different grouping
	// reorders the lines of final_cost.txt (each patch's own costs, rects and trajectory stay the same).  Kept at the
	// per-event grouping, both files are byte-identical to those of `while (!replayer.finished()) replayer.next();`.
	void replay(Replayer& replayer)
	{
		std::vector<common::EventSample> chunk;
		std::optional<common::ImageSample> image;
		while (!replayer.finished())
		{
			chunk.clear();
			replayer.nextChunk(chunk, image);
			for (const common::EventSample& e : chunk)
			{
				eventCallback(e);
			}
			if (image)
			{
				imageCallback(*image);
			}
		}
	}

	// evaluator.cpp:106-118 (the VO is the hook's owner's)
	void reset()
	{
		corners_.clear();
		patches_.clear();
		keyframes_.clear();
		tracker::DetectorParams dp;
		dp.drawImages = params_.drawImages;
		dp.imageSize = params_.imageSize;
		pump_.reset();
		tracker_ = std::make_unique<tracker::FeatureDetector>(dp);
		tracker_->useDeviceFrontEnd();
		pump_ = std::make_unique<EventPump>(*tracker_, params_);
		imageNum_ = 0;
		events_ = 0;
		finished_ = false;
	}

	// evaluator.cpp:120-123
	void setTrackerParams(const tracker::DetectorParams& params)
	{
		pump_->flush();
		tracker_->setParams(params);
	}
	void setParams(const EvaluatorParams& params)
	{
		params_ = params;
		pump_->flush();
		pump_ = std::make_unique<EventPump>(*tracker_, params_);
	}
	void setKeyframeHook(KeyframeHook onKeyframe) { onKeyframe_ = std::move(onKeyframe); }

	// evaluator.cpp:125-150: <outputDir>/trajectory.txt, "feature_id timestamp x y"
	void saveFeaturesTrajectory(const tracker::Patches& patches) const
	{
		tools::saveFeaturesTrajectory(patches, params_.outputDir + "/trajectory.txt");
	}
	// evaluator.cpp:209-225: <outputDir>/final_cost.txt, "trackId loss timeStampMicrosecond" (loss fixed, 8 digits)
	void saveFinalCosts(const std::vector<tracker::OptimizerFinalLoss>& vectorFinalCosts) const
	{
		const std::string file = params_.outputDir + "/final_cost.txt";
		std::ofstream costFile(file);
		if (!costFile)
		{
			throw std::runtime_error("tools::Evaluator: cannot write " + file);
		}
		for (const auto& v : vectorFinalCosts)
		{
			costFile << v.trackId << " " << std::fixed << std::setprecision(8) << v.lossValue << " "
					 << v.timeStampMicrosecond << std::endl;
		}
	}

	// Not in the reference: <outputDir>/angular_velocity.txt, one line per compensation window,
	// "t_ref_seconds wx wy wz r_at_zero r iterations status" (rad/s; status EBO_ROT_*)
	void saveAngularVelocities(const std::vector<tracker::AngularVelocityEstimate>& estimates) const
	{
		const std::string file = params_.outputDir + "/angular_velocity.txt";
		FILE* f = std::fopen(file.c_str(), "w");
		if (!f)
		{
			throw std::runtime_error("tools::Evaluator: cannot write " + file);
		}
		for (const auto& e : estimates)
		{
			std::fprintf(f, "%.6f %.17g %.17g %.17g %.17g %.17g %d %d\n", static_cast<double>(e.tRefUs) * 1e-6, e.omega[0], e.omega[1],
						 e.omega[2], e.summary.r_initial, e.summary.r_final, e.summary.iterations, e.summary.status);
		}
		std::fclose(f);
	}
	const std::vector<tracker::AngularVelocityEstimate>& angularVelocities() const { return pump_->angularVelocities(); }

	// Not in the reference: <outputDir>/depth.txt, "x y depth confidence" per kept pixel in row-major order (confidence in
	// votes, 1/1024 of an event each); <outputDir>/points.txt, "X Y Z" of the same pixels in the world frame; and
	// <outputDir>/depth_windows.txt, the reference view first ("reference" and its pose) and then one line per window the
	// mapper saw: "t_ref_us events used" and the pose it was voted with (R row-major, then t; zeros when not used)
	void saveDepthMap(const visual_odometry::DepthMap& map, const std::vector<visual_odometry::DepthWindow>& windows) const
	{
		FILE* fd = std::fopen((params_.outputDir + "/depth.txt").c_str(), "w");
		FILE* fp = std::fopen((params_.outputDir + "/points.txt").c_str(), "w");
		FILE* fw = std::fopen((params_.outputDir + "/depth_windows.txt").c_str(), "w");
		if (!fd || !fp || !fw)
		{
			for (FILE* f : {fd, fp, fw})
			{
				if (f)
				{
					std::fclose(f);
				}
			}
			throw std::runtime_error("tools::Evaluator: cannot write depth.txt, points.txt or depth_windows.txt in " + params_.outputDir);
		}
		size_t k = 0;
		for (int y = 0; y < map.height; ++y)
		{
			for (int x = 0; x < map.width; ++x)
			{
				const size_t p = static_cast<size_t>(y) * map.width + x;
				if (map.index[p] >= 0)
				{
					std::fprintf(fd, "%d %d %.17g %u\n", x, y, map.depth[p], map.confidence[p]);
					const common::Vector3d& q = map.points[k++];
					std::fprintf(fp, "%.17g %.17g %.17g\n", q[0], q[1], q[2]);
				}
			}
		}
		double m[12];
		visual_odometry::DepthMapper::toAbi(map.reference, m);
		std::fprintf(fw, "reference");
		for (const double v : m)
		{
			std::fprintf(fw, " %.17g", v);
		}
		std::fprintf(fw, "\n");
		for (const auto& w : windows)
		{
			visual_odometry::DepthMapper::toAbi(w.pose, m);
			std::fprintf(fw, "%lld %llu %d", static_cast<long long>(w.tRefUs), static_cast<unsigned long long>(w.events), w.used ? 1 : 0);
			for (const double v : m)
			{
				std::fprintf(fw, " %.17g", w.used ? v : 0.0);
			}
			std::fprintf(fw, "\n");
		}
		std::fclose(fd);
		std::fclose(fp);
		std::fclose(fw);
	}
	// Not in the reference (EvaluatorParams::trackMap): <outputDir>/tracked_poses.txt, one line per tracked window: "t_ref_us"
	// and the tracked pose, camera to world (R row-major, then t) -- the pose lines of depth_windows.txt; and
	// <outputDir>/map_track.txt, one line per tracked window: "t_ref_us winner termination iterations num_evals_jac
	// num_evals_cost initial_cost final_cost visible_start visible_final lost" of the window's winner (zeros when lost)
	void saveTrackedPoses(const std::vector<visual_odometry::MapTrackWindow>& windows) const
	{
		FILE* fp = std::fopen((params_.outputDir + "/tracked_poses.txt").c_str(), "w");
		FILE* fm = std::fopen((params_.outputDir + "/map_track.txt").c_str(), "w");
		if (!fp || !fm)
		{
			for (FILE* f : {fp, fm})
			{
				if (f)
				{
					std::fclose(f);
				}
			}
			throw std::runtime_error("tools::Evaluator: cannot write tracked_poses.txt or map_track.txt in " + params_.outputDir);
		}
		for (const auto& w : windows)
		{
			std::fprintf(fp, "%lld", static_cast<long long>(w.tRefUs));
			for (const double v : w.pose)
			{
				std::fprintf(fp, " %.17g", v);
			}
			std::fprintf(fp, "\n");
			const ebo_map_track_result& r = w.result;
			std::fprintf(fm, "%lld %d %d %d %d %d %.17g %.17g %d %d %d\n", static_cast<long long>(w.tRefUs), w.winner, r.termination,
						 r.iterations, r.num_evals_jac, r.num_evals_cost, r.initial_cost, r.final_cost, r.visible_start, r.visible_final,
						 w.lost ? 1 : 0);
		}
		std::fclose(fp);
		std::fclose(fm);
	}
	const std::vector<visual_odometry::MapTrackWindow>& trackedWindows() const { return pump_->trackedWindows(); }

	// after finish(): the map that was written
	const visual_odometry::DepthMap& depthMap() const { return depthMap_; }
	const std::vector<visual_odometry::DepthWindow>& depthWindows() const { return pump_->depthWindows(); }

	// evaluator.cpp:165-171: the patches of a VO run, keyed by their current timestamp
	void setPatches(const tracker::Patches& patches)
	{
		for (const auto& patch : patches)
		{
			keyframes_[patch.getCurrentTimestamp().count()].push_back(patch);
		}
	}

	// evaluator.cpp:23-30
	tracker::Patches const& getPatches() const
	{
		if (params_.visOdometryExperiment)
		{
			return patches_;
		}
		return tracker_->getPatches();
	}
	tracker::Mat64 const& getCompensatedEventImage()
	{
		pump_->flush();
		return tracker_->getCompensatedEventImage();
	}
	tracker::Mat64 const& getIntegratedEventImage()
	{
		pump_->flush();
		return tracker_->getIntegratedEventImage();
	}

	// not in the reference
	tracker::FeatureDetector& detector() { return *tracker_; }
	size_t windows() const { return pump_->windows(); }
	size_t images() const { return imageNum_; }
	size_t events() const { return events_; }
	const EvaluatorParams& params() const { return params_; }

   private:
	EvaluatorParams params_;
	KeyframeHook onKeyframe_;
	std::unique_ptr<tracker::FeatureDetector> tracker_;
	std::unique_ptr<EventPump> pump_;
	std::unordered_map<size_t, tracker::Patches> keyframes_;
	tracker::Corners corners_;
	tracker::Patches patches_;
	size_t imageNum_ = 0;
	size_t events_ = 0;
	bool finished_ = false;
	visual_odometry::DepthMap depthMap_;
};

}  // namespace tools
