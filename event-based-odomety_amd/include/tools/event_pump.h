// tools/event_pump.h — the event side of tools::Evaluator and tools::Replayer, reduced to
// what drives the motion-compensation path:
//   * tools::EvaluatorParams::{compensationFrequencyTime 300000 us, compensationFrequencyEvents
//     15000} (tools/evaluator/include/evaluator/evaluator.h:21-22);
//   * tools::Evaluator::eventCallback (tools/evaluator/src/evaluator.cpp:32-45):
//       addEvent -> [updatePatches: frame-based tracker, out of scope] ->
//       if (ts - lastCompensation >= time || events >= count)
//           compensateEventsContrast(getEvents()); integrateEvents(getEvents()); clearEvents();
//   * reading events.txt (Davis240cReader) and pumping them in timestamp order
//     (Replayer::next without the image stream).
// This is the plumbing of BASELINE config 1; it computes nothing itself.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <functional>
#include <memory>
#include <stdexcept>
#include <string>
#include <vector>

#include "../feature_tracker/angular_velocity.h"
#include "../feature_tracker/feature_detector.h"
#include "../visual_odometry/depth_mapper.h"
#include "../visual_odometry/map_tracker.h"

namespace tools
{
struct EvaluatorParams
{
	tracker::Size imageSize = {240, 180};
	// where tools::Evaluator writes trajectory.txt and final_cost.txt (tools/recording_evaluator.h)
	std::string outputDir = "/tmp";
	bool drawImages = false;
	// compensate whole image each k microseconds
	uint32_t compensationFrequencyTime = 300000;
	uint32_t compensationFrequencyEvents = 15000;
	// tools::Evaluator::imageCallback: trackerExperiment = only the first two images reach the detector;
	// visOdometryExperiment = the patches come from Evaluator::setPatches, not from the detector
	bool trackerExperiment = false;
	bool visOdometryExperiment = false;
	// Windows compensated together (EventPump, not in the reference).  1: every window is compensated when it fires,
	// as in the reference.  > 1: a window that fires is queued; when windowBatch are queued (and at the end of
	// replay() / on flush()) ONE batched device call compensates them all (FeatureDetector::compensateWindows), then
	// the callback runs for every window in order with the detector holding that window's results.  Use it when
	// nothing has to read a window's results before the next event arrives ("Recordings").
	size_t windowBatch = 1;
	// the recording's calibration (tools/evaluator/include/evaluator/evaluator.h:18); all zero = none given
	common::CameraModelParams<double> cameraModelParams;
	// true: EventPump / Evaluator install cameraModelParams as the detector's rectification on construction
	// (FeatureDetector::setRectification: events are undistorted as they are loaded).  With all-zero parameters
	// that is an error through the detector's error policy, not a silent no-op.
	bool rectifyEvents = false;
	// true (implies rectifyEvents): frames are rectified too (FeatureDetector::rectifyFrames), into rectifiedCamera;
	// tracker, image front end and compensation then share one pinhole geometry.  An all-zero rectifiedCamera means
	// the one fitted to the sensor (common::fitRectifiedCamera), which keeps every corner in view.
	bool rectifyFrames = false;
	common::CameraModelParams<double> rectifiedCamera;
	// true: the camera's angular velocity is estimated on every compensation window (tracker::AngularVelocityEstimator,
	// feature_tracker/angular_velocity.h) from the events the compensation has just loaded -- no second upload; with
	// windowBatch > 1 one batched solve per flushed queue.  The camera is the rectified one when events are rectified,
	// else cameraModelParams when it has no distortion; otherwise the pump refuses at construction (rectifyEvents).
	bool estimateAngularVelocity = false;
	ebo_rotation_params rotationParams = tracker::defaultRotationParams();
	ebo_rot_solver_opts rotationSolver = tracker::defaultRotationSolver();
	// true: every compensation window votes into ONE space-sweep depth volume (visual_odometry::DepthMapper,
	// visual_odometry/depth_mapper.h) from the events the compensation has just loaded -- no second upload; with
	// windowBatch > 1 on the batch context, one call per flushed queue.  depthPoses is the pose source (timed poses, camera
	// to world, ascending), depthReferenceTime the time of the reference view, inside their span; a window whose reference
	// time lies outside it is left out.  The camera is chosen as for estimateAngularVelocity.
	bool depthMap = false;
	ebo_depth_params depthParams = visual_odometry::defaultDepthParams();
	common::GroundTruth depthPoses;
	common::timestamp_t depthReferenceTime{0};
	// true (needs depthMap): one pass over the recording maps and then tracks.  Windows whose reference time is before
	// trackMapSplit are voted into the volume as above; at the first window at or past it the map is extracted, and that
	// window and every later one is tracked against it (visual_odometry::MapTracker, visual_odometry/map_tracker.h) instead
	// of voted, chained from depthPoses' pose at the split, with trackStarts (1 or 13) starts a window.
	bool trackMap = false;
	common::timestamp_t trackMapSplit{0};
	int trackStarts = 1;
};

class EventPump
{
   public:
	// called after every compensation with the detector holding that window's results
	using WindowCallback = std::function<void(tracker::FeatureDetector&, size_t /*events in window*/)>;

	EventPump(tracker::FeatureDetector& tracker, const EvaluatorParams& params = EvaluatorParams())
		: tracker_(tracker), params_(params)
	{
		if (params_.rectifyFrames)
		{
			common::CameraModelParams<double> r = params_.rectifiedCamera;
			if (r.fx == 0 && r.fy == 0 && r.cx == 0 && r.cy == 0)
			{
				// a calibration the fit refuses leaves r all zero, which setRectification reports through the error policy
				const ebo_camera cam = common::toEboCamera(params_.cameraModelParams);
				ebo_camera fitted{};
				if (tracker_.handle() && ebo_fit_rectified_camera(tracker_.handle(), &cam, &fitted) == EBO_OK)
				{
					r.fx = fitted.fx;
					r.fy = fitted.fy;
					r.cx = fitted.cx;
					r.cy = fitted.cy;
				}
			}
			tracker_.setRectification(params_.cameraModelParams, r);
			if (tracker_.rectifying())
			{
				tracker_.rectifyFrames(true);
			}
		}
		else if (params_.rectifyEvents)
		{
			tracker_.setRectification(params_.cameraModelParams);
		}
		if (params_.estimateAngularVelocity)
		{
			rotation_.reset(new tracker::AngularVelocityEstimator(
				tracker::AngularVelocityEstimator::cameraFor(tracker_.handle(), params_.cameraModelParams), params_.rotationParams,
				params_.rotationSolver));
		}
		if (params_.depthMap)
		{
			depth_.reset(new visual_odometry::DepthMapper(
				visual_odometry::DepthMapper::cameraFor(tracker_.handle(), params_.cameraModelParams), params_.depthPoses, params_.depthParams));
			depth_->begin(params_.depthReferenceTime);
		}
	}

	void onWindow(WindowCallback cb) { onWindow_ = std::move(cb); }

	// tools::Evaluator::eventCallback
	void eventCallback(const common::EventSample& sample)
	{
		tracker_.addEvent(sample);
		closeWindowIfDue(sample);
	}

	// the window rule alone, for a caller that has handed `sample` to addEvent itself (tools::Evaluator calls
	// updatePatches in between, as the reference's eventCallback does)
	void closeWindowIfDue(const common::EventSample& sample)
	{
		if ((sample.timestamp - tracker_.getLastCompensation()).count() >=
				static_cast<long long>(params_.compensationFrequencyTime) ||
			tracker_.getEvents().size() >= params_.compensationFrequencyEvents)
		{
			if (params_.windowBatch > 1)
			{
				queueWindow(sample);
				return;
			}
			const size_t n = tracker_.getEvents().size();
			tracker_.compensateEventsContrast(tracker_.getEvents());
			tracker_.integrateEvents(tracker_.getEvents());
			if (rotation_)
			{
				// the window integrateEvents has just loaded is resident in the detector's context
				appendEstimates(rotation_->estimate(tracker_.handle()));
			}
			if (depth_)
			{
				voteOrTrack(tracker_.handle());
			}
			if (onWindow_)
			{
				onWindow_(tracker_, n);
			}
			tracker_.clearEvents();
			++windows_;
		}
	}

	// Replayer: deliver every event of a recording in order (and, batched, compensate what is queued at the end).
	void replay(const std::vector<common::EventSample>& events)
	{
		for (const auto& e : events)
		{
			eventCallback(e);
		}
		flush();
	}

	// windowBatch > 1: compensate the queued windows now and run their callbacks in order.  The queue is emptied
	// first: under DetectorParams::ERRORS_THROW a refused window throws from here after the callbacks of the windows
	// before it, and the windows after it in the batch are dropped.  Nothing to do with windowBatch = 1.
	void flush()
	{
		if (queueOffsets_.size() < 2)
		{
			return;
		}
		std::vector<ebo_event> events;
		std::vector<size_t> offsets;
		events.swap(queueEvents_);
		offsets.swap(queueOffsets_);
		queueOffsets_.assign(1, 0);
		queueEvents_.reserve(events.capacity());
		tracker_.compensateWindows(events, offsets, params_.windowBatch, [&](size_t w) {
			if (onWindow_)
			{
				onWindow_(tracker_, offsets[w + 1] - offsets[w]);
			}
			++windows_;
		});
		if (rotation_)
		{
			// One batched compensation normally leaves exactly these windows resident in the batch context.  A queue that
			// the compensation had to split (windowBatch above FeatureDetector::kMaxBatchWindows, max_events) or that lost
			// a window is estimated chunk by chunk from a second load; a window the loader refuses alone gets an entry with
			// status EBO_ROT_RUNNING and no estimate, so a run the compensation tolerated is not ended here.
			ebo_ctx* batch = tracker_.batchHandle();
			int resident = 0;
			const int nw = static_cast<int>(offsets.size() - 1);
			if (batch && ebo_num_windows(batch, &resident) == EBO_OK && resident == nw)
			{
				appendEstimates(rotation_->estimate(batch));
			}
			else
			{
				appendEstimates(rotation_->estimateWindows(
					batch, events, offsets, std::min(params_.windowBatch, tracker::FeatureDetector::kMaxBatchWindows)));
			}
		}
		if (depth_)
		{
			// as above: the batch context holds exactly the queue's windows, or they are loaded again chunk by chunk
			ebo_ctx* batch = tracker_.batchHandle();
			int resident = 0;
			if (batch && ebo_num_windows(batch, &resident) == EBO_OK && resident == static_cast<int>(offsets.size() - 1))
			{
				voteOrTrack(batch);
			}
			else if (params_.trackMap)
			{
				// window by window: a window the loader refuses alone is neither voted nor tracked
				for (size_t w = 0; w + 1 < offsets.size(); ++w)
				{
					const size_t one[2] = {0, offsets[w + 1] - offsets[w]};
					if (batch && ebo_set_windows(batch, events.data() + offsets[w], one, 1) == EBO_OK)
					{
						voteOrTrack(batch);
					}
				}
			}
			else
			{
				depth_->addWindows(batch, events, offsets, std::min(params_.windowBatch, tracker::FeatureDetector::kMaxBatchWindows));
			}
		}
	}
	// EvaluatorParams::estimateAngularVelocity: one estimate per compensated window, in order
	const std::vector<tracker::AngularVelocityEstimate>& angularVelocities() const { return angularVelocities_; }
	// EvaluatorParams::depthMap: the depth map of everything voted so far (queued windows are flushed first); the volume
	// is closed, and the windows the mapper saw stay readable through depthWindows()
	visual_odometry::DepthMap finishDepthMap()
	{
		if (!depth_)
		{
			throw std::runtime_error("tools::EventPump: EvaluatorParams::depthMap is not set");
		}
		flush();
		return mapTracker_ ? trackedMap_ : depth_->finish();  // trackMap: the map the tracker was given at the split
	}
	// EvaluatorParams::trackMap: one entry per tracked window, in order (empty before the split is reached)
	const std::vector<visual_odometry::MapTrackWindow>& trackedWindows() const
	{
		static const std::vector<visual_odometry::MapTrackWindow> none;
		return mapTracker_ ? mapTracker_->windows() : none;
	}
	const std::vector<visual_odometry::DepthWindow>& depthWindows() const
	{
		static const std::vector<visual_odometry::DepthWindow> none;
		return depth_ ? depth_->windows() : none;
	}
	size_t queuedWindows() const { return queueOffsets_.size() - 1; }

	size_t windows() const { return windows_; }

	// Davis240cReader::getEvents on <dir>/events.txt
	static std::vector<common::EventSample> readEvents(const std::string& path, size_t maxEvents = 1u << 24)
	{
		std::vector<ebo_event> raw(maxEvents);
		size_t n = 0;
		const int rc = ebo_read_events_txt(path.c_str(), raw.data(), raw.size(), &n);
		if (rc != EBO_OK)
		{
			throw std::runtime_error("cannot parse " + path);  // the reference throws on a bad sign
		}
		std::vector<common::EventSample> out(n);
		for (size_t i = 0; i < n; ++i)
		{
			out[i].value.point = {raw[i].x, raw[i].y};
			out[i].value.sign = raw[i].sign > 0 ? common::POSITIVE : common::NEGATIVE;
			out[i].timestamp = common::timestamp_t(raw[i].t_us);
		}
		return out;
	}

	// the packed binary sidecar of the same recording (ebo_write_events_bin): no parsing
	static std::vector<common::EventSample> readEventsBin(const std::string& path, size_t maxEvents = 1u << 24)
	{
		std::vector<ebo_event> raw(maxEvents);
		size_t n = 0;
		if (ebo_read_events_bin(path.c_str(), raw.data(), raw.size(), &n) != EBO_OK)
		{
			throw std::runtime_error("cannot read " + path);
		}
		std::vector<common::EventSample> out(n);
		for (size_t i = 0; i < n; ++i)
		{
			out[i].value.point = {raw[i].x, raw[i].y};
			out[i].value.sign = raw[i].sign > 0 ? common::POSITIVE : common::NEGATIVE;
			out[i].timestamp = common::timestamp_t(raw[i].t_us);
		}
		return out;
	}
	static void writeEventsBin(const std::string& path, const std::vector<common::EventSample>& events)
	{
		const std::vector<ebo_event> raw = common::toEboEvents(events);
		if (ebo_write_events_bin(path.c_str(), raw.data(), raw.size()) != EBO_OK)
		{
			throw std::runtime_error("cannot write " + path);
		}
	}

   private:
	void appendEstimates(const std::vector<tracker::AngularVelocityEstimate>& est)
	{
		angularVelocities_.insert(angularVelocities_.end(), est.begin(), est.end());
	}

	// the windows resident in ctx: voted into the volume, or -- EvaluatorParams::trackMap, from the split on -- tracked
	void voteOrTrack(ebo_ctx* ctx)
	{
		if (!params_.trackMap)
		{
			depth_->addResidentWindows(ctx);
			return;
		}
		const int64_t split = params_.trackMapSplit.count();
		int n = 0, first = 0;
		if (!ctx || ebo_num_windows(ctx, &n) != EBO_OK)
		{
			throw std::runtime_error("tools::EventPump: no context to map or track in");
		}
		for (first = 0; first < n; ++first)
		{
			int64_t tRef = 0;
			uint64_t count = 0;
			if (ebo_window_info(ctx, first, &tRef, &count) != EBO_OK || tRef >= split)
			{
				break;
			}
		}
		if (!mapTracker_)
		{
			depth_->addResidentWindows(ctx, split);
			if (first == n)
			{
				return;
			}
			const auto at = visual_odometry::syncGroundTruth(params_.depthPoses, params_.trackMapSplit);
			if (!at.has_value())
			{
				throw std::runtime_error("tools::EventPump: trackMapSplit lies outside depthPoses' time span");
			}
			trackedMap_ = depth_->finish();
			mapTracker_.reset(new visual_odometry::MapTracker(
				visual_odometry::DepthMapper::cameraFor(ctx, params_.cameraModelParams), trackedMap_.points));
			mapTracker_->starts = params_.trackStarts;
			visual_odometry::DepthMapper::toAbi(at.value(), trackPose_);
		}
		mapTracker_->trackResidentWindows(ctx, first, trackPose_);
	}

	// the batched form of the compensation branch: the held events join the queue, the detector's list is
	// cleared and lastCompensation moves to the window's last timestamp as compensateEventsContrast would move it
	void queueWindow(const common::EventSample& sample)
	{
		for (const auto& e : tracker_.getEvents())
		{
			queueEvents_.push_back(ebo_event{e.value.point.x, e.value.point.y, static_cast<int32_t>(e.value.sign), 0,
											 e.timestamp.count()});  // common::toEboEvents
		}
		queueOffsets_.push_back(queueEvents_.size());
		tracker_.clearEvents();
		tracker_.setLastCompensation(sample.timestamp);
		if (queuedWindows() >= params_.windowBatch)
		{
			flush();
		}
	}

	tracker::FeatureDetector& tracker_;
	EvaluatorParams params_;
	WindowCallback onWindow_;
	size_t windows_ = 0;
	std::vector<ebo_event> queueEvents_;
	std::vector<size_t> queueOffsets_ = std::vector<size_t>(1, 0);
	std::unique_ptr<tracker::AngularVelocityEstimator> rotation_;
	std::vector<tracker::AngularVelocityEstimate> angularVelocities_;
	std::unique_ptr<visual_odometry::DepthMapper> depth_;
	std::unique_ptr<visual_odometry::MapTracker> mapTracker_;
	visual_odometry::DepthMap trackedMap_;
	double trackPose_[12] = {};
};

// tools::Replayer (tools/replayer/src/replayer.cpp:42-131) for the two streams that decide WHEN the
// tracker is called: events and image TIMESTAMPS (the frames themselves belong to the frame-based
// detector, out of scope; an ImageSample here is a timestamp and the file name of images.txt).
// next() delivers the earlier of the next event and the next image (an image wins a tie, :73);
// nextInterval(d) plays until d has passed since the first sample delivered; nextImage() plays up to
// and including the next image; finished() = the events ran out (a next() found none left) or no
// image is left, as in the reference.
enum class EventType
{
	EVENT,
	IMAGE
};
struct ImageStamp
{
	common::timestamp_t timestamp;
	std::string file;
};

class StreamPump
{
   public:
	StreamPump(std::vector<common::EventSample> events, std::vector<ImageStamp> images)
		: events_(std::move(events)), images_(std::move(images))
	{
		hasEvents_ = !events_.empty();
		reset();
	}

	// <dir>/events.txt and <dir>/images.txt ("<seconds> <file>" per line, Davis240cReader::getImages)
	static StreamPump fromDirectory(const std::string& dir)
	{
		std::vector<ImageStamp> images;
		FILE* fp = std::fopen((dir + "/images.txt").c_str(), "rb");
		if (!fp)
		{
			throw std::runtime_error("cannot open " + dir + "/images.txt");
		}
		char line[1024];
		while (std::fgets(line, sizeof(line), fp))
		{
			char* end = nullptr;
			const double sec = std::strtod(line, &end);
			if (end == line)
			{
				continue;
			}
			std::string file(end);
			while (!file.empty() && (file.back() == '\n' || file.back() == '\r' || file.back() == ' '))
			{
				file.pop_back();
			}
			while (!file.empty() && file.front() == ' ')
			{
				file.erase(file.begin());
			}
			images.push_back({common::timestamp_t(static_cast<int64_t>(sec * 1000000.0)), file});
		}
		std::fclose(fp);
		return StreamPump(EventPump::readEvents(dir + "/events.txt"), std::move(images));
	}

	void addEventCallback(std::function<void(const common::EventSample&)> cb) { eventCallbacks_.push_back(std::move(cb)); }
	void addImageCallback(std::function<void(const ImageStamp&)> cb) { imageCallbacks_.push_back(std::move(cb)); }

	bool finished() const { return !hasEvents_ || imageIt_ == images_.size(); }

	void reset()
	{
		eventIt_ = 0;
		imageIt_ = 0;
		hasEvents_ = !events_.empty();
		lastTimestamp_ = common::timestamp_t(0);
		imageArrived_ = false;
	}

	void next()
	{
		if (hasEvents_ && eventIt_ == events_.size())
		{
			hasEvents_ = false;  // the reader has no further chunk (replayer.cpp:58-71)
		}
		const bool haveEvent = eventIt_ < events_.size(), haveImage = imageIt_ < images_.size();
		if (haveEvent && (!haveImage || events_[eventIt_].timestamp < images_[imageIt_].timestamp))
		{
			lastTimestamp_ = events_[eventIt_].timestamp;
			for (auto& cb : eventCallbacks_)
			{
				cb(events_[eventIt_]);
			}
			++eventIt_;
		}
		else if (haveImage)
		{
			lastTimestamp_ = images_[imageIt_].timestamp;
			imageArrived_ = true;
			for (auto& cb : imageCallbacks_)
			{
				cb(images_[imageIt_]);
			}
			++imageIt_;
		}
	}

	void nextInterval(const common::timestamp_t& interval)
	{
		if (finished())
		{
			return;
		}
		next();
		const auto firstTime = lastTimestamp_;
		do
		{
			next();
		} while ((lastTimestamp_ - firstTime) < interval && !finished());
	}

	void nextImage()
	{
		if (finished())
		{
			return;
		}
		imageArrived_ = false;
		while (!imageArrived_ && (eventIt_ < events_.size() || imageIt_ < images_.size()))
		{
			next();
		}
	}

   private:
	std::vector<common::EventSample> events_;
	std::vector<ImageStamp> images_;
	size_t eventIt_ = 0, imageIt_ = 0;
	bool hasEvents_ = false, imageArrived_ = false;
	common::timestamp_t lastTimestamp_{0};
	std::vector<std::function<void(const common::EventSample&)>> eventCallbacks_;
	std::vector<std::function<void(const ImageStamp&)>> imageCallbacks_;
};

}  // namespace tools
