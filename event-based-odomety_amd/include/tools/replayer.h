// tools/replayer.h — tools::Replayer (tools/replayer/include/replayer/replayer.h, src/replayer.cpp) over a whole
// DAVIS240C recording: events and decoded frames, merged by time.
//
//   auto rec = std::make_shared<tools::Davis240cRecording>(dir);
//   tools::Replayer replayer(rec);
//   replayer.addEventCallback(...); replayer.addImageCallback(...);   // const common::EventSample& / ImageSample&
//   while (!replayer.finished()) replayer.next();
//
// The merge and tie rules are tools::StreamPump's (event_pump.h), which are the reference's: next() delivers the earlier
// of the next event and the next image, the image on a tie; nextInterval(d) plays until d has passed since the first
// sample it delivered; nextImage() plays up to and including the next image; finished() = the events ran out (a next()
// found none left) or no image is left.  Events are read EVENT_LENGTH at a time (Davis240cReader::getEvents); a frame
// is decoded when it is delivered, not up front.  getGroundTruth() is groundtruth.txt (empty without one, as the
// reference's constructor catches the reader's error); like the reference, the replayer registers ground-truth
// callbacks but never calls them.
#pragma once

#include <functional>
#include <memory>
#include <optional>
#include <stdexcept>
#include <vector>

#include "../dataset_reader/davis240c_recording.h"

namespace tools
{
class Replayer
{
   public:
	explicit Replayer(std::shared_ptr<Davis240cRecording> reader) : reader_(std::move(reader))
	{
		if (!reader_)
		{
			throw std::runtime_error("tools::Replayer: no recording");
		}
		images_ = reader_->getImageStamps();
		try
		{
			groundTruth_ = reader_->getGroundTruth();
		}
		catch (const std::runtime_error&)
		{
			groundTruth_.clear();  // replayer.cpp:24-31: "No Ground truth"
		}
		reset();
	}

	void reset()
	{
		events_ = std::make_unique<Davis240cReader>(reader_->path());  // the events from the start of events.txt
		chunk_.clear();
		eventIt_ = 0;
		imageIt_ = 0;
		hasEvents_ = loadEvents();
		lastTimestamp_ = common::timestamp_t(0);
		imageArrived_ = false;
	}

	bool finished() const { return !hasEvents_ || imageIt_ == images_.size(); }

	void addGroundTruthCallback(std::function<void(const common::GroundTruthSample&)> callback)
	{
		groundTruthCallbacks_.push_back(std::move(callback));
	}
	void addEventCallback(std::function<void(const common::EventSample&)> callback)
	{
		eventCallbacks_.push_back(std::move(callback));
	}
	void addImageCallback(std::function<void(const common::ImageSample&)> callback)
	{
		imageCallbacks_.push_back(std::move(callback));
	}

	void next()
	{
		step(
			[this](const common::EventSample& e) {
				for (auto& cb : eventCallbacks_)
				{
					cb(e);
				}
			},
			[this](const common::ImageSample& image) {
				for (auto& cb : imageCallbacks_)
				{
					cb(image);
				}
			});
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
		while (!imageArrived_ && (hasEvents_ || imageIt_ < images_.size()))
		{
			next();
		}
	}

	// Not in the reference: what `while (!finished()) next();` would deliver up to and including the next image,
	// without calling the callbacks -- the events into `events` (appended, in order), the image (decoded) into
	// `image` (empty when the replay finished before one).  tools::Evaluator::replay feeds the tracker this way.
	void nextChunk(std::vector<common::EventSample>& events, std::optional<common::ImageSample>& image)
	{
		image.reset();
		while (!finished() && !image)
		{
			step([&events](const common::EventSample& e) { events.push_back(e); },
				 [&image](const common::ImageSample& s) { image = s; });
		}
	}

	common::timestamp_t getLastTimestamp() const { return lastTimestamp_; }
	const common::GroundTruth& getGroundTruth() const { return groundTruth_; }

   private:
	// the next EVENT_LENGTH events of events.txt into chunk_; false at the end of the file
	bool loadEvents()
	{
		auto events = events_->getEvents();
		if (!events.has_value())
		{
			chunk_.clear();
			return false;
		}
		chunk_.assign(events->begin(), events->end());
		eventIt_ = 0;
		return true;
	}

	// replayer.cpp:56-98 with StreamPump's guards
	template <class OnEvent, class OnImage>
	void step(OnEvent&& onEvent, OnImage&& onImage)
	{
		if (hasEvents_ && eventIt_ == chunk_.size())
		{
			hasEvents_ = loadEvents();  // the reader's next chunk, or none (replayer.cpp:58-71)
		}
		const bool haveEvent = hasEvents_ && eventIt_ < chunk_.size(), haveImage = imageIt_ < images_.size();
		if (haveEvent && (!haveImage || chunk_[eventIt_].timestamp < images_[imageIt_].timestamp))
		{
			lastTimestamp_ = chunk_[eventIt_].timestamp;
			onEvent(chunk_[eventIt_]);
			++eventIt_;
		}
		else if (haveImage)
		{
			lastTimestamp_ = images_[imageIt_].timestamp;
			imageArrived_ = true;
			onImage(reader_->getImage(images_[imageIt_]));  // decoded on delivery
			++imageIt_;
		}
	}

	std::shared_ptr<Davis240cRecording> reader_;
	std::unique_ptr<Davis240cReader> events_;
	std::vector<Davis240cRecording::ImageStamp> images_;
	common::GroundTruth groundTruth_;
	std::vector<common::EventSample> chunk_;
	size_t eventIt_ = 0, imageIt_ = 0;
	bool hasEvents_ = false, imageArrived_ = false;
	common::timestamp_t lastTimestamp_{0};
	std::vector<std::function<void(const common::GroundTruthSample&)>> groundTruthCallbacks_;
	std::vector<std::function<void(const common::EventSample&)>> eventCallbacks_;
	std::vector<std::function<void(const common::ImageSample&)>> imageCallbacks_;
};

}  // namespace tools
