// recording_test.cpp — tools::Davis240cRecording, tools::Replayer and tools::Evaluator (tools/recording_evaluator.h)
// driven from tests/test_recording_cpu.py and tests/test_gpu_recording.py, which hold the known answers and compare.
//
//   recording_test reader DIR OUTDIR      CPU: images / ground truth / calibration of DIR as one JSON line; the decoded
//                                         frames as OUTDIR/frame_<i>.raw ([h][w] bytes).  A reader error is reported
//                                         in the JSON ("error"), not as a failure of the program.
//   recording_test replay DIR             CPU: the deliveries of tools::Replayer (next / nextImage / nextInterval /
//                                         reset / nextChunk) and of tools::StreamPump on DIR, as JSON.
//   recording_test track DIR OUT callbacks|replay WINDOW_BATCH [tracker|full]
//                                         GPU: tools::Evaluator over tools::Replayer (per-event callbacks or
//                                         Evaluator::replay), results in OUT; one JSON line.
//   recording_test manual DIR OUT FRAMES  GPU: this file's own loop over tracker::FeatureDetector in the evaluator's call
//                                         order (tracker experiment), events from DIR/events.txt, frames from FRAMES
//                                         (records {int64 t_us, int32 w, int32 h, w*h bytes}); results in OUT.
// Built twice by recording.mk: plain, and with -Istubs_opencv (common::Image8 = cv::Mat).
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iomanip>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include <dataset_reader/davis240c_recording.h>
#include <feature_tracker/feature_detector.h>
#include <tools/evaluator.h>
#include <tools/event_pump.h>
#include <tools/recording_evaluator.h>
#include <tools/replayer.h>

static const uint8_t* pixelsOf(const common::Image8& im)
{
#ifdef EBO_HAVE_OPENCV
	return im.data;
#else
	return im.data.data();
#endif
}

static std::string jsonString(const std::string& s)
{
	std::string out = "\"";
	for (char c : s)
	{
		if (c == '"' || c == '\\')
		{
			out += '\\';
		}
		if (static_cast<unsigned char>(c) < 0x20)
		{
			char buf[8];
			std::snprintf(buf, sizeof(buf), "\\u%04x", c);
			out += buf;
			continue;
		}
		out += c;
	}
	return out + "\"";
}

static int readerMode(const std::string& dir, const std::string& outDir)
{
	tools::Davis240cRecording rec(dir);
	std::string json = "{";
	try
	{
		const common::ImageSequence images = rec.getImages();
		json += "\"images\": [";
		for (size_t i = 0; i < images.size(); ++i)
		{
			const common::Image8& im = images[i].value;
			const std::string file = outDir + "/frame_" + std::to_string(i) + ".raw";
			std::FILE* fp = std::fopen(file.c_str(), "wb");
			if (!fp || std::fwrite(pixelsOf(im), 1, static_cast<size_t>(im.rows) * im.cols, fp) != static_cast<size_t>(im.rows) * im.cols)
			{
				std::printf("cannot write %s\n", file.c_str());
				return 1;
			}
			std::fclose(fp);
			json += std::string(i ? ", " : "") + "{\"t_us\": " + std::to_string(images[i].timestamp.count()) +
					", \"rows\": " + std::to_string(im.rows) + ", \"cols\": " + std::to_string(im.cols) + "}";
		}
		json += "], ";
	}
	catch (const std::runtime_error& e)
	{
		json += "\"images_error\": " + jsonString(e.what()) + ", ";
	}
	try
	{
		const common::GroundTruth gt = rec.getGroundTruth();
		json += "\"groundtruth\": [";
		for (size_t i = 0; i < gt.size(); ++i)
		{
			const auto m = gt[i].value.matrix();
			char buf[128];
			json += std::string(i ? ", " : "") + "{\"t_us\": " + std::to_string(gt[i].timestamp.count()) + ", \"matrix\": [";
			for (int r = 0; r < 4; ++r)
			{
				for (int c = 0; c < 4; ++c)
				{
					std::snprintf(buf, sizeof(buf), "%s%.17g", (r || c) ? ", " : "", m(r, c));
					json += buf;
				}
			}
			const auto t = gt[i].value.translation();
			std::snprintf(buf, sizeof(buf), "], \"translation\": [%.17g, %.17g, %.17g]}", t(0), t(1), t(2));
			json += buf;
		}
		json += "], ";
	}
	catch (const std::runtime_error& e)
	{
		json += "\"groundtruth_error\": " + jsonString(e.what()) + ", ";
	}
	try
	{
		const common::CameraModelParams<double> c = rec.getCalibration();
		char buf[512];
		std::snprintf(buf, sizeof(buf),
					  "\"calibration\": {\"fx\": %.17g, \"fy\": %.17g, \"cx\": %.17g, \"cy\": %.17g, \"k1\": %.17g, \"k2\": %.17g, "
					  "\"p1\": %.17g, \"p2\": %.17g, \"k3\": %.17g}",
					  c.fx, c.fy, c.cx, c.cy, c.k1, c.k2, c.p1, c.p2, c.k3);
		json += buf;
	}
	catch (const std::runtime_error& e)
	{
		json += "\"calibration_error\": " + jsonString(e.what());
	}
	// the event side is the base class's, unchanged
	size_t events = 0;
	while (auto ev = rec.getEvents())
	{
		events += ev->size();
	}
	json += ", \"events\": " + std::to_string(events) + "}";
	std::printf("%s\n", json.c_str());
	return 0;
}

struct Log
{
	std::string json = "[";
	bool first = true;
	void add(int64_t t, char kind)
	{
		json += std::string(first ? "" : ", ") + "[" + std::to_string(t) + ", \"" + kind + "\"]";
		first = false;
	}
	std::string done() { return json + "]"; }
};

static int replayMode(const std::string& dir)
{
	auto rec = std::make_shared<tools::Davis240cRecording>(dir);
	Log next, nextImage, interval, afterReset, chunks, pumpNext, pumpImage, pumpInterval;
	Log* cur = &next;
	tools::Replayer r(rec);
	r.addEventCallback([&](const common::EventSample& s) { cur->add(s.timestamp.count(), 'E'); });
	r.addImageCallback([&](const common::ImageSample& s) { cur->add(s.timestamp.count(), 'I'); });
	size_t gtCalls = 0;
	r.addGroundTruthCallback([&](const common::GroundTruthSample&) { ++gtCalls; });
	while (!r.finished())
	{
		r.next();
	}
	r.reset();
	cur = &nextImage;
	r.nextImage();
	r.nextImage();
	r.reset();
	cur = &interval;
	r.nextInterval(common::timestamp_t(3));
	r.reset();
	cur = &afterReset;
	r.next();
	r.reset();
	std::string chunkJson = "[";
	while (!r.finished())
	{
		std::vector<common::EventSample> ev;
		std::optional<common::ImageSample> image;
		r.nextChunk(ev, image);
		for (const auto& e : ev)
		{
			chunks.add(e.timestamp.count(), 'E');
		}
		if (image)
		{
			chunks.add(image->timestamp.count(), 'I');
		}
		chunkJson += std::string(chunkJson.size() > 1 ? ", " : "") + std::to_string(ev.size());
	}
	chunkJson += "]";

	Log* pcur = &pumpNext;
	auto makePump = [&]() {
		tools::StreamPump p = tools::StreamPump::fromDirectory(dir);
		p.addEventCallback([&](const common::EventSample& s) { pcur->add(s.timestamp.count(), 'E'); });
		p.addImageCallback([&](const tools::ImageStamp& s) { pcur->add(s.timestamp.count(), 'I'); });
		return p;
	};
	{
		tools::StreamPump p = makePump();
		while (!p.finished())
		{
			p.next();
		}
	}
	{
		pcur = &pumpImage;
		tools::StreamPump p = makePump();
		p.nextImage();
		p.nextImage();
	}
	{
		pcur = &pumpInterval;
		tools::StreamPump p = makePump();
		p.nextInterval(common::timestamp_t(3));
	}
	std::printf("{\"next\": %s, \"nextImage2\": %s, \"nextInterval3\": %s, \"afterReset\": %s, \"chunks\": %s, "
				"\"chunkEvents\": %s, \"pumpNext\": %s, \"pumpNextImage2\": %s, \"pumpNextInterval3\": %s, "
				"\"groundTruth\": %zu, \"groundTruthCallbacks\": %zu}\n",
				next.done().c_str(), nextImage.done().c_str(), interval.done().c_str(), afterReset.done().c_str(),
				chunks.done().c_str(), chunkJson.c_str(), pumpNext.done().c_str(), pumpImage.done().c_str(),
				pumpInterval.done().c_str(), r.getGroundTruth().size(), gtCalls);
	return 0;
}

static int trackMode(const std::string& dir, const std::string& out, const std::string& how, size_t windowBatch,
					 bool trackerExperiment)
{
	tools::EvaluatorParams p;
	p.outputDir = out;
	p.trackerExperiment = trackerExperiment;
	p.windowBatch = windowBatch;
	size_t keyframes = 0;
	size_t windows = 0, images = 0;
	{
		tools::Evaluator evaluator(p, [&](const tracker::Patches&, const common::timestamp_t&) { ++keyframes; });
		tools::Replayer replayer(std::make_shared<tools::Davis240cRecording>(dir));
		if (how == "replay")
		{
			evaluator.replay(replayer);
		}
		else
		{
			replayer.addEventCallback([&](const common::EventSample& s) { evaluator.eventCallback(s); });
			replayer.addImageCallback([&](const common::ImageSample& s) { evaluator.imageCallback(s); });
			while (!replayer.finished())
			{
				replayer.next();
			}
		}
		evaluator.finish();
		windows = evaluator.windows();
		images = evaluator.images();
	}
	std::printf("{\"windows\": %zu, \"images\": %zu, \"keyframes\": %zu}\n", windows, images, keyframes);
	return 0;
}

// The evaluator's call order written out by hand over the FeatureDetector API (tracker experiment): per event addEvent,
// updatePatches, then a full window (>= 300 ms since the last compensation or >= 15000 events held) is compensated,
// integrated and cleared; the first two frames go to newImage; at the end preExit and the two files.  The merge of the
// two streams: an event goes first only when strictly earlier than the next frame; the replay ends once the events
// have run out or no frame is left.
static int manualMode(const std::string& dir, const std::string& out, const std::string& framesFile)
{
	struct Frame
	{
		int64_t t;
		common::Image8 image;
	};
	std::vector<Frame> frames;
	{
		std::FILE* fp = std::fopen(framesFile.c_str(), "rb");
		if (!fp)
		{
			std::printf("cannot open %s\n", framesFile.c_str());
			return 1;
		}
		int64_t t = 0;
		int32_t wh[2];
		while (std::fread(&t, 8, 1, fp) == 1 && std::fread(wh, 4, 2, fp) == 2)
		{
			std::vector<uint8_t> px(static_cast<size_t>(wh[0]) * wh[1]);
			if (std::fread(px.data(), 1, px.size(), fp) != px.size())
			{
				std::printf("truncated %s\n", framesFile.c_str());
				return 1;
			}
			frames.push_back({t, common::makeImage8(wh[1], wh[0], px.data())});
		}
		std::fclose(fp);
	}
	const std::vector<common::EventSample> events = tools::EventPump::readEvents(dir + "/events.txt");
	tracker::DetectorParams dp;
	tracker::FeatureDetector d(dp);
	d.useDeviceFrontEnd();
	size_t ei = 0, fi = 0, windows = 0, seen = 0;
	bool eventsLeft = !events.empty();
	while (eventsLeft && fi < frames.size())
	{
		if (ei == events.size())
		{
			eventsLeft = false;
		}
		if (ei < events.size() && events[ei].timestamp.count() < frames[fi].t)
		{
			const common::EventSample& e = events[ei++];
			d.addEvent(e);
			d.updatePatches(e);
			if ((e.timestamp - d.getLastCompensation()).count() >= 300000 || d.getEvents().size() >= 15000)
			{
				d.compensateEventsContrast(d.getEvents());
				d.integrateEvents(d.getEvents());
				d.clearEvents();
				++windows;
			}
		}
		else
		{
			const Frame& f = frames[fi++];
			if (++seen <= 2)
			{
				d.newImage(common::ImageSample(f.image, common::timestamp_t(f.t)));
			}
		}
	}
	d.preExit();
	tools::saveFeaturesTrajectory(d.getArchivedPatches(), out + "/trajectory.txt");
	std::ofstream costs(out + "/final_cost.txt");
	for (const tracker::OptimizerFinalLoss& c : d.getOptimizedFinalCosts())
	{
		costs << c.trackId << ' ' << std::fixed << std::setprecision(8) << c.lossValue << ' ' << c.timeStampMicrosecond << '\n';
	}
	std::printf("{\"windows\": %zu, \"images\": %zu, \"events\": %zu}\n", windows, seen, ei);
	return 0;
}

int main(int argc, char** argv)
{
	const std::string mode = argc > 1 ? argv[1] : "";
	try
	{
		if (mode == "reader" && argc == 4)
		{
			return readerMode(argv[2], argv[3]);
		}
		if (mode == "replay" && argc == 3)
		{
			return replayMode(argv[2]);
		}
		if (mode == "track" && (argc == 6 || argc == 7))
		{
			return trackMode(argv[2], argv[3], argv[4], std::strtoul(argv[5], nullptr, 10),
							 argc == 6 || std::string(argv[6]) == "tracker");
		}
		if (mode == "manual" && argc == 5)
		{
			return manualMode(argv[2], argv[3], argv[4]);
		}
	}
	catch (const std::exception& e)
	{
		std::printf("exception: %s\n", e.what());
		return 1;
	}
	std::printf("usage: %s reader DIR OUTDIR | replay DIR | track DIR OUT callbacks|replay WINDOW_BATCH [tracker|full] | "
				"manual DIR OUT FRAMES\n",
				argv[0]);
	return 2;
}
