// track_recording — the reference's feature-tracking experiment on a DAVIS240C recording directory, without OpenCV:
//
//   track_recording --dataset DIR --out DIR [--tracker-experiment] [--window-batch N] [--rectify]
//
// DIR holds events.txt, images.txt + the frames (8-bit grey PNG), optionally groundtruth.txt / calib.txt.
// --rectify: the events of every compensation window are undistorted with the recording's calib.txt as they are
// loaded (tools::EvaluatorParams::rectifyEvents); frames and tracked patches stay in raw coordinates.  The
// recording is played through tools::Replayer into tools::Evaluator::replay (tools/recording_evaluator.h; the files
// equal those of per-event callbacks).
// Writes OUT/trajectory.txt and OUT/final_cost.txt and prints one JSON line: frames, events, tracks (archived patches),
// compensation windows, total ms (construction to the files written), ms per frame interval and Mevents/s.
// Built by `make -C event-based-odomety_amd/csrc track_recording`.
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <memory>
#include <string>

#include "../include/dataset_reader/davis240c_recording.h"
#include "../include/tools/recording_evaluator.h"
#include "../include/tools/replayer.h"

static int usage(const char* argv0)
{
	std::fprintf(stderr, "usage: %s --dataset DIR --out DIR [--tracker-experiment] [--window-batch N] [--rectify]\n", argv0);
	return 2;
}

int main(int argc, char** argv)
{
	std::string dataset, out;
	bool trackerExperiment = false;
	size_t windowBatch = 1;
	bool rectify = false;
	for (int i = 1; i < argc; ++i)
	{
		const std::string a = argv[i];
		if (a == "--dataset" && i + 1 < argc)
		{
			dataset = argv[++i];
		}
		else if (a == "--out" && i + 1 < argc)
		{
			out = argv[++i];
		}
		else if (a == "--tracker-experiment")
		{
			trackerExperiment = true;
		}
		else if (a == "--rectify")
		{
			rectify = true;
		}
		else if (a == "--window-batch" && i + 1 < argc)
		{
			char* end = nullptr;
			const unsigned long v = std::strtoul(argv[++i], &end, 10);
			if (!end || *end || v == 0)
			{
				return usage(argv[0]);
			}
			windowBatch = v;
		}
		else
		{
			return usage(argv[0]);
		}
	}
	if (dataset.empty() || out.empty())
	{
		return usage(argv[0]);
	}
	try
	{
		const auto t0 = std::chrono::steady_clock::now();
		tools::EvaluatorParams p;
		p.outputDir = out;
		p.trackerExperiment = trackerExperiment;
		p.windowBatch = windowBatch;
		const auto recording = std::make_shared<tools::Davis240cRecording>(dataset);
		if (rectify)
		{
			p.cameraModelParams = recording->getCalibration();
			p.rectifyEvents = true;
		}
		size_t events = 0, frames = 0, tracks = 0, windows = 0;
		{
			tools::Evaluator evaluator(p);
			tools::Replayer replayer(recording);
			evaluator.replay(replayer);
			evaluator.finish();
			frames = evaluator.images();
			events = evaluator.events();
			windows = evaluator.windows();
			tracks = evaluator.detector().getArchivedPatches().size();
		}
		const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		std::printf("{\"frames\": %zu, \"events\": %zu, \"tracks\": %zu, \"windows\": %zu, \"total_ms\": %.3f, "
					"\"ms_per_frame_interval\": %.4f, \"mevents_per_s\": %.4f, \"tracker_experiment\": %s, "
					"\"window_batch\": %zu, \"rectify\": %s}\n",
					frames, events, tracks, windows, ms, frames > 1 ? ms / static_cast<double>(frames - 1) : 0.0,
					ms > 0 ? static_cast<double>(events) / (ms * 1e3) : 0.0, trackerExperiment ? "true" : "false",
					windowBatch, rectify ? "true" : "false");
	}
	catch (const std::exception& e)
	{
		std::fprintf(stderr, "track_recording: %s\n", e.what());
		return 1;
	}
	return 0;
}
