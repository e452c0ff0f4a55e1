// FeatureDetector::rectifyFrames and tools::EvaluatorParams::rectifyFrames on a recording directory.
// Built by tests/cpp/rectify.mk, run by tests/test_gpu_rectify_facade.py.
//
//   rectify_frames_test replay <dataset> <out> plain|null|fitted
//       tools::Evaluator over the whole recording (the device front end), trajectory.txt and final_cost.txt into <out>,
//       and patches.txt: one line per archived patch (track id, init time, final rect, flow direction as its bits).
//       plain: no rectification; null: rectifyFrames with rectifiedCamera = K of calib.txt; fitted: the fitted camera.
//   rectify_frames_test hooks <dataset> <out>
//       One detector with the device front end's hooks wrapped: the images handed to detectFeatures / gradients /
//       addImage by the first newImage go to <out>/hook_{detect,gradients,add}.bin; the events of the recording up to
//       the second frame are routed (half per event, half as one chunk) and <out>/patch_events.txt gets the first
//       patch's rect and its events "x y t sign", newest first; the refusals of rectifyFrames, projectBatch against the
//       host model and fitRectifiedCamera are checked here.  Prints "all passed".
#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <memory>
#include <optional>
#include <string>
#include <vector>

#include <common/camera_model.h>
#include <dataset_reader/davis240c_recording.h>
#include <tools/recording_evaluator.h>
#include <tools/replayer.h>

namespace
{
int failures = 0;
#define CHECK(cond, ...)                                  \
	do                                                    \
	{                                                     \
		if (!(cond))                                      \
		{                                                 \
			++failures;                                   \
			std::printf("FAIL %s:%d ", __FILE__, __LINE__); \
			std::printf(__VA_ARGS__);                     \
			std::printf("\n");                            \
		}                                                 \
	} while (0)

void dumpImage(const std::string& path, const common::Image8& image)
{
	FILE* f = std::fopen(path.c_str(), "wb");
	if (f)
	{
		std::fwrite(image.data.data(), 1, image.data.size(), f);
		std::fclose(f);
	}
}

common::CameraModelParams<double> pinholeOf(const common::CameraModelParams<double>& c)
{
	common::CameraModelParams<double> r;
	r.fx = c.fx;
	r.fy = c.fy;
	r.cx = c.cx;
	r.cy = c.cy;
	return r;
}

int replay(const std::string& dataset, const std::string& out, const std::string& mode)
{
	const auto recording = std::make_shared<tools::Davis240cRecording>(dataset);
	tools::EvaluatorParams p;
	p.outputDir = out;
	if (mode != "plain")
	{
		p.cameraModelParams = recording->getCalibration();
		p.rectifyFrames = true;
		if (mode == "null")
		{
			p.rectifiedCamera = pinholeOf(p.cameraModelParams);
		}
	}
	tools::Evaluator evaluator(p, {});
	CHECK(evaluator.detector().rectifyingFrames() == (mode != "plain"), "rectifyingFrames() after construction");
	CHECK(evaluator.detector().rectifying() == (mode != "plain"), "rectifyFrames implies rectifyEvents");
	tools::Replayer replayer(recording);
	evaluator.replay(replayer);
	evaluator.finish();
	FILE* f = std::fopen((out + "/patches.txt").c_str(), "w");
	if (!f)
	{
		return 1;
	}
	for (const tracker::Patch& patch : evaluator.detector().getArchivedPatches())
	{
		const double dir = patch.getFlowDir();
		uint64_t bits;
		std::memcpy(&bits, &dir, sizeof(bits));
		std::fprintf(f, "%lld %lld %.17g %.17g %.17g %.17g %016llx %zu\n", static_cast<long long>(patch.getTrackId()),
					 static_cast<long long>(patch.getInitTime().count()), patch.getPatch().x, patch.getPatch().y,
					 patch.getPatch().width, patch.getPatch().height, static_cast<unsigned long long>(bits),
					 patch.getTrajectory().size());
	}
	std::fclose(f);
	std::printf("%s: %zu frames, %zu events, %zu windows, %zu archived patches\n", mode.c_str(), evaluator.images(),
				evaluator.events(), evaluator.windows(), evaluator.detector().getArchivedPatches().size());
	return failures ? 1 : 0;
}

int hooks(const std::string& dataset, const std::string& out)
{
	const auto recording = std::make_shared<tools::Davis240cRecording>(dataset);
	const common::CameraModelParams<double> cam = recording->getCalibration();
	tracker::DetectorParams dp;
	dp.errorPolicy = tracker::DetectorParams::ERRORS_STATUS;
	tracker::FeatureDetector det(dp);
	det.useDeviceFrontEnd();
	tracker::FrontEndHooks inner = det.frontEndHooks(), wrapped = inner;
	int seen[3] = {0, 0, 0};
	wrapped.detectFeatures = [&](const common::Image8& image) {
		if (seen[0]++ == 0)
		{
			dumpImage(out + "/hook_detect.bin", image);
		}
		return inner.detectFeatures(image);
	};
	wrapped.gradients = [&](const common::Image8& image, tracker::Mat64& gx, tracker::Mat64& gy) {
		if (seen[1]++ == 0)
		{
			dumpImage(out + "/hook_gradients.bin", image);
		}
		inner.gradients(image, gx, gy);
	};
	wrapped.addImage = [&](const common::Image8& image) {
		if (seen[2]++ == 0)
		{
			dumpImage(out + "/hook_add.bin", image);
		}
		inner.addImage(image);
	};
	det.setFrontEndHooks(wrapped);

	// needs a rectification
	det.rectifyFrames(true);
	CHECK(det.status() == EBO_ERR_STATE && !det.rectifyingFrames(), "rectifyFrames without a rectification: status %d", det.status());
	const common::CameraModelParams<double> fitted = common::fitRectifiedCamera(det.handle(), cam);
	CHECK(fitted.fx > 0 && fitted.k1 == 0 && fitted.p2 == 0, "fitRectifiedCamera");
	// the one-argument form keeps K; the overload installs the fitted camera
	det.setRectification(cam);
	CHECK(det.ok() && det.rectifying(), "setRectification(camera)");
	CHECK(det.rectifiedCamera().fx == cam.fx && det.rectifiedCamera().cy == cam.cy && det.rectifiedCamera().k1 == 0, "the rectified camera keeps K");
	det.setRectification(cam, cam);  // a rectified camera has no distortion
	CHECK(det.status() == EBO_ERR_ARG && !det.rectifying(), "setRectification(camera, distorted): status %d", det.status());
	det.setRectification(cam, fitted);
	CHECK(det.ok() && det.rectifying(), "setRectification(camera, fitted): %s", det.lastError().c_str());
	CHECK(std::memcmp(&fitted, &(const common::CameraModelParams<double>&)det.rectifiedCamera(), sizeof(fitted)) == 0, "rectifiedCamera()");
	det.rectifyFrames(true);
	CHECK(det.ok() && det.rectifyingFrames(), "rectifyFrames(true): %s", det.lastError().c_str());

	tools::Replayer replayer(recording);
	std::vector<common::EventSample> chunk;
	std::optional<common::ImageSample> image;
	replayer.nextChunk(chunk, image);
	CHECK(image.has_value(), "the first chunk ends in a frame");
	if (!image)
	{
		return 1;
	}
	det.newImage(*image);
	CHECK(det.ok(), "newImage: %s", det.lastError().c_str());
	CHECK(seen[0] == 1 && seen[1] == 1 && seen[2] == 1, "hooks called %d %d %d times", seen[0], seen[1], seen[2]);
	// after the first image the geometry is fixed
	det.rectifyFrames(false);
	CHECK(det.status() == EBO_ERR_STATE && det.rectifyingFrames(), "rectifyFrames(false) after newImage: status %d", det.status());
	det.rectifyFrames(true);  // no change: allowed
	CHECK(det.ok(), "rectifyFrames(true) again");

	chunk.clear();
	image.reset();
	replayer.nextChunk(chunk, image);
	CHECK(chunk.size() > 100, "only %zu events before the second frame", chunk.size());
	const size_t half = chunk.size() / 2;
	const size_t kept = std::min<size_t>(half, 1000);  // (below DetectorParams::maxNumEventsToStore)
	for (size_t i = 0; i < half; ++i)
	{
		if (i < kept)
		{
			det.addEvent(chunk[i]);
		}
		det.updatePatches(chunk[i]);
	}
	det.updatePatches(std::vector<common::EventSample>(chunk.begin() + half, chunk.end()));
	CHECK(det.ok(), "updatePatches: %s", det.lastError().c_str());
	// getEvents() stays raw
	size_t k = 0;
	bool raw = det.getEvents().size() == kept;
	for (const common::EventSample& e : det.getEvents())
	{
		raw = raw && std::memcmp(&e, &chunk[k++], sizeof(e)) == 0;
	}
	CHECK(raw, "getEvents() must stay raw");
	FILE* f = std::fopen((out + "/patch_events.txt").c_str(), "w");
	FILE* fr = std::fopen((out + "/raw_events.txt").c_str(), "w");
	CHECK(f && fr && !det.getPatches().empty(), "no patch after the first image");
	if (f && fr && !det.getPatches().empty())
	{
		const tracker::Patch& patch = det.getPatches().front();
		std::fprintf(f, "%.17g %.17g %.17g %.17g %zu\n", patch.getPatch().x, patch.getPatch().y, patch.getPatch().width,
					 patch.getPatch().height, patch.getNumOfEvents());
		for (const common::EventSample& e : patch.getEvents())
		{
			std::fprintf(f, "%d %d %lld %d\n", e.value.point.x, e.value.point.y, static_cast<long long>(e.timestamp.count()),
						 static_cast<int>(e.value.sign));
		}
		for (const common::EventSample& e : chunk)
		{
			std::fprintf(fr, "%d %d %lld %d\n", e.value.point.x, e.value.point.y, static_cast<long long>(e.timestamp.count()),
						 static_cast<int>(e.value.sign));
		}
	}
	if (f) std::fclose(f);
	if (fr) std::fclose(fr);

	// projectBatch on the detector's context: the bits of the host model
	{
		const common::CameraModel<double> model(cam);
		std::vector<common::CameraModel<double>::Vec3> points;
		for (int i = 0; i < 500; ++i)
		{
			points.emplace_back(((i * 37) % 41 - 20) * 0.05, ((i * 91) % 31 - 15) * 0.05, 0.5 + 0.01 * i);
		}
		const auto pixels = model.projectBatch(det.handle(), points);
		CHECK(pixels.size() == points.size(), "projectBatch size");
		for (size_t i = 0; i < pixels.size(); ++i)
		{
			const auto host = model.project(points[i]);
			CHECK(std::memcmp(&host, &pixels[i], sizeof(host)) == 0, "projectBatch: point %zu differs", i);
		}
		CHECK(model.projectBatch(det.handle(), {}).empty(), "projectBatch of nothing");
	}
	// clearRectification switches frames off too
	det.clearRectification();
	CHECK(!det.rectifying() && !det.rectifyingFrames(), "clearRectification");

	if (failures)
	{
		std::printf("%d failures\n", failures);
		return 1;
	}
	std::printf("all passed\n");
	return 0;
}
}  // namespace

int main(int argc, char** argv)
{
	try
	{
		if (argc == 5 && std::strcmp(argv[1], "replay") == 0)
		{
			return replay(argv[2], argv[3], argv[4]);
		}
		if (argc == 4 && std::strcmp(argv[1], "hooks") == 0)
		{
			return hooks(argv[2], argv[3]);
		}
	}
	catch (const std::exception& e)
	{
		std::fprintf(stderr, "rectify_frames_test: %s\n", e.what());
		return 1;
	}
	std::fprintf(stderr, "usage: %s replay <dataset> <out> plain|null|fitted | hooks <dataset> <out>\n", argv[0]);
	return 2;
}
