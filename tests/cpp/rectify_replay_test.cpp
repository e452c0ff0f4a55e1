// tools::EventPump with EvaluatorParams::rectifyEvents against the pump fed host-rectified events without the flag.
// Built by tests/cpp/camera.mk, run by tests/test_gpu_camera_facade.py.
//
//   rectify_replay_test check <raw.bin> <rectified.bin> <fx fy cx cy k1 k2 k3 p1 p2> <time_us> <count>
//       raw.bin: a recording; rectified.bin: the same events with every in-sensor coordinate replaced through the
//       camera's rectification table on the host (tests/camera_ref.py).  For windowBatch 1 and 7 every callback (n,
//       getLastCompensation, patch flows, motion field, both images, summary, status) and the final detector state of
//       the raw replay WITH rectifyEvents equal those of the rectified replay WITHOUT it, bit for bit; the raw replay
//       without the flag differs (the fixture is not trivial); clearRectification restores it; all-zero camera
//       parameters with rectifyEvents are an error through the detector's error policy; unprojectBatch on the
//       detector's context gives the bits of the host CameraModel.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <common/camera_model.h>
#include <tools/event_pump.h>

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

uint64_t fnv(const void* p, size_t bytes)
{
	const unsigned char* b = static_cast<const unsigned char*>(p);
	uint64_t h = 1469598103934665603ull;
	for (size_t i = 0; i < bytes; ++i)
	{
		h = (h ^ b[i]) * 1099511628211ull;
	}
	return h;
}

struct Snap
{
	size_t n = 0;
	int64_t lastCompensation = 0;
	std::vector<double> flows;
	uint64_t field = 0, warped = 0, integrated = 0;
	ebo_summary summary{};
	int status = 0;
	bool operator==(const Snap& o) const
	{
		return n == o.n && lastCompensation == o.lastCompensation && flows.size() == o.flows.size() &&
			   std::memcmp(flows.data(), o.flows.data(), flows.size() * sizeof(double)) == 0 && field == o.field &&
			   warped == o.warped && integrated == o.integrated &&
			   std::memcmp(&summary, &o.summary, sizeof(summary)) == 0 && status == o.status;
	}
};

Snap snap(tracker::FeatureDetector& d, size_t n)
{
	Snap s;
	s.n = n;
	s.lastCompensation = d.getLastCompensation().count();
	s.flows = d.getPatchFlows();
	s.field = fnv(d.getMotionField().data(), d.getMotionField().size() * sizeof(float));
	const size_t npix = static_cast<size_t>(d.getCompensatedEventImage().rows) * d.getCompensatedEventImage().cols;
	s.warped = fnv(d.getCompensatedEventImage().ptr(), npix * sizeof(double));
	s.integrated = fnv(d.getIntegratedEventImage().ptr(), npix * sizeof(double));
	s.summary = d.getLastSummary();
	s.status = d.status();
	return s;
}

struct Run
{
	std::vector<Snap> calls;
	Snap final;
};

Run replay(const std::vector<common::EventSample>& events, size_t batch, uint32_t time, uint32_t count,
		   const common::CameraModelParams<double>* camera, bool thenClear = false)
{
	tracker::DetectorParams dp;
	tracker::FeatureDetector det(dp);
	tools::EvaluatorParams ep;
	ep.compensationFrequencyTime = time;
	ep.compensationFrequencyEvents = count;
	ep.windowBatch = batch;
	if (camera)
	{
		ep.cameraModelParams = *camera;
		ep.rectifyEvents = true;
	}
	tools::EventPump pump(det, ep);
	CHECK(det.rectifying() == (camera != nullptr), "rectifying() after construction");
	if (thenClear)
	{
		det.clearRectification();
	}
	Run r;
	pump.onWindow([&](tracker::FeatureDetector& d, size_t n) { r.calls.push_back(snap(d, n)); });
	pump.replay(events);
	r.final = snap(det, 0);
	return r;
}

bool same(const Run& a, const Run& b)
{
	if (a.calls.size() != b.calls.size() || !(a.final == b.final))
	{
		return false;
	}
	for (size_t w = 0; w < a.calls.size(); ++w)
	{
		if (!(a.calls[w] == b.calls[w]))
		{
			return false;
		}
	}
	return true;
}
}  // namespace

int main(int argc, char** argv)
{
	if (argc != 15 || std::strcmp(argv[1], "check") != 0)
	{
		std::fprintf(stderr, "usage: %s check <raw.bin> <rectified.bin> <nine camera parameters> <time_us> <count>\n", argv[0]);
		return 2;
	}
	const auto raw = tools::EventPump::readEventsBin(argv[2]);
	const auto rectified = tools::EventPump::readEventsBin(argv[3]);
	double nine[9];
	for (int i = 0; i < 9; ++i)
	{
		nine[i] = std::strtod(argv[4 + i], nullptr);
	}
	common::CameraModelParams<double> cam;
	std::memcpy(&cam, nine, sizeof(cam));
	const uint32_t time = static_cast<uint32_t>(std::strtoul(argv[13], nullptr, 10));
	const uint32_t count = static_cast<uint32_t>(std::strtoul(argv[14], nullptr, 10));

	for (size_t batch : {size_t(1), size_t(7)})
	{
		const Run want = replay(rectified, batch, time, count, nullptr);
		const Run plain = replay(raw, batch, time, count, nullptr);
		const Run got = replay(raw, batch, time, count, &cam);
		const Run cleared = replay(raw, batch, time, count, &cam, true);
		CHECK(want.calls.size() > 14, "windowBatch %zu: only %zu windows", batch, want.calls.size());
		CHECK(same(got, want), "windowBatch %zu: rectifyEvents differs from host-rectified events", batch);
		CHECK(!same(plain, want), "windowBatch %zu: the fixture is trivial (raw == rectified)", batch);
		CHECK(same(cleared, plain), "windowBatch %zu: clearRectification does not restore the raw replay", batch);
		for (size_t w = 0; w < std::min(got.calls.size(), want.calls.size()); ++w)
		{
			CHECK(got.calls[w] == want.calls[w], "windowBatch %zu: window %zu differs", batch, w);
		}
		std::printf("windowBatch %zu: %zu windows\n", batch, want.calls.size());
	}

	// all-zero camera parameters with rectifyEvents: an error through the detector's error policy
	{
		tracker::DetectorParams dp;
		dp.errorPolicy = tracker::DetectorParams::ERRORS_THROW;
		tracker::FeatureDetector det(dp);
		tools::EvaluatorParams ep;
		ep.rectifyEvents = true;
		bool threw = false;
		try
		{
			tools::EventPump pump(det, ep);
		}
		catch (const std::runtime_error&)
		{
			threw = true;
		}
		CHECK(threw && !det.rectifying(), "ERRORS_THROW: zero parameters must throw");
		dp.errorPolicy = tracker::DetectorParams::ERRORS_STATUS;
		tracker::FeatureDetector quiet(dp);
		tools::EventPump pump(quiet, ep);
		CHECK(quiet.status() == EBO_ERR_RANGE && !quiet.rectifying() && !quiet.lastError().empty(),
			  "ERRORS_STATUS: status %d", quiet.status());
	}

	// unprojectBatch on the detector's context: the bits of the host model
	{
		tracker::DetectorParams dp;
		tracker::FeatureDetector det(dp);
		const common::CameraModel<double> model(cam);
		std::vector<common::CameraModel<double>::Vec2> corners;
		for (int i = 0; i < 500; ++i)
		{
			corners.emplace_back((i * 37) % 240 + 0.25 * (i % 4), (i * 91) % 180 + 0.5 * (i % 2));
		}
		const auto bearings = model.unprojectBatch(det.handle(), corners);
		CHECK(bearings.size() == corners.size(), "unprojectBatch size");
		for (size_t i = 0; i < bearings.size(); ++i)
		{
			const auto host = model.unproject(corners[i]);
			CHECK(std::memcmp(&host, &bearings[i], sizeof(host)) == 0, "unprojectBatch: corner %zu differs", i);
		}
		CHECK(model.unprojectBatch(det.handle(), {}).empty(), "unprojectBatch of nothing");
	}

	if (failures)
	{
		std::printf("%d failures\n", failures);
		return 1;
	}
	std::printf("all passed\n");
	return 0;
}
