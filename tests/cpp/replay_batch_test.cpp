// tools::EventPump with EvaluatorParams::windowBatch > 1 against the unbatched pump (windowBatch = 1), which calls
// compensateEventsContrast + integrateEvents per window as tools::Evaluator::eventCallback does.  Built and run by
// tests/test_gpu_replay_windows.py.
//
//   replay_batch_test check <good.bin> <bad.bin> <time_us> <count>
//       good.bin: a recording; bad.bin: the same with one event outside the packed coordinate range.  For windowBatch
//       7 and 64 every callback (n, getLastCompensation, patch flows, motion field, both images, summary, status) and
//       the final detector state equal the unbatched run's, bit for bit; under ERRORS_STATUS with bad.bin too; under
//       ERRORS_THROW bad.bin throws, after the same callbacks as the unbatched run's before its throw.
//   replay_batch_test time <recording.bin> <windowBatch>...
//       ms per window of a replay through the pump (reference defaults; the best of two warm replays), one line per
//       windowBatch, after the host side alone (addEvent, the list conversion, clearEvents).
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../event-based-odomety_amd/include/tools/event_pump.h"

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

// what a callback (or the end of a replay) can read from the detector
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
	size_t held = 0;  // events after the last window, still in the detector
	bool threw = false;
};

Run replay(const std::vector<common::EventSample>& events, int policy, size_t batch, uint32_t time, uint32_t count)
{
	tracker::DetectorParams dp;
	dp.errorPolicy = policy;
	tracker::FeatureDetector det(dp);
	tools::EvaluatorParams ep;
	ep.compensationFrequencyTime = time;
	ep.compensationFrequencyEvents = count;
	ep.windowBatch = batch;
	tools::EventPump pump(det, ep);
	Run r;
	pump.onWindow([&](tracker::FeatureDetector& d, size_t n) { r.calls.push_back(snap(d, n)); });
	try
	{
		pump.replay(events);
	}
	catch (const std::runtime_error&)
	{
		r.threw = true;
	}
	r.final = snap(det, 0);
	r.held = det.getEvents().size();
	if (!r.threw)
	{
		CHECK(pump.windows() == r.calls.size(), "windows() %zu, callbacks %zu", pump.windows(), r.calls.size());
	}
	return r;
}

std::vector<common::EventSample> load(const char* path) { return tools::EventPump::readEventsBin(path); }

int check(const char* good, const char* bad, uint32_t time, uint32_t count)
{
	const auto evGood = load(good), evBad = load(bad);
	using P = tracker::DetectorParams;
	// the whole recording
	const Run ref = replay(evGood, P::ERRORS_THROW, 1, time, count);
	CHECK(!ref.threw && ref.calls.size() > 64, "unbatched run: %zu windows", ref.calls.size());
	CHECK(!ref.calls.empty() && ref.calls[0].n == 1, "the first event fires a one-event window");
	for (size_t batch : {7, 64})
	{
		const Run r = replay(evGood, P::ERRORS_THROW, batch, time, count);
		CHECK(!r.threw && r.calls.size() == ref.calls.size(), "windowBatch %zu: %zu windows against %zu", batch,
			  r.calls.size(), ref.calls.size());
		for (size_t w = 0; w < std::min(r.calls.size(), ref.calls.size()); ++w)
		{
			CHECK(r.calls[w] == ref.calls[w], "windowBatch %zu: window %zu differs (n %zu / %zu)", batch, w,
				  r.calls[w].n, ref.calls[w].n);
		}
		CHECK(r.final == ref.final && r.held == ref.held, "windowBatch %zu: final state differs", batch);
	}
	// one refused window, ERRORS_STATUS: the same callbacks and status() at every window
	const Run refS = replay(evBad, P::ERRORS_STATUS, 1, time, count);
	size_t refused = 0;
	for (const Snap& s : refS.calls)
	{
		refused += s.status != EBO_OK;
	}
	CHECK(refused == 1 && !refS.threw, "unbatched ERRORS_STATUS: %zu refused windows", refused);
	for (size_t batch : {7, 64})
	{
		const Run r = replay(evBad, P::ERRORS_STATUS, batch, time, count);
		CHECK(!r.threw && r.calls.size() == refS.calls.size(), "ERRORS_STATUS windowBatch %zu: %zu windows against %zu",
			  batch, r.calls.size(), refS.calls.size());
		for (size_t w = 0; w < std::min(r.calls.size(), refS.calls.size()); ++w)
		{
			CHECK(r.calls[w] == refS.calls[w], "ERRORS_STATUS windowBatch %zu: window %zu differs (status %d / %d)", batch,
				  w, r.calls[w].status, refS.calls[w].status);
		}
		CHECK(r.final == refS.final && r.held == refS.held, "ERRORS_STATUS windowBatch %zu: final state differs", batch);
	}
	// ERRORS_THROW: the refused window throws; the callbacks before it are those of the unbatched run
	const Run refT = replay(evBad, P::ERRORS_THROW, 1, time, count);
	CHECK(refT.threw && refT.calls.size() > 7, "unbatched ERRORS_THROW: threw %d after %zu windows", refT.threw,
		  refT.calls.size());
	for (size_t batch : {7, 64})
	{
		const Run r = replay(evBad, P::ERRORS_THROW, batch, time, count);
		CHECK(r.threw && r.calls.size() == refT.calls.size(), "ERRORS_THROW windowBatch %zu: threw %d after %zu windows against %zu",
			  batch, r.threw, r.calls.size(), refT.calls.size());
		for (size_t w = 0; w < std::min(r.calls.size(), refT.calls.size()); ++w)
		{
			CHECK(r.calls[w] == refT.calls[w], "ERRORS_THROW windowBatch %zu: window %zu differs", batch, w);
		}
		CHECK(r.final.lastCompensation == refT.final.lastCompensation && r.final.status == refT.final.status,
			  "ERRORS_THROW windowBatch %zu: state at the throw differs", batch);
	}
	std::printf("%zu windows, refused window %zu of %zu\n", ref.calls.size(), refT.calls.size(), refS.calls.size());
	if (failures)
	{
		std::printf("%d failures\n", failures);
		return 1;
	}
	std::printf("all passed\n");
	return 0;
}

int timeReplay(const char* path, int argc, char** argv)
{
	const auto events = load(path);
	const int64_t span = events.back().timestamp.count() - events.front().timestamp.count() + 1000000;
	// the host side alone: addEvent per event (std::list), the list converted once per 15 000 events, clearEvents
	{
		tracker::DetectorParams dp;
		tracker::FeatureDetector det(dp);
		size_t windows = 0, sink = 0;
		const auto t0 = std::chrono::steady_clock::now();
		for (const auto& e : events)
		{
			det.addEvent(e);
			if (det.getEvents().size() >= 15000)
			{
				sink += common::toEboEvents(det.getEvents()).size();
				det.clearEvents();
				++windows;
			}
		}
		const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
		std::printf("{\"host_only\": true, \"windows\": %zu, \"ms_per_window\": %.4f, \"events\": %zu}\n", windows,
					ms / windows, sink);
	}
	for (int a = 0; a < argc; ++a)
	{
		const size_t batch = std::strtoul(argv[a], nullptr, 10);
		tracker::DetectorParams dp;
		tracker::FeatureDetector det(dp);
		tools::EvaluatorParams ep;
		ep.windowBatch = batch;
		tools::EventPump pump(det, ep);
		double best = 1e30;
		size_t windows = 0;
		std::vector<common::EventSample> shifted = events;
		for (int rep = 0; rep < 3; ++rep)  // the first replay loads the code objects and sizes buffers and work tables
		{
			for (auto& e : shifted)
			{
				e.timestamp += common::timestamp_t(rep ? span : 0);  // the same recording again, later
			}
			const size_t before = pump.windows();
			const auto t0 = std::chrono::steady_clock::now();
			pump.replay(shifted);
			const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
			windows = pump.windows() - before;
			if (rep > 0)
			{
				best = std::min(best, ms);
			}
		}
		std::printf("{\"windowBatch\": %zu, \"windows\": %zu, \"ms_per_window\": %.4f}\n", batch, windows, best / windows);
		std::fflush(stdout);
	}
	return 0;
}
}  // namespace

int main(int argc, char** argv)
{
	if (argc == 6 && std::strcmp(argv[1], "check") == 0)
	{
		return check(argv[2], argv[3], static_cast<uint32_t>(std::strtoul(argv[4], nullptr, 10)),
					 static_cast<uint32_t>(std::strtoul(argv[5], nullptr, 10)));
	}
	if (argc >= 4 && std::strcmp(argv[1], "time") == 0)
	{
		return timeReplay(argv[2], argc - 3, argv + 3);
	}
	std::fprintf(stderr, "usage: %s check <good.bin> <bad.bin> <time_us> <count> | time <recording.bin> <windowBatch>...\n",
				 argv[0]);
	return 2;
}
