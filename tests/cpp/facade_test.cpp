// facade_test.cpp — the C++ façade (tracker::FeatureDetector, tracker::contrastFunctor,
// tracker::ContrastBatch, tracker::totalVarianceFunctor) driven the way the reference's
// evaluator drives it (tools/evaluator/src/evaluator.cpp:32-45), checked against the
// CPU oracle.  Mirrors the style of the reference's own gtest files; gtest is not in
// this image, so plain checks.  Run by tests/test_gpu_facade.py on the GPU box.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <vector>
#include <memory>
#include <string>

#include "../../event-based-odomety_amd/include/feature_tracker/contrast_functor.h"
#include "../../event-based-odomety_amd/include/feature_tracker/feature_detector.h"
#include "../../event-based-odomety_amd/include/feature_tracker/optimizer.h"
#include "../../event-based-odomety_amd/include/feature_tracker/tracked_patches.h"
#include "../../event-based-odomety_amd/include/feature_tracker/total_variance.h"
#include "../../event-based-odomety_amd/include/tools/event_pump.h"
#include "../../oracle/ebo_oracle.h"

static int g_fail = 0;
#define EXPECT_TRUE(c)                                                      \
	do                                                                      \
	{                                                                       \
		if (!(c))                                                           \
		{                                                                   \
			std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #c);        \
			++g_fail;                                                       \
		}                                                                   \
	} while (0)
#define EXPECT_NEAR(a, b, tol) EXPECT_TRUE(std::fabs((a) - (b)) <= (tol))

// Scratch files go under $TMPDIR (the pytest driver passes a directory of the test's own), /tmp without it: a fixed
// name in a shared /tmp belongs to whichever user wrote it first.
static std::string scratchDir()
{
	const char* dir = std::getenv("TMPDIR");
	return dir && *dir ? dir : "/tmp";
}

static unsigned long long g_state = 88172645463325252ull;
static unsigned rnd()
{
	g_state ^= g_state << 13;
	g_state ^= g_state >> 7;
	g_state ^= g_state << 17;
	return static_cast<unsigned>(g_state >> 11);
}

// an edge drifting at (0.4, -0.2) px/ms plus noise, 240x180 sensor
static std::vector<common::EventSample> makeEvents(int n)
{
	std::vector<common::EventSample> ev;
	for (int i = 0; i < n; ++i)
	{
		const long t = 100000 + static_cast<long>(i) * 30000 / n;
		const double dt = (t - 115000) * 1e-3;
		common::EventSample e;
		if (rnd() % 10 == 0)
		{
			e.value.point = {static_cast<int>(rnd() % 240), static_cast<int>(rnd() % 180)};
		}
		else
		{
			const double s = (rnd() % 2000) / 1000.0 - 1.0;
			const int k = rnd() % 6;
			const double cx = 30 + 36 * k, cy = 40 + 20 * k;
			int x = static_cast<int>(cx + s * 9 + 0.4 * dt + (rnd() % 3) - 1);
			int y = static_cast<int>(cy + s * 15 - 0.2 * dt + (rnd() % 3) - 1);
			x = x < 0 ? 0 : (x > 239 ? 239 : x);
			y = y < 0 ? 0 : (y > 179 ? 179 : y);
			e.value.point = {x, y};
		}
		e.value.sign = (rnd() & 1) ? common::POSITIVE : common::NEGATIVE;
		e.timestamp = common::timestamp_t(t);
		ev.push_back(e);
	}
	return ev;
}

static std::vector<orc_event> toOracle(const std::list<common::EventSample>& l)
{
	std::vector<orc_event> out;
	for (const auto& e : l)
	{
		out.push_back({e.value.point.x, e.value.point.y, static_cast<int32_t>(e.value.sign), 0, e.timestamp.count()});
	}
	return out;
}

// tracker::Patches is a std::list (the reference's type)
template <class L>
static auto nth(L& l, size_t i) -> decltype(*l.begin())
{
	return *std::next(l.begin(), static_cast<std::ptrdiff_t>(i));
}

int main()
{
	const auto samples = makeEvents(20000);

	// ---- FeatureDetector in the evaluator's call order --------------------------------
	tracker::DetectorParams params;  // reference defaults: 240x180, 20x20 patches, TV 1e3
	params.loss = EBO_LOSS_VARIANCE;
	tracker::FeatureDetector detector(params);
	for (const auto& s : samples)
	{
		detector.addEvent(s);
	}
	EXPECT_TRUE(detector.getEvents().size() == 15000);  // capped at maxNumEventsToStore
	EXPECT_TRUE(detector.getEvents().front().timestamp == samples[5000].timestamp);
	const std::list<common::EventSample> window = detector.getEvents();
	detector.compensateEventsContrast(detector.getEvents());
	detector.integrateEvents(detector.getEvents());
	EXPECT_TRUE(detector.getLastCompensation() == window.back().timestamp);
	detector.clearEvents();
	EXPECT_TRUE(detector.getEvents().empty());

	const std::vector<orc_event> oev = toOracle(window);
	orc_params op;
	orc_default_params(&op);
	op.loss = 1;
	orc_solver_opts oo;
	orc_default_solver(&oo);
	const int P = detector.numPatchesX() * detector.numPatchesY();
	EXPECT_TRUE(detector.numPatchesX() == 12 && detector.numPatchesY() == 9);
	std::vector<double> oflows(2 * P), oimg(240 * 180), oint(240 * 180), oimg2(240 * 180);
	orc_summary os;
	orc_compensate_events_contrast(oev.data(), oev.size(), &op, &oo, oflows.data(), oimg.data(), &os);
	double maxd = 0;
	for (int i = 0; i < 2 * P; ++i)
	{
		maxd = std::fmax(maxd, std::fabs(oflows[i] - detector.getPatchFlows()[i]));
	}
	std::printf("FeatureDetector::compensateEventsContrast: max |flow - oracle| = %.3e, iterations %d vs %d\n",
				maxd, detector.getLastSummary().iterations, os.iterations);
	EXPECT_TRUE(maxd <= 1e-5);
	EXPECT_TRUE(detector.getLastSummary().iterations == os.iterations);
	// final image: bit exact for the same flows
	orc_final_count_image(oev.data(), oev.size(), &op, detector.getPatchFlows().data(), oimg2.data());
	orc_integrate_events(oev.data(), oev.size(), 240, 180, oint.data());
	bool sameC = true, sameI = true;
	double sum = 0;
	for (int y = 0; y < 180; ++y)
	{
		for (int x = 0; x < 240; ++x)
		{
			sameC = sameC && detector.getCompensatedEventImage().at<double>(y, x) == oimg2[y * 240 + x];
			sameI = sameI && detector.getIntegratedEventImage().at<double>(y, x) == oint[y * 240 + x];
			sum += detector.getIntegratedEventImage().at<double>(y, x);
		}
	}
	EXPECT_TRUE(sameC);
	EXPECT_TRUE(sameI);
	EXPECT_TRUE(sum == 15000.0);

	// compensateEventsContrast left the solved flows at the patch corners of the motion
	// field (feature_detector.cpp:418-431)
	EXPECT_TRUE(detector.getMotionField()[2 * (20 * 240 + 20)] ==
				static_cast<float>(detector.getPatchFlows()[2 * (1 * 12 + 1)]));
	// motion-field variant (compensateEvents): zero field == un-warped counts
	detector.setMotionField(std::vector<float>(240 * 180 * 2, 0.0f));
	detector.compensateEvents(window);
	bool sameF = true;
	for (int i = 0; i < 240 * 180; ++i)
	{
		sameF = sameF && detector.getCompensatedEventImage().ptr()[i] == oint[i];
	}
	EXPECT_TRUE(sameF);

	// compensateEvents as the reference runs it (feature_detector.cpp:243-296): trajectories of
	// tracked patches -> interpolateMotionField (optimizeFlowTV = true by default) -> warp loop
	{
		std::vector<tracker::FeatureDetector::Trajectory> trajs;
		std::vector<size_t> off(1, 0);
		std::vector<double> txy;
		std::vector<int64_t> tts;
		const int64_t tMid = static_cast<int32_t>((window.front().timestamp + window.back().timestamp).count() * 0.5);
		for (int k = 0; k < 9; ++k)
		{
			tracker::FeatureDetector::Trajectory tr;
			const double vx = 0.3 * (k % 3 - 1) + 0.05 * k, vy = 0.2 * (k / 3 - 1);  // px per ms
			for (int i = -2; i <= 2; ++i)
			{
				const int64_t t = tMid + 100 + 20000 * i;
				common::Sample<common::Point2d> smp;
				smp.value.x = 30.0 + 22.0 * k + vx * 20.0 * i;
				smp.value.y = 25.0 + 15.0 * k + vy * 20.0 * i;
				smp.timestamp = common::timestamp_t(t);
				tr.push_back(smp);
				txy.push_back(smp.value.x);
				txy.push_back(smp.value.y);
				tts.push_back(t);
			}
			trajs.push_back(tr);
			off.push_back(tts.size());
		}
		detector.setPatchTrajectories(trajs);
		detector.compensateEvents(window);
		std::vector<float> ofield(240 * 180 * 2);
		std::vector<int32_t> ofix(2 * 9);
		int32_t nfix = 0;
		orc_init_motion_field(240, 180, 1e-3, 1, 9, off.data(), txy.data(), tts.data(), tMid, ofield.data(), &nfix,
							  ofix.data());
		EXPECT_TRUE(nfix == 9);
		orc_summary fs;
		orc_interpolate_motion_field(240, 180, 0, ofield.data(), nfix, ofix.data(), nullptr, &fs);
		EXPECT_TRUE(detector.getLastFieldSummary().iterations == fs.iterations);
		EXPECT_NEAR(detector.getLastFieldSummary().final_cost, fs.final_cost, 1e-9 * fs.final_cost);
		double worst = 0;
		for (size_t i = 0; i < ofield.size(); ++i)
		{
			worst = std::max(worst, std::fabs(static_cast<double>(ofield[i]) - detector.getMotionField()[i]));
		}
		EXPECT_TRUE(worst < 2e-7);  // float32 storage: at most one ulp apart
		// the count image through the facade's own field is bit exact
		std::vector<double> oimgF(240 * 180);
		orc_compensate_events_field(oev.data(), oev.size(), 240, 180, 1e-3, detector.getMotionField().data(),
									oimgF.data());
		bool sameT = true;
		for (int i = 0; i < 240 * 180; ++i)
		{
			sameT = sameT && detector.getCompensatedEventImage().ptr()[i] == oimgF[i];
		}
		EXPECT_TRUE(sameT);
		detector.setPatchTrajectories({});
	}

	// ---- contrastFunctor with the reference's constructor ---------------------------------
	const tracker::Rect2i rect(20, 40, 20, 20);
	std::list<common::EventSample> patchEvents;
	for (const auto& e : window)
	{
		if (rect.contains(e.value.point))  // feature_detector.cpp:348-355
		{
			patchEvents.push_back(e);
		}
	}
	EXPECT_TRUE(patchEvents.size() > 100);
	tracker::contrastFunctor functor(patchEvents, rect, params.compensateScale, EBO_LOSS_VARIANCE);
	const std::vector<orc_event> pev = toOracle(patchEvents);
	orc_functor_consts k;
	orc_default_consts(&k);
	const double motions[3][2] = {{0.0, 0.0}, {0.4, -0.2}, {-0.7, 0.3}};
	for (const auto& m : motions)
	{
		double r = 0, rj = 0, J[2] = {0, 0}, ro = 0, Jo[2];
		EXPECT_TRUE(functor(m, &r));
		const double* blocks[1] = {m};
		double* jac[1] = {J};
		EXPECT_TRUE(functor.Evaluate(blocks, &rj, jac));
		orc_contrast_eval(pev.data(), pev.size(), rect.x, rect.y, rect.width, rect.height, 1e-3, &k, 1, m, &ro, Jo);
		EXPECT_NEAR(r, ro, 1e-9 * std::fabs(ro));
		EXPECT_NEAR(rj, ro, 1e-9 * std::fabs(ro));
		EXPECT_NEAR(J[0], Jo[0], 1e-9 * std::fabs(Jo[0]) + 1e-10);
		EXPECT_NEAR(J[1], Jo[1], 1e-9 * std::fabs(Jo[1]) + 1e-10);
		double rv = 0;
		EXPECT_TRUE(functor.Evaluate(blocks, &rv, nullptr));  // jacobians == nullptr: value only
		EXPECT_NEAR(rv, ro, 1e-9 * std::fabs(ro));
	}

	// ---- ContrastBatch: every data term in one launch (the EvaluationCallback surface) ------
	tracker::ContrastBatch batch(params.compensateScale, EBO_LOSS_VARIANCE);
	std::vector<double> x(2 * 6, 0.0);
	std::vector<std::list<common::EventSample>> lists(6);
	std::vector<tracker::Rect2i> rects;
	for (int i = 0; i < 6; ++i)
	{
		rects.emplace_back(20 + 36 * i, 30 + 20 * i, 24, 22);
		for (const auto& e : window)
		{
			if (rects[i].contains(e.value.point))
			{
				lists[i].push_back(e);
			}
		}
		x[2 * i] = 0.1 * i - 0.2;
		x[2 * i + 1] = 0.05 * i;
		batch.addPatch(lists[i], rects[i], &x[2 * i]);
	}
	batch.PrepareForEvaluation(true, true);
	EXPECT_TRUE(batch.ok());
	for (int i = 0; i < 6; ++i)
	{
		if (lists[i].empty())
		{
			continue;
		}
		const std::vector<orc_event> bev = toOracle(lists[i]);
		double ro, Jo[2];
		orc_contrast_eval(bev.data(), bev.size(), rects[i].x, rects[i].y, rects[i].width, rects[i].height, 1e-3, &k, 1,
						  &x[2 * i], &ro, Jo);
		EXPECT_NEAR(batch.residual(i), ro, 1e-9 * std::fabs(ro));
		EXPECT_NEAR(batch.jacobian(i)[0], Jo[0], 1e-9 * std::fabs(Jo[0]) + 1e-10);
		EXPECT_NEAR(batch.jacobian(i)[1], Jo[1], 1e-9 * std::fabs(Jo[1]) + 1e-10);
	}

	// ---- totalVarianceFunctor (host) ------------------------------------------------------------
	tracker::totalVarianceFunctor tv(1e3);
	const double a[2] = {0.5, -0.25}, b[2] = {0.25, 0.0};
	double res[2], ores[2];
	tv(a, b, res);
	orc_tv_eval(1e3, a, b, ores, nullptr, nullptr);
	EXPECT_TRUE(res[0] == ores[0] && res[1] == ores[1]);

	// ---- error behaviour: no exceptions cross the functor, status instead ---------------------
	std::list<common::EventSample> far = patchEvents;
	far.back().timestamp += common::timestamp_t(1ll << 33);
	tracker::contrastFunctor bad(far, rect, params.compensateScale, EBO_LOSS_VARIANCE);
	double rr = 0;
	EXPECT_TRUE(!bad(motions[0], &rr));

	// ---- EventPump: events.txt -> reader -> evaluator's window rule -> detector --------------
	{
		const std::string path = scratchDir() + "/ebo_facade_events.txt";
		FILE* fp = std::fopen(path.c_str(), "w");
		for (const auto& s : samples)
		{
			std::fprintf(fp, "%.9f %d %d %d\n", s.timestamp.count() * 1e-6, s.value.point.x, s.value.point.y,
						 s.value.sign == common::POSITIVE ? 1 : 0);
		}
		std::fclose(fp);
		const auto read = tools::EventPump::readEvents(path);
		EXPECT_TRUE(read.size() == samples.size());
		EXPECT_TRUE(read[777].value.point.x == samples[777].value.point.x);
		EXPECT_TRUE(read[777].value.sign == samples[777].value.sign);
		// the packed binary sidecar gives the same events back without parsing
		const std::string pathBin = scratchDir() + "/ebo_facade_events.ebo";
		tools::EventPump::writeEventsBin(pathBin, read);
		const auto readBin = tools::EventPump::readEventsBin(pathBin);
		bool sameBin = readBin.size() == read.size();
		for (size_t i = 0; i < read.size() && sameBin; ++i)
		{
			sameBin = readBin[i].timestamp == read[i].timestamp && readBin[i].value.point.x == read[i].value.point.x &&
					  readBin[i].value.point.y == read[i].value.point.y && readBin[i].value.sign == read[i].value.sign;
		}
		EXPECT_TRUE(sameBin);
		tracker::DetectorParams p2;
		p2.loss = EBO_LOSS_VARIANCE;
		tracker::FeatureDetector det2(p2);
		tools::EventPump pump(det2);
		size_t seen = 0, lastN = 0;
		pump.onWindow([&](tracker::FeatureDetector& d, size_t n) {
			++seen;
			lastN = n;
			double s = 0;
			for (int i = 0; i < 240 * 180; ++i)
			{
				s += d.getIntegratedEventImage().ptr()[i];
			}
			EXPECT_TRUE(s == static_cast<double>(n));
		});
		pump.replay(read);
		// t starts at 100 ms: the first event is not yet 300 ms past lastCompensation = 0, so the
		// first window closes at 15000 events; the remaining 5000 events stay pending
		EXPECT_TRUE(pump.windows() == 1 && seen == 1 && lastN == 15000);
		EXPECT_TRUE(det2.getEvents().size() == 5000);
	}

	// ---- tracker::Optimizer::optimize over tracked patches (optimizer.cpp:62-206) ------------
	{
		const int W = 240, H = 180;
		tracker::Mat64 gx(H, W), gy(H, W);
		std::vector<double> grid(static_cast<size_t>(W) * H * 2);
		for (int y = 0; y < H; ++y)
		{
			for (int x = 0; x < W; ++x)
			{
				// gradient of a few smooth blobs
				double vx = 0, vy = 0;
				for (int k = 0; k < 5; ++k)
				{
					const double cx = 40 + 38 * k, cy = 40 + 25 * k, sg = 6 + k;
					const double e = std::exp(-((x - cx) * (x - cx) + (y - cy) * (y - cy)) / (2 * sg * sg));
					vx += -(x - cx) / (sg * sg) * e;
					vy += -(y - cy) / (sg * sg) * e;
				}
				gx.at<double>(y, x) = vx;
				gy.at<double>(y, x) = vy;
				grid[2 * (static_cast<size_t>(y) * W + x)] = vx;
				grid[2 * (static_cast<size_t>(y) * W + x) + 1] = vy;
			}
		}
		tracker::OptimizerParams op;
		tracker::Optimizer optimizer(op, tracker::Size(W, H));
		optimizer.setGrad(gx, gy);
		std::vector<tracker::Patch> patchStore;
		patchStore.reserve(8);
		// (a fifth blob at k = 4 drives the LM to a 90-degree rotation with the patch half outside
		// the image, where two correct solvers stop agreeing; see tests/test_optimizer.py)
		for (int k = 0; k < 4; ++k)
		{
			patchStore.emplace_back(tracker::Corner(42.0 + 38 * k, 38.0 + 25 * k), 12, common::timestamp_t(1000));
			tracker::Patch& p = patchStore.back();
			p.setTrackId(k);
			p.setNumOfEvents(120);
			p.setFlowDir(0.4 + 0.3 * k);
			// one event on each of the 280 pixels where the predicted nabla (gradient projected on
			// the flow, sampled one pixel off) is strongest, with the opposite sign: a well-posed
			// tracking problem whose answer is a shift of about one pixel
			const double fc = std::cos(0.4 + 0.3 * k), fs = std::sin(0.4 + 0.3 * k);
			std::vector<std::pair<double, int>> strength;
			for (int y = 0; y < 25; ++y)
			{
				for (int x = 0; x < 25; ++x)
				{
					const int ix = 30 + 38 * k + x + 1, iy = 26 + 25 * k + y;
					strength.push_back({-std::fabs(gx.at<double>(iy, ix) * fc + gy.at<double>(iy, ix) * fs), y * 25 + x});
				}
			}
			std::sort(strength.begin(), strength.end());
			p.setNumOfEvents(280);
			for (int i = 0; i < 280; ++i)
			{
				const int x = strength[i].second % 25, y = strength[i].second / 25;
				const int ix = 30 + 38 * k + x + 1, iy = 26 + 25 * k + y;
				const double pred = gx.at<double>(iy, ix) * fc + gy.at<double>(iy, ix) * fs;
				common::EventSample e;
				e.value.point = {30 + 38 * k + x, 26 + 25 * k + y};
				e.value.sign = pred < 0 ? common::POSITIVE : common::NEGATIVE;
				e.timestamp = common::timestamp_t(2000 + 40 * i);
				p.addEvent(e);
			}
		}
		std::vector<tracker::Patch*> batch;
		for (auto& p : patchStore)
		{
			batch.push_back(&p);
		}
		// the oracle's version of the same sequence, from copies of the patches' state
		struct Expect
		{
			std::vector<double> nabla, mc;
			double pose[4], flow, rect[4];
			orc_summary sum;
			int32_t updated;
		};
		std::vector<Expect> ex(batch.size());
		for (size_t i = 0; i < batch.size(); ++i)
		{
			const tracker::Patch& p = *batch[i];
			std::vector<orc_event> pe;
			for (const auto& e : p.getEvents())
			{
				pe.push_back({e.value.point.x, e.value.point.y, static_cast<int32_t>(e.value.sign), 0, e.timestamp.count()});
			}
			const tracker::Rect2d r = p.getPatch();
			Expect& E = ex[i];
			E.nabla.assign(25 * 25, 0.0);
			int64_t cur = 0, last = 0;
			orc_patch_integrate(pe.data(), pe.size(), r.x, r.y, r.width, r.height, E.nabla.data(), &cur, &last);
			std::vector<double> nn(25 * 25);
			orc_normalize_nabla(E.nabla.data(), 25 * 25, nn.data());
			std::copy(p.getWarp().data(), p.getWarp().data() + 4, E.pose);
			E.flow = p.getFlow();
			orc_optimizer_solve(grid.data(), W, H, r.x, r.y, r.width, r.height, nn.data(), op.huberLoss, nullptr, E.pose,
								&E.flow, &E.sum);
			E.flow = std::fmod(E.flow, 2 * M_PI);
			const tracker::Corner c0 = p.toCorner();
			orc_patch_update_rect(E.pose, c0.x, c0.y, r.width, r.height, E.rect);  // initPoint_ == first corner
			const double nc[2] = {E.rect[0] + 12.0, E.rect[1] + 12.0};
			const double pc[2] = {c0.x, c0.y};
			E.mc.assign(25 * 25, 0.0);
			orc_patch_integrate_mc(pe.data(), pe.size(), E.rect[0], E.rect[1], E.rect[2], E.rect[3], pc, 1000, nc, cur,
								   cur, E.mc.data(), &E.updated);
		}
		optimizer.optimize(batch);
		EXPECT_TRUE(optimizer.getFinalCosts().size() == batch.size());
		for (size_t i = 0; i < batch.size(); ++i)
		{
			const tracker::Patch& p = *batch[i];
			const Expect& E = ex[i];
			bool sameN = true, sameM = true;
			for (int k = 0; k < 25 * 25; ++k)
			{
				sameN = sameN && p.getIntegratedNabla().ptr()[k] == E.nabla[k];
				sameM = sameM && p.getCompenatedIntegratedNabla().ptr()[k] == E.mc[k];
			}
			std::printf("Optimizer patch %zu: cost %.12g vs oracle %.12g (initial %.6g), iterations %d vs %d, "
						"warp (%.9f %.9f %.9f %.9f) vs (%.9f %.9f %.9f %.9f)\n",
						i, p.getFinalCosts().back(), E.sum.final_cost, E.sum.initial_cost,
						optimizer.getLastSummaries()[i].iterations, E.sum.iterations, p.getWarp().data()[0],
						p.getWarp().data()[1], p.getWarp().data()[2], p.getWarp().data()[3], E.pose[0], E.pose[1],
						E.pose[2], E.pose[3]);
			EXPECT_TRUE(sameN);  // integer counts: bit exact
			EXPECT_TRUE(E.updated == 1 && sameM);
			EXPECT_TRUE(optimizer.getLastSummaries()[i].iterations == E.sum.iterations);
			EXPECT_NEAR(p.getFinalCosts().back(), E.sum.final_cost, 1e-7 * E.sum.final_cost + 1e-13);
			for (int k = 0; k < 4; ++k)
			{
				EXPECT_NEAR(p.getWarp().data()[k], E.pose[k], 1e-5);
			}
			EXPECT_NEAR(static_cast<double>(p.getFlow()), static_cast<double>(static_cast<float>(E.flow)), 1e-5);
			EXPECT_NEAR(p.getPatch().x, E.rect[0], 1e-5);
			EXPECT_NEAR(p.getPatch().y, E.rect[1], 1e-5);
			EXPECT_TRUE(p.getTrajectory().size() == 2);
			EXPECT_TRUE(!p.isLost() && p.isInit());
		}
		// optimize(Patch&): the reference's signature, one patch
		tracker::Patch single(tracker::Corner(80.0, 63.0), 12, common::timestamp_t(1000));
		single.setFlowDir(1.0);
		for (const auto& e : patchStore[1].getEvents())
		{
			single.addEvent(e);
		}
		optimizer.optimize(single);
		EXPECT_TRUE(single.getFinalCosts().size() == 1 && single.getTrajectory().size() == 2);
	}

	// ---- the reference's own updatePatchTest (feature_detector_test.cpp:43-97): three patches of
	// extent 11 at (0,0), (5,5), (20,20), events in [0,30)^2; the detector's patches hold the events
	// a manual isInPatch/addEvent loop gives them -- per event and as one chunk ---------------------
	{
		const common::timestamp_t timestamp(0);
		tracker::Patches patches = {tracker::Patch({0, 0}, 11, timestamp), tracker::Patch({5, 5}, 11, timestamp),
									tracker::Patch({20, 20}, 11, timestamp)};
		tracker::TrackedPatches perEvent(tracker::Size(240, 180)), chunked(tracker::Size(240, 180));
		perEvent.setPatches(patches);
		chunked.setPatches(patches);
		std::vector<common::EventSample> all;
		std::srand(7);
		for (size_t i = 0; i < 200; ++i)
		{
			common::EventSample event;
			event.timestamp = common::timestamp_t(i);
			event.value.point = {std::rand() % 30, std::rand() % 30};
			event.value.sign = std::rand() % 2 == 1 ? common::POSITIVE : common::NEGATIVE;
			perEvent.updatePatches(event);
			all.push_back(event);
			for (auto& patch : patches)
			{
				if (patch.isInPatch(event.value.point))
				{
					patch.addEvent(event);
				}
			}
		}
		chunked.updatePatches(all);
		for (const tracker::TrackedPatches* d : {&perEvent, &chunked})
		{
			EXPECT_TRUE(d->getPatches().size() == patches.size());
			for (size_t i = 0; i < patches.size(); ++i)
			{
				const auto& got = nth(d->getPatches(), i).getEvents();
				const auto& want = nth(patches, i).getEvents();
				EXPECT_TRUE(got.size() == want.size() && !want.empty());
				for (size_t k = 0; k < got.size() && k < want.size(); ++k)
				{
					EXPECT_TRUE(got[k].timestamp == want[k].timestamp);
				}
			}
		}
	}

	// ---- FeatureDetector::updatePatches (feature_detector.cpp:585-619): the per-event call against
	// the chunked one (device routing + lock-step rounds) on the same stream ----------------------
	{
		const int W = 240, H = 180;
		tracker::Mat64 gx(H, W), gy(H, W);
		for (int y = 0; y < H; ++y)
		{
			for (int x = 0; x < W; ++x)
			{
				double vx = 0, vy = 0;
				for (int k = 0; k < 5; ++k)
				{
					const double cx = 40 + 38 * k, cy = 40 + 25 * k, sg = 6 + k;
					const double e = std::exp(-((x - cx) * (x - cx) + (y - cy) * (y - cy)) / (2 * sg * sg));
					vx += -(x - cx) / (sg * sg) * e;
					vy += -(y - cy) / (sg * sg) * e;
				}
				gx.at<double>(y, x) = vx;
				gy.at<double>(y, x) = vy;
			}
		}
		// the detector's own gradient images for the event-count estimate, scaled so that the estimates
		// land inside Patch::setNumOfEvents' clamp [100, 300] and differ from patch to patch
		tracker::Mat64 gxBig(H, W), gyBig(H, W);
		for (int y = 0; y < H; ++y)
		{
			for (int x = 0; x < W; ++x)
			{
				gxBig.at<double>(y, x) = 4.0 * gx.at<double>(y, x) + 0.25 + 0.001 * x;
				gyBig.at<double>(y, x) = 4.0 * gy.at<double>(y, x) - 0.2 + 0.0015 * y;
			}
		}
		tracker::OptimizerParams op;
		auto build = [&](tracker::TrackedPatches& tp) {
			auto opt = std::make_shared<tracker::Optimizer>(op, tracker::Size(W, H));
			opt->setGrad(gx, gy);
			tp.setOptimizer(common::timestamp_t(1000), opt);
			tp.setGradients(gxBig, gyBig);  // gradX_ / gradY_ of the detector: updateNumOfEvents' estimate runs on the device
			for (int k = 0; k < 4; ++k)
			{
				tracker::Patch p(tracker::Corner(42.0 + 38 * k, 38.0 + 25 * k), 12, common::timestamp_t(1000));
				p.setTrackId(k);
				p.setFlowDir(0.4 + 0.3 * k);
				tp.addPatch(p);
			}
			// a patch nobody initialised (collects events, is never optimised) and one that starts
			// next to the border (lost by updateNumOfEvents after its first optimisation)
			tracker::Patch cold(tracker::Corner(120.0, 90.0), 12, common::timestamp_t(1000));
			tp.addPatch(cold);
			tracker::Patch edge(tracker::Corner(4.0, 100.0), 12, common::timestamp_t(1000));
			edge.setFlowDir(0.2);
			tp.addPatch(edge);
			return opt;
		};
		// a stream: events drifting over the blobs (plus noise), 6000 of them
		std::vector<common::EventSample> stream;
		uint64_t st = 12345;
		auto rnd = [&]() {
			st = st * 6364136223846793005ull + 1442695040888963407ull;
			return static_cast<uint32_t>(st >> 33);
		};
		for (int i = 0; i < 6000; ++i)
		{
			common::EventSample e;
			const int k = static_cast<int>(rnd() % 6);
			const double drift = 1e-3 * i;
			int x, y;
			if (k < 4)
			{
				x = static_cast<int>(42.0 + 38 * k + drift + static_cast<int>(rnd() % 21) - 10);
				y = static_cast<int>(38.0 + 25 * k + static_cast<int>(rnd() % 21) - 10);
			}
			else if (k == 4)
			{
				x = static_cast<int>(rnd() % W);
				y = static_cast<int>(rnd() % H);
			}
			else
			{
				x = static_cast<int>(4 + rnd() % 22);
				y = static_cast<int>(90 + rnd() % 22);
			}
			e.value.point = {x, y};
			e.value.sign = (rnd() & 1) ? common::POSITIVE : common::NEGATIVE;
			e.timestamp = common::timestamp_t(2000 + 37 * i);
			stream.push_back(e);
		}
		tracker::TrackedPatches seq(tracker::Size(W, H)), bat(tracker::Size(W, H));
		auto optSeq = build(seq);
		auto optBat = build(bat);
		for (const auto& e : stream)
		{
			seq.updatePatches(e);
		}
		// two chunks, so that state carries over a chunk border
		std::vector<common::EventSample> a(stream.begin(), stream.begin() + 2500), b(stream.begin() + 2500, stream.end());
		bat.updatePatches(a);
		const int roundsA = bat.lastRounds();
		bat.updatePatches(b);
		std::printf("updatePatches: %zu optimisations per-event, %zu chunked, rounds %d + %d\n",
					optSeq->getFinalCosts().size(), optBat->getFinalCosts().size(), roundsA, bat.lastRounds());
		EXPECT_TRUE(optSeq->getFinalCosts().size() == optBat->getFinalCosts().size());
		EXPECT_TRUE(optSeq->getFinalCosts().size() >= 8);
		int adapted = 0;
		for (size_t i = 0; i < seq.getPatches().size(); ++i)
		{
			const tracker::Patch& p = nth(seq.getPatches(), i);
			const tracker::Patch& q = nth(bat.getPatches(), i);
			EXPECT_TRUE(p.isLost() == q.isLost() && p.isInit() == q.isInit());
			EXPECT_TRUE(p.getFinalCosts().size() == q.getFinalCosts().size());
			EXPECT_TRUE(p.getTrajectory().size() == q.getTrajectory().size());
			EXPECT_TRUE(p.getEvents().size() == q.getEvents().size());
			EXPECT_TRUE(p.eventsUntilReady() == q.eventsUntilReady());
			EXPECT_TRUE(p.getNumOfEvents() == q.getNumOfEvents());
			if (!p.isLost() && p.isInit() && !p.getFinalCosts().empty())
			{
				// updateNumOfEvents' estimate at the patch's final state, against the oracle's restatement
				std::vector<double> interleaved(2 * static_cast<size_t>(W) * H);
				for (int yy = 0; yy < H; ++yy)
				{
					for (int xx = 0; xx < W; ++xx)
					{
						interleaved[2 * (static_cast<size_t>(yy) * W + xx)] = gxBig.at<double>(yy, xx);
						interleaved[2 * (static_cast<size_t>(yy) * W + xx) + 1] = gyBig.at<double>(yy, xx);
					}
				}
				uint64_t est = 0;
				const tracker::Rect2d& rr = p.getPatch();
				orc_estimate_num_events(interleaved.data(), W, H, rr.x, rr.y, rr.width, rr.height, p.getWarp().data(), p.getFlow(), &est);
				const size_t clamped = std::min<size_t>(std::max<size_t>(est, 100), 300);
				const bool inside = !(rr.x < 0 || rr.y < 0 || rr.x + rr.width >= W || rr.y + rr.height >= H);
				if (inside)
				{
					EXPECT_TRUE(p.getNumOfEvents() == clamped);
					adapted += p.getNumOfEvents() != 75 ? 1 : 0;
				}
			}
			bool sameEvents = p.getEvents().size() == q.getEvents().size();
			for (size_t k = 0; sameEvents && k < p.getEvents().size(); ++k)
			{
				sameEvents = p.getEvents()[k].timestamp == q.getEvents()[k].timestamp &&
							 p.getEvents()[k].value.point.x == q.getEvents()[k].value.point.x;
			}
			EXPECT_TRUE(sameEvents);
			// the same calls in the same order on the same device code: identical, not just close
			EXPECT_TRUE(p.getPatch().x == q.getPatch().x && p.getPatch().y == q.getPatch().y);
			for (int k = 0; k < 4; ++k)
			{
				EXPECT_TRUE(p.getWarp().data()[k] == q.getWarp().data()[k]);
			}
			for (size_t k = 0; k < p.getFinalCosts().size() && k < q.getFinalCosts().size(); ++k)
			{
				EXPECT_TRUE(p.getFinalCosts()[k] == q.getFinalCosts()[k]);
			}
			std::printf("  patch %zu: %zu optimisations, lost %d, centre (%.4f, %.4f)\n", i, p.getFinalCosts().size(),
						int(p.isLost()), p.toCorner().x, p.toCorner().y);
		}
		EXPECT_TRUE(adapted >= 3);  // the tracked patches adapt their event count without any estimator hook
		// timing, 100 tracked patches (25 copies of the four) over the same 6000-event stream
		{
			auto many = [&](tracker::TrackedPatches& tp) {
				auto opt = std::make_shared<tracker::Optimizer>(op, tracker::Size(W, H));
				opt->setGrad(gx, gy);
				tp.setOptimizer(common::timestamp_t(1000), opt);
				for (int c = 0; c < 25; ++c)
				{
					for (int k = 0; k < 4; ++k)
					{
						tracker::Patch p(tracker::Corner(42.0 + 38 * k, 38.0 + 25 * k), 12, common::timestamp_t(1000));
						p.setFlowDir(0.4 + 0.3 * k);
						tp.addPatch(p);
					}
				}
				return opt;
			};
			tracker::TrackedPatches s100(tracker::Size(W, H)), b100(tracker::Size(W, H));
			auto o1 = many(s100);
			auto o2 = many(b100);
			const auto t0 = std::chrono::steady_clock::now();
			for (const auto& e : stream)
			{
				s100.updatePatches(e);
			}
			const auto t1 = std::chrono::steady_clock::now();
			b100.updatePatches(stream);
			const auto t2 = std::chrono::steady_clock::now();
			std::printf("updatePatches, 100 patches x 6000 events: per-event %.1f ms (%zu optimisations), chunked %.1f ms "
						"(%zu optimisations in %d rounds)\n",
						std::chrono::duration<double, std::milli>(t1 - t0).count(), o1->getFinalCosts().size(),
						std::chrono::duration<double, std::milli>(t2 - t1).count(), o2->getFinalCosts().size(),
						b100.lastRounds());
			EXPECT_TRUE(o1->getFinalCosts().size() == o2->getFinalCosts().size());
			EXPECT_TRUE(nth(s100.getPatches(), 57).getPatch().x == nth(b100.getPatches(), 57).getPatch().x);
		}
		EXPECT_TRUE(nth(seq.getPatches(), 4).getFinalCosts().empty());   // never initialised
		EXPECT_TRUE(nth(seq.getPatches(), 5).isLost() && nth(seq.getPatches(), 5).getFinalCosts().size() == 1);  // centre within 5 px of the border
	}

	// ---- Patch::warpImage: the reference's warpImageTest (patch_test.cpp:62-108) through the facade ----
	for (int n : {11, 15})
	{
		// cv::line(gradX, {c, 0}, {c, n-1}, 1); cv::line(gradY, {0, c}, {n-1, c}, 1)
		const int c0 = n / 2;
		tracker::Mat64 gradX(n, n), gradY(n, n);
		for (int k = 0; k < n; ++k)
		{
			gradX.at<double>(k, c0) = 1.0;
			gradY.at<double>(c0, k) = 1.0;
		}
		tracker::Patch patch(tracker::Corner(c0, c0), 5, common::timestamp_t(0));
		const float angle = static_cast<float>(M_PI / 4);
		patch.setFlowDir(angle);
		patch.setWarp(common::Pose2d(M_PI / 4, common::Point2d(0.0, 0.0)));  // Sophus::SE2d::rot(M_PI / 4)
		tracker::OptimizerParams wp;
		tracker::Optimizer holder(wp, tracker::Size(n, n));  // the frame's gradient images live in its context
		holder.setGrad(gradX, gradY);                        // patch.setGrad(gradX, gradY)
		EXPECT_TRUE(patch.warpImage(holder.handle()));
		const tracker::Mat64& image = patch.getPredictedNabla();
		EXPECT_TRUE(image.rows == 11 && image.cols == 11);
		bool anyNegative = false;
		for (int i = 1; i < 10; ++i)
		{
			for (int j = 1; j < 10; ++j)
			{
				if (i == j || i == 10 - j)
				{
					EXPECT_TRUE(image.at<double>(i, j) <= 0);  // EXPECT_LE(image.at<double>(i, j), 0)
				}
				anyNegative = anyNegative || image.at<double>(i, j) < 0;
			}
		}
		// n = 11 is the reference's set-up: the rect touches the border, warpImage returns early (patch.cpp:145-150)
		// and the image is still Patch::init's zeros; n = 15 clears the border and the warp runs
		EXPECT_TRUE(anyNegative == (n == 15));
		// against the oracle's restatement, pixel by pixel
		std::vector<double> grad(static_cast<size_t>(n) * n * 2);
		for (int k = 0; k < n * n; ++k)
		{
			grad[2 * k] = gradX.ptr()[k];
			grad[2 * k + 1] = gradY.ptr()[k];
		}
		std::vector<double> want(121, 0.0);
		int updated = -1;
		const tracker::Rect2d& r = patch.getPatch();
		EXPECT_TRUE(orc_patch_warp_image(grad.data(), n, n, r.x, r.y, r.width, r.height, patch.getWarp().data(), patch.getFlowDir(),
										 want.data(), &updated) == 0);
		EXPECT_TRUE(updated == (n == 15 ? 1 : 0));
		for (int k = 0; k < 121; ++k)
		{
			EXPECT_TRUE(std::fabs(want[k] - image.ptr()[k]) <= 1e-15);
		}
	}

	std::printf(g_fail ? "facade_test: %d FAILED\n" : "facade_test: all passed\n", g_fail);
	return g_fail ? 1 : 0;
}
