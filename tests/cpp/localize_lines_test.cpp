// Driver of the odometry front end (event-based-odomety_amd/include/visual_odometry/visual_odometry.h) for
// tests/test_abspose_cpu.py and tests/test_gpu_odometry_facade.py.
//
//   localize_lines_test self
//       host only: the conformance table, the threshold and the RANSAC parameters, and the bookkeeping that needs no
//       device: the first keyframe, the optimizer hook, deleteLandmarks, deleteKeyframe within the limit
//   localize_lines_test run <fx fy cx cy k1 k2 k3 p1 p2> <x.f64> <visible.f64> <frames> <numOfInliers>
//                           <numOfActiveFrames> <seed> [<refine.f64>]
//       x: raw float64 [frames][n][3], the same n points in each keyframe's camera frame; visible: float64
//       [frames][n], non-zero where the keyframe holds the track.  The points are projected with
//       CameraModel::project, Keyframes are built from patches at those corners (track ids 3 i + 5, timestamps
//       1000 + 50000 k) and a VisualOdometryFrontEnd is run as the body of a keyframe hook; with refine.f64
//       ([frames][12]) a localize refinement returns that keyframe's pose.  One JSON line (%.17g, so that the test
//       reads back the very doubles).
//
// Built with -ffp-contract=off (abspose.mk).
#include <visual_odometry/visual_odometry.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

// ---- conformance with visual_odometry/visual_odometry.h:40-100 (the context handle and the seed are this project's) ----
namespace conformance
{
using namespace visual_odometry;
using F = VisualOdometryFrontEnd;
using K = Keyframe;
static_assert(std::is_constructible<F, ebo_ctx*, const common::CameraModelParams<double>&, const VisualOdometryParams&>::value,
			  "VisualOdometryFrontEnd(ctx, calibration, params)");
static_assert(std::is_constructible<F, ebo_ctx*, const common::CameraModelParams<double>&, const VisualOdometryParams&, uint64_t>::value,
			  "VisualOdometryFrontEnd(ctx, calibration, params, seed)");
static_assert(std::is_same<decltype(&F::newKeyframeCandidate), void (F::*)(K&)>::value, "void newKeyframeCandidate(Keyframe&)");
static_assert(std::is_same<decltype(&F::getMapLandmarks), MapLandmarks const& (F::*)()>::value, "MapLandmarks const& getMapLandmarks()");
static_assert(std::is_same<decltype(&F::getActiveFrames), std::map<size_t, K> const& (F::*)() const>::value,
			  "std::map<size_t, Keyframe> const& getActiveFrames() const");
static_assert(std::is_same<decltype(&F::getStoredFrames), std::list<K> const& (F::*)() const>::value,
			  "std::list<Keyframe> const& getStoredFrames() const");
static_assert(std::is_same<decltype(&F::getStoredLandmarks),
						   std::vector<std::pair<tracker::TrackId, common::Vector3d>> const& (F::*)() const>::value,
			  "std::vector<std::pair<TrackId, Vector3d>> const& getStoredLandmarks() const");
static_assert(std::is_same<decltype(&F::isNewKeyframeNeeded), bool (F::*)(K&, Match&)>::value, "bool isNewKeyframeNeeded(Keyframe&, Match&)");
static_assert(std::is_same<decltype(&F::initCameras), bool (F::*)(K&, Match&)>::value, "bool initCameras(Keyframe&, Match&)");
static_assert(std::is_same<decltype(&F::localizeCamera), void (F::*)(const K&, Match&)>::value, "void localizeCamera(const Keyframe&, Match&)");
static_assert(std::is_same<decltype(&F::addKeyframe), void (F::*)(const K&, const Match&)>::value, "void addKeyframe(const Keyframe&, const Match&)");
static_assert(std::is_same<decltype(&F::addNewLandmarks), void (F::*)(const K&, const Match&)>::value,
			  "void addNewLandmarks(const Keyframe&, const Match&)");
static_assert(std::is_same<decltype(&F::deleteKeyframe), void (F::*)()>::value, "void deleteKeyframe()");
static_assert(std::is_same<decltype(&F::deleteLandmarks), void (F::*)(const K&)>::value, "void deleteLandmarks(const Keyframe&)");
static_assert(std::is_same<decltype(&F::localizeThreshold), double (F::*)() const>::value, "double localizeThreshold() const");
static_assert(std::is_same<decltype(&F::setOptimizer), void (F::*)(F::Optimizer)>::value, "void setOptimizer(Optimizer)");
static_assert(std::is_same<decltype(&F::setLocalizeRefinement), void (F::*)(F::LocalizeRefinement)>::value,
			  "void setLocalizeRefinement(LocalizeRefinement)");
static_assert(std::is_same<F::Optimizer, std::function<void(std::map<size_t, K>&, MapLandmarks&)>>::value, "Optimizer");
static_assert(std::is_same<decltype(&F::lastMatch), const Match& (F::*)() const>::value, "const Match& lastMatch() const");
static_assert(std::is_same<decltype(&F::lastLocalize), const ebo_two_view_result& (F::*)() const>::value, "lastLocalize()");
static_assert(std::is_same<decltype(&F::twoView), TwoViewInitializer& (F::*)()>::value, "TwoViewInitializer& twoView()");
}  // namespace conformance

namespace
{
int fail(const char* what)
{
	std::fprintf(stderr, "self check failed: %s\n", what);
	return 1;
}

std::vector<double> readAll(const char* path)
{
	std::vector<double> v;
	FILE* f = std::fopen(path, "rb");
	if (!f)
	{
		std::fprintf(stderr, "cannot open %s\n", path);
		std::exit(2);
	}
	double buf[1024];
	size_t n;
	while ((n = std::fread(buf, sizeof(double), 1024, f)) > 0)
	{
		v.insert(v.end(), buf, buf + n);
	}
	std::fclose(f);
	return v;
}

// host only: nothing here touches the device (the context pointer is never used)
int self()
{
	common::CameraModelParams<double> calib{};
	visual_odometry::VisualOdometryParams vp;
	visual_odometry::VisualOdometryFrontEnd fe(nullptr, calib, vp, 3);
	// visual_odometry.cpp:240-241 at the default reprojectionError = 3: a float
	const float want = static_cast<float>(1.0 - std::cos(std::atan2(3.0, 200.)));
	if (fe.localizeThreshold() != static_cast<double>(want) || !(fe.localizeThreshold() > 1.1e-4 && fe.localizeThreshold() < 1.2e-4))
	{
		return fail("localizeThreshold");
	}
	if (fe.ransacParams().threshold != fe.localizeThreshold() || fe.ransacParams().seed != 3 || fe.ransacParams().max_iterations != 1000 ||
		fe.ransacParams().probability != 0.99)
	{
		return fail("RANSAC parameters");
	}
	if (fe.twoView().ransacParams().threshold != vp.ransacThreshold || fe.twoView().ransacParams().seed != 3)
	{
		return fail("two-view RANSAC parameters");
	}
	if (!fe.getActiveFrames().empty() || !fe.getStoredFrames().empty() || !fe.getStoredLandmarks().empty() ||
		!fe.getMapLandmarks().landmarks.empty() || !fe.getMapLandmarks().observations.empty())
	{
		return fail("a new front end is empty");
	}
	// the first candidate: identity pose, every landmark an "inlier", one observation each, no triangulation (and so
	// no device call); the optimizer hook sees the active set
	tracker::Patches patches;
	for (const int id : {7, 3, 11})
	{
		tracker::Patch p(tracker::Corner(10.0 + id, 20.0 + 2 * id), 4, common::timestamp_t(1000));
		p.setTrackId(id);
		patches.push_back(p);
	}
	visual_odometry::Keyframe k1(patches, common::timestamp_t(1000));
	k1.pose = common::Pose3d(common::Matrix3d::Identity(), common::Vector3d(1.0, 2.0, 3.0));
	int calls = 0;
	size_t seenActive = 0;
	fe.setOptimizer([&](std::map<size_t, visual_odometry::Keyframe>& active, visual_odometry::MapLandmarks&) {
		++calls;
		seenActive = active.size();
	});
	fe.newKeyframeCandidate(k1);
	if (k1.pose.translation()[0] != 0.0 || fe.getActiveFrames().size() != 1 || fe.getActiveFrames().count(1000) != 1)
	{
		return fail("the first keyframe is added at the identity");
	}
	if (calls != 1 || seenActive != 1) return fail("optimizer hook");
	if (fe.lastMatch().inliers.size() != 3 || fe.getMapLandmarks().observations.size() != 3 || !fe.getMapLandmarks().landmarks.empty())
	{
		return fail("first keyframe: one observation per landmark, nothing triangulated");
	}
	for (const auto& obs : fe.getMapLandmarks().observations)
	{
		if (obs.second.size() != 1 || obs.second.front() != 1000) return fail("observation lists");
	}
	// deleteLandmarks: the keyframe leaves the lists, tracks nobody observes leave the map (no landmark: nothing stored)
	fe.deleteLandmarks(k1);
	if (!fe.getMapLandmarks().observations.empty() || !fe.getStoredLandmarks().empty()) return fail("deleteLandmarks");
	// deleteKeyframe does nothing while the active set is within numOfActiveFrames
	fe.deleteKeyframe();
	if (fe.getActiveFrames().size() != 1 || !fe.getStoredFrames().empty()) return fail("deleteKeyframe within the limit");
	std::printf("{\"self\": \"ok\", \"threshold\": %.17g}\n", fe.localizeThreshold());
	return 0;
}

void printPose(const common::Pose3d& T)
{
	double m[12];
	T.toArray(m);
	std::printf("[");
	for (int i = 0; i < 12; ++i)
	{
		std::printf("%s%.17g", i ? ", " : "", m[i]);
	}
	std::printf("]");
}

template <class C>
void printInts(const C& v)
{
	std::printf("[");
	bool first = true;
	for (const auto x : v)
	{
		std::printf("%s%lld", first ? "" : ", ", static_cast<long long>(x));
		first = false;
	}
	std::printf("]");
}

int run(int argc, char** argv)
{
	double nine[9];
	for (int i = 0; i < 9; ++i)
	{
		nine[i] = std::strtod(argv[2 + i], nullptr);
	}
	const auto cam = common::CameraModel<double>::fromData(nine);
	const std::vector<double> x = readAll(argv[11]), vis = readAll(argv[12]);
	const size_t frames = std::strtoul(argv[13], nullptr, 10);
	visual_odometry::VisualOdometryParams vp;
	vp.numOfInliers = std::strtoul(argv[14], nullptr, 10);
	vp.numOfActiveFrames = std::strtoul(argv[15], nullptr, 10);
	const uint64_t seed = std::strtoull(argv[16], nullptr, 10);
	std::vector<double> refine;
	if (argc == 18)
	{
		refine = readAll(argv[17]);
	}
	if (frames == 0 || vis.size() % frames != 0 || x.size() != 3 * vis.size() || (!refine.empty() && refine.size() != 12 * frames))
	{
		std::fprintf(stderr, "the input files do not fit the frame count\n");
		return 2;
	}
	const size_t n = vis.size() / frames;
	ebo_params prm;
	ebo_default_params(&prm);
	ebo_ctx* ctx = nullptr;
	if (ebo_create(&prm, &ctx) != EBO_OK)
	{
		std::fprintf(stderr, "ebo_create: %s\n", ebo_last_error(nullptr));
		return 3;
	}
	{
		common::CameraModelParams<double> calib;
		std::memcpy(&calib, nine, sizeof(calib));
		visual_odometry::VisualOdometryFrontEnd frontEnd(ctx, calib, vp, seed);
		size_t current = 0;
		if (!refine.empty())
		{
			frontEnd.setLocalizeRefinement([&](const common::Pose3d&, const visual_odometry::bearingVectors_t&,
											   const std::vector<common::Vector3d>&,
											   const std::vector<int>&) { return common::Pose3d(refine.data() + 12 * current); });
		}
		std::vector<std::vector<size_t>> optimizerCalls;
		frontEnd.setOptimizer([&](std::map<size_t, visual_odometry::Keyframe>& active, visual_odometry::MapLandmarks&) {
			std::vector<size_t> keys;
			for (const auto& kf : active)
			{
				keys.push_back(kf.first);
			}
			optimizerCalls.push_back(keys);
		});
		typedef common::CameraModel<double>::Vec3 Vec3;
		std::printf("{\"threshold\": %.17g, \"candidates\": [", frontEnd.localizeThreshold());
		// the front end as the body of a keyframe hook (tools::Evaluator::KeyframeHook's signature)
		const std::function<void(const tracker::Patches&, const common::timestamp_t&)> hook =
			[&](const tracker::Patches& patches, const common::timestamp_t& t) {
				visual_odometry::Keyframe keyframe(patches, t);
				frontEnd.newKeyframeCandidate(keyframe);
				const bool added = frontEnd.getActiveFrames().count(static_cast<size_t>(t.count())) != 0;
				const ebo_two_view_result& r = frontEnd.lastLocalize();
				std::printf("%s{\"timestamp\": %lld, \"added\": %s, \"pose\": ", current ? ", " : "", static_cast<long long>(t.count()),
							added ? "true" : "false");
				printPose(keyframe.pose);
				std::printf(", \"Tw2c\": ");
				printPose(frontEnd.lastMatch().Tw2c);
				std::printf(", \"inliers\": ");
				printInts(frontEnd.lastMatch().inliers);
				std::printf(", \"localize\": [%d, %d, %d, %d]}", r.found, r.winner, r.iterations, r.n_inliers);
			};
		for (size_t k = 0; k < frames; ++k)
		{
			current = k;
			const common::timestamp_t t(1000 + 50000 * static_cast<long long>(k));
			tracker::Patches patches;
			for (size_t j = 0; j < n; ++j)
			{
				const size_t i = n - 1 - j;  // track ids that are neither dense nor in list order
				if (vis[k * n + i] == 0.0)
				{
					continue;
				}
				const double* p = &x[3 * (k * n + i)];
				const auto u = cam->project(Vec3(p[0], p[1], p[2]));
				tracker::Patch patch(tracker::Corner(u[0], u[1]), 4, t);
				patch.setTrackId(static_cast<tracker::TrackId>(3 * i + 5));
				patches.push_back(patch);
			}
			hook(patches, t);
		}
		std::printf("], \"active\": [");
		bool first = true;
		for (const auto& kf : frontEnd.getActiveFrames())
		{
			std::printf("%s[%zu, ", first ? "" : ", ", kf.first);
			printPose(kf.second.pose);
			std::printf("]");
			first = false;
		}
		std::printf("], \"stored_frames\": [");
		first = true;
		for (const auto& kf : frontEnd.getStoredFrames())
		{
			std::printf("%s[%lld, ", first ? "" : ", ", static_cast<long long>(kf.timestamp.count()));
			printPose(kf.pose);
			std::printf("]");
			first = false;
		}
		std::vector<tracker::TrackId> ids;
		for (const auto& lm : frontEnd.getMapLandmarks().landmarks)
		{
			ids.push_back(lm.first);
		}
		std::sort(ids.begin(), ids.end());
		std::printf("], \"landmarks\": [");
		for (size_t i = 0; i < ids.size(); ++i)
		{
			const common::Vector3d& p = frontEnd.getMapLandmarks().landmarks.at(ids[i]);
			std::printf("%s[%d, %.17g, %.17g, %.17g]", i ? ", " : "", ids[i], p[0], p[1], p[2]);
		}
		ids.clear();
		for (const auto& obs : frontEnd.getMapLandmarks().observations)
		{
			ids.push_back(obs.first);
		}
		std::sort(ids.begin(), ids.end());
		std::printf("], \"observations\": [");
		for (size_t i = 0; i < ids.size(); ++i)
		{
			std::printf("%s[%d, ", i ? ", " : "", ids[i]);
			printInts(frontEnd.getMapLandmarks().observations.at(ids[i]));
			std::printf("]");
		}
		std::printf("], \"stored_landmarks\": [");
		first = true;
		for (const auto& lm : frontEnd.getStoredLandmarks())
		{
			std::printf("%s[%d, %.17g, %.17g, %.17g]", first ? "" : ", ", lm.first, lm.second[0], lm.second[1], lm.second[2]);
			first = false;
		}
		std::printf("], \"optimizer_calls\": [");
		for (size_t i = 0; i < optimizerCalls.size(); ++i)
		{
			std::printf("%s", i ? ", " : "");
			printInts(optimizerCalls[i]);
		}
		std::printf("]}\n");
	}
	ebo_destroy(ctx);
	return 0;
}
}  // namespace

int main(int argc, char** argv)
{
	if (argc >= 2 && std::strcmp(argv[1], "self") == 0)
	{
		return self();
	}
	if ((argc == 17 || argc == 18) && std::strcmp(argv[1], "run") == 0)
	{
		return run(argc, argv);
	}
	std::fprintf(stderr,
				 "usage: %s self | run <nine camera parameters> <x.f64> <visible.f64> <frames> <numOfInliers> <numOfActiveFrames> <seed> "
				 "[<refine.f64>]\n",
				 argv[0]);
	return 2;
}
