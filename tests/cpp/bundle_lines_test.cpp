// bundle_lines_test — the bundle-adjustment members of the odometry façade (visual_odometry/bundle_adjustment.h and the
// two use... members of VisualOdometryFrontEnd), pinned by signature and run on a window handed over in a file.
//
//   bundle_lines_test adjust <problem.f64> <out.f64>
//       problem.f64 is tools/bundle_adjust_serial.cpp's (fix_points 0; the options that follow uv are not read: of
//       the options the façade takes the iteration count alone): frame k becomes the active keyframe with
//       timestamp 1000 (k + 1) holding a patch per observation (track id 3 l + 5 for point l), point l the map's
//       landmark of that track, observed by those keyframes.  Calls visual_odometry::bundleAdjust with the file's Huber
//       width and iteration count and writes iterations, termination, initial and final cost, the keyframes' poses in
//       map order and the landmarks in ascending track id.  The façade fixes the first two frames itself.
//   bundle_lines_test refine <problem.f64> <out.f64>
//       one frame: the observations' uv are read as bearing vectors (u, v, 1) / |(u, v, 1)|, every point an inlier, and
//       visual_odometry::refinePose refines the frame's pose; writes iterations, termination, costs and the pose.
//   bundle_lines_test frontend <fx fy cx cy k1 k2 k3 p1 p2> <x.f64> <visible.f64> <frames> <numOfInliers>
//                               <numOfActiveFrames> <seed> <hooks>
//       localize_lines_test's `run` (the same files, track ids 3 i + 5, timestamps 1000 + 50000 k, patches at the
//       projected corners) with, when hooks is 1, useDeviceBundleAdjustment() and useDeviceLocalizeRefinement()
//       installed: the keyframes go through newKeyframeCandidate.  One JSON line (%.17g): per candidate the
//       timestamp, added, the keyframe's pose as the candidate left it, the match's inliers, the localisation, and
//       (iterations, termination) of the last refinement and of the last bundle adjustment; then the active frames,
//       stored frames, landmarks, observations and stored landmarks as they stand at the end.
#include <cmath>
#include <cstdio>
#include <algorithm>
#include <cstdlib>
#include <string>
#include <type_traits>
#include <vector>

#include <visual_odometry/visual_odometry.h>

using namespace visual_odometry;
using F = VisualOdometryFrontEnd;
static_assert(std::is_same<decltype(&F::useDeviceBundleAdjustment), void (F::*)()>::value, "void useDeviceBundleAdjustment()");
static_assert(std::is_same<decltype(&F::useDeviceLocalizeRefinement), void (F::*)()>::value, "void useDeviceLocalizeRefinement()");
static_assert(std::is_same<decltype(&F::lastBundleAdjustment), const ebo_summary& (F::*)() const>::value, "lastBundleAdjustment()");
static_assert(std::is_same<decltype(&F::lastRefinement), const ebo_summary& (F::*)() const>::value, "lastRefinement()");
static_assert(std::is_same<decltype(&bundleAdjust), ebo_summary (*)(ebo_ctx*, const common::CameraModelParams<double>&, double, size_t,
																	   std::map<size_t, Keyframe>&, MapLandmarks&)>::value,
			  "bundleAdjust");
static_assert(std::is_same<decltype(&refinePose),
						   common::Pose3d (*)(ebo_ctx*, double, size_t, const common::Pose3d&, const bearingVectors_t&,
											  const std::vector<common::Vector3d>&, const std::vector<int>&, ebo_summary*)>::value,
			  "refinePose");

static std::vector<double> readAll(const char* path)
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

static void printPose(const common::Pose3d& pose)
{
	double m[12];
	pose.toArray(m);
	std::printf("[");
	for (int i = 0; i < 12; ++i)
	{
		std::printf("%s%.17g", i ? ", " : "", m[i]);
	}
	std::printf("]");
}

template <class C>
static void printInts(const C& v)
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

static int frontend(char** argv)
{
	double nine[9];
	for (int i = 0; i < 9; ++i)
	{
		nine[i] = std::strtod(argv[2 + i], nullptr);
	}
	const auto cam = common::CameraModel<double>::fromData(nine);
	const std::vector<double> x = readAll(argv[11]), vis = readAll(argv[12]);
	const size_t frames = std::strtoul(argv[13], nullptr, 10);
	VisualOdometryParams vp;
	vp.numOfInliers = std::strtoul(argv[14], nullptr, 10);
	vp.numOfActiveFrames = std::strtoul(argv[15], nullptr, 10);
	const uint64_t seed = std::strtoull(argv[16], nullptr, 10);
	const bool hooks = std::strtoul(argv[17], nullptr, 10) != 0;
	if (frames == 0 || vis.size() % frames != 0 || x.size() != 3 * vis.size())
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
	try
	{
		common::CameraModelParams<double> calib;
		calib.fx = nine[0], calib.fy = nine[1], calib.cx = nine[2], calib.cy = nine[3], calib.k1 = nine[4], calib.k2 = nine[5],
		calib.k3 = nine[6], calib.p1 = nine[7], calib.p2 = nine[8];
		VisualOdometryFrontEnd frontEnd(ctx, calib, vp, seed);
		if (hooks)
		{
			frontEnd.useDeviceBundleAdjustment();
			frontEnd.useDeviceLocalizeRefinement();
		}
		typedef common::CameraModel<double>::Vec3 Vec3;
		std::printf("{\"threshold\": %.17g, \"candidates\": [", frontEnd.localizeThreshold());
		for (size_t k = 0; k < frames; ++k)
		{
			const common::timestamp_t t(1000 + 50000 * static_cast<long long>(k));
			tracker::Patches patches;
			for (size_t j = 0; j < n; ++j)
			{
				const size_t i = n - 1 - j;
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
			Keyframe keyframe(patches, t);
			frontEnd.newKeyframeCandidate(keyframe);
			const bool added = frontEnd.getActiveFrames().count(static_cast<size_t>(t.count())) != 0;
			const ebo_two_view_result& r = frontEnd.lastLocalize();
			std::printf("%s{\"timestamp\": %lld, \"added\": %s, \"pose\": ", k ? ", " : "", static_cast<long long>(t.count()),
						added ? "true" : "false");
			printPose(keyframe.pose);
			std::printf(", \"inliers\": ");
			printInts(frontEnd.lastMatch().inliers);
			std::printf(", \"localize\": [%d, %d, %d, %d], \"refine\": [%d, %d], \"bundle\": [%d, %d]}", r.found, r.winner, r.iterations,
						r.n_inliers, frontEnd.lastRefinement().iterations, frontEnd.lastRefinement().termination,
						frontEnd.lastBundleAdjustment().iterations, frontEnd.lastBundleAdjustment().termination);
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
		std::printf("]}\n");
	}
	catch (const std::exception& e)
	{
		std::fprintf(stderr, "%s\n", e.what());
		ebo_destroy(ctx);
		return 1;
	}
	ebo_destroy(ctx);
	return 0;
}

int main(int argc, char** argv)
{
	if (argc == 18 && std::string(argv[1]) == "frontend")
	{
		return frontend(argv);
	}
	if (argc != 4)
	{
		std::fprintf(stderr, "usage: %s adjust|refine <problem.f64> <out.f64> | frontend <nine camera parameters> <x.f64> <visible.f64> <frames> "
							"<numOfInliers> <numOfActiveFrames> <seed> <hooks>\n", argv[0]);
		return 2;
	}
	const std::string mode = argv[1];
	const std::vector<double> in = readAll(argv[2]);
	const int nF = static_cast<int>(in[0]), nP = static_cast<int>(in[1]), nN = static_cast<int>(in[2]);
	const size_t maxIterations = static_cast<size_t>(in[4]);
	const double huber = in[9];
	common::CameraModelParams<double> calib;
	calib.fx = in[10], calib.fy = in[11], calib.cx = in[12], calib.cy = in[13], calib.k1 = in[14], calib.k2 = in[15], calib.k3 = in[16],
	calib.p1 = in[17], calib.p2 = in[18];
	const double* poses = in.data() + 19;
	const double* points = poses + 13 * nF;
	const double* of = points + 3 * nP;
	const double* op = of + nN;
	const double* uv = op + nN;
	ebo_params prm;
	ebo_default_params(&prm);
	ebo_ctx* ctx = nullptr;
	if (ebo_create(&prm, &ctx) != EBO_OK)
	{
		std::fprintf(stderr, "ebo_create: %s\n", ebo_last_error(nullptr));
		return 1;
	}
	std::vector<double> out;
	try
	{
		if (mode == "adjust")
		{
			std::map<size_t, Keyframe> active;
			MapLandmarks map;
			for (int k = 0; k < nF; ++k)
			{
				tracker::Patches patches;
				for (int i = 0; i < nN; ++i)
				{
					if (static_cast<int>(of[i]) == k)
					{
						tracker::Patch p(tracker::Corner(uv[2 * i], uv[2 * i + 1]), 4, common::timestamp_t(1000 * (k + 1)));
						p.setTrackId(3 * static_cast<int>(op[i]) + 5);
						patches.push_back(p);
					}
				}
				Keyframe kf(patches, common::timestamp_t(1000 * (k + 1)));
				kf.pose = common::Pose3d(poses + 12 * k);
				active[static_cast<size_t>(1000 * (k + 1))] = kf;
			}
			for (int l = 0; l < nP; ++l)
			{
				map.landmarks[3 * l + 5] = common::Vector3d(points[3 * l], points[3 * l + 1], points[3 * l + 2]);
			}
			for (int i = 0; i < nN; ++i)
			{
				map.observations[3 * static_cast<int>(op[i]) + 5].push_back(static_cast<size_t>(1000 * (static_cast<int>(of[i]) + 1)));
			}
			const ebo_summary s = bundleAdjust(ctx, calib, huber, maxIterations, active, map);
			out = {static_cast<double>(s.iterations), static_cast<double>(s.termination), s.initial_cost, s.final_cost};
			for (const auto& kf : active)
			{
				double m[12];
				kf.second.pose.toArray(m);
				out.insert(out.end(), m, m + 12);
			}
			for (int l = 0; l < nP; ++l)
			{
				const common::Vector3d& p = map.landmarks.at(3 * l + 5);
				out.insert(out.end(), {p[0], p[1], p[2]});
			}
		}
		else
		{
			bearingVectors_t f(nP);
			std::vector<common::Vector3d> pts(nP);
			std::vector<int> inliers;
			for (int i = 0; i < nN; ++i)
			{
				const int l = static_cast<int>(op[i]);
				const double n = std::sqrt((uv[2 * i] * uv[2 * i] + uv[2 * i + 1] * uv[2 * i + 1]) + 1.0);
				f[l] = common::Vector3d(uv[2 * i] / n, uv[2 * i + 1] / n, 1.0 / n);
				pts[l] = common::Vector3d(points[3 * l], points[3 * l + 1], points[3 * l + 2]);
			}
			for (int l = 0; l < nP; ++l)
			{
				inliers.push_back(l);
			}
			ebo_summary s{};
			const common::Pose3d refined = refinePose(ctx, huber, maxIterations, common::Pose3d(poses), f, pts, inliers, &s);
			out = {static_cast<double>(s.iterations), static_cast<double>(s.termination), s.initial_cost, s.final_cost};
			double m[12];
			refined.toArray(m);
			out.insert(out.end(), m, m + 12);
			// the bearing vectors' own uv, which is what the refinement saw
			for (int l = 0; l < nP; ++l)
			{
				out.push_back(f[l][0] / f[l][2]);
				out.push_back(f[l][1] / f[l][2]);
			}
		}
	}
	catch (const std::exception& e)
	{
		std::fprintf(stderr, "%s\n", e.what());
		ebo_destroy(ctx);
		return 1;
	}
	ebo_destroy(ctx);
	FILE* fo = std::fopen(argv[3], "wb");
	if (!fo || std::fwrite(out.data(), sizeof(double), out.size(), fo) != out.size())
	{
		std::fprintf(stderr, "cannot write %s\n", argv[3]);
		return 2;
	}
	std::fclose(fo);
	return 0;
}
