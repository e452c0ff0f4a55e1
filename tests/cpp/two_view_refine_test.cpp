// Driver of the two-view facade's device refinement (visual_odometry/relative_refinement.h,
// TwoViewInitializer::useDeviceRefinement, VisualOdometryFrontEnd::twoView()) for tests/test_gpu_twoview_refine_facade.py.
//
//   two_view_refine_test init <fx fy cx cy k1 k2 k3 p1 p2> <x1.f64> <x2.f64> <numOfInliers> <seed> <refine: 0 | 1> <front end: 0 | 1>
//       x1 / x2: raw float64 [n][3], the same n points in the frames of camera 1 and camera 2, turned into two Keyframes
//       exactly as two_view_lines_test does (same corners, same track ids 3 i + 5, same order of the patches).  With
//       `front end` 0 a TwoViewInitializer is run as the body of a keyframe hook; with 1 a VisualOdometryFrontEnd is,
//       and the refinement is installed through its twoView().  One JSON line (%.17g): the RANSAC's answer, the
//       refinement's summary, the match and the second keyframe's pose.
//
// Built with -ffp-contract=off (twoview_refine.mk).
#include <visual_odometry/visual_odometry.h>

#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <type_traits>

namespace
{
using namespace visual_odometry;
static_assert(std::is_same<decltype(&refineRelativePose),
						   common::Pose3d (*)(ebo_ctx*, size_t, const common::Pose3d&, const bearingVectors_t&, const bearingVectors_t&,
											  const std::vector<int>&, ebo_summary*)>::value,
			  "refineRelativePose(ctx, maxNumIterations, model, f1, f2, inliers, summary)");
static_assert(std::is_same<decltype(&TwoViewInitializer::useDeviceRefinement), void (TwoViewInitializer::*)()>::value, "useDeviceRefinement()");
static_assert(std::is_same<decltype(&TwoViewInitializer::lastRefinement), const ebo_summary& (TwoViewInitializer::*)() const>::value,
			  "const ebo_summary& lastRefinement() const");
static_assert(std::is_copy_constructible<TwoViewInitializer>::value, "the initializer stays copyable");

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

void printPose(const char* name, const common::Pose3d& T)
{
	double m[12];
	T.toArray(m);
	std::printf("\"%s\": [", name);
	for (int i = 0; i < 12; ++i)
	{
		std::printf("%s%.17g", i ? ", " : "", m[i]);
	}
	std::printf("]");
}

void report(bool initialised, const ebo_two_view_result& r, const ebo_summary& s, const Match& match, const common::Pose3d& pose)
{
	std::printf("{\"initialised\": %s, \"found\": %d, \"winner\": %d, \"iterations\": %d, \"ransac_inliers\": %d, ", initialised ? "true" : "false",
				r.found, r.winner, r.iterations, r.n_inliers);
	printPose("ransac_model", common::Pose3d(&r.model[0][0]));
	std::printf(", \"refinement\": {\"iterations\": %d, \"num_evals_cost\": %d, \"num_evals_jac\": %d, \"termination\": %d, "
				"\"initial_cost\": %.17g, \"final_cost\": %.17g}, \"inliers\": [",
				s.iterations, s.num_evals_cost, s.num_evals_jac, s.termination, s.initial_cost, s.final_cost);
	for (size_t i = 0; i < match.inliers.size(); ++i)
	{
		std::printf("%s%d", i ? ", " : "", match.inliers[i]);
	}
	std::printf("], ");
	printPose("Tw2c", match.Tw2c);
	std::printf(", ");
	printPose("pose", pose);
	std::printf("}\n");
}

int init(char** argv)
{
	double nine[9];
	for (int i = 0; i < 9; ++i)
	{
		nine[i] = std::strtod(argv[2 + i], nullptr);
	}
	const auto cam = common::CameraModel<double>::fromData(nine);
	const std::vector<double> x1 = readAll(argv[11]), x2 = readAll(argv[12]);
	VisualOdometryParams vp;
	vp.numOfInliers = static_cast<size_t>(std::strtoul(argv[13], nullptr, 10));
	const uint64_t seed = std::strtoull(argv[14], nullptr, 10);
	const bool refine = std::atoi(argv[15]) != 0, frontEnd = std::atoi(argv[16]) != 0;
	const size_t n = x1.size() / 3;
	if (x2.size() != x1.size() || n == 0)
	{
		std::fprintf(stderr, "the two point files differ in length\n");
		return 2;
	}
	typedef common::CameraModel<double>::Vec3 Vec3;
	tracker::Patches patches1, patches2;
	for (size_t k = 0; k < n; ++k)
	{
		const size_t i = n - 1 - k;
		const auto u1 = cam->project(Vec3(x1[3 * i], x1[3 * i + 1], x1[3 * i + 2]));
		const auto u2 = cam->project(Vec3(x2[3 * i], x2[3 * i + 1], x2[3 * i + 2]));
		tracker::Patch p1(tracker::Corner(u1[0], u1[1]), 4, common::timestamp_t(1000));
		tracker::Patch p2(tracker::Corner(u2[0], u2[1]), 4, common::timestamp_t(51000));
		p1.setTrackId(static_cast<tracker::TrackId>(3 * i + 5));
		p2.setTrackId(static_cast<tracker::TrackId>(3 * i + 5));
		patches1.push_back(p1);
		patches2.push_front(p2);
	}
	tracker::Patch lone(tracker::Corner(50.0, 60.0), 4, common::timestamp_t(1000));
	lone.setTrackId(1);
	patches1.push_back(lone);

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
		Keyframe k1(patches1, common::timestamp_t(1000)), k2(patches2, common::timestamp_t(51000));
		if (frontEnd)
		{
			VisualOdometryFrontEnd fe(ctx, calib, vp, seed);
			if (refine)
			{
				fe.twoView().useDeviceRefinement();
			}
			k1.pose = common::Pose3d();
			Match match;
			const bool ok = fe.twoView().initCameras(k1, k2, match);
			report(ok, fe.twoView().lastRansac(), fe.twoView().lastRefinement(), match, k2.pose);
		}
		else
		{
			TwoViewInitializer initializer(ctx, calib, vp, seed);
			if (refine)
			{
				initializer.useDeviceRefinement();
			}
			initializer.newKeyframeCandidate(k1);
			initializer.newKeyframeCandidate(k2);
			report(initializer.initialised(), initializer.lastRansac(), initializer.lastRefinement(), initializer.match(),
				   initializer.secondKeyframe().pose);
		}
	}
	ebo_destroy(ctx);
	return 0;
}
}  // namespace

int main(int argc, char** argv)
{
	if (argc == 17 && std::strcmp(argv[1], "init") == 0)
	{
		return init(argv);
	}
	std::fprintf(stderr, "usage: %s init <nine camera parameters> <x1.f64> <x2.f64> <numOfInliers> <seed> <refine 0|1> <front end 0|1>\n", argv[0]);
	return 2;
}
