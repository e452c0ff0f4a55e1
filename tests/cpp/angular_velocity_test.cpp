// angular_velocity_test.cpp — tracker::AngularVelocityEstimator (feature_tracker/angular_velocity.h) against the C ABI.
//
//   angular_velocity_test <events.bin> <w> <h> <fx> <fy> <cx> <cy>
//
// events.bin is an ebo_write_events_bin file holding ONE window.  The program loads it into a context, estimates
// through the facade and through ebo_solve_rotation directly, and checks that both give the same bits; that the image
// of rotationally compensated events is ebo_rotation_image's; that cameraFor returns the recording's pinhole camera
// when there is no rectification, the rectified camera when one is set, and refuses a distorted camera without one
// with a message that names --rectify; that estimateWindows, which loads chunk by chunk, gives the bits of the resident
// windows and leaves a refused window without an estimate.  Prints "omega wx wy wz status iterations evaluations" (%.17g) and "all passed".
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "feature_tracker/angular_velocity.h"

static int fails = 0;
#define CHECK(cond)                                                       \
	do                                                                    \
	{                                                                     \
		if (!(cond))                                                      \
		{                                                                 \
			std::printf("FAILED line %d: %s\n", __LINE__, #cond);         \
			++fails;                                                      \
		}                                                                 \
	} while (0)

int main(int argc, char** argv)
{
	if (argc != 8)
	{
		std::fprintf(stderr, "usage: angular_velocity_test <events.bin> <w> <h> <fx> <fy> <cx> <cy>\n");
		return 2;
	}
	const int w = std::atoi(argv[2]), h = std::atoi(argv[3]);
	common::CameraModelParams<double> pinhole;
	pinhole.fx = std::atof(argv[4]);
	pinhole.fy = std::atof(argv[5]);
	pinhole.cx = std::atof(argv[6]);
	pinhole.cy = std::atof(argv[7]);
	std::vector<ebo_event> ev(1u << 20);
	size_t n = 0;
	if (ebo_read_events_bin(argv[1], ev.data(), ev.size(), &n) != EBO_OK || n == 0)
	{
		std::fprintf(stderr, "cannot read %s\n", argv[1]);
		return 2;
	}
	ebo_params prm;
	ebo_default_params(&prm);
	prm.image_w = w;
	prm.image_h = h;
	prm.loss = EBO_LOSS_VARIANCE;
	ebo_ctx* ctx = nullptr;
	if (ebo_create(&prm, &ctx) != EBO_OK)
	{
		std::fprintf(stderr, "ebo_create: %s\n", ebo_last_error(nullptr));
		return 2;
	}
	// the camera: no rectification and no distortion -> the recording's own
	const common::CameraModelParams<double> cam = tracker::AngularVelocityEstimator::cameraFor(ctx, pinhole);
	CHECK(cam.fx == pinhole.fx && cam.fy == pinhole.fy && cam.cx == pinhole.cx && cam.cy == pinhole.cy && cam.k1 == 0);
	// a distorted camera with no rectification is refused, and the message says what to do
	common::CameraModelParams<double> lens = pinhole;
	lens.k1 = -0.3;
	bool refused = false;
	try
	{
		tracker::AngularVelocityEstimator::cameraFor(ctx, lens);
	}
	catch (const std::runtime_error& e)
	{
		refused = std::strstr(e.what(), "--rectify") != nullptr;
	}
	CHECK(refused);

	CHECK(ebo_set_window(ctx, ev.data(), n) == EBO_OK);
	tracker::AngularVelocityEstimator av(cam);
	CHECK(av.params().sigma_blur == 1.0 && av.solver().max_iterations == 100);
	std::vector<double> image;
	const std::vector<tracker::AngularVelocityEstimate> est = av.estimate(ctx, &image);
	CHECK(est.size() == 1);
	// the C ABI directly
	double omega[3] = {0, 0, 0};
	ebo_rot_summary s{};
	const ebo_camera k = common::toEboCamera(cam);
	const ebo_rotation_params rp = tracker::defaultRotationParams();
	const ebo_rot_solver_opts so = tracker::defaultRotationSolver();
	CHECK(ebo_solve_rotation(ctx, &k, &rp, &so, nullptr, omega, &s) == EBO_OK);
	CHECK(std::memcmp(omega, est[0].omega.data(), sizeof(omega)) == 0);
	CHECK(std::memcmp(&s, &est[0].summary, sizeof(s)) == 0);
	int64_t tRef = 0;
	uint64_t nEv = 0;
	CHECK(ebo_window_info(ctx, 0, &tRef, &nEv) == EBO_OK && tRef == est[0].tRefUs && nEv == est[0].events);
	std::vector<double> direct(static_cast<size_t>(w) * h);
	CHECK(image.size() == direct.size());
	CHECK(ebo_rotation_image(ctx, &k, omega, nullptr, direct.data()) == EBO_OK);
	CHECK(image.size() == direct.size() && std::memcmp(image.data(), direct.data(), direct.size() * sizeof(double)) == 0);
	// a start of its own and one iteration
	ebo_rot_solver_opts one = so;
	one.max_iterations = 1;
	av.setSolver(one);
	const std::vector<double> start = {omega[0], omega[1], omega[2]};
	const auto again = av.estimate(ctx, nullptr, &start);
	CHECK(again.size() == 1 && again[0].summary.iterations <= 1);
	// windows that are not resident, in chunks of what a context admits: five slices of the window, a context of two
	// windows at a time -- the same bits as all five resident in a larger context; a window the loader refuses (a
	// coordinate outside the event record's range) gets its entry without an estimate and costs no other window
	{
		av.setSolver(so);
		std::vector<ebo_event> five(ev.begin(), ev.begin() + n);
		std::vector<size_t> off;
		for (size_t w = 0; w <= 5; ++w)
		{
			off.push_back(n * w / 5);
		}
		ebo_params big = prm, small = prm;
		big.max_windows = 5;
		small.max_windows = 2;
		ebo_ctx *ctx5 = nullptr, *ctx2 = nullptr;
		CHECK(ebo_create(&big, &ctx5) == EBO_OK && ebo_create(&small, &ctx2) == EBO_OK);
		CHECK(ebo_set_windows(ctx5, five.data(), off.data(), 5) == EBO_OK);
		const auto resident = av.estimate(ctx5);
		CHECK(ebo_set_windows(ctx2, five.data(), off.data(), 5) != EBO_OK);  // more than the context admits
		const auto chunked = av.estimateWindows(ctx2, five, off, 2);
		CHECK(resident.size() == 5 && chunked.size() == 5);
		for (size_t w = 0; w < 5 && w < resident.size() && w < chunked.size(); ++w)
		{
			CHECK(std::memcmp(resident[w].omega.data(), chunked[w].omega.data(), 3 * sizeof(double)) == 0);
			CHECK(std::memcmp(&resident[w].summary, &chunked[w].summary, sizeof(ebo_rot_summary)) == 0);
			CHECK(resident[w].tRefUs == chunked[w].tRefUs && resident[w].events == chunked[w].events);
		}
		five[off[3] + 7].x = 20000;
		const auto holed = av.estimateWindows(ctx2, five, off, 2);
		CHECK(holed.size() == 5);
		for (size_t w = 0; w < 5 && w < holed.size(); ++w)
		{
			if (w == 3)
			{
				CHECK(holed[w].summary.status == EBO_ROT_RUNNING && holed[w].omega[0] == 0.0 && holed[w].events == off[4] - off[3]);
				CHECK(holed[w].tRefUs == chunked[w].tRefUs);
			}
			else
			{
				CHECK(std::memcmp(holed[w].omega.data(), chunked[w].omega.data(), 3 * sizeof(double)) == 0);
				CHECK(std::memcmp(&holed[w].summary, &chunked[w].summary, sizeof(ebo_rot_summary)) == 0);
			}
		}
		ebo_destroy(ctx5);
		ebo_destroy(ctx2);
	}
	// with a rectification set, the camera is the rectified one whatever the recording's says
	common::CameraModelParams<double> rect = pinhole;
	rect.fx = pinhole.fx * 0.9;
	const ebo_camera lensK = common::toEboCamera(lens), rectK = common::toEboCamera(rect);
	CHECK(ebo_set_rectification_camera(ctx, &lensK, &rectK) == EBO_OK);
	const common::CameraModelParams<double> got = tracker::AngularVelocityEstimator::cameraFor(ctx, lens);
	CHECK(got.fx == rect.fx && got.fy == rect.fy && got.cx == rect.cx && got.cy == rect.cy && got.k1 == 0);
	// the library refuses the distorted camera itself
	tracker::AngularVelocityEstimator bad(lens);
	bool threw = false;
	try
	{
		bad.estimate(ctx);
	}
	catch (const std::runtime_error&)
	{
		threw = true;
	}
	CHECK(threw);
	std::printf("omega %.17g %.17g %.17g %d %d %d\n", omega[0], omega[1], omega[2], s.status, s.iterations, s.evaluations);
	ebo_destroy(ctx);
	if (fails == 0)
	{
		std::printf("all passed\n");
	}
	return fails == 0 ? 0 : 1;
}
