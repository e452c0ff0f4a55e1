// feature_tracker/angular_velocity.h — tracker::AngularVelocityEstimator: the camera's angular velocity from the events
// of whole compensation windows, by rotational contrast maximisation (include/ebo.h, "angular velocity from events",
// rules V1-V9 and N1-N5).  Not in the reference.
//
//   tracker::AngularVelocityEstimator av(tracker::AngularVelocityEstimator::cameraFor(detector.handle(), calibration));
//   detector.compensateEventsContrast(detector.getEvents());       // the window is resident in the detector's context
//   auto est = av.estimate(detector.handle());                      // one estimate per resident window
//   est[0].omega;  est[0].summary.status;  est[0].tRefUs
//
// estimate() works on the windows resident in the context it is given -- the detector's own after a compensation, or
// any context after ebo_set_window* -- and uploads nothing.  Errors of the library are thrown as std::runtime_error.
#pragma once

#include <algorithm>
#include <array>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/ebo.h"
#include "../common/camera_model.h"

namespace tracker
{
struct AngularVelocityEstimate
{
	std::array<double, 3> omega{};  // rad/s, camera frame
	ebo_rot_summary summary{};      // status EBO_ROT_*, iterations, evaluations, r at omega0 and at the result
	int64_t tRefUs = 0;             // the window's reference time
	uint64_t events = 0;            // the window's events
};

inline ebo_rotation_params defaultRotationParams()
{
	ebo_rotation_params p;
	ebo_default_rotation_params(&p);
	return p;
}
inline ebo_rot_solver_opts defaultRotationSolver()
{
	ebo_rot_solver_opts o;
	ebo_default_rot_solver_opts(&o);
	return o;
}

class AngularVelocityEstimator
{
   public:
	explicit AngularVelocityEstimator(const common::CameraModelParams<double>& pinhole,
									  const ebo_rotation_params& params = defaultRotationParams(),
									  const ebo_rot_solver_opts& solver = defaultRotationSolver())
		: camera_(common::toEboCamera(pinhole)), params_(params), solver_(solver)
	{
	}

	// The camera the events of `ctx` live in: the rectified camera when a rectification is set; else the recording's
	// own, when it has no distortion; else nothing can be estimated without rectifying.
	static common::CameraModelParams<double> cameraFor(ebo_ctx* ctx, const common::CameraModelParams<double>& recording)
	{
		common::CameraModelParams<double> out;
		ebo_camera r{};
		if (ctx && ebo_rectified_camera(ctx, &r) == EBO_OK)
		{
			out.fx = r.fx;
			out.fy = r.fy;
			out.cx = r.cx;
			out.cy = r.cy;
			return out;
		}
		if (recording.k1 == 0 && recording.k2 == 0 && recording.p1 == 0 && recording.p2 == 0 && recording.fx != 0 && recording.fy != 0)
		{
			out.fx = recording.fx;
			out.fy = recording.fy;
			out.cx = recording.cx;
			out.cy = recording.cy;
			return out;
		}
		throw std::runtime_error(
			"tracker::AngularVelocityEstimator: the camera has distortion (or no calibration) and no rectification is set: "
			"rectify the events at load (tools::EvaluatorParams::rectifyEvents, track_recording --rectify)");
	}

	const ebo_camera& camera() const { return camera_; }
	const ebo_rotation_params& params() const { return params_; }
	const ebo_rot_solver_opts& solver() const { return solver_; }
	void setParams(const ebo_rotation_params& p) { params_ = p; }
	void setSolver(const ebo_rot_solver_opts& o) { solver_ = o; }

	// One estimate per window resident in ctx, from omega0 = 0 (or omega0 [windows][3]).  images (optional) receives the
	// image of rotationally compensated events of every window at its estimate, double [windows][h][w] row-major.
	std::vector<AngularVelocityEstimate> estimate(ebo_ctx* ctx, std::vector<double>* images = nullptr,
													const std::vector<double>* omega0 = nullptr) const
	{
		int n = 0;
		if (!ctx || ebo_num_windows(ctx, &n) != EBO_OK)
		{
			throw std::runtime_error("tracker::AngularVelocityEstimator: no context");
		}
		if (omega0 && omega0->size() != 3 * static_cast<size_t>(n))
		{
			throw std::runtime_error("tracker::AngularVelocityEstimator: omega0 holds three numbers per resident window");
		}
		std::vector<double> omega(3 * static_cast<size_t>(std::max(n, 1)));
		std::vector<ebo_rot_summary> summary(static_cast<size_t>(std::max(n, 1)));
		check(ctx, ebo_solve_rotation(ctx, &camera_, &params_, &solver_, omega0 ? omega0->data() : nullptr, omega.data(), summary.data()));
		std::vector<AngularVelocityEstimate> out(static_cast<size_t>(n));
		for (int w = 0; w < n; ++w)
		{
			out[w].omega = {omega[3 * w], omega[3 * w + 1], omega[3 * w + 2]};
			out[w].summary = summary[w];
			check(ctx, ebo_window_info(ctx, w, &out[w].tRefUs, &out[w].events));
		}
		if (images)
		{
			int npx = 0, npy = 0, x = 0, y = 0, pw = 0, ph = 0;
			// the sensor's size from the grid: the last patch ends at the sensor's corner
			check(ctx, ebo_grid(ctx, &npx, &npy));
			check(ctx, ebo_patch_rect(ctx, npx - 1, npy - 1, &x, &y, &pw, &ph));
			images->assign(static_cast<size_t>(n) * (x + pw) * (y + ph), 0.0);
			check(ctx, ebo_rotation_image(ctx, &camera_, omega.data(), nullptr, images->data()));
		}
		return out;
	}

	// The same for windows that are NOT resident: window w = events[offsets[w] .. offsets[w + 1]), loaded into ctx in
	// chunks of at most maxWindows (what the context admits) and estimated chunk by chunk.  A chunk the loader refuses
	// is loaded window by window; a window it refuses alone gets no estimate: omega zero, status EBO_ROT_RUNNING, the
	// reference time the loaders would have given it, its event count.  One entry per window, in order.
	std::vector<AngularVelocityEstimate> estimateWindows(ebo_ctx* ctx, const std::vector<ebo_event>& events,
															 const std::vector<size_t>& offsets, size_t maxWindows) const
	{
		std::vector<AngularVelocityEstimate> out;
		const size_t nw = offsets.empty() ? 0 : offsets.size() - 1;
		const size_t cap = std::max<size_t>(1, maxWindows);
		auto load = [&](size_t a, size_t b) {
			std::vector<size_t> off(b - a + 1);
			for (size_t w = a; w <= b; ++w)
			{
				off[w - a] = offsets[w] - offsets[a];
			}
			return ctx && ebo_set_windows(ctx, events.data() + offsets[a], off.data(), static_cast<int>(b - a)) == EBO_OK;
		};
		auto append = [&](const std::vector<AngularVelocityEstimate>& est) { out.insert(out.end(), est.begin(), est.end()); };
		for (size_t a = 0; a < nw; a += cap)
		{
			const size_t b = std::min(nw, a + cap);
			if (load(a, b))
			{
				append(estimate(ctx));
				continue;
			}
			for (size_t w = a; w < b; ++w)
			{
				if (load(w, w + 1))
				{
					append(estimate(ctx));
					continue;
				}
				AngularVelocityEstimate none;
				none.summary.status = EBO_ROT_RUNNING;
				none.events = offsets[w + 1] - offsets[w];
				if (none.events > 0)
				{
					(void)ebo_window_ref_time(events[offsets[w]].t_us, events[offsets[w + 1] - 1].t_us, &none.tRefUs);
				}
				out.push_back(none);
			}
		}
		return out;
	}

   private:
	static void check(ebo_ctx* ctx, int rc)
	{
		if (rc != EBO_OK)
		{
			throw std::runtime_error(std::string("tracker::AngularVelocityEstimator: ") + ebo_last_error(ctx));
		}
	}

	ebo_camera camera_;
	ebo_rotation_params params_;
	ebo_rot_solver_opts solver_;
};
}  // namespace tracker
