// visual_odometry/depth_mapper.h — visual_odometry::DepthMapper: a semi-dense depth map of a reference view from the
// events of compensation windows with known poses, by space-sweep voting (include/ebo.h, "depth from events", rules
// M1-M9).  Not in the reference.
//
//   visual_odometry::DepthMapper mapper(visual_odometry::DepthMapper::cameraFor(detector.handle(), calibration),
//                                       recording->getGroundTruth());
//   mapper.begin(referenceTime);
//   detector.compensateEventsContrast(detector.getEvents());   // the window is resident in the detector's context
//   mapper.addResidentWindows(detector.handle());               // votes it with the pose at its reference time
//   ...
//   visual_odometry::DepthMap map = mapper.finish();            // map.depth, map.points (world frame)
//
// The pose source is a list of timed poses, camera to world, in ascending time; the pose at a window's reference time
// comes from syncGroundTruth (aligner.h), and a window outside the poses' time span is left out.  The volume lives in
// the context of the first addResidentWindows after begin, and every later call has to name the same context.  Nothing
// is uploaded: the windows are the ones a loader of that context made resident.  Errors of the library are thrown as
// std::runtime_error.
#pragma once

#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/ebo.h"
#include "../common/camera_model.h"
#include "aligner.h"

namespace visual_odometry
{
inline ebo_depth_params defaultDepthParams()
{
	ebo_depth_params p;
	ebo_default_depth_params(&p);
	return p;
}

// one window the mapper has seen, in order
struct DepthWindow
{
	int64_t tRefUs = 0;
	uint64_t events = 0;
	bool used = false;  // false: outside the poses' time span, or refused by the loader
	common::Pose3d pose;
};

struct DepthMap
{
	int width = 0, height = 0;
	std::vector<int32_t> index;        // [height][width]: the plane, -1 where not kept
	std::vector<uint32_t> confidence;  // [height][width]: the best plane's votes, in 1/1024 of an event
	std::vector<double> depth;         // [height][width]: 0 where not kept
	std::vector<common::Vector3d> points;        // the kept pixels, row-major, in the world frame
	std::vector<common::Vector3d> pointsCamera;  // the same in the reference camera's frame
	common::Pose3d reference;                    // the reference view, camera to world
};

class DepthMapper
{
   public:
	DepthMapper(const common::CameraModelParams<double>& pinhole, common::GroundTruth poses,
				const ebo_depth_params& params = defaultDepthParams())
		: camera_(common::toEboCamera(pinhole)), params_(params), poses_(std::move(poses))
	{
	}

	// The camera the events of `ctx` live in: the rectified camera when a rectification is set; else the recording's
	// own, when it has no distortion; else nothing can be mapped without rectifying.
	static common::CameraModelParams<double> cameraFor(ebo_ctx* ctx, const common::CameraModelParams<double>& recording)
	{
		common::CameraModelParams<double> out;
		ebo_camera r{};
		const bool rectified = ctx && ebo_rectified_camera(ctx, &r) == EBO_OK;
		if (!rectified)
		{
			if (recording.k1 != 0 || recording.k2 != 0 || recording.p1 != 0 || recording.p2 != 0 || recording.fx == 0 || recording.fy == 0)
			{
				throw std::runtime_error(
					"visual_odometry::DepthMapper: the camera has distortion (or no calibration) and no rectification is set: "
					"rectify the events at load (tools::EvaluatorParams::rectifyEvents, track_recording --rectify)");
			}
			r = common::toEboCamera(recording);
		}
		out.fx = r.fx;
		out.fy = r.fy;
		out.cx = r.cx;
		out.cy = r.cy;
		return out;
	}

	const ebo_camera& camera() const { return camera_; }
	const ebo_depth_params& params() const { return params_; }
	const common::Pose3d& reference() const { return reference_; }
	const std::vector<DepthWindow>& windows() const { return windows_; }
	bool begun() const { return begun_; }

	// The pose of the reference view is the pose source's at referenceTime, which has to lie inside its span.  The
	// volume itself is opened by the first addResidentWindows, in that call's context.
	void begin(const common::timestamp_t& referenceTime)
	{
		const auto pose = syncGroundTruth(poses_, referenceTime);
		if (!pose.has_value())
		{
			throw std::runtime_error("visual_odometry::DepthMapper: the reference time lies outside the poses' time span");
		}
		close();
		reference_ = pose.value();
		windows_.clear();
		begun_ = true;
	}

	// Votes every window resident in ctx with the pose at its reference time.  Returns the number of windows voted.
	// beforeUs: a window whose reference time is not before it takes no part and is not recorded (the windows a
	// tools::EventPump tracks against the map instead of voting them, visual_odometry/map_tracker.h).
	size_t addResidentWindows(ebo_ctx* ctx, int64_t beforeUs = INT64_MAX)
	{
		int n = 0;
		if (!begun_ || !ctx || ebo_num_windows(ctx, &n) != EBO_OK)
		{
			throw std::runtime_error("visual_odometry::DepthMapper: addResidentWindows needs begin() and a context");
		}
		open(ctx);
		std::vector<double> poses(12 * static_cast<size_t>(n > 0 ? n : 1), 0.0);
		std::vector<uint8_t> use(static_cast<size_t>(n > 0 ? n : 1), 0);
		size_t used = 0;
		for (int w = 0; w < n; ++w)
		{
			DepthWindow info;
			check(ebo_window_info(ctx, w, &info.tRefUs, &info.events));
			if (info.tRefUs >= beforeUs)
			{
				continue;
			}
			const auto pose = syncGroundTruth(poses_, common::timestamp_t(info.tRefUs));
			if (pose.has_value())
			{
				info.used = true;
				info.pose = pose.value();
				toAbi(info.pose, &poses[12 * static_cast<size_t>(w)]);
				use[static_cast<size_t>(w)] = 1;
				++used;
			}
			windows_.push_back(info);
		}
		if (n > 0)
		{
			check(ebo_dsi_add_windows(ctx, poses.data(), use.data()));
		}
		return used;
	}

	// The same for windows that are NOT resident: window w = events[offsets[w] .. offsets[w + 1]), loaded into ctx in
	// chunks of at most maxWindows and voted chunk by chunk.  A chunk the loader refuses is loaded window by window; a
	// window it refuses alone is recorded as not used.
	void addWindows(ebo_ctx* ctx, const std::vector<ebo_event>& events, const std::vector<size_t>& offsets, size_t maxWindows)
	{
		const size_t nw = offsets.empty() ? 0 : offsets.size() - 1;
		const size_t cap = maxWindows > 0 ? maxWindows : 1;
		auto load = [&](size_t a, size_t b) {
			std::vector<size_t> off(b - a + 1);
			for (size_t w = a; w <= b; ++w)
			{
				off[w - a] = offsets[w] - offsets[a];
			}
			return ctx && ebo_set_windows(ctx, events.data() + offsets[a], off.data(), static_cast<int>(b - a)) == EBO_OK;
		};
		for (size_t a = 0; a < nw; a += cap)
		{
			const size_t b = a + cap < nw ? a + cap : nw;
			if (load(a, b))
			{
				addResidentWindows(ctx);
				continue;
			}
			for (size_t w = a; w < b; ++w)
			{
				if (load(w, w + 1))
				{
					addResidentWindows(ctx);
					continue;
				}
				DepthWindow none;
				none.events = offsets[w + 1] - offsets[w];
				if (none.events > 0)
				{
					(void)ebo_window_ref_time(events[offsets[w]].t_us, events[offsets[w + 1] - 1].t_us, &none.tRefUs);
				}
				windows_.push_back(none);
			}
		}
	}

	// The depth map of what has been voted; closes the volume.  Without a single addResidentWindows there is no volume
	// and the map is empty (width = height = 0).
	DepthMap finish()
	{
		DepthMap map;
		map.reference = reference_;
		begun_ = false;
		if (!ctx_)
		{
			return map;
		}
		int npx = 0, npy = 0, x = 0, y = 0, pw = 0, ph = 0;
		// the sensor's size from the grid: the last patch ends at the sensor's corner
		check(ebo_grid(ctx_, &npx, &npy));
		check(ebo_patch_rect(ctx_, npx - 1, npy - 1, &x, &y, &pw, &ph));
		map.width = x + pw;
		map.height = y + ph;
		const size_t np = static_cast<size_t>(map.width) * map.height;
		map.index.assign(np, -1);
		map.confidence.assign(np, 0u);
		map.depth.assign(np, 0.0);
		std::vector<double> pts(3 * np, 0.0);
		int kept = 0;
		check(ebo_dsi_depth(ctx_, map.index.data(), map.confidence.data(), map.depth.data(), pts.data(), static_cast<int>(np), &kept));
		for (int i = 0; i < kept; ++i)
		{
			const common::Vector3d p(pts[3 * i], pts[3 * i + 1], pts[3 * i + 2]);
			map.pointsCamera.push_back(p);
			map.points.push_back(reference_ * p);
		}
		close();
		return map;
	}

	~DepthMapper() { close(); }
	DepthMapper(const DepthMapper&) = delete;
	DepthMapper& operator=(const DepthMapper&) = delete;

	// a pose as the C ABI takes it here: R row-major, then t
	static void toAbi(const common::Pose3d& pose, double* out12)
	{
		for (int i = 0; i < 3; ++i)
		{
			for (int j = 0; j < 3; ++j)
			{
				out12[3 * i + j] = pose.rotationMatrix()(i, j);
			}
			out12[9 + i] = pose.translation()[i];
		}
	}

   private:
	void open(ebo_ctx* ctx)
	{
		if (ctx_ == ctx)
		{
			return;
		}
		if (ctx_)
		{
			throw std::runtime_error("visual_odometry::DepthMapper: the volume lives in another context than this call's");
		}
		double ref[12];
		toAbi(reference_, ref);
		ctx_ = ctx;
		const int rc = ebo_dsi_begin(ctx, &camera_, ref, &params_);
		if (rc != EBO_OK)
		{
			ctx_ = nullptr;
			throw std::runtime_error(std::string("visual_odometry::DepthMapper: ") + ebo_last_error(ctx));
		}
	}
	void close()
	{
		if (ctx_)
		{
			(void)ebo_dsi_end(ctx_);
			ctx_ = nullptr;
		}
	}
	void check(int rc) const
	{
		if (rc != EBO_OK)
		{
			throw std::runtime_error(std::string("visual_odometry::DepthMapper: ") + ebo_last_error(ctx_));
		}
	}

	ebo_camera camera_;
	ebo_depth_params params_;
	common::GroundTruth poses_;
	common::Pose3d reference_;
	std::vector<DepthWindow> windows_;
	ebo_ctx* ctx_ = nullptr;
	bool begun_ = false;
};
}  // namespace visual_odometry
