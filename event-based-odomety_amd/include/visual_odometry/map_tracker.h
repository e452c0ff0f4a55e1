// visual_odometry/map_tracker.h — visual_odometry::MapTracker: the camera's pose from the events of compensation windows
// and a map of world points, by aligning the map to each window's blurred event image (include/ebo.h, "pose from events
// against a map", rules E1-E9).  Not in the reference.
//
//   visual_odometry::MapTracker tracker(camera, map.points);           // e.g. DepthMapper::finish()'s points
//   tracker.starts = 13;                                                // the prediction and +- one step per direction
//   detector.compensateEventsContrast(detector.getEvents());           // the window is resident in the detector's context
//   tracker.trackResidentWindows(detector.handle(), 0, pose);          // chained: pose in, the last window's pose out
//   tracker.trackResidentWindows(batchContext, timedPoses);            // or with a prior: every window in one launch
//
// Poses are 12 doubles, R row-major and then t, camera to world (DepthMapper::toAbi).  Nothing of the windows is uploaded:
// they are the ones a loader of that context made resident, their images are made once per call on the device and stay
// there.  Among a window's units the winner is the one with the lowest final cost whose termination is not 2, ties to the
// lowest index; a window without a winner keeps its start pose and is reported as lost.  Errors of the library are thrown
// as std::runtime_error.
#pragma once

#include <algorithm>
#include <cstdint>
#include <stdexcept>
#include <string>
#include <vector>

#include "../../../include/ebo.h"
#include "../common/camera_model.h"
#include "aligner.h"
#include "depth_mapper.h"

namespace visual_odometry
{
inline ebo_solver_opts defaultMapTrackOpts()
{
	ebo_solver_opts o;
	ebo_default_map_track_opts(&o);
	return o;
}

// one window the tracker has seen, in order
struct MapTrackWindow
{
	int64_t tRefUs = 0;
	uint64_t events = 0;
	bool lost = true;
	int winner = -1;                // index among the window's starts, -1 when lost
	ebo_map_track_result result{};  // the winner's (all zero when lost)
	double start[12] = {};          // the pose the window started from (start 0 of its units)
	double pose[12] = {};           // the winner's pose, or the start when lost
};

class MapTracker
{
   public:
	MapTracker(const common::CameraModelParams<double>& pinhole, const std::vector<common::Vector3d>& map,
			   const ebo_solver_opts& opts = defaultMapTrackOpts(), double zMin = 0.05)
		: opts(opts), zMin(zMin), camera_(common::toEboCamera(pinhole))
	{
		ebo_default_rotation_params(&eventImage);
		points_.reserve(3 * map.size());
		for (const auto& p : map)
		{
			points_.push_back(p[0]);
			points_.push_back(p[1]);
			points_.push_back(p[2]);
		}
	}

	ebo_solver_opts opts;
	double zMin;
	ebo_rotation_params eventImage;  // sigma_blur of the event images
	int starts = 1;                  // 1 or 13
	double translationStep = 0.05;   // of the 12 extra starts, through B4's update
	double rotationStep = 0.015;

	const ebo_camera& camera() const { return camera_; }
	size_t mapPoints() const { return points_.size() / 3; }
	const std::vector<MapTrackWindow>& windows() const { return windows_; }

	// The winner rule on one window's results: -1 when every unit failed.
	static int winnerOf(const ebo_map_track_result* results, int n)
	{
		int best = -1;
		for (int i = 0; i < n; ++i)
		{
			if (results[i].termination != 2 && (best < 0 || results[i].final_cost < results[best].final_cost))
			{
				best = i;
			}
		}
		return best;
	}

	// Chained: windows firstWindow .. of those resident in ctx, in order; window k starts from window k - 1's result, the
	// first from pose, which is left holding the last window's.  One launch of `starts` units per window.  omegas
	// ([resident windows][3], e.g. the angular-velocity estimates) sharpen the images; null: zeros.  Returns the number of
	// windows tracked (not lost).
	size_t trackResidentWindows(ebo_ctx* ctx, int firstWindow, double* pose, const double* omegas = nullptr)
	{
		const int n = residentWindows(ctx);
		checkStarts();
		size_t tracked = 0;
		bool made = false;
		for (int w = firstWindow < 0 ? 0 : firstWindow; w < n; ++w)
		{
			MapTrackWindow info;
			check(ctx, ebo_window_info(ctx, w, &info.tRefUs, &info.events));
			std::vector<double> poses(12 * static_cast<size_t>(starts));
			fillStarts(pose, poses.data());
			const std::vector<int> unitWindow(static_cast<size_t>(starts), w);
			std::vector<ebo_map_track_result> results(static_cast<size_t>(starts));
			check(ctx, ebo_map_track_resident(ctx, &camera_, &eventImage, omegas, made ? 0 : 1, static_cast<int>(mapPoints()),
											   points_.data(), starts, unitWindow.data(), poses.data(), zMin, &opts, results.data(), nullptr));
			made = true;
			take(info, pose, poses.data(), results.data());
			std::copy(info.pose, info.pose + 12, pose);
			tracked += info.lost ? 0 : 1;
			windows_.push_back(info);
		}
		return tracked;
	}

	// With a prior: every resident window starts from the prior's pose at its reference time (syncGroundTruth), all windows
	// in one launch.  A window outside the prior's time span is not solved and is reported as lost.
	size_t trackResidentWindows(ebo_ctx* ctx, const common::GroundTruth& prior, const double* omegas = nullptr)
	{
		const int n = residentWindows(ctx);
		checkStarts();
		std::vector<MapTrackWindow> infos(static_cast<size_t>(n));
		std::vector<double> poses;
		std::vector<int> unitWindow, owner;
		for (int w = 0; w < n; ++w)
		{
			MapTrackWindow& info = infos[static_cast<size_t>(w)];
			check(ctx, ebo_window_info(ctx, w, &info.tRefUs, &info.events));
			const auto at = syncGroundTruth(prior, common::timestamp_t(info.tRefUs));
			if (!at.has_value())
			{
				continue;
			}
			DepthMapper::toAbi(at.value(), info.start);
			poses.resize(poses.size() + 12 * static_cast<size_t>(starts));
			fillStarts(info.start, poses.data() + poses.size() - 12 * static_cast<size_t>(starts));
			unitWindow.insert(unitWindow.end(), static_cast<size_t>(starts), w);
			owner.push_back(w);
		}
		std::vector<ebo_map_track_result> results(unitWindow.size() ? unitWindow.size() : 1);
		if (!unitWindow.empty())
		{
			check(ctx, ebo_map_track_resident(ctx, &camera_, &eventImage, omegas, 1, static_cast<int>(mapPoints()), points_.data(),
											   static_cast<int>(unitWindow.size()), unitWindow.data(), poses.data(), zMin, &opts,
											   results.data(), nullptr));
		}
		size_t tracked = 0;
		for (size_t k = 0; k < owner.size(); ++k)
		{
			MapTrackWindow& info = infos[static_cast<size_t>(owner[k])];
			const double start[12] = {info.start[0], info.start[1], info.start[2], info.start[3], info.start[4],  info.start[5],
									  info.start[6], info.start[7], info.start[8], info.start[9], info.start[10], info.start[11]};
			take(info, start, poses.data() + 12 * starts * k, results.data() + starts * k);
			tracked += info.lost ? 0 : 1;
		}
		windows_.insert(windows_.end(), infos.begin(), infos.end());
		return tracked;
	}

   private:
	static int residentWindows(ebo_ctx* ctx)
	{
		int n = 0;
		if (!ctx || ebo_num_windows(ctx, &n) != EBO_OK)
		{
			throw std::runtime_error("visual_odometry::MapTracker: trackResidentWindows needs a context");
		}
		return n;
	}
	void checkStarts() const
	{
		if (starts != 1 && starts != 13)
		{
			throw std::runtime_error("visual_odometry::MapTracker: starts is 1 or 13");
		}
	}
	void fillStarts(const double* pose, double* out) const
	{
		if (starts == 13)
		{
			ebo_map_track_starts(pose, translationStep, rotationStep, out);
		}
		else
		{
			std::copy(pose, pose + 12, out);
		}
	}
	// a window's units -> its entry: the winner's pose and result, or the start and lost
	void take(MapTrackWindow& info, const double* start, const double* poses, const ebo_map_track_result* results) const
	{
		std::copy(start, start + 12, info.start);
		info.winner = winnerOf(results, starts);
		info.lost = info.winner < 0;
		if (info.lost)
		{
			std::copy(start, start + 12, info.pose);
			info.result = ebo_map_track_result{};
			return;
		}
		std::copy(poses + 12 * info.winner, poses + 12 * (info.winner + 1), info.pose);
		info.result = results[info.winner];
	}
	static void check(ebo_ctx* ctx, int rc)
	{
		if (rc != EBO_OK)
		{
			throw std::runtime_error(std::string("visual_odometry::MapTracker: ") + ebo_last_error(ctx));
		}
	}

	ebo_camera camera_;
	std::vector<double> points_;
	std::vector<MapTrackWindow> windows_;
};
}  // namespace visual_odometry
