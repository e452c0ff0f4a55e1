// visual_odometry/keyframe.h — Landmarks, Match, MapLandmarks and Keyframe with the reference's members
// (visual_odometry/include/visual_odometry/keyframe.h:10-41, src/keyframe.cpp), over the stand-in vector types of
// common/data_types.h instead of Eigen and Sophus.
#pragma once

#include <list>
#include <unordered_map>
#include <vector>

#include "../common/data_types.h"

#ifdef EBO_HAVE_SOPHUS
#error "visual_odometry/ here is written over the stand-in types of common/data_types.h: with Sophus and Eigen on the include path use the reference's own visual_odometry headers"
#endif
#include "../feature_tracker/patch.h"

namespace visual_odometry
{
using Landmarks = std::unordered_map<tracker::TrackId, common::Vector2d>;

struct Match
{
	common::Pose3d Tw2c;
	std::vector<tracker::TrackId> inliers;
};

struct MapLandmarks
{
	std::unordered_map<tracker::TrackId, common::Vector3d> landmarks;
	std::unordered_map<tracker::TrackId, std::list<size_t>> observations;
};

class Keyframe
{
   public:
	Keyframe() {}
	// keyframe.cpp:5-14: every patch contributes its corner as the landmark of its track
	Keyframe(const tracker::Patches& patches, const common::timestamp_t& timestamp) : timestamp(timestamp)
	{
		for (const tracker::Patch& p : patches)
		{
			const tracker::Corner c = p.toCorner();
			landmarks_[p.getTrackId()] = common::Vector2d(c.x, c.y);
		}
	}

	const Landmarks& getLandmarks() const { return landmarks_; }

	// keyframe.cpp:16-31: the tracks that both keyframes hold.  They come in this keyframe's hash-map order, which
	// the language does not define: a caller that needs an order sorts them (visual_odometry::TwoViewInitializer does).
	std::vector<tracker::TrackId> getSharedTracks(const Keyframe& frame) const
	{
		std::vector<tracker::TrackId> shared;
		for (const auto& mine : landmarks_)
		{
			if (frame.landmarks_.count(mine.first) != 0)
			{
				shared.push_back(mine.first);
			}
		}
		return shared;
	}

	common::Pose3d pose;
	common::timestamp_t timestamp{};

   private:
	Landmarks landmarks_;
};
}  // namespace visual_odometry
