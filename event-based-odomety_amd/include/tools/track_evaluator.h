// tools/track_evaluator.h — tools::TrackEvaluator: the two figures the reference's report judges the feature tracker
// by, mean track error (Table 1) and feature age (Table 2), for the tracks of a DAVIS recording.  The reference has no
// such code; the protocol is the published one for event-based trackers on real recordings (include/ebo.h, "track
// evaluation", V1-V9): KLT tracks on the recording's frames, seeded at each event track's position on the first frame
// inside its life, are the ground truth.
//
//   auto recording = std::make_shared<tools::Davis240cRecording>(dir);
//   tools::TrackEvaluator te(recording, tools::TrackEvaluator::readTracks(out + "/trajectory.txt"));   // or trackPoints(patches)
//   te.rectifyFrames(recording->getCalibration(), rectifiedCamera);      // optional: tracks in rectified pixels
//   te.referenceTracks();                  // the KLT tracks as track points (id, frame time, x, y)
//   te.evaluate({2.0, 5.0});               // ebo_track_error_result [track][tau]
//   te.summary(5.0);                       // ebo_track_error_summary_result of one of the evaluated taus
//
// A track is the points of one id, ids in the order of their first point, put in time order (a stable sort; sample
// indices such as `cut` count in that order).  The sort is needed for the tracker's own files: a patch's first two
// points, its corner on the first frame and the LK position on the second, carry the frames' times, and the event-based
// points that follow begin inside that frame interval.  The evaluator owns a context of the frames' size.  Plumbing over include/ebo.h (ebo_track_seeds, ebo_reference_tracks, ebo_track_errors,
// ebo_track_error_summary): nothing here computes.  Needs no OpenCV: frames are decoded by ebo_read_png8.
#pragma once

#include <algorithm>
#include <cstdint>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "../dataset_reader/davis240c_recording.h"

namespace tools
{
class TrackEvaluator
{
   public:
	TrackEvaluator(std::shared_ptr<Davis240cRecording> recording, const std::vector<ebo_track_point>& points)
		: recording_(std::move(recording))
	{
		// group by id, ids in the order of their first point; then each track in time order
		std::unordered_map<int64_t, size_t> index;
		std::vector<std::vector<ebo_track_point>> groups;
		for (const ebo_track_point& p : points)
		{
			const auto it = index.find(p.id);
			if (it == index.end())
			{
				index.emplace(p.id, groups.size());
				ids_.push_back(p.id);
				groups.emplace_back();
				groups.back().push_back(p);
			}
			else
			{
				groups[it->second].push_back(p);
			}
		}
		estOff_.push_back(0);
		for (auto& g : groups)
		{
			std::stable_sort(g.begin(), g.end(), [](const ebo_track_point& a, const ebo_track_point& b) { return a.t_us < b.t_us; });
			for (const ebo_track_point& p : g)
			{
				estT_.push_back(p.t_us);
				estXy_.push_back(p.x);
				estXy_.push_back(p.y);
			}
			estOff_.push_back(static_cast<int>(estT_.size()));
		}
	}
	~TrackEvaluator()
	{
		if (ctx_)
		{
			ebo_destroy(ctx_);
		}
	}
	TrackEvaluator(const TrackEvaluator&) = delete;
	TrackEvaluator& operator=(const TrackEvaluator&) = delete;

	// a trajectory.txt as tools::saveFeaturesTrajectory writes it
	static std::vector<ebo_track_point> readTracks(const std::string& file)
	{
		size_t n = 0;
		std::vector<ebo_track_point> out(1 << 16);
		int rc = ebo_read_tracks_txt(file.c_str(), out.data(), out.size(), &n);
		if (rc == EBO_ERR_ARG && n > out.size())
		{
			out.resize(n);
			rc = ebo_read_tracks_txt(file.c_str(), out.data(), out.size(), &n);
		}
		if (rc != EBO_OK)
		{
			throw std::runtime_error("tools::TrackEvaluator: cannot read " + file);
		}
		out.resize(n);
		return out;
	}

	// The frames go through ebo_rectify_image (camera -> rectifiedCamera) before KLT sees them: for tracks that live in
	// rectified pixels (EvaluatorParams::rectifyFrames).  Before referenceTracks().
	void rectifyFrames(const common::CameraModelParams<double>& camera, const common::CameraModelParams<double>& rectifiedCamera)
	{
		if (haveReference_)
		{
			throw std::logic_error("tools::TrackEvaluator::rectifyFrames: only before referenceTracks()");
		}
		rectify_ = true;
		camera_ = common::toEboCamera(camera);
		rectified_ = common::toEboCamera(rectifiedCamera);
	}
	// ebo_lk_track's parameters for the reference tracks (default: ebo_default_lk_params)
	void setLkParams(const ebo_lk_params& lk)
	{
		lk_ = lk;
		haveLk_ = true;
	}

	size_t tracks() const { return ids_.size(); }
	const std::vector<int64_t>& ids() const { return ids_; }
	const std::vector<int64_t>& frameTimes() const { return frameT_; }
	// per track: the frame its reference track starts at (-1: no frame within its life) and the last it reaches
	const std::vector<int>& firstFrames() const { return first_; }
	const std::vector<int>& lastFrames() const { return last_; }

	// The KLT reference tracks (computed once): one point per track and frame in [first, last], the track's id, the
	// frame's time.  What OUT/groundtruth_tracks.txt holds.
	const std::vector<ebo_track_point>& referenceTracks()
	{
		if (haveReference_)
		{
			return reference_;
		}
		loadFrames();
		const int n = static_cast<int>(ids_.size()), F = static_cast<int>(frameT_.size());
		std::vector<int> seedFrame(ids_.size(), -1);
		std::vector<float> seedXy(2 * ids_.size(), 0.0f);
		if (ebo_track_seeds(n, estOff_.data(), estT_.data(), estXy_.data(), F, frameT_.data(), seedFrame.data(), seedXy.data()) != EBO_OK)
		{
			throw std::runtime_error("tools::TrackEvaluator: a track's times decrease, or the frames' times do not increase");
		}
		first_.assign(ids_.size(), -1);
		last_.assign(ids_.size(), -1);
		std::vector<double> xy(2 * ids_.size() * frameT_.size(), 0.0);
		check(ebo_reference_tracks(ctx_, F, frames_.data(), frameT_.data(), n, seedFrame.data(), seedXy.data(), haveLk_ ? &lk_ : nullptr,
								   first_.data(), last_.data(), xy.data()),
			  "ebo_reference_tracks");
		gtOff_.assign(1, 0);
		for (size_t k = 0; k < ids_.size(); ++k)
		{
			for (int f = first_[k]; first_[k] >= 0 && f <= last_[k]; ++f)
			{
				ebo_track_point p;
				p.id = ids_[k];
				p.t_us = frameT_[static_cast<size_t>(f)];
				p.x = xy[2 * (k * frameT_.size() + static_cast<size_t>(f))];
				p.y = xy[2 * (k * frameT_.size() + static_cast<size_t>(f)) + 1];
				reference_.push_back(p);
				gtT_.push_back(p.t_us);
				gtXy_.push_back(p.x);
				gtXy_.push_back(p.y);
			}
			gtOff_.push_back(static_cast<int>(gtT_.size()));
		}
		frames_.clear();
		frames_.shrink_to_fit();
		haveReference_ = true;
		return reference_;
	}

	// ebo_track_errors of every track against its reference track at every tau: [track][tau], tracks as ids()
	const std::vector<ebo_track_error_result>& evaluate(const std::vector<double>& taus)
	{
		referenceTracks();
		taus_ = taus;
		results_.assign(ids_.size() * taus.size(), ebo_track_error_result{});
		check(ebo_track_errors(ctx_, static_cast<int>(ids_.size()), estOff_.data(), estT_.data(), estXy_.data(), gtOff_.data(), gtT_.data(),
							   gtXy_.data(), static_cast<int>(taus.size()), taus.data(), results_.data(), nullptr),
			  "ebo_track_errors");
		return results_;
	}

	// ebo_track_error_summary over the results of `tau`, one of the thresholds last evaluated
	ebo_track_error_summary_result summary(double tau) const
	{
		for (size_t j = 0; j < taus_.size(); ++j)
		{
			if (taus_[j] == tau)
			{
				ebo_track_error_summary_result s{};
				if (ebo_track_error_summary(static_cast<int>(ids_.size()), results_.data() + j, static_cast<int>(taus_.size()), &s) != EBO_OK)
				{
					throw std::runtime_error("tools::TrackEvaluator: ebo_track_error_summary");
				}
				return s;
			}
		}
		throw std::invalid_argument("tools::TrackEvaluator::summary: a tau that evaluate() was not given");
	}

   private:
	void check(int rc, const char* what) const
	{
		if (rc != EBO_OK)
		{
			throw std::runtime_error(std::string("tools::TrackEvaluator: ") + what + ": " + ebo_last_error(ctx_));
		}
	}
	// every frame of images.txt, decoded (and rectified); the context is made at the first frame's size
	void loadFrames()
	{
		const auto stamps = recording_->getImageStamps();
		if (stamps.empty())
		{
			throw std::runtime_error("tools::TrackEvaluator: the recording has no frames");
		}
		int32_t w = 0, h = 0;
		std::vector<uint8_t> raw;
		for (size_t f = 0; f < stamps.size(); ++f)
		{
			const std::string file = recording_->path() + "/" + stamps[f].file;
			int32_t fw = 0, fh = 0;
			if (ebo_read_png8(file.c_str(), &fw, &fh, nullptr, 0) != EBO_OK)
			{
				throw std::runtime_error("tools::TrackEvaluator: cannot read frame " + file + ": " + ebo_last_error(nullptr));
			}
			if (f == 0)
			{
				w = fw;
				h = fh;
				ebo_params prm;
				ebo_default_params(&prm);
				prm.image_w = w;
				prm.image_h = h;
				if (ebo_create(&prm, &ctx_) != EBO_OK)
				{
					ctx_ = nullptr;
					throw std::runtime_error(std::string("tools::TrackEvaluator: ebo_create: ") + ebo_last_error(nullptr));
				}
				if (rectify_)
				{
					check(ebo_set_rectification_camera(ctx_, &camera_, &rectified_), "ebo_set_rectification_camera");
				}
				frames_.resize(stamps.size() * static_cast<size_t>(w) * static_cast<size_t>(h));
				raw.resize(static_cast<size_t>(w) * static_cast<size_t>(h));
			}
			else if (fw != w || fh != h)
			{
				throw std::runtime_error("tools::TrackEvaluator: frame " + file + " has another size than the first");
			}
			uint8_t* dst = frames_.data() + f * raw.size();
			if (ebo_read_png8(file.c_str(), &fw, &fh, rectify_ ? raw.data() : dst, raw.size()) != EBO_OK)
			{
				throw std::runtime_error("tools::TrackEvaluator: cannot read frame " + file + ": " + ebo_last_error(nullptr));
			}
			if (rectify_)
			{
				check(ebo_rectify_image(ctx_, raw.data(), dst), "ebo_rectify_image");
			}
			frameT_.push_back(stamps[f].timestamp.count());
		}
	}

	std::shared_ptr<Davis240cRecording> recording_;
	ebo_ctx* ctx_ = nullptr;
	std::vector<int64_t> ids_;
	std::vector<int> estOff_, gtOff_;
	std::vector<int64_t> estT_, gtT_, frameT_;
	std::vector<double> estXy_, gtXy_;
	std::vector<uint8_t> frames_;
	std::vector<int> first_, last_;
	std::vector<ebo_track_point> reference_;
	std::vector<double> taus_;
	std::vector<ebo_track_error_result> results_;
	bool rectify_ = false, haveLk_ = false, haveReference_ = false;
	ebo_camera camera_{}, rectified_{};
	ebo_lk_params lk_{};
};

}  // namespace tools
