// dataset_reader/davis240c_recording.h — the whole of a DAVIS240C recording directory: tools::Davis240cRecording adds
// the three getters tools::Davis240cReader leaves out (it throws "not on the event path" for them), with the
// reference's return types and line formats (tools/dataset_reader/src/davis240c_reader.cpp:18-58,93-151,207-275):
//
//   tools::Davis240cRecording rec(path);   // events.txt, images.txt + images/*.png, groundtruth.txt, calib.txt
//   rec.getImages()         // common::ImageSequence: "<seconds> <file relative to path>" per line, frames decoded
//   rec.getGroundTruth()    // common::GroundTruth:   "t tx ty tz qx qy qz qw" per line, quaternion normalised
//   rec.getCalibration()    // common::CameraModelParams<double>: "fx fy cx cy k1 k2 p1 p2 k3" (first line)
//   rec.getImageStamps() / rec.getImage(stamp)   // images.txt without decoding, and one frame (tools::Replayer)
//
// Lines: as on the event side (dataset_reader.h:33-97), only '\n'-terminated lines count; a trailing '\r' of a file
// name is dropped.  Times: std::stod, then duration_cast<microseconds> of duration<double> (truncation).  Frames are
// decoded by the library (ebo_read_png8: 8-bit greyscale PNG, what cv::imread(path, CV_8U) returns for a DAVIS frame).
// Difference to the reference: a frame file that cannot be read or decoded throws std::runtime_error naming the file
// (cv::imread would hand back an empty cv::Mat and the tracker would run on it).
//
// Without Sophus and OpenCV on the include path the value types are stand-ins with the members the tracker side uses:
// common::Pose3d (common/data_types.h: matrix(), rotationMatrix(), translation()), common::GroundTruthSample,
// and common::GroundTruth (common::CameraModelParams<Scalar> and CameraModel are in common/camera_model.h).  With
// Sophus, common::Pose3d is Sophus::SE3d as in the reference (common/geometry.h:14).
#pragma once

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <stdexcept>
#include <string>
#include <vector>

#include "../common/camera_model.h"  // common::CameraModelParams<Scalar>
#include "davis240c_reader.h"

namespace common
{
// common::Pose3d is in common/data_types.h: Sophus::SE3d with Sophus on the include path, the stand-in without
#ifdef EBO_HAVE_SOPHUS
inline Pose3d makePose3d(double qw, double qx, double qy, double qz, double tx, double ty, double tz)
{
	return Sophus::SE3d(Eigen::Quaterniond(qw, qx, qy, qz), Sophus::SE3d::Point(tx, ty, tz));  // (SO3 normalises)
}
#else
inline Pose3d makePose3d(double qw, double qx, double qy, double qz, double tx, double ty, double tz)
{
	return Pose3d(qw, qx, qy, qz, tx, ty, tz);
}
#endif

using GroundTruthSample = Sample<Pose3d>;
using GroundTruth = std::vector<GroundTruthSample>;

// an 8-bit single-channel image of the given pixels (a cv::Mat of CV_8U with OpenCV on the include path)
inline Image8 makeImage8(int rows, int cols, const uint8_t* pixels)
{
#ifdef EBO_HAVE_OPENCV
	cv::Mat m(rows, cols, CV_8U);
	std::memcpy(m.data, pixels, static_cast<size_t>(rows) * cols);
	return m;
#else
	Image8 m(rows, cols);
	std::memcpy(m.data.data(), pixels, static_cast<size_t>(rows) * cols);
	return m;
#endif
}
}  // namespace common

namespace tools
{
class Davis240cRecording : public Davis240cReader
{
   public:
	// one line of images.txt before its frame is decoded
	struct ImageStamp
	{
		common::timestamp_t timestamp;
		std::string file;  // as written in images.txt: relative to the recording's directory
	};

	explicit Davis240cRecording(const std::string& path) : Davis240cReader(path), dir_(path) {}

	const std::string& path() const { return dir_; }

	// davis240c_reader.cpp:214-234: every frame of images.txt, decoded
	common::ImageSequence getImages() const
	{
		common::ImageSequence out;
		for (const ImageStamp& s : getImageStamps())
		{
			out.push_back(getImage(s));
		}
		return out;
	}

	// images.txt alone: the times and file names, no frame decoded
	std::vector<ImageStamp> getImageStamps() const
	{
		std::vector<ImageStamp> out;
		forEachLine(dir_ + "/images.txt", [&](std::string& line) {
			size_t pos = line.find(' ');
			ImageStamp s;
			s.timestamp = toTimestamp(std::stod(line.substr(0, pos)));
			s.file = pos == std::string::npos ? std::string() : line.substr(pos + 1);
			if (!s.file.empty() && s.file.back() == '\r')
			{
				s.file.pop_back();
			}
			out.push_back(std::move(s));
		});
		return out;
	}

	// davis240c_reader.cpp:93-107 for one line of images.txt, the frame read when this is called
	common::ImageSample getImage(const ImageStamp& stamp) const
	{
		return common::ImageSample(readImage(dir_ + "/" + stamp.file), stamp.timestamp);
	}
	common::ImageSample getImageSample(std::string& line) const
	{
		size_t pos = line.find(' ');
		const common::timestamp_t timestamp = toTimestamp(std::stod(line.substr(0, pos)));
		line = line.substr(pos + 1);
		return common::ImageSample(readImage(dir_ + "/" + line), timestamp);
	}

	// cv::imread(file, CV_8U) for the PNG frames of a DAVIS recording (ebo_read_png8); throws naming the file
	static common::Image8 readImage(const std::string& file)
	{
		int32_t w = 0, h = 0;
		int rc = ebo_read_png8(file.c_str(), &w, &h, nullptr, 0);
		std::vector<uint8_t> px;
		if (rc == EBO_OK)
		{
			px.resize(static_cast<size_t>(w) * h);
			rc = ebo_read_png8(file.c_str(), &w, &h, px.data(), px.size());
		}
		if (rc != EBO_OK)
		{
			throw std::runtime_error("tools::Davis240cRecording: cannot read frame " + file + ": " + ebo_last_error(nullptr));
		}
		return common::makeImage8(h, w, px.data());
	}

	// davis240c_reader.cpp:236-255
	common::GroundTruth getGroundTruth() const
	{
		common::GroundTruth out;
		forEachLine(dir_ + "/groundtruth.txt", [&](std::string& line) { out.push_back(getGroundTruthSample(line)); });
		return out;
	}
	// davis240c_reader.cpp:109-151: "t tx ty tz qx qy qz qw"
	common::GroundTruthSample getGroundTruthSample(std::string& line) const
	{
		double v[8];
		for (int i = 0; i < 7; ++i)
		{
			const size_t pos = line.find(' ');
			v[i] = std::stod(line.substr(0, pos));
			line = line.substr(pos + 1);
		}
		v[7] = std::stod(line);
		return common::GroundTruthSample(common::makePose3d(v[7], v[4], v[5], v[6], v[1], v[2], v[3]), toTimestamp(v[0]));
	}

	// davis240c_reader.cpp:257-275: the first line of calib.txt
	common::CameraModelParams<double> getCalibration() const
	{
		std::vector<common::CameraModelParams<double>> lines;
		forEachLine(dir_ + "/calib.txt", [&](std::string& line) { lines.push_back(getCalibrationLine(line)); });
		if (lines.empty())
		{
			throw std::runtime_error("tools::Davis240cRecording: no calibration line in " + dir_ + "/calib.txt");
		}
		return lines[0];
	}
	// davis240c_reader.cpp:18-58: "fx fy cx cy k1 k2 p1 p2 k3"
	common::CameraModelParams<double> getCalibrationLine(std::string& line) const
	{
		double v[9];
		for (int i = 0; i < 9; ++i)
		{
			const size_t pos = line.find(' ');
			v[i] = std::stod(line.substr(0, pos));
			if (pos == std::string::npos && i < 8)
			{
				throw std::runtime_error("tools::Davis240cRecording: a calibration line holds nine numbers");
			}
			line = line.substr(pos + 1);
		}
		common::CameraModelParams<double> p;
		p.fx = v[0];
		p.fy = v[1];
		p.cx = v[2];
		p.cy = v[3];
		p.k1 = v[4];
		p.k2 = v[5];
		p.p1 = v[6];
		p.p2 = v[7];
		p.k3 = v[8];
		return p;
	}

   private:
	// std::chrono::duration_cast<timestamp_t>(std::chrono::duration<double>(seconds)): truncation
	static common::timestamp_t toTimestamp(double seconds)
	{
		return std::chrono::duration_cast<common::timestamp_t>(std::chrono::duration<double>(seconds));
	}
	// the '\n'-terminated lines of a file (a last line without '\n' does not count, as in dataset_reader.h:43-52)
	template <class F>
	static void forEachLine(const std::string& file, F&& f)
	{
		std::FILE* fp = std::fopen(file.c_str(), "rb");
		if (!fp)
		{
			throw std::runtime_error("tools::Davis240cRecording: cannot open " + file);
		}
		std::string text;
		char buf[1 << 16];
		size_t got = 0;
		while ((got = std::fread(buf, 1, sizeof(buf), fp)) > 0)
		{
			text.append(buf, got);
		}
		std::fclose(fp);
		size_t start = 0, nl = 0;
		while ((nl = text.find('\n', start)) != std::string::npos)
		{
			std::string line = text.substr(start, nl - start);
			start = nl + 1;
			f(line);
		}
	}

	std::string dir_;
};

}  // namespace tools
