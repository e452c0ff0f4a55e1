// common/data_types.h — the event types of the reference
// (common/include/common/data_types.h:10-38, common/include/common/geometry.h:10-14)
// without the OpenCV/Sophus dependency: only what the event-warping path touches.
// Field names, order and layout are the reference's, so code written against
// common::EventSample compiles unchanged and an array of EventSample can be handed to
// the C ABI as an array of ebo_event.
#pragma once

#include <chrono>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <deque>
#include <list>
#include <stdexcept>
#include <vector>

#include "../../../include/ebo.h"
#include "camera_model.h"

// With OpenCV on the include path the OpenCV value types ARE the reference's types (common/include/common/geometry.h,
// data_types.h:39): the stand-ins below give way to them, so that code written against the reference -- cv::Point2i in
// an Event, cv::Mat in an ImageSample -- compiles without a rename.
#if defined(__has_include)
#if __has_include(<opencv2/core.hpp>)
#include <opencv2/core.hpp>
#define EBO_HAVE_OPENCV 1
#endif
// With Sophus on the include path common::Pose3d is Sophus::SE3d as in the reference (common/geometry.h:14) and the
// stand-in below gives way to it (the stand-in headers under visual_odometry/ are then not available).
#if __has_include(<sophus/se3.hpp>)
#include <sophus/se3.hpp>
#define EBO_HAVE_SOPHUS 1
#endif
#endif

namespace common
{
#ifdef EBO_HAVE_OPENCV
using Point2i = cv::Point2i;
using Point2d = cv::Point2d;
#else
// cv::Point2i stand-in (two ints, x then y).
struct Point2i
{
	int x = 0;
	int y = 0;
	Point2i() = default;
	Point2i(int x_, int y_) : x(x_), y(y_) {}
};

struct Point2d
{
	double x = 0.0;
	double y = 0.0;
	Point2d() = default;
	Point2d(double x_, double y_) : x(x_), y(y_) {}
};
#endif

using timestamp_t = std::chrono::microseconds;

// Sophus::SE2d stand-in for common::Pose2d (common/include/common/geometry.h): the storage
// the tracker hands to Ceres — unit complex (cos, sin), then the translation — and the few
// operations the tracker path calls (matrix2x3, inverse, data).
struct Pose2d
{
	double d[4] = {1.0, 0.0, 0.0, 0.0};
	Pose2d() = default;
	Pose2d(double theta, const Point2d& t);
	double* data() { return d; }
	const double* data() const { return d; }
	struct Matrix2x3
	{
		double m[2][3];
		double operator()(int r, int c) const { return m[r][c]; }
	};
	Matrix2x3 matrix2x3() const
	{
		return Matrix2x3{{{d[0], -d[1], d[2]}, {d[1], d[0], d[3]}}};
	}
	Pose2d inverse() const
	{
		Pose2d r;
		const double c = d[0], s = -d[1];
		r.d[0] = c;
		r.d[1] = s;
		r.d[2] = -(c * d[2] - s * d[3]);
		r.d[3] = -(s * d[2] + c * d[3]);
		return r;
	}
};

// Eigen::Vector2d / Vector3d / Matrix3d stand-ins for the geometry types below and for visual_odometry/.
using Vector2d = FixedVec<double, 2>;
using Vector3d = FixedVec<double, 3>;
struct Matrix3d
{
	double m[3][3] = {{0, 0, 0}, {0, 0, 0}, {0, 0, 0}};
	double& operator()(int r, int c) { return m[r][c]; }
	const double& operator()(int r, int c) const { return m[r][c]; }
	static Matrix3d Identity()
	{
		Matrix3d r;
		r.m[0][0] = r.m[1][1] = r.m[2][2] = 1.0;
		return r;
	}
};

#ifdef EBO_HAVE_SOPHUS
using Pose3d = Sophus::SE3d;
#else
// Sophus::SE3d stand-in for common::Pose3d (common/include/common/geometry.h:14): a rotation matrix and a translation,
// and the operations the recording reader and the visual odometry call.  The arithmetic of * and inverse() is the
// pose rule of include/ebo.h ("two-view geometry", rule 1): every dot product is (a0 * b0 + a1 * b1) + a2 * b2, so
// that compiled with -ffp-contract=off it gives the bits of ebo_triangulate and of tests/twoview_ref.py.
class Pose3d
{
   public:
	struct Matrix4
	{
		double m[4][4];
		double operator()(int r, int c) const { return m[r][c]; }
	};

	Pose3d() : R_(Matrix3d::Identity()) {}
	Pose3d(const Matrix3d& rotation, const Vector3d& translation) : R_(rotation), t_(translation) {}
	// Sophus::SE3d(Eigen::Quaterniond(qw, qx, qy, qz), t): the quaternion is normalised (Eigen's normalize()) and
	// turned into a matrix as Eigen::Quaterniond::toRotationMatrix does
	Pose3d(double qw, double qx, double qy, double qz, double tx, double ty, double tz) : t_(tx, ty, tz)
	{
		const double n = std::sqrt(qx * qx + qy * qy + qz * qz + qw * qw);
		if (!(n > 0.0) || !std::isfinite(n))
		{
			throw std::runtime_error("common::Pose3d: the quaternion has no direction");
		}
		const double x = qx / n, y = qy / n, z = qz / n, w = qw / n;
		const double x2 = 2 * x, y2 = 2 * y, z2 = 2 * z;
		const double twx = x2 * w, twy = y2 * w, twz = z2 * w;
		const double txx = x2 * x, txy = y2 * x, txz = z2 * x;
		const double tyy = y2 * y, tyz = z2 * y, tzz = z2 * z;
		const double r[3][3] = {{1 - (tyy + tzz), txy - twz, txz + twy},
								{txy + twz, 1 - (txx + tzz), tyz - twx},
								{txz - twy, tyz + twx, 1 - (txx + tyy)}};
		for (int i = 0; i < 3; ++i)
		{
			for (int j = 0; j < 3; ++j)
			{
				R_.m[i][j] = r[i][j];
			}
		}
	}
	// [R | t] as the C ABI takes a pose or a two-view model: double [3][4], row-major
	explicit Pose3d(const double* m34)
	{
		for (int i = 0; i < 3; ++i)
		{
			for (int j = 0; j < 3; ++j)
			{
				R_.m[i][j] = m34[4 * i + j];
			}
			t_[i] = m34[4 * i + 3];
		}
	}
	void toArray(double* m34) const
	{
		for (int i = 0; i < 3; ++i)
		{
			for (int j = 0; j < 3; ++j)
			{
				m34[4 * i + j] = R_.m[i][j];
			}
			m34[4 * i + 3] = t_[i];
		}
	}
	// (Ra, ta)(Rb, tb) = (Ra Rb, Ra tb + ta)
	Pose3d operator*(const Pose3d& o) const
	{
		Pose3d r;
		for (int i = 0; i < 3; ++i)
		{
			for (int j = 0; j < 3; ++j)
			{
				r.R_.m[i][j] = (R_.m[i][0] * o.R_.m[0][j] + R_.m[i][1] * o.R_.m[1][j]) + R_.m[i][2] * o.R_.m[2][j];
			}
			r.t_[i] = ((R_.m[i][0] * o.t_[0] + R_.m[i][1] * o.t_[1]) + R_.m[i][2] * o.t_[2]) + t_[i];
		}
		return r;
	}
	// R p + t
	Vector3d operator*(const Vector3d& p) const
	{
		Vector3d r;
		for (int i = 0; i < 3; ++i)
		{
			r[i] = ((R_.m[i][0] * p[0] + R_.m[i][1] * p[1]) + R_.m[i][2] * p[2]) + t_[i];
		}
		return r;
	}
	// (R^T, -(R^T t))
	Pose3d inverse() const
	{
		Pose3d r;
		for (int i = 0; i < 3; ++i)
		{
			for (int j = 0; j < 3; ++j)
			{
				r.R_.m[i][j] = R_.m[j][i];
			}
			r.t_[i] = -((R_.m[0][i] * t_[0] + R_.m[1][i] * t_[1]) + R_.m[2][i] * t_[2]);
		}
		return r;
	}
	Vector3d& translation() { return t_; }
	const Vector3d& translation() const { return t_; }
	const Matrix3d& rotationMatrix() const { return R_; }
	Matrix4 matrix() const
	{
		Matrix4 out{};
		for (int i = 0; i < 3; ++i)
		{
			for (int j = 0; j < 3; ++j)
			{
				out.m[i][j] = R_.m[i][j];
			}
			out.m[i][3] = t_[i];
		}
		out.m[3][3] = 1.0;
		return out;
	}

   private:
	Matrix3d R_;
	Vector3d t_;
};
#endif

template <typename T>
struct Sample
{
	Sample(const T& value_, const timestamp_t timestamp_) : value(value_), timestamp(timestamp_) {}
	Sample() {}

	T value;
	timestamp_t timestamp;
};

enum EventPolarity
{
	NEGATIVE = -1,
	POSITIVE = 1
};

struct Event
{
	Point2i point;
	EventPolarity sign;
};

// CV_8U single-channel cv::Mat stand-in: what ImageSample carries to FeatureDetector::newImage
// (data_types.h:39).  The event-warping path never reads pixels; the front-end hooks do.
#ifdef EBO_HAVE_OPENCV
using Image8 = cv::Mat;
#else
struct Image8
{
	int rows = 0;
	int cols = 0;
	std::vector<uint8_t> data;  // row-major
	Image8() = default;
	Image8(int r, int c) : rows(r), cols(c), data(static_cast<size_t>(r) * c, 0) {}
};
#endif

using EventSample = Sample<Event>;
using ImageSample = Sample<Image8>;
using EventSequence = std::deque<EventSample>;
using ImageSequence = std::vector<ImageSample>;

static_assert(sizeof(EventSample) == sizeof(ebo_event), "EventSample must match ebo_event");
static_assert(offsetof(EventSample, timestamp) == offsetof(ebo_event, t_us), "timestamp offset");
static_assert(offsetof(Event, sign) == offsetof(ebo_event, sign), "sign offset");

// list / deque of EventSample -> contiguous ebo_event array for the C ABI.
template <class Container>
inline std::vector<ebo_event> toEboEvents(const Container& events)
{
	std::vector<ebo_event> out;
	out.reserve(events.size());
	for (const auto& e : events)
	{
		ebo_event r;
		r.x = e.value.point.x;
		r.y = e.value.point.y;
		r.sign = static_cast<int32_t>(e.value.sign);
		r.reserved = 0;
		r.t_us = e.timestamp.count();
		out.push_back(r);
	}
	return out;
}

inline Pose2d::Pose2d(double theta, const Point2d& t)
{
	d[0] = std::cos(theta);
	d[1] = std::sin(theta);
	d[2] = t.x;
	d[3] = t.y;
}

}  // namespace common
