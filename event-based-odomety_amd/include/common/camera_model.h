// common/camera_model.h — common::CameraModelParams and common::CameraModel with the reference's public members
// (common/include/common/camera_model.h:13-126): a pinhole camera with radial-tangential distortion.
//
//   common::CameraModel<double> cam(params);
//   cam.project(p)          // Vec3 in the camera frame -> Vec2 pixel
//   cam.unproject(px)       // Vec2 pixel -> unit bearing Vec3 (ten fixed-point iterations, as the reference)
//   cam.unprojectBatch(ctx, corners)   // the same for many pixels on the device (ebo_camera_unproject)
//   cam.projectBatch(ctx, points)      // project for many points on the device (ebo_camera_project)
//   common::fitRectifiedCamera(ctx, params)   // the zero-distortion camera that keeps the context's sensor in view
//
// The arithmetic is the rule written out in include/ebo.h ("camera model"), operation by operation, so that
// CameraModel<double> compiled with -ffp-contract=off gives the bits of the device kernels and of
// tests/camera_ref.py.  It is a template over the scalar: double, or a dual number with + - * / and an
// unqualified sqrt (a later bundle adjustment differentiates through it).
//
// Without Eigen on the include path Vec2 / Vec3 are fixed arrays with operator[] and operator(), enough for caller
// statements such as cam.unproject(corner)[2].  k3 is a field of the parameters and is never used, as in the reference.
#pragma once

#include <cmath>
#include <cstddef>
#include <memory>
#include <stdexcept>
#include <string>
#include <type_traits>
#include <vector>

#include "../../../include/ebo.h"

namespace common
{
// common/camera_model.h:13-24 (field order of the struct; calib.txt orders them fx fy cx cy k1 k2 p1 p2 k3)
template <typename Scalar = double>
struct CameraModelParams
{
	Scalar fx = 0;
	Scalar fy = 0;
	Scalar cx = 0;
	Scalar cy = 0;
	Scalar k1 = 0;
	Scalar k2 = 0;
	Scalar k3 = 0;
	Scalar p1 = 0;
	Scalar p2 = 0;
};

// the same nine numbers as the C ABI takes them (include/ebo.h: ebo_camera)
inline ebo_camera toEboCamera(const CameraModelParams<double>& p)
{
	return ebo_camera{p.fx, p.fy, p.cx, p.cy, p.k1, p.k2, p.k3, p.p1, p.p2};
}

// The rectified camera fitted to the context's image size (include/ebo.h: ebo_fit_rectified_camera, rule C3): zero
// distortion, and the undistorted border of the sensor spans it exactly along the tighter axis.
inline CameraModelParams<double> fitRectifiedCamera(ebo_ctx* ctx, const CameraModelParams<double>& p)
{
	const ebo_camera cam = toEboCamera(p);
	ebo_camera r{};
	if (ebo_fit_rectified_camera(ctx, &cam, &r) != EBO_OK)
	{
		throw std::runtime_error(std::string("common::fitRectifiedCamera: ") + ebo_last_error(ctx));
	}
	CameraModelParams<double> out;
	out.fx = r.fx;
	out.fy = r.fy;
	out.cx = r.cx;
	out.cy = r.cy;
	return out;
}

// Eigen::Matrix<Scalar, N, 1> stand-in
template <typename Scalar, int N>
struct FixedVec
{
	Scalar v[N] = {};
	FixedVec() = default;
	FixedVec(const Scalar& a, const Scalar& b)
	{
		static_assert(N == 2, "two components");
		v[0] = a;
		v[1] = b;
	}
	FixedVec(const Scalar& a, const Scalar& b, const Scalar& c)
	{
		static_assert(N == 3, "three components");
		v[0] = a;
		v[1] = b;
		v[2] = c;
	}
	Scalar& operator[](int i) { return v[i]; }
	const Scalar& operator[](int i) const { return v[i]; }
	Scalar& operator()(int i) { return v[i]; }
	const Scalar& operator()(int i) const { return v[i]; }
	Scalar* data() { return v; }
	const Scalar* data() const { return v; }
	const Scalar& x() const { return v[0]; }
	const Scalar& y() const { return v[1]; }
	const Scalar& z() const
	{
		static_assert(N >= 3, "three components");
		return v[2];
	}
};

template <typename Scalar = double>
class CameraModel
{
   public:
	typedef FixedVec<Scalar, 2> Vec2;
	typedef FixedVec<Scalar, 3> Vec3;

	CameraModel(const CameraModelParams<Scalar> p) : param_(p) {}

	// ((2 * p1) * x) * y + p2 * (r2 + (2 * x) * x)
	inline Scalar getTangentialDistortion(const Scalar& p1, const Scalar& p2, const Scalar& x, const Scalar& y,
										  const Scalar& r2) const
	{
		const Scalar cross = ((Scalar(2) * p1) * x) * y;
		const Scalar own = p2 * (r2 + (Scalar(2) * x) * x);
		return cross + own;
	}

	// (1 + k1 * r2) + (k2 * r2) * r2
	inline Scalar getRadialDistortion(const Scalar& r2) const
	{
		const Scalar second = (param_.k2 * r2) * r2;
		return (Scalar(1) + param_.k1 * r2) + second;
	}

	inline Vec2 project(const Vec3& p) const
	{
		const Scalar a = p[0] / p[2];
		const Scalar b = p[1] / p[2];
		const Scalar r2 = a * a + b * b;
		const Scalar radial = getRadialDistortion(r2);
		const Scalar aD = a * radial + getTangentialDistortion(param_.p1, param_.p2, a, b, r2);
		const Scalar bD = b * radial + getTangentialDistortion(param_.p2, param_.p1, b, a, r2);
		return Vec2(param_.fx * aD + param_.cx, param_.fy * bD + param_.cy);
	}

	Vec3 unproject(const Vec2& p) const
	{
		const Scalar aD = (p[0] - param_.cx) / param_.fx;
		const Scalar bD = (p[1] - param_.cy) / param_.fy;
		Scalar a = aD;
		Scalar b = bD;
		for (int step = 0; step < kUndistortSteps; ++step)
		{
			const Scalar r2 = a * a + b * b;
			const Scalar radial = getRadialDistortion(r2);
			const Scalar shiftA = getTangentialDistortion(param_.p1, param_.p2, a, b, r2);
			const Scalar shiftB = getTangentialDistortion(param_.p2, param_.p1, b, a, r2);
			a = (aD - shiftA) / radial;
			b = (bD - shiftB) / radial;
		}
		using std::sqrt;
		const Scalar length = sqrt((a * a + b * b) + Scalar(1));
		return Vec3(a / length, b / length, Scalar(1) / length);
	}

	// unproject for many pixels in one launch on the context's device (include/ebo.h: ebo_camera_unproject)
	std::vector<Vec3> unprojectBatch(ebo_ctx* ctx, const std::vector<Vec2>& corners) const
	{
		static_assert(std::is_same<Scalar, double>::value, "the device kernel is float64");
		static_assert(sizeof(Vec2) == 2 * sizeof(double) && sizeof(Vec3) == 3 * sizeof(double), "packed arrays");
		std::vector<Vec3> out(corners.size());
		const ebo_camera cam = toEboCamera(param_);
		const int rc = ebo_camera_unproject(ctx, &cam, static_cast<int>(corners.size()),
											corners.empty() ? nullptr : corners[0].data(), out.empty() ? nullptr : out[0].data());
		if (rc != EBO_OK)
		{
			throw std::runtime_error(std::string("common::CameraModel::unprojectBatch: ") + ebo_last_error(ctx));
		}
		return out;
	}

	// project for many points in one launch on the context's device (include/ebo.h: ebo_camera_project)
	std::vector<Vec2> projectBatch(ebo_ctx* ctx, const std::vector<Vec3>& points) const
	{
		static_assert(std::is_same<Scalar, double>::value, "the device kernel is float64");
		static_assert(sizeof(Vec2) == 2 * sizeof(double) && sizeof(Vec3) == 3 * sizeof(double), "packed arrays");
		std::vector<Vec2> out(points.size());
		const ebo_camera cam = toEboCamera(param_);
		const int rc = ebo_camera_project(ctx, &cam, static_cast<int>(points.size()), points.empty() ? nullptr : points[0].data(),
										  out.empty() ? nullptr : out[0].data());
		if (rc != EBO_OK)
		{
			throw std::runtime_error(std::string("common::CameraModel::projectBatch: ") + ebo_last_error(ctx));
		}
		return out;
	}

	Scalar* getParams() { return reinterpret_cast<Scalar*>(&param_); }

	static std::shared_ptr<CameraModel<Scalar>> fromData(const Scalar* params)
	{
		CameraModelParams<Scalar> p;
		p.fx = params[0];
		p.fy = params[1];
		p.cx = params[2];
		p.cy = params[3];
		p.k1 = params[4];
		p.k2 = params[5];
		p.k3 = params[6];
		p.p1 = params[7];
		p.p2 = params[8];
		return std::make_shared<CameraModel<Scalar>>(p);
	}

   private:
	static constexpr int kUndistortSteps = 10;
	CameraModelParams<Scalar> param_;
};

}  // namespace common
