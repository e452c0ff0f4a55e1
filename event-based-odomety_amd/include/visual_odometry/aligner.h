// visual_odometry/aligner.h — the ground-truth side of the reference's odometry path on the device: ErrorMetricValue,
// align_points_sim3 and align_cameras_sim3 with the reference's names and argument order after the context
// (visual_odometry/include/visual_odometry/aligner.h, src/aligner.cpp:27-114), over ebo_align_sim3 (include/ebo.h,
// "trajectory alignment", rules S1-S7: this project's own statement; parity with Eigen's JacobiSVD is not claimed,
// INTEGRATION.md §7 lists the differences), and syncGroundTruth, the body of
// VisualOdometryFrontEnd::syncGtAndImage (visual_odometry.cpp:522-561), host only, without Sophus.
//
//   alignPrefixes: what the reference does serially, one alignment of all keyframes so far after every new keyframe,
//     as ONE call over every prefix of the final trajectory.
//   relativePoseErrors / relativePoseErrorsPrefixes: the relative pose error beside the ATE, over ebo_trajectory_rpe
//     (include/ebo.h, rules T1-T7); the reference has none.
//   common::Sim3: Sophus::Sim3d's stand-in, as far as the path uses it: scale, rotation, translation, inverse(), and
//     the product with a point and with a pose.
#pragma once

#include <algorithm>
#include <cmath>
#include <list>
#include <optional>
#include <stdexcept>
#include <vector>

#include "../dataset_reader/davis240c_recording.h"  // common::GroundTruth
#include "triangulation.h"

namespace common
{
// x -> scale * (rotation * x) + translation
struct Sim3
{
	double scale = 1.0;
	Matrix3d rotation = Matrix3d::Identity();
	Vector3d translation;

	Vector3d operator*(const Vector3d& p) const
	{
		Vector3d r;
		for (int i = 0; i < 3; ++i)
		{
			r[i] = scale * ((rotation(i, 0) * p[0] + rotation(i, 1) * p[1]) + rotation(i, 2) * p[2]) + translation[i];
		}
		return r;
	}
	// a pose keeps its own rotation's length: (rotation * R, *this * t)
	Pose3d operator*(const Pose3d& T) const
	{
		const Pose3d turned = Pose3d(rotation, Vector3d()) * T;
		return Pose3d(turned.rotationMatrix(), *this * T.translation());
	}
	// x -> (1 / scale) * (rotation^T * (x - translation))
	Sim3 inverse() const
	{
		Sim3 r;
		r.scale = 1.0 / scale;
		for (int i = 0; i < 3; ++i)
		{
			for (int j = 0; j < 3; ++j)
			{
				r.rotation(i, j) = rotation(j, i);
			}
		}
		for (int i = 0; i < 3; ++i)
		{
			r.translation[i] =
				-(r.scale * ((rotation(0, i) * translation[0] + rotation(1, i) * translation[1]) + rotation(2, i) * translation[2]));
		}
		return r;
	}
};
}  // namespace common

namespace visual_odometry
{
struct ErrorMetricValue
{
	double rmse = 0;
	double mean = 0;
	double min = 0;
	double max = 0;
	double count = 0;  //!< number of elements involved in the evaluation
};

// one segment's answer: status as ebo_align_result's (0 aligned, 1 fewer than 3 points, 2 a non-finite input,
// 3 degenerate); unless it is 0, sim is the identity and ate is zero but for its count
struct Alignment
{
	common::Sim3 sim;
	ErrorMetricValue ate;
	int status = 1;
};

namespace detail
{
inline Alignment toAlignment(const ebo_align_result& r)
{
	Alignment a;
	a.sim.scale = r.scale;
	for (int i = 0; i < 3; ++i)
	{
		for (int j = 0; j < 3; ++j)
		{
			a.sim.rotation(i, j) = r.R[3 * i + j];
		}
		a.sim.translation[i] = r.t[i];
	}
	a.ate.rmse = r.rmse;
	a.ate.mean = r.mean;
	a.ate.min = r.min;
	a.ate.max = r.max;
	a.ate.count = static_cast<double>(r.count);
	a.status = r.status;
	return a;
}

inline std::vector<Alignment> alignSegments(ebo_ctx* ctx, const std::vector<common::Vector3d>& data, const std::vector<common::Vector3d>& model,
											const std::vector<int>& begin, const std::vector<int>& end, bool fixScale, const char* who)
{
	if (data.size() != model.size())
	{
		throw std::invalid_argument(std::string(who) + ": data and model differ in length");
	}
	std::vector<ebo_align_result> results(begin.size());
	check(ctx,
		  ebo_align_sim3(ctx, static_cast<int>(data.size()), packed(data), packed(model), static_cast<int>(begin.size()), begin.data(),
						 end.data(), fixScale ? 1 : 0, results.data()),
		  who);
	std::vector<Alignment> out;
	out.reserve(results.size());
	for (const ebo_align_result& r : results)
	{
		out.push_back(toAlignment(r));
	}
	return out;
}
}  // namespace detail

// aligner.cpp:27-88: the similarity T with data ~ T * model in the least-squares sense, and the translational error
inline Alignment alignPoints(ebo_ctx* ctx, const std::vector<common::Vector3d>& data, const std::vector<common::Vector3d>& model,
							 bool fixScale = false)
{
	return detail::alignSegments(ctx, data, model, {0}, {static_cast<int>(data.size())}, fixScale, "align_points_sim3")[0];
}

inline common::Sim3 align_points_sim3(ebo_ctx* ctx, const std::vector<common::Vector3d>& data, const std::vector<common::Vector3d>& model,
									  ErrorMetricValue* ate)
{
	const Alignment a = alignPoints(ctx, data, model);
	if (ate)
	{
		*ate = a.ate;
	}
	return a.sim;
}

// aligner.cpp:95-114: camera i of the list against reference_poses[i], by their centres.  The reference does not look
// at the lengths; here fewer reference poses than cameras is an error
inline common::Sim3 align_cameras_sim3(ebo_ctx* ctx, const std::vector<common::Pose3d>& reference_poses, const std::list<Keyframe>& cameras,
									   ErrorMetricValue* ate)
{
	if (reference_poses.size() < cameras.size())
	{
		throw std::invalid_argument("align_cameras_sim3: fewer reference poses than cameras");
	}
	std::vector<common::Vector3d> reference_centers, camera_centers;
	size_t i = 0;
	for (const auto& kf : cameras)
	{
		reference_centers.push_back(reference_poses[i].translation());
		camera_centers.push_back(kf.pose.translation());
		++i;
	}
	return align_points_sim3(ctx, reference_centers, camera_centers, ate);
}

// every prefix of length first .. K of a K-pose trajectory in ONE call: entry k - first is the alignment of the first k
// poses, what the reference computes after its k-th keyframe
inline std::vector<Alignment> alignPrefixes(ebo_ctx* ctx, const std::vector<common::Vector3d>& reference_centres,
											const std::vector<common::Vector3d>& camera_centres, size_t first, bool fixScale = false)
{
	std::vector<int> begin, end;
	for (size_t k = first; k <= camera_centres.size(); ++k)
	{
		begin.push_back(0);
		end.push_back(static_cast<int>(k));
	}
	return detail::alignSegments(ctx, reference_centres, camera_centres, begin, end, fixScale, "alignPrefixes");
}

// The relative pose error of one step size (include/ebo.h, "trajectory evaluation: relative pose error", rules T1-T7;
// the reference has no counterpart): the drift of the estimate over `delta` poses against the ground truth's, the
// translation in the ground truth's unit and the rotation in radians.  status as ebo_rpe_result's (0 evaluated, 1 no
// pair, 2 a non-finite input); unless it is 0 both metrics are zero but for their count
struct RelativeErrors
{
	ErrorMetricValue translation;
	ErrorMetricValue rotation;
	int delta = 0;
	int status = 1;
};

namespace detail
{
inline std::vector<double> packedPoses(const std::vector<common::Pose3d>& poses)
{
	std::vector<double> out(12 * poses.size());
	for (size_t i = 0; i < poses.size(); ++i)
	{
		poses[i].toArray(&out[12 * i]);
	}
	return out;
}

inline RelativeErrors toRelativeErrors(const ebo_rpe_result& r, int delta)
{
	RelativeErrors e;
	e.translation.rmse = r.trans_rmse;
	e.translation.mean = r.trans_mean;
	e.translation.min = r.trans_min;
	e.translation.max = r.trans_max;
	e.rotation.rmse = r.rot_rmse;
	e.rotation.mean = r.rot_mean;
	e.rotation.min = r.rot_min;
	e.rotation.max = r.rot_max;
	e.translation.count = e.rotation.count = static_cast<double>(r.count);
	e.delta = delta;
	e.status = r.status;
	return e;
}

// entry [g][k]: segment g at deltas[k]
inline std::vector<std::vector<RelativeErrors>> relativeErrorsOfSegments(ebo_ctx* ctx, const std::vector<common::Pose3d>& reference_poses,
																		 const std::vector<common::Pose3d>& camera_poses,
																		 const std::vector<int>& begin, const std::vector<int>& end,
																		 const std::vector<double>& scales, const std::vector<int>& deltas,
																		 const char* who)
{
	if (reference_poses.size() != camera_poses.size())
	{
		throw std::invalid_argument(std::string(who) + ": reference and camera poses differ in length");
	}
	if (!scales.empty() && scales.size() != begin.size())
	{
		throw std::invalid_argument(std::string(who) + ": one scale per segment, or none");
	}
	const std::vector<double> gt = packedPoses(reference_poses), est = packedPoses(camera_poses);
	std::vector<ebo_rpe_result> results(begin.size() * deltas.size());
	check(ctx,
		  ebo_trajectory_rpe(ctx, static_cast<int>(reference_poses.size()), gt.data(), est.data(), static_cast<int>(begin.size()),
							 begin.data(), end.data(), scales.empty() ? nullptr : scales.data(), static_cast<int>(deltas.size()),
							 deltas.data(), results.data()),
		  who);
	std::vector<std::vector<RelativeErrors>> out(begin.size());
	for (size_t g = 0; g < begin.size(); ++g)
	{
		for (size_t k = 0; k < deltas.size(); ++k)
		{
			out[g].push_back(toRelativeErrors(results[g * deltas.size() + k], deltas[k]));
		}
	}
	return out;
}
}  // namespace detail

// camera pose i against reference pose i, both camera (or body) to world, over steps of deltas[k] poses: entry k is the
// relative pose error at deltas[k], with the camera translations multiplied by `scale` (an alignment's, for an estimate
// with a free scale).  No alignment is needed: a rigid motion of either trajectory changes nothing
inline std::vector<RelativeErrors> relativePoseErrors(ebo_ctx* ctx, const std::vector<common::Pose3d>& reference_poses,
													  const std::vector<common::Pose3d>& camera_poses, const std::vector<int>& deltas,
													  double scale = 1.0)
{
	return detail::relativeErrorsOfSegments(ctx, reference_poses, camera_poses, {0}, {static_cast<int>(camera_poses.size())}, {scale}, deltas,
											"relativePoseErrors")[0];
}

// every prefix of length first .. K of a K-pose trajectory in ONE call: entry [k - first][d] is the error of the first k
// poses at deltas[d], what an evaluation after the k-th keyframe gives.  scales: one per prefix (alignPrefixes' scales),
// or empty for 1
inline std::vector<std::vector<RelativeErrors>> relativePoseErrorsPrefixes(ebo_ctx* ctx, const std::vector<common::Pose3d>& reference_poses,
																			const std::vector<common::Pose3d>& camera_poses,
																			const std::vector<int>& deltas, size_t first,
																			const std::vector<double>& scales = {})
{
	std::vector<int> begin, end;
	for (size_t k = first; k <= camera_poses.size(); ++k)
	{
		begin.push_back(0);
		end.push_back(static_cast<int>(k));
	}
	return detail::relativeErrorsOfSegments(ctx, reference_poses, camera_poses, begin, end, scales, deltas, "relativePoseErrorsPrefixes");
}

namespace detail
{
// log of a rigid motion as Sophus::SE3d::log states it (through the unit quaternion of the rotation; below 1e-10 the
// series): (upsilon, omega)
inline void se3Log(const common::Pose3d& T, double (&upsilon)[3], double (&omega)[3])
{
	const common::Matrix3d& R = T.rotationMatrix();
	// the unit quaternion (w >= 0) of R, by the largest of the four squares
	double q[4];  // w, x, y, z
	const double tr = R(0, 0) + R(1, 1) + R(2, 2);
	if (tr > 0.0)
	{
		const double s = 2.0 * std::sqrt(tr + 1.0);
		q[0] = 0.25 * s;
		q[1] = (R(2, 1) - R(1, 2)) / s;
		q[2] = (R(0, 2) - R(2, 0)) / s;
		q[3] = (R(1, 0) - R(0, 1)) / s;
	}
	else
	{
		int i = 0;
		if (R(1, 1) > R(0, 0)) i = 1;
		if (R(2, 2) > R(i, i)) i = 2;
		const int j = (i + 1) % 3, k = (i + 2) % 3;
		const double s = 2.0 * std::sqrt(((R(i, i) - R(j, j)) - R(k, k)) + 1.0);
		q[1 + i] = 0.25 * s;
		q[0] = (R(k, j) - R(j, k)) / s;
		q[1 + j] = (R(j, i) + R(i, j)) / s;
		q[1 + k] = (R(k, i) + R(i, k)) / s;
		if (q[0] < 0.0)
		{
			for (double& c : q) c = -c;
		}
	}
	const double n2 = (q[1] * q[1] + q[2] * q[2]) + q[3] * q[3];
	const double n = std::sqrt(n2);
	const double k = n < 1e-10 ? 2.0 / q[0] - (2.0 / 3.0) * n2 / (q[0] * q[0] * q[0]) : 2.0 * std::atan2(n, q[0]) / n;
	const double theta = k * n;
	for (int i = 0; i < 3; ++i)
	{
		omega[i] = k * q[1 + i];
	}
	// V^-1 = I - Omega / 2 + c Omega^2
	const double half = 0.5 * theta;
	const double c = std::fabs(theta) < 1e-10 ? 1.0 / 12.0 : (1.0 - theta * std::cos(half) / (2.0 * std::sin(half))) / (theta * theta);
	const common::Vector3d& t = T.translation();
	const double wt[3] = {omega[1] * t[2] - omega[2] * t[1], omega[2] * t[0] - omega[0] * t[2], omega[0] * t[1] - omega[1] * t[0]};
	const double wwt[3] = {omega[1] * wt[2] - omega[2] * wt[1], omega[2] * wt[0] - omega[0] * wt[2], omega[0] * wt[1] - omega[1] * wt[0]};
	for (int i = 0; i < 3; ++i)
	{
		upsilon[i] = (t[i] - 0.5 * wt[i]) + c * wwt[i];
	}
}

// exp as Sophus::SE3d::exp states it
inline common::Pose3d se3Exp(const double (&upsilon)[3], const double (&omega)[3])
{
	const double theta2 = (omega[0] * omega[0] + omega[1] * omega[1]) + omega[2] * omega[2];
	const double theta = std::sqrt(theta2);
	const bool small = theta < 1e-10;
	const double half = 0.5 * theta;
	const double imag = small ? (0.5 - theta2 / 48.0) + theta2 * theta2 / 3840.0 : std::sin(half) / theta;
	const double real = small ? (1.0 - theta2 / 8.0) + theta2 * theta2 / 384.0 : std::cos(half);
	const common::Pose3d rot(real, imag * omega[0], imag * omega[1], imag * omega[2], 0.0, 0.0, 0.0);
	const double wu[3] = {omega[1] * upsilon[2] - omega[2] * upsilon[1], omega[2] * upsilon[0] - omega[0] * upsilon[2],
						  omega[0] * upsilon[1] - omega[1] * upsilon[0]};
	const double wwu[3] = {omega[1] * wu[2] - omega[2] * wu[1], omega[2] * wu[0] - omega[0] * wu[2], omega[0] * wu[1] - omega[1] * wu[0]};
	common::Vector3d t;
	if (small)
	{
		t = rot * common::Vector3d(upsilon[0], upsilon[1], upsilon[2]);  // V = the rotation
	}
	else
	{
		const double a = (1.0 - std::cos(theta)) / theta2, b = (theta - std::sin(theta)) / (theta2 * theta);
		for (int i = 0; i < 3; ++i)
		{
			t[i] = (upsilon[i] + a * wu[i]) + b * wwu[i];
		}
	}
	return common::Pose3d(rot.rotationMatrix(), t);
}

// Sophus::interpolate: prev * exp(p * log(prev^-1 * next))
inline common::Pose3d interpolate(const common::Pose3d& prev, const common::Pose3d& next, double p)
{
	double upsilon[3], omega[3];
	se3Log(prev.inverse() * next, upsilon, omega);
	for (int i = 0; i < 3; ++i)
	{
		upsilon[i] = p * upsilon[i];
		omega[i] = p * omega[i];
	}
	return prev * se3Exp(upsilon, omega);
}
}  // namespace detail

// visual_odometry.cpp:522-561 over samples in ascending time: nothing at or after `timestamp` -> none; a sample AT
// it -> that sample's pose, bit for bit; nothing before it -> none; otherwise the two neighbours interpolated at
// p = float(timestamp - previous) / (next - previous), the quotient taken in float as the reference takes it
inline std::optional<common::Pose3d> syncGroundTruth(const common::GroundTruth& samples, const common::timestamp_t& timestamp)
{
	auto lowerBoundIt = std::lower_bound(samples.begin(), samples.end(), timestamp,
										 [](const common::GroundTruthSample& a, const common::timestamp_t& t) { return a.timestamp < t; });
	if (lowerBoundIt == samples.end())
	{
		return {};
	}
	if (lowerBoundIt->timestamp == timestamp)
	{
		return std::make_optional(lowerBoundIt->value);
	}
	if (lowerBoundIt == samples.begin())
	{
		return {};
	}
	const common::GroundTruthSample& nextPose = *lowerBoundIt;
	const common::GroundTruthSample& prevPose = *(lowerBoundIt - 1);
	const float p = static_cast<float>((timestamp - prevPose.timestamp).count()) / (nextPose.timestamp - prevPose.timestamp).count();
	return std::make_optional(detail::interpolate(prevPose.value, nextPose.value, static_cast<double>(p)));
}
}  // namespace visual_odometry
