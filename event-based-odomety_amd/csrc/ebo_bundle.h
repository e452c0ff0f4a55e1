// ebo_bundle.h — what the three builds of the bundle adjustment share: the limits of a problem, the sizes of the
// work memory the solve carves (csrc/ebo_bundle.inc's kernel, csrc/ebo_bundle.cpp's entry, tools/bundle_adjust_serial.cpp)
// and the default options (ebo_default_ba_opts).  Plain host C++, no HIP.
#pragma once

#include <stddef.h>

#include "../../include/ebo.h"

namespace ebo
{
constexpr int kBaLanes = 256;
constexpr int kBaMaxFrames = 24;
constexpr int kBaMaxPoints = 4096;
constexpr int kBaMaxObs = 65535;
constexpr int kBaMaxProblems = 65535;
constexpr int kBaMaxDim = 6 * kBaMaxFrames;

// doubles of work memory for F frames, P points and N observations (totals of a call), in the order the solve carves
// them: current and candidate poses and points, res Jc Jp W Y per observation, U | g per frame, V | g and the inverse
// per point, scale and step per parameter, the tree's input
inline size_t ba_work_doubles(size_t F, size_t P, size_t N)
{
	return 24 * F + 6 * P + 56 * N + 42 * F + 21 * P + 2 * (6 * F + 3 * P) + (N + 12 * F + 3 * P);
}
// ints: the [P][F] tables, P + 1 point starts per problem, slot and list per frame
inline size_t ba_work_ints(size_t F, size_t P, size_t table, size_t problems)
{
	return table + P + problems + 2 * F;
}
// doubles of the reduced system's packed lower triangle for `frames` frames, all of them free
inline size_t ba_reduced_doubles(int frames)
{
	const size_t dim = 6 * static_cast<size_t>(frames);
	return dim * (dim + 1) / 2;
}

// Ceres' Solver::Options defaults, which the reference leaves untouched (visual_odometry.cpp:488-491)
inline void ba_default_opts(ebo_solver_opts& o)
{
	o = ebo_solver_opts{};
	o.max_num_iterations = 50;
	o.use_nonmonotonic = 0;
	o.function_tolerance = 1e-6;
	o.gradient_tolerance = 1e-10;
	o.parameter_tolerance = 1e-8;
	o.initial_radius = 1e4;
	o.max_radius = 1e16;
	o.min_radius = 1e-32;
	o.min_relative_decrease = 1e-3;
	o.min_lm_diagonal = 1e-6;
	o.max_lm_diagonal = 1e32;
	o.max_consecutive_nonmonotonic = 5;
	o.max_consecutive_invalid = 5;
	o.jacobi_scaling = 1;
	o.mode = EBO_SOLVE_GLOBAL;
}
}  // namespace ebo
