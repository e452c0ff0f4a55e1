// ebo_maptrack.h — what the three builds of the map tracker share (csrc/ebo_maptrack.inc's kernel, csrc/ebo_maptrack.cpp's
// entries, tools/map_track_serial.cpp): the limits, the lane count, the call's constants and the default options
// (ebo_default_map_track_opts).  Plain host C++, no HIP.
#pragma once

#include <stddef.h>

#include "ebo_bundle.h"

namespace ebo
{
constexpr int kMtLanes = 256;
constexpr int kMtMaxUnits = 65535;
constexpr int kMtMaxPoints = 1 << 20;
constexpr int kMtMaxIterations = 10000;  // opts->max_num_iterations: bounds the trace, [units][iterations + 1][4] doubles
constexpr int kMtSums = 28;  // E7: 21 of J'J (packed lower triangle), 6 of J'r, 1 of r r

// one call: the camera (C1), the images' shape and the arrays every unit shares
struct MtCall
{
	double fx, fy, cx, cy;
	double z_min;
	int w, h;
	int n_images, n_points;
	const double* images;  // [n_images][h][w]
	const double* points;  // [n_points][3]
};

// ebo_default_ba_opts' values; E8 names max_num_iterations on its own because a tracker may want fewer
inline void mt_default_opts(ebo_solver_opts& o)
{
	ba_default_opts(o);
	o.max_num_iterations = 50;
}
}  // namespace ebo
