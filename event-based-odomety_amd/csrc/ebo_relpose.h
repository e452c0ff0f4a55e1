// ebo_relpose.h — what the builds of the relative-pose refinement share: the lane count of its sums, the limits of a
// call and the size of the work memory (csrc/ebo_relpose.inc's kernel, csrc/ebo_relpose.cpp's entry,
// tools/relpose_refine_serial.cpp).  Plain host C++, no HIP.
#pragma once

#include <stddef.h>

namespace ebo
{
constexpr int kRpLanes = 64;          // partial sums of a tree (R6): one wave
constexpr int kRpVars = 5;            // (a, b, om_x, om_y, om_z)
constexpr int kRpMinInliers = 5;      // a pair with fewer listed inliers is not refined
constexpr int kRpMaxPoints = 65535;   // correspondences per pair, the RANSAC entry's limit
constexpr int kRpMaxPairs = 65535;
constexpr int kRpRowDoubles = 6 * kRpVars + 6;  // work memory per listed inlier: the scaled Jacobian [6][5], the chords [6]

// doubles of work memory for `inliers` listed inliers (the total of a call)
inline size_t rp_work_doubles(size_t inliers)
{
	return kRpRowDoubles * inliers;
}
}  // namespace ebo
