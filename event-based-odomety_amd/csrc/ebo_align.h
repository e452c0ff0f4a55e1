// ebo_align.h — what the builds of the trajectory alignment share: the limits of a call and the sweep count of its
// Jacobi iteration (csrc/ebo_align.inc's kernel, csrc/ebo_align.cpp's entry, tools/align_sim3_serial.cpp).  The lane
// count of its sums is ebo_relpose.h's kRpLanes: the tree is R6's.  Plain host C++, no HIP.
#pragma once

namespace ebo
{
constexpr int kAlSweeps = 8;                  // jacobi(G, 8)
constexpr int kAlMinPoints = 3;               // a segment with fewer points is not aligned (status 1)
constexpr int kAlMaxSegmentPoints = 1 << 24;  // points per segment: double(n) and the counts of S7 stay exact far beyond
constexpr int kAlMaxSegments = 65535;
}  // namespace ebo
