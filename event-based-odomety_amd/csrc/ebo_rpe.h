// ebo_rpe.h — what the builds of the relative pose error share: the limits of a call and the angle rule's constants
// (csrc/ebo_rpe.inc's kernel, csrc/ebo_rpe.cpp's entry, tools/rpe_serial.cpp).  The lane count of its sums is
// ebo_relpose.h's kRpLanes: the tree is R6's.  Plain host C++, no HIP.
#pragma once

namespace ebo
{
constexpr int kRpeMaxSegments = 65535;
constexpr int kRpeMaxDeltas = 16;
constexpr int kRpeMaxSegmentPoses = 1 << 24;  // poses per segment: double(n_pairs) and the counts of T6 stay exact far beyond
constexpr int kRpePoseDoubles = 12;           // [R | t], row-major [3][4]
constexpr int kRpeHalvings = 2;               // T5: u <- u / (1 + sqrt(1 + u * u)), twice: the angle is an eighth of its first size
constexpr int kRpeTerms = 13;                 // T5: the odd powers u^1 .. u^25 of the arctangent's series
constexpr double kRpePi = 3.141592653589793;  // double(pi)
}  // namespace ebo
