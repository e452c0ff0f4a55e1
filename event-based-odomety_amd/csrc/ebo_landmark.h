// ebo_landmark.h — what the builds of landmark maintenance share: the limits of a call and the shape of L2's sums
// (csrc/ebo_landmark.inc's kernel, csrc/ebo_landmark.cpp's entries, tools/landmark_serial.cpp).  Plain host C++, no HIP.
#pragma once

namespace ebo
{
constexpr int kLmMaxObs = 512;              // observations per landmark: what one wave's LDS stages (24 KB)
constexpr int kLmMaxLandmarks = 1 << 20;    // landmarks per call
constexpr int kLmMaxHypotheses = 4096;
constexpr int kLmPartials = 16;             // L2: partial j takes the observations o = j (mod 16)
constexpr int kLmTerms = 9;                 // L2: M00 M01 M02 M11 M12 M22 b0 b1 b2
constexpr int kLmSweeps = 8;                // L3: jacobi(M, 8)
constexpr int kLmPoseDoubles = 12;          // [R | t], row-major [3][4]
constexpr int kLmGroupMaxObs = kLmMaxObs / 4;  // the most a landmark may hold when four share a wave
}  // namespace ebo
