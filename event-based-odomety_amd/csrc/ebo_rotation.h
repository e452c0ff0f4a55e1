// ebo_rotation.h — what the device side and the host side of the rotational contrast maximisation share
// (csrc/ebo_rotation.inc's kernels, csrc/ebo_rotation.cpp's entries, tools/rotation_serial.cpp).  Plain host C++, no HIP.
#pragma once

#include <stdint.h>

namespace ebo
{
constexpr int kRotChunkMax = 64;
constexpr int kRotBlock = 256;
struct RotWindows
{
	int n = 0;
	int win[kRotChunkMax];
};
struct RotConsts
{
	double fx, fy, cx, cy;
	double g[7];          // V5's weights, d = -3 .. 3 (0 0 0 1 0 0 0 for sigma_blur = 0)
	double np;            // w * h as a double
	double two_over_np;   // 2 / np
	int32_t w, h;
	int32_t upw;          // units per window (P + 1: the stray unit, which takes no part)
	int32_t P;
	int32_t tile;         // 1: the vote accumulates a patch's surroundings in LDS; 0 (A/B build only): every tap a global atomic
	int32_t reserved;
};
}  // namespace ebo
