// ebo_depth.h — what the device side and the host side of the space-sweep depth map share (csrc/ebo_depth.inc's
// kernels, csrc/ebo_depth.cpp's entries, tools/dsi_serial.cpp).  Plain host C++, no HIP.
#pragma once

#include <stdint.h>

namespace ebo
{
constexpr int kDsiChunkMax = 64;    // windows per vote launch
constexpr int kDsiBlock = 256;
constexpr int kDsiMaxPlanes = 256;  // M1
constexpr int kDsiMaxRadius = 7;    // M6, M7
constexpr uint64_t kDsiMaxEvents = 1ull << 21;  // M4: 2^21 events of at most 2^10 a voxel stay below 2^32
struct DsiWindows
{
	int n = 0;
	int win[kDsiChunkMax];
};
struct DsiConsts
{
	double fx, fy, cx, cy;
	int32_t w, h;
	int32_t upw;     // units per window (P + 1: the stray unit, which takes no part)
	int32_t nz;      // planes of the volume
	int32_t planes;  // planes per workgroup of the vote: grid.z = ceil(nz / planes)
	int32_t tile;    // 1: a plane's votes of a patch are accumulated in LDS; 0: every tap a global atomic
};
// M2's relative pose of one window, made on the host
struct DsiPose
{
	double Rr[9];  // row-major
	double tr[3];
};
}  // namespace ebo
