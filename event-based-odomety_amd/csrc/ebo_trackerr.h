// ebo_trackerr.h — what the builds of the track evaluation share: the limits of a call and rule V3's two steps, the
// search and the interpolation, which the kernel (csrc/ebo_trackerr.inc), the host's seeds (csrc/ebo_trackerr.cpp,
// ebo_track_seeds) and tools/track_errors_serial.cpp all take from here.  The lane count of its sums is ebo_relpose.h's
// kRpLanes: the tree is R6's.  Plain C++; under hipcc the two functions are compiled for both sides.
#pragma once

#include <cstdint>

#ifdef __HIPCC__
#define TE_HD __host__ __device__ inline
#else
#define TE_HD inline
#endif

namespace ebo
{
constexpr int kTeMaxTracks = 65535;
constexpr int kTeMaxTaus = 8;
constexpr int kTeMaxTrackSamples = 1 << 24;  // samples per track, of either side: double(n_inliers) stays exact far beyond

// the trip count of te_search over n >= 1 times: ceil(log2 n), the same for every sample of a track
TE_HD int te_steps(int n)
{
	int steps = 0;
	for (int d = n - 1; d > 0; d /= 2)
	{
		++steps;
	}
	return steps;
}

// V3's index: the largest j in [0, n) with t[j] <= T, for non-decreasing t with t[0] <= T; `steps` = te_steps(n).  The
// distance hi - lo halves with every trip whichever way it goes, so the count does not depend on T.  Never outside
// [0, n), whatever t holds.
TE_HD int te_search(const int64_t* t, int n, int steps, int64_t T)
{
	int lo = 0, hi = n - 1;
	for (int s = 0; s < steps; ++s)
	{
		const int mid = lo + (hi - lo + 1) / 2;
		if (t[mid] <= T)
		{
			lo = mid;
		}
		else
		{
			hi = mid - 1;
		}
	}
	return lo;
}

// V3's value: component c of the track (t, xy) at time T, j = te_search's index.  A sample exactly at T is returned as
// it is; otherwise subtract, multiply, add, one rounding each.  j + 1 is read only when t[j] != T, and never beyond the
// last sample: ordered times have t[n - 1] == T there, and for others the index is held back.
TE_HD void te_interp(const int64_t* t, const double* xy, int n, int j, int64_t T, double& gx, double& gy)
{
	gx = xy[2 * static_cast<size_t>(j)];
	gy = xy[2 * static_cast<size_t>(j) + 1];
	if (t[j] != T)
	{
		const int k = j + 1 < n ? j + 1 : j;
		const double w = static_cast<double>(T - t[j]) / static_cast<double>(t[k] - t[j]);
		gx = gx + w * (xy[2 * static_cast<size_t>(k)] - gx);
		gy = gy + w * (xy[2 * static_cast<size_t>(k) + 1] - gy);
	}
}
}  // namespace ebo
