// ransac_walk.h — the serial stopping rule of both RANSAC paths (include/ebo.h: rule 6 for two-view geometry, A5 for
// absolute pose): the answer the reference's one-hypothesis-at-a-time loop would give, read off the inlier counts of all
// hypotheses.  No HIP: tests/cpp/ransac_walk_test.cpp runs it on the CPU against both numpy restatements.
#pragma once

#include <algorithm>
#include <cmath>

namespace ebo
{
// count[0 .. maxIterations): inliers of each hypothesis among the group's n points; sampleSize: points a hypothesis
// draws, a power of two (8 or 4).  A hypothesis wins only by strictly more inliers than every one before it; after a
// new best the loop needs k = log(1 - probability) / log(1 - w^sampleSize) hypotheses, w = best / n, the argument of
// the second log clamped to [1e-15, 1 - 1e-15].  The power is formed by squaring (w2 = w * w, w4 = w2 * w2, ...),
// every product rounded on its own.
inline void ransac_walk(const int* count, int n, int maxIterations, double probability, int sampleSize, int& best, int& winner,
						int& iterations)
{
	best = -1;
	winner = -1;
	double k = static_cast<double>(maxIterations);
	int h = 0;
	for (;; ++h)
	{
		if (count[h] > best)
		{
			best = count[h];
			winner = h;
			double ws = static_cast<double>(best) / static_cast<double>(n);
			for (int s = 1; s < sampleSize; s *= 2)
			{
				ws = ws * ws;
			}
			const double x = std::min(std::max(1.0 - ws, 1e-15), 1.0 - 1e-15);
			k = std::log(1.0 - probability) / std::log(x);
		}
		if (static_cast<double>(h + 1) >= k || h + 1 == maxIterations)
		{
			break;
		}
	}
	iterations = h + 1;
}
}  // namespace ebo
