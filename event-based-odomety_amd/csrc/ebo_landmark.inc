// ebo_landmark.inc — landmark maintenance on the device: robust N-view triangulation of a landmark from its WHOLE
// observation list (consensus over two-observation hypotheses, then least squares over the winner's inliers) and the
// audit of an existing landmark against its observations under the current poses, every landmark of a call in one
// launch.  The reference triangulates a landmark once, from the first two keyframes that see it
// (visual_odometry.cpp:353-405), and never removes one (its TODOs at :169 and :407).  Included inside
// ebo_kernels.hip's anonymous namespace, after ebo_abspose.inc, whose score (A1) and cofactors it uses, with
// ebo_twoview.inc's dot, 3 x 3 Jacobi rotation and ebo_ransac.inc's sampler.  The rules are written out in
// include/ebo.h ("landmark maintenance", L1-L7); tests/landmark_ref.py restates them in numpy.  Every float64
// operation is rounded on its own (__dadd_rn / __dsub_rn / __dmul_rn / __ddiv_rn / __dsqrt_rn).

__device__ __forceinline__ bool lm_finite(double x)
{
	return fabs(x) < __builtin_inf();
}

// L1: the world ray of one observation, r = (d, e): d = R f, e = t - c_ref
__device__ __forceinline__ void lm_ray(const double* __restrict__ pose, const double (&f)[3], const double (&cref)[3], double (&r)[6])
{
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		r[i] = tv_dot3(pose[4 * i], pose[4 * i + 1], pose[4 * i + 2], f[0], f[1], f[2]);
		r[3 + i] = __dsub_rn(pose[4 * i + 3], cref[i]);
	}
}

// L2: the nine terms of one observation, in the order M00 M01 M02 M11 M12 M22 b0 b1 b2
__device__ __forceinline__ void lm_terms(const double (&r)[6], double (&t)[kLmTerms])
{
	const double dd = tv_dot3(r[0], r[1], r[2], r[0], r[1], r[2]);
	const double a00 = __dsub_rn(dd, __dmul_rn(r[0], r[0]));
	const double a11 = __dsub_rn(dd, __dmul_rn(r[1], r[1]));
	const double a22 = __dsub_rn(dd, __dmul_rn(r[2], r[2]));
	const double a01 = -__dmul_rn(r[0], r[1]);
	const double a02 = -__dmul_rn(r[0], r[2]);
	const double a12 = -__dmul_rn(r[1], r[2]);
	t[0] = a00;
	t[1] = a01;
	t[2] = a02;
	t[3] = a11;
	t[4] = a12;
	t[5] = a22;
	t[6] = tv_dot3(a00, a01, a02, r[3], r[4], r[5]);
	t[7] = tv_dot3(a01, a11, a12, r[3], r[4], r[5]);
	t[8] = tv_dot3(a02, a12, a22, r[3], r[4], r[5]);
}

// L2's sums over a set of two observations.  By the rule, partial a mod 16 is (+0 + T_a), partial b mod 16 is
// (+0 + T_b) (or ((+0 + T_a) + T_b) in one partial) and the tree then adds partials that are +0.  (+0 + x) is never
// -0, a sum with such a term is -0 only when both are, and x + (+0) = x for every x that is not -0: so
// (+0 + T_a) + (+0 + T_b) has the rule's bits in either case and in either order of a and b.
__device__ __forceinline__ void lm_pair_sums(const double (&ra)[6], const double (&rb)[6], double (&S)[kLmTerms])
{
	double ta[kLmTerms], tb[kLmTerms];
	lm_terms(ra, ta);
	lm_terms(rb, tb);
#pragma unroll
	for (int k = 0; k < kLmTerms; ++k)
	{
		S[k] = __dadd_rn(__dadd_rn(0.0, ta[k]), __dadd_rn(0.0, tb[k]));
	}
}

__device__ __forceinline__ void lm_matrix(const double (&S)[kLmTerms], double (&M)[3][3])
{
	M[0][0] = S[0];
	M[0][1] = M[1][0] = S[1];
	M[0][2] = M[2][0] = S[2];
	M[1][1] = S[3];
	M[1][2] = M[2][1] = S[4];
	M[2][2] = S[5];
}

// L2: the point of the sums S; false (X untouched) when there is none
__device__ __forceinline__ bool lm_solve(const double (&S)[kLmTerms], const double (&cref)[3], double (&X)[3])
{
	double M[3][3], C[3][3];
	lm_matrix(S, M);
	const double D = ap_cof(M, C);
	if (!(D > 0.0))
	{
		return false;
	}
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		X[i] = __dadd_rn(cref[i], __ddiv_rn(tv_dot3(C[0][i], C[1][i], C[2][i], S[6], S[7], S[8]), D));
	}
	return true;
}

// L3: the parallax of `count` observations whose sums are S (only M is read)
__device__ __forceinline__ double lm_parallax(const double (&S)[kLmTerms], double count)
{
	double M[3][3], V[3][3];
	lm_matrix(S, M);
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
#pragma unroll
		for (int j = 0; j < 3; ++j)
		{
			V[i][j] = (i == j) ? 1.0 : 0.0;
		}
	}
	for (int sweep = 0; sweep < kLmSweeps; ++sweep)
	{
		tv_rot3<0, 1>(M, V);
		tv_rot3<0, 2>(M, V);
		tv_rot3<1, 2>(M, V);
	}
	double lo = M[0][0];
	lo = M[1][1] < lo ? M[1][1] : lo;
	lo = M[2][2] < lo ? M[2][2] : lo;
	return __ddiv_rn(__dmul_rn(2.0, lo), count);
}

// L4's gate on the two rays of a hypothesis
__device__ __forceinline__ bool lm_gate(const double (&ra)[6], const double (&rb)[6], double minParallax)
{
	const double g = tv_dot3(ra[0], ra[1], ra[2], rb[0], rb[1], rb[2]);
	const double n2 = __dmul_rn(tv_dot3(ra[0], ra[1], ra[2], ra[0], ra[1], ra[2]), tv_dot3(rb[0], rb[1], rb[2], rb[0], rb[1], rb[2]));
	return n2 > 0.0 && __dsub_rn(1.0, __ddiv_rn(g, __dsqrt_rn(n2))) >= minParallax;
}

// L4: the h-th pair (a, b), a < b, of m observations in lexicographic order
__device__ __forceinline__ void lm_unrank(int h, int m, int& a, int& b)
{
	int first = 0, rem = h;
	while (rem >= m - 1 - first)
	{
		rem -= m - 1 - first;
		++first;
	}
	a = first;
	b = first + 1 + rem;
}

// L4: hypothesis h of a landmark of m observations
__device__ __forceinline__ void lm_hypothesis(bool exhaustive, unsigned long long seed, int h, int m, int& a, int& b)
{
	if (exhaustive)
	{
		lm_unrank(h, m, a, b);
	}
	else
	{
		int smp[2];
		ransac_sample<2>(seed, 0, h, m, smp);
		a = smp[0];
		b = smp[1];
	}
}

// A1 for observation (pose, f) under the point X
__device__ __forceinline__ double lm_score(const double* __restrict__ pose, const double* __restrict__ f, const double (&X)[3])
{
	const TvPoseRT T = tv_load_pose(pose);
	const double fv[3] = {f[0], f[1], f[2]};
	return ap_score(T, fv, X);
}

#ifndef EBO_LANDMARK_RULES_ONLY  // tools/landmark_serial.cpp compiles the rules above for the host and stops here

struct LmParamsArg
{
	double threshold, minParallax;
	int minInliers, maxHypotheses;
	unsigned long long seed;
};

template <int W>
__device__ __forceinline__ int lm_sum_int(int v)
{
#pragma unroll
	for (int s = W / 2; s > 0; s /= 2)
	{
		v += __shfl_xor(v, s, W);
	}
	return v;
}

// L2's sums over the observations of a landmark that are inliers under the point Xq, every lane of the group
// receiving them.  Lane j < 16 of the group is partial j: it walks o = j, j + 16, .. in ascending order; the tree is
// four shuffles among those sixteen lanes.  The other lanes of a wider group carry zeros.
template <int W>
__device__ __forceinline__ void lm_inlier_sums(int lane, int m, long long base, const int* __restrict__ obsPose,
											   const double* __restrict__ poses, const double* __restrict__ obsF,
											   const double (*rays)[6], const double (&Xq)[3], double threshold, double (&S)[kLmTerms])
{
	double part[kLmTerms];
#pragma unroll
	for (int k = 0; k < kLmTerms; ++k)
	{
		part[k] = 0.0;
	}
	if (lane < kLmPartials)
	{
		for (int o = lane; o < m; o += kLmPartials)
		{
			const double sc = lm_score(poses + kLmPoseDoubles * static_cast<size_t>(obsPose[base + o]), obsF + 3 * (base + o), Xq);
			if (sc < threshold)
			{
				double r[6], t[kLmTerms];
#pragma unroll
				for (int k = 0; k < 6; ++k)
				{
					r[k] = rays[o][k];
				}
				lm_terms(r, t);
#pragma unroll
				for (int k = 0; k < kLmTerms; ++k)
				{
					part[k] = __dadd_rn(part[k], t[k]);
				}
			}
		}
	}
#pragma unroll
	for (int s = kLmPartials / 2; s > 0; s /= 2)
	{
#pragma unroll
		for (int k = 0; k < kLmTerms; ++k)
		{
			part[k] = __dadd_rn(part[k], __shfl_down(part[k], s, kLmPartials));  // lanes >= s add what no later step reads
		}
	}
#pragma unroll
	for (int k = 0; k < kLmTerms; ++k)
	{
		S[k] = __shfl(part[k], 0, W);
	}
}

// One group of W lanes per landmark, 64 / W landmarks per wave; W = 64 stages up to kLmMaxObs observations of its
// landmark, W = 16 up to kLmGroupMaxObs of each of its four (the entry chooses).  SOLVE: L1-L6 (ebo_triangulate_tracks);
// otherwise L7 on the given points (ebo_landmark_scores).  The results do not depend on W: the counts are integers, the
// winner is the first of the largest, the maximum is exact and L2's sums are taken by sixteen lanes either way.
template <bool SOLVE, int W>
__global__ void __launch_bounds__(64) k_landmarks(int nPoses, const double* __restrict__ poses, int nLm, const int* __restrict__ offsets,
												   const int* __restrict__ obsPose, const double* __restrict__ obsF,
												   const double* __restrict__ points, LmParamsArg prm,
												   ebo_landmark_result* __restrict__ results, double* __restrict__ scores,
												   unsigned char* __restrict__ flags)
{
	constexpr int kGroups = 64 / W, kSlots = kLmMaxObs / kGroups;
	__shared__ double sRays[kGroups][kSlots][6];
	const int lane = static_cast<int>(threadIdx.x) % W, grp = static_cast<int>(threadIdx.x) / W;
	const int l = static_cast<int>(blockIdx.x) * kGroups + grp;
	const bool live = l < nLm;
	const long long base = live ? offsets[l] : 0;
	int m = live ? offsets[l + 1] - offsets[l] : 0;
	// the entry has refused such a landmark; never past the staging area
	m = m < 0 ? 0 : (m > kSlots ? kSlots : m);
	double(*rays)[6] = sRays[grp];

	// L6's scan and L1, the whole wave together
	int bad = 0;
	double cref[3] = {0.0, 0.0, 0.0};
	if (m > 0)
	{
		const int k0 = obsPose[base];
		if (k0 >= 0 && k0 < nPoses)
		{
#pragma unroll
			for (int i = 0; i < 3; ++i)
			{
				cref[i] = poses[kLmPoseDoubles * static_cast<size_t>(k0) + 4 * i + 3];
			}
		}
	}
	for (int o = lane; o < m; o += W)
	{
		const int k = obsPose[base + o];
		const double f[3] = {obsF[3 * (base + o)], obsF[3 * (base + o) + 1], obsF[3 * (base + o) + 2]};
		bool ok = k >= 0 && k < nPoses && lm_finite(f[0]) && lm_finite(f[1]) && lm_finite(f[2]);
		double r[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
		if (ok)
		{
			const double* P = poses + kLmPoseDoubles * static_cast<size_t>(k);
#pragma unroll
			for (int i = 0; i < kLmPoseDoubles; ++i)
			{
				ok = ok && lm_finite(P[i]);
			}
			lm_ray(P, f, cref, r);
		}
		bad |= ok ? 0 : 1;
#pragma unroll
		for (int i = 0; i < 6; ++i)
		{
			rays[o][i] = r[i];
		}
	}
	double X[3] = {0.0, 0.0, 0.0};
	if (!SOLVE && live)
	{
#pragma unroll
		for (int i = 0; i < 3; ++i)
		{
			X[i] = points[3 * static_cast<size_t>(l) + i];
			bad |= lm_finite(X[i]) ? 0 : 1;
		}
	}
	__syncthreads();
	bad = lm_sum_int<W>(bad);
	if (!live)
	{
		return;
	}

	// from here on a group goes its own way; every shuffle stays inside a group, whose lanes stay together
	int status = 0, winner = -1, H = 0, nIn = 0;
	double parallax = 0.0, scoreMax = 0.0;
	bool scored = false;
	if (bad)
	{
		status = 2;
	}
	else if (m < (SOLVE ? 2 : 1))
	{
		status = 1;
	}
	else if (SOLVE)
	{
		// L4: a lane per hypothesis in rounds of W
		const long long nPairs = static_cast<long long>(m) * (m - 1) / 2;
		const bool exhaustive = nPairs <= prm.maxHypotheses;
		H = exhaustive ? static_cast<int>(nPairs) : prm.maxHypotheses;
		int bestCount = -1, bestH = 0x7fffffff;
		for (int h = lane; h < H; h += W)
		{
			int a, b;
			lm_hypothesis(exhaustive, prm.seed, h, m, a, b);
			double ra[6], rb[6], S[kLmTerms], Xh[3];
#pragma unroll
			for (int k = 0; k < 6; ++k)
			{
				ra[k] = rays[a][k];
				rb[k] = rays[b][k];
			}
			if (!lm_gate(ra, rb, prm.minParallax))
			{
				continue;
			}
			lm_pair_sums(ra, rb, S);
			if (!lm_solve(S, cref, Xh))
			{
				continue;
			}
			int count = 0;
			for (int o = 0; o < m; ++o)
			{
				const double sc = lm_score(poses + kLmPoseDoubles * static_cast<size_t>(obsPose[base + o]), obsF + 3 * (base + o), Xh);
				count += sc < prm.threshold ? 1 : 0;
			}
			if (count > bestCount)  // a lane's h ascends: the first of its largest
			{
				bestCount = count;
				bestH = h;
			}
		}
#pragma unroll
		for (int s = W / 2; s > 0; s /= 2)
		{
			const int oc = __shfl_xor(bestCount, s, W), oh = __shfl_xor(bestH, s, W);
			if (oc > bestCount || (oc == bestCount && oh < bestH))
			{
				bestCount = oc;
				bestH = oh;
			}
		}
		if (bestCount < 2)
		{
			status = 3;
		}
		else
		{
			// L5: the winner's point again (every lane alike), then least squares over its inliers
			winner = bestH;
			int a, b;
			lm_hypothesis(exhaustive, prm.seed, winner, m, a, b);
			double ra[6], rb[6], S[kLmTerms], Xh[3] = {0.0, 0.0, 0.0};
#pragma unroll
			for (int k = 0; k < 6; ++k)
			{
				ra[k] = rays[a][k];
				rb[k] = rays[b][k];
			}
			lm_pair_sums(ra, rb, S);
			(void)lm_solve(S, cref, Xh);
			lm_inlier_sums<W>(lane, m, base, obsPose, poses, obsF, rays, Xh, prm.threshold, S);
			const bool havePoint = lm_solve(S, cref, X);
			parallax = lm_parallax(S, static_cast<double>(bestCount));
			if (!havePoint || !(parallax >= prm.minParallax))
			{
				status = 4;
			}
		}
	}
	if (status == 0)
	{
		// L5's re-selection (L7: the selection) under X
		int haveMax = 0;
		for (int o = lane; o < m; o += W)
		{
			const double sc = lm_score(poses + kLmPoseDoubles * static_cast<size_t>(obsPose[base + o]), obsF + 3 * (base + o), X);
			const bool in = sc < prm.threshold;
			nIn += in ? 1 : 0;
			if (lm_finite(sc) && (!haveMax || sc > scoreMax))
			{
				scoreMax = sc;
				haveMax = 1;
			}
			if (scores)
			{
				scores[base + o] = sc;
			}
			if (flags)
			{
				flags[base + o] = in ? 1 : 0;
			}
		}
		nIn = lm_sum_int<W>(nIn);
#pragma unroll
		for (int s = W / 2; s > 0; s /= 2)
		{
			const int oh = __shfl_xor(haveMax, s, W);
			const double ov = __shfl_xor(scoreMax, s, W);
			if (oh && (!haveMax || ov > scoreMax))
			{
				scoreMax = ov;
				haveMax = 1;
			}
		}
		scoreMax = haveMax ? scoreMax : 0.0;
		scored = true;
		if (!SOLVE)
		{
			// L7: the parallax of the inliers' rays
			double S[kLmTerms];
			lm_inlier_sums<W>(lane, m, base, obsPose, poses, obsF, rays, X, prm.threshold, S);
			parallax = nIn > 0 ? lm_parallax(S, static_cast<double>(nIn)) : 0.0;
			if (!(parallax >= prm.minParallax))
			{
				status = 4;
			}
		}
		if (status == 0 && nIn < prm.minInliers)
		{
			status = 5;
		}
	}
	if (!scored)
	{
		for (int o = lane; o < m; o += W)
		{
			if (scores)
			{
				scores[base + o] = 0.0;
			}
			if (flags)
			{
				flags[base + o] = 0;
			}
		}
	}
	if (lane == 0)
	{
		ebo_landmark_result* out = results + l;
#pragma unroll
		for (int i = 0; i < 3; ++i)
		{
			out->point[i] = status == 0 ? X[i] : 0.0;
		}
		out->parallax = parallax;
		out->score_max = scoreMax;
		out->status = status;
		out->n_obs = live ? offsets[l + 1] - offsets[l] : 0;
		out->n_inliers = nIn;
		out->winner = winner;
		out->hypotheses = H;
		out->reserved = 0;
	}
}

#endif  // EBO_LANDMARK_RULES_ONLY
