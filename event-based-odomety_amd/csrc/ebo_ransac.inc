// ebo_ransac.inc — what the two RANSAC paths (two-view geometry, absolute pose) share on the device: the counter-based
// sampler and the three kernels around a hypothesis (inlier counts, the winners' inlier flags, per-point scores).
// Included by ebo_twoview.inc between its rules and its kernels.  What a hypothesis IS stays with each path
// (k_tv_hypotheses, k_ap_hypotheses); a problem type P tells the kernels here the rest:
//   P::kSample                   points a hypothesis draws: a group with fewer has no hypothesis
//   P::score(T, a, b)            the score of one point (a, b: its entries of the path's two [n][3] arrays) under pose T
// TvProblem is at the head of ebo_twoview.inc's kernels, ApProblem of ebo_abspose.inc's.  A "group" is what one RANSAC
// runs over: a keyframe pair's correspondences, or a frame's (bearing vector, landmark) pairs.

// rule 3 / A2: K distinct indices of [0, n) from (seed, group, h), a partial Fisher-Yates shuffle kept as K records
template <int K>
__device__ __forceinline__ void ransac_sample(unsigned long long seed, int group, int h, int n, int (&out)[K])
{
	const unsigned long long G = 0x9E3779B97F4A7C15ull;
	unsigned long long x = tv_mix(seed + G);
	x = tv_mix((x ^ static_cast<unsigned long long>(group)) + G);
	x = tv_mix((x ^ static_cast<unsigned long long>(h)) + G);
	int pos[K], val[K];
#pragma unroll
	for (int d = 0; d < K; ++d)
	{
		const unsigned long long r = tv_mix((x ^ static_cast<unsigned long long>(d)) + G);
		const int j = d + static_cast<int>(static_cast<unsigned int>(r >> 32) % static_cast<unsigned int>(n - d));
		int vj = j, vd = d;
#pragma unroll
		for (int e = 0; e < K; ++e)
		{
			if (e < d)  // later records override earlier ones
			{
				vj = (pos[e] == j) ? val[e] : vj;
				vd = (pos[e] == d) ? val[e] : vd;
			}
		}
		out[d] = vj;
		pos[d] = j;
		val[d] = vd;
	}
}

#ifndef EBO_TWOVIEW_RULES_ONLY  // the host tools compile the rules above and stop here

constexpr int kRansacTile = 1024;     // points of a group staged in LDS at a time (48 KB)
constexpr int kRansacHypChunk = 8;    // hypotheses scored per workgroup of the counting kernel

// a [3][4] model that travels as a kernel argument
struct TvModelArg
{
	double m[12];
};

__device__ __forceinline__ TvPoseRT tv_pose_of(const TvModelArg& a)
{
	TvPoseRT T;
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
#pragma unroll
		for (int j = 0; j < 3; ++j)
		{
			T.R[i][j] = a.m[4 * i + j];
		}
		T.t[i] = a.m[4 * i + 3];
	}
	return T;
}

// Counting kernel: unit of work = (group, hypothesis, point).  A workgroup stages one tile of one group's two arrays
// in LDS and scores it against kRansacHypChunk hypotheses, one wave per hypothesis at a time; a wave counts its
// inliers with ballots and adds the integer to counts[] (zeroed before the launch): exact and order-free.
// grid = (ceil(H / kRansacHypChunk), groups, tiles of the largest group)
template <class P>
__global__ void __launch_bounds__(256) k_ransac_count(int H, const int* __restrict__ offsets, const double* __restrict__ a,
													  const double* __restrict__ b, const double* __restrict__ models,
													  const int* __restrict__ valid, double threshold, int* __restrict__ counts)
{
	__shared__ double sa[3 * kRansacTile];
	__shared__ double sb[3 * kRansacTile];
	const int group = blockIdx.y;
	const long long base = offsets[group];
	const int n = offsets[group + 1] - offsets[group];
	const int t0 = blockIdx.z * kRansacTile;
	if (n < P::kSample || t0 >= n)
	{
		return;  // the whole workgroup leaves together
	}
	const int nt = min(kRansacTile, n - t0);
	for (int e = threadIdx.x; e < 3 * nt; e += 256)
	{
		sa[e] = a[3 * (base + t0) + e];
		sb[e] = b[3 * (base + t0) + e];
	}
	__syncthreads();
	const int wave = threadIdx.x / 64, lane = threadIdx.x % 64;
	for (int hh = wave; hh < kRansacHypChunk; hh += 4)
	{
		const int h = blockIdx.x * kRansacHypChunk + hh;
		if (h >= H)
		{
			break;
		}
		const long long g = static_cast<long long>(group) * H + h;
		if (!valid[g])
		{
			continue;
		}
		const TvPoseRT T = tv_load_pose(models + 12 * g);
		int cnt = 0;
		for (int i0 = 0; i0 < nt; i0 += 64)
		{
			const int i = i0 + lane;
			bool in = false;
			if (i < nt)
			{
				const double pa[3] = {sa[3 * i], sa[3 * i + 1], sa[3 * i + 2]};
				const double pb[3] = {sb[3 * i], sb[3 * i + 1], sb[3 * i + 2]};
				in = P::score(T, pa, pb) < threshold;
			}
			cnt += __popcll(__ballot(in));
		}
		if (lane == 0 && cnt)
		{
			atomicAdd(counts + g, cnt);
		}
	}
}

// one lane per point: score and inlier flag for a given model (either output may be null)
template <class P>
__global__ void __launch_bounds__(256) k_ransac_scores(TvModelArg model, int n, const double* __restrict__ a,
													   const double* __restrict__ b, double threshold,
													   double* __restrict__ scores, unsigned char* __restrict__ flags)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
	{
		return;
	}
	const TvPoseRT T = tv_pose_of(model);
	const size_t o = 3 * static_cast<size_t>(i);
	const double pa[3] = {a[o], a[o + 1], a[o + 2]};
	const double pb[3] = {b[o], b[o + 1], b[o + 2]};
	const double s = P::score(T, pa, pb);
	if (scores)
	{
		scores[i] = s;
	}
	if (flags)
	{
		flags[i] = s < threshold ? 1 : 0;
	}
}

// the winners' inlier flags, all groups in one launch: grid = (ceil(largest group / 256), groups).  winner[group] < 0
// (no hypothesis: fewer than P::kSample points) clears the group's flags.  Lane 0 of a group's first workgroup copies
// the winner's model to winModels[group][12] (zeros when there is none).
template <class P>
__global__ void __launch_bounds__(256) k_ransac_winner_flags(int H, const int* __restrict__ offsets, const double* __restrict__ a,
															 const double* __restrict__ b, const double* __restrict__ models,
															 const int* __restrict__ valid, const int* __restrict__ winner,
															 double threshold, unsigned char* __restrict__ flags,
															 double* __restrict__ winModels)
{
	const int group = blockIdx.y;
	const long long base = offsets[group];
	const int n = offsets[group + 1] - offsets[group];
	const int w = winner[group];
	const long long g = static_cast<long long>(group) * H + (w < 0 ? 0 : w);
	const bool have = w >= 0 && w < H && valid[g] != 0;
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i == 0)
	{
		for (int e = 0; e < 12; ++e)
		{
			winModels[12 * group + e] = have ? models[12 * g + e] : 0.0;
		}
	}
	if (i >= n)
	{
		return;
	}
	unsigned char f = 0;
	if (have)
	{
		const TvPoseRT T = tv_load_pose(models + 12 * g);
		const size_t o = 3 * static_cast<size_t>(base + i);
		const double pa[3] = {a[o], a[o + 1], a[o + 2]};
		const double pb[3] = {b[o], b[o + 1], b[o + 2]};
		f = P::score(T, pa, pb) < threshold ? 1 : 0;
	}
	flags[base + i] = f;
}

#endif  // EBO_TWOVIEW_RULES_ONLY
