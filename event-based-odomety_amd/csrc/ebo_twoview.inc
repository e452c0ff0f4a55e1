// ebo_twoview.inc — two-view geometry on the device: eight-point RANSAC hypotheses and the per-point closed forms
// (the score, midpoint triangulation, the epipolar test); the kernels that count and list a hypothesis's inliers are
// ebo_ransac.inc's, shared with absolute pose.  Replaces what the reference does serially in
// VisualOdometryFrontEnd::findInliersRansac (visual_odometry.cpp:288-341) and triangulation.cpp:7-63.  Included
// inside ebo_kernels.hip's anonymous namespace, after ebo_camera.inc.  The rules
// are written out in include/ebo.h ("two-view geometry"); tests/twoview_ref.py restates them in numpy.  Every float64
// operation is rounded on its own (__dadd_rn / __dsub_rn / __dmul_rn / __ddiv_rn / __dsqrt_rn).

constexpr int kTvLanes = 16;          // lanes that share one hypothesis
constexpr int kTvGroups = 16;         // hypotheses per 256-lane workgroup
constexpr int kTvStride = 81 + 72 + 24 + 24;  // doubles of LDS per hypothesis: V, A (later the sample scores), f1, f2
constexpr int kTvSweeps9 = 10;
constexpr int kTvSweeps3 = 8;

__device__ __forceinline__ double tv_dot3(double a0, double a1, double a2, double b0, double b1, double b2)
{
	return __dadd_rn(__dadd_rn(__dmul_rn(a0, b0), __dmul_rn(a1, b1)), __dmul_rn(a2, b2));
}

struct TvPoseRT
{
	double R[3][3];
	double t[3];
};

__device__ __forceinline__ TvPoseRT tv_load_pose(const double* __restrict__ m)
{
	TvPoseRT T;
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
#pragma unroll
		for (int j = 0; j < 3; ++j)
		{
			T.R[i][j] = m[4 * i + j];
		}
		T.t[i] = m[4 * i + 3];
	}
	return T;
}

// rule 1: midpoint triangulation, p in camera-1 coordinates
__device__ __forceinline__ void tv_triangulate2(const TvPoseRT& T, const double (&f1)[3], const double (&f2)[3], double (&p)[3])
{
	double g[3];
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		g[i] = tv_dot3(T.R[i][0], T.R[i][1], T.R[i][2], f2[0], f2[1], f2[2]);
	}
	const double b0 = tv_dot3(T.t[0], T.t[1], T.t[2], f1[0], f1[1], f1[2]);
	const double b1 = tv_dot3(T.t[0], T.t[1], T.t[2], g[0], g[1], g[2]);
	const double a00 = tv_dot3(f1[0], f1[1], f1[2], f1[0], f1[1], f1[2]);
	const double fg = tv_dot3(f1[0], f1[1], f1[2], g[0], g[1], g[2]);
	const double a01 = -fg, a10 = fg;
	const double a11 = -tv_dot3(g[0], g[1], g[2], g[0], g[1], g[2]);
	const double det = __dsub_rn(__dmul_rn(a00, a11), __dmul_rn(a01, a10));
	const double l0 = __ddiv_rn(__dsub_rn(__dmul_rn(a11, b0), __dmul_rn(a01, b1)), det);
	const double l1 = __ddiv_rn(__dsub_rn(__dmul_rn(a00, b1), __dmul_rn(a10, b0)), det);
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		const double x = __dmul_rn(l0, f1[i]);
		const double z = __dadd_rn(T.t[i], __dmul_rn(l1, g[i]));
		p[i] = __ddiv_rn(__dadd_rn(x, z), 2.0);
	}
}

// rule 2: the bearing-vector reprojection score
__device__ __forceinline__ double tv_score(const TvPoseRT& T, const double (&f1)[3], const double (&f2)[3])
{
	double p[3];
	tv_triangulate2(T, f1, f2, p);
	const double n1 = __dsqrt_rn(tv_dot3(p[0], p[1], p[2], p[0], p[1], p[2]));
	const double r10 = __ddiv_rn(p[0], n1), r11 = __ddiv_rn(p[1], n1), r12 = __ddiv_rn(p[2], n1);
	const double d0 = __dsub_rn(p[0], T.t[0]), d1 = __dsub_rn(p[1], T.t[1]), d2 = __dsub_rn(p[2], T.t[2]);
	double q[3];
#pragma unroll
	for (int j = 0; j < 3; ++j)
	{
		q[j] = tv_dot3(T.R[0][j], T.R[1][j], T.R[2][j], d0, d1, d2);
	}
	const double n2 = __dsqrt_rn(tv_dot3(q[0], q[1], q[2], q[0], q[1], q[2]));
	const double r20 = __ddiv_rn(q[0], n2), r21 = __ddiv_rn(q[1], n2), r22 = __ddiv_rn(q[2], n2);
	const double s1 = __dsub_rn(1.0, tv_dot3(f1[0], f1[1], f1[2], r10, r11, r12));
	const double s2 = __dsub_rn(1.0, tv_dot3(f2[0], f2[1], f2[2], r20, r21, r22));
	return __dadd_rn(s1, s2);
}

// rule 3: splitmix64's finaliser; the counter-based sampler built on it is ransac_sample<8> (ebo_ransac.inc)
__device__ __forceinline__ unsigned long long tv_mix(unsigned long long z)
{
	z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
	z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
	return z ^ (z >> 31);
}

// the rotation of rule 4 from (app, aqq, apq != 0): t, c, s
__device__ __forceinline__ void tv_rotation(double app, double aqq, double apq, double& t, double& c, double& s)
{
	const double th = __ddiv_rn(__dsub_rn(aqq, app), __dmul_rn(2.0, apq));
	const double den = __dadd_rn(fabs(th), __dsqrt_rn(__dadd_rn(__dmul_rn(th, th), 1.0)));
	t = __ddiv_rn(th < 0.0 ? -1.0 : 1.0, den);
	c = __ddiv_rn(1.0, __dsqrt_rn(__dadd_rn(__dmul_rn(t, t), 1.0)));
	s = __dmul_rn(t, c);
}

// one rotation of the 3 x 3 Jacobi iteration, in registers (P, Q are compile-time, so every index is)
template <int P, int Q>
__device__ __forceinline__ void tv_rot3(double (&M)[3][3], double (&V)[3][3])
{
	const double apq = M[P][Q];
	if (apq != 0.0)
	{
		const double app = M[P][P], aqq = M[Q][Q];
		double t, c, s;
		tv_rotation(app, aqq, apq, t, c, s);
		constexpr int K = 3 - P - Q;
		const double mkp = __dsub_rn(__dmul_rn(c, M[K][P]), __dmul_rn(s, M[K][Q]));
		const double mkq = __dadd_rn(__dmul_rn(s, M[K][P]), __dmul_rn(c, M[K][Q]));
		M[K][P] = M[P][K] = mkp;
		M[K][Q] = M[Q][K] = mkq;
		const double tapq = __dmul_rn(t, apq);
		M[P][P] = __dsub_rn(app, tapq);
		M[Q][Q] = __dadd_rn(aqq, tapq);
		M[P][Q] = M[Q][P] = 0.0;
#pragma unroll
		for (int k = 0; k < 3; ++k)
		{
			const double vkp = __dsub_rn(__dmul_rn(c, V[k][P]), __dmul_rn(s, V[k][Q]));
			const double vkq = __dadd_rn(__dmul_rn(s, V[k][P]), __dmul_rn(c, V[k][Q]));
			V[k][P] = vkp;
			V[k][Q] = vkq;
		}
	}
}

__device__ __forceinline__ double tv_det3(const double (&R)[3][3])
{
	const double a = __dsub_rn(__dmul_rn(R[1][1], R[2][2]), __dmul_rn(R[1][2], R[2][1]));
	const double b = __dsub_rn(__dmul_rn(R[1][0], R[2][2]), __dmul_rn(R[1][2], R[2][0]));
	const double c = __dsub_rn(__dmul_rn(R[1][0], R[2][1]), __dmul_rn(R[1][1], R[2][0]));
	return __dadd_rn(__dsub_rn(__dmul_rn(R[0][0], a), __dmul_rn(R[0][1], b)), __dmul_rn(R[0][2], c));
}

__device__ __forceinline__ void tv_cross(const double (&a)[3], const double (&b)[3], double (&o)[3])
{
	o[0] = __dsub_rn(__dmul_rn(a[1], b[2]), __dmul_rn(a[2], b[1]));
	o[1] = __dsub_rn(__dmul_rn(a[2], b[0]), __dmul_rn(a[0], b[2]));
	o[2] = __dsub_rn(__dmul_rn(a[0], b[1]), __dmul_rn(a[1], b[0]));
}

#include "ebo_ransac.inc"  // rule 3's sampler, and (kernels only) the counting, score and winner kernels

#ifndef EBO_TWOVIEW_RULES_ONLY  // tools/two_view_serial.cpp compiles the rules above for the host and stops here

// what ebo_ransac.inc's kernels need to know of this path
struct TvProblem
{
	static constexpr int kSample = 8;
	static __device__ __forceinline__ double score(const TvPoseRT& T, const double (&f1)[3], const double (&f2)[3])
	{
		return tv_score(T, f1, f2);
	}
};

// Hypothesis kernel: one 16-lane group per (pair, hypothesis).  The 8 x 9 matrix A and the 9 x 9 matrix V of its
// one-sided Jacobi iteration live in LDS; lane k of the group owns row k of both in every rotation (the element
// updates of one rotation are independent, so the bits do not depend on how lanes share them); every lane repeats
// the scalar part (column products, rotation angle, the 3 x 3 SVD, the candidates), which keeps the group in step
// without broadcasts.  Lanes 0-7 score one sample point each.  Loop counts are fixed, so every __syncthreads is reached by the whole workgroup.
// models: [nPairs * H][3][4], all zero where valid[] is 0;  samplesOut: [nPairs * H][8] or null.
__global__ void __launch_bounds__(256) k_tv_hypotheses(int nPairs, int H, const int* __restrict__ offsets,
													   const double* __restrict__ f1, const double* __restrict__ f2,
													   unsigned long long seed, double* __restrict__ models,
													   int* __restrict__ valid, int* __restrict__ samplesOut)
{
	__shared__ double lds[kTvGroups * kTvStride];
	const int grp = threadIdx.x / kTvLanes, l = threadIdx.x % kTvLanes;
	const long long g = static_cast<long long>(blockIdx.x) * kTvGroups + grp;
	const bool exists = g < static_cast<long long>(nPairs) * H;
	int pair = 0, h = 0, n = 0;
	long long base = 0;
	if (exists)
	{
		pair = static_cast<int>(g / H);
		h = static_cast<int>(g % H);
		base = offsets[pair];
		n = offsets[pair + 1] - offsets[pair];
	}
	const bool live = n >= 8;
	double* V = lds + grp * kTvStride;
	double* A = V + 81;
	double* S1 = A + 72;
	double* S2 = S1 + 24;

	int smp[8] = {0, 0, 0, 0, 0, 0, 0, 0};
	if (live)
	{
		ransac_sample<8>(seed, pair, h, n, smp);
	}
	if (l < 8)
	{
		int mine = 0;
#pragma unroll
		for (int d = 0; d < 8; ++d)
		{
			mine = (d == l) ? smp[d] : mine;
		}
#pragma unroll
		for (int k = 0; k < 3; ++k)
		{
			S1[3 * l + k] = live ? f1[3 * (base + mine) + k] : 0.0;
			S2[3 * l + k] = live ? f2[3 * (base + mine) + k] : 0.0;
		}
		if (live && samplesOut)
		{
			samplesOut[8 * g + l] = mine;
		}
	}
	__syncthreads();
	// A: row i = (f2x * f1, f2y * f1, f2z * f1)
	for (int e = l; e < 72; e += kTvLanes)
	{
		const int i = e / 9, j = e % 9;
		A[e] = __dmul_rn(S2[3 * i + j / 3], S1[3 * i + j % 3]);
	}
	if (l < 9)
	{
		for (int j = 0; j < 9; ++j)
		{
			V[9 * l + j] = (l == j) ? 1.0 : 0.0;
		}
	}
	__syncthreads();
	// one-sided Jacobi on the columns of A: every lane forms the three column products of the rotation, lane k
	// rotates row k of A (k < 8) and of V (k < 9)
	const int k = l < 9 ? l : 0;
	const int ka = l < 8 ? l : 0;
	for (int sweep = 0; sweep < kTvSweeps9; ++sweep)
	{
		for (int p = 0; p < 8; ++p)
		{
			for (int q = p + 1; q < 9; ++q)
			{
				double app = __dmul_rn(A[p], A[p]), aqq = __dmul_rn(A[q], A[q]), apq = __dmul_rn(A[p], A[q]);
#pragma unroll
				for (int i = 1; i < 8; ++i)
				{
					const double x = A[9 * i + p], y = A[9 * i + q];
					app = __dadd_rn(app, __dmul_rn(x, x));
					aqq = __dadd_rn(aqq, __dmul_rn(y, y));
					apq = __dadd_rn(apq, __dmul_rn(x, y));
				}
				const double akp = A[9 * ka + p], akq = A[9 * ka + q], vkp = V[9 * k + p], vkq = V[9 * k + q];
				__syncthreads();
				if (apq != 0.0 && l < 9)
				{
					double t, c, s;
					tv_rotation(app, aqq, apq, t, c, s);
					if (l < 8)
					{
						A[9 * ka + p] = __dsub_rn(__dmul_rn(c, akp), __dmul_rn(s, akq));
						A[9 * ka + q] = __dadd_rn(__dmul_rn(s, akp), __dmul_rn(c, akq));
					}
					V[9 * k + p] = __dsub_rn(__dmul_rn(c, vkp), __dmul_rn(s, vkq));
					V[9 * k + q] = __dadd_rn(__dmul_rn(s, vkp), __dmul_rn(c, vkq));
				}
				__syncthreads();
			}
		}
	}
	// the column of V whose rotated column of A is the shortest (the first of equals): the eigenvector of A^T A for
	// its smallest eigenvalue; F[b][a] = e[3a + b], so that f1^T F f2 = 0
	int jmin = 0;
	double dmin = 0.0;
	for (int j = 0; j < 9; ++j)
	{
		double dj = __dmul_rn(A[j], A[j]);
		for (int i = 1; i < 8; ++i)
		{
			dj = __dadd_rn(dj, __dmul_rn(A[9 * i + j], A[9 * i + j]));
		}
		if (j == 0 || dj < dmin)
		{
			dmin = dj;
			jmin = j;
		}
	}
	__syncthreads();  // A is dead from here on: the sample scores go there
	double F[3][3];
#pragma unroll
	for (int a = 0; a < 3; ++a)
	{
#pragma unroll
		for (int b = 0; b < 3; ++b)
		{
			F[b][a] = V[9 * (3 * a + b) + jmin];
		}
	}
	// 3 x 3 SVD: Jacobi on F^T F gives V and the squared singular values
	double G3[3][3], V3[3][3];
#pragma unroll
	for (int j = 0; j < 3; ++j)
	{
#pragma unroll
		for (int c = 0; c < 3; ++c)
		{
			G3[j][c] = tv_dot3(F[0][j], F[1][j], F[2][j], F[0][c], F[1][c], F[2][c]);
			V3[j][c] = (j == c) ? 1.0 : 0.0;
		}
	}
	for (int sweep = 0; sweep < kTvSweeps3; ++sweep)
	{
		tv_rot3<0, 1>(G3, V3);
		tv_rot3<0, 2>(G3, V3);
		tv_rot3<1, 2>(G3, V3);
	}
	double dd[3] = {G3[0][0], G3[1][1], G3[2][2]};
	double vc[3][3];  // vc[c] = column c of V3
#pragma unroll
	for (int c = 0; c < 3; ++c)
	{
#pragma unroll
		for (int r = 0; r < 3; ++r)
		{
			vc[c][r] = V3[r][c];
		}
	}
	// stable descending order: compare-exchange (0,1) (1,2) (0,1), swapping only when strictly smaller
#define TV_CSWAP(a, b)                                \
	{                                                 \
		const bool sw = dd[a] < dd[b];                \
		const double da = dd[a], db = dd[b];          \
		dd[a] = sw ? db : da;                         \
		dd[b] = sw ? da : db;                         \
		_Pragma("unroll") for (int r = 0; r < 3; ++r) \
		{                                             \
			const double xa = vc[a][r], xb = vc[b][r]; \
			vc[a][r] = sw ? xb : xa;                  \
			vc[b][r] = sw ? xa : xb;                  \
		}                                             \
	}
	TV_CSWAP(0, 1)
	TV_CSWAP(1, 2)
	TV_CSWAP(0, 1)
#undef TV_CSWAP
	const double s0 = __dsqrt_rn(dd[0]), s1 = __dsqrt_rn(dd[1]);
	const bool okSv = (s0 > 0.0) && (s1 > 0.0);
	double u0[3], u1[3], u2[3], v2[3];
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		u0[i] = __ddiv_rn(tv_dot3(F[i][0], F[i][1], F[i][2], vc[0][0], vc[0][1], vc[0][2]), s0);
		u1[i] = __ddiv_rn(tv_dot3(F[i][0], F[i][1], F[i][2], vc[1][0], vc[1][1], vc[1][2]), s1);
	}
	const double n0 = __dsqrt_rn(tv_dot3(u0[0], u0[1], u0[2], u0[0], u0[1], u0[2]));
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		u0[i] = __ddiv_rn(u0[i], n0);
	}
	const double hh = tv_dot3(u0[0], u0[1], u0[2], u1[0], u1[1], u1[2]);
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		u1[i] = __dsub_rn(u1[i], __dmul_rn(hh, u0[i]));
	}
	const double n1 = __dsqrt_rn(tv_dot3(u1[0], u1[1], u1[2], u1[0], u1[1], u1[2]));
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		u1[i] = __ddiv_rn(u1[i], n1);
	}
	tv_cross(u0, u1, u2);
	tv_cross(vc[0], vc[1], v2);
	// rule 5: Ra = U W V^T, Rb = U W^T V^T, entry by entry; negated when the determinant is negative
	TvPoseRT Ca, Cb;
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
#pragma unroll
		for (int j = 0; j < 3; ++j)
		{
			const double a = __dmul_rn(u1[i], vc[0][j]);
			const double b = __dmul_rn(u0[i], vc[1][j]);
			const double c = __dmul_rn(u2[i], v2[j]);
			Ca.R[i][j] = __dadd_rn(__dsub_rn(a, b), c);
			Cb.R[i][j] = __dadd_rn(__dsub_rn(b, a), c);
		}
		Ca.t[i] = u2[i];
		Cb.t[i] = u2[i];
	}
	const bool negA = tv_det3(Ca.R) < 0.0, negB = tv_det3(Cb.R) < 0.0;
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
#pragma unroll
		for (int j = 0; j < 3; ++j)
		{
			Ca.R[i][j] = negA ? -Ca.R[i][j] : Ca.R[i][j];
			Cb.R[i][j] = negB ? -Cb.R[i][j] : Cb.R[i][j];
		}
	}
	// the four candidates (Ra,+) (Ra,-) (Rb,+) (Rb,-) scored on the 8 sample points: lane i < 8 scores point i.
	// The scores go where A was.
	double* SC = A;
	if (l < 8)
	{
		const double a1[3] = {S1[3 * l], S1[3 * l + 1], S1[3 * l + 2]};
		const double a2[3] = {S2[3 * l], S2[3 * l + 1], S2[3 * l + 2]};
		TvPoseRT T = Ca;
		SC[l] = tv_score(T, a1, a2);
		T.t[0] = -u2[0], T.t[1] = -u2[1], T.t[2] = -u2[2];
		SC[8 + l] = tv_score(T, a1, a2);
		T = Cb;
		SC[16 + l] = tv_score(T, a1, a2);
		T.t[0] = -u2[0], T.t[1] = -u2[1], T.t[2] = -u2[2];
		SC[24 + l] = tv_score(T, a1, a2);
	}
	__syncthreads();
	if (l == 0 && exists)
	{
		double best = __builtin_inf();
		int bc = -1;
#pragma unroll
		for (int c = 0; c < 4; ++c)
		{
			double tot = SC[8 * c];
			for (int i = 1; i < 8; ++i)
			{
				tot = __dadd_rn(tot, SC[8 * c + i]);
			}
			if (isfinite(tot) && tot < best)
			{
				best = tot;
				bc = c;
			}
		}
		const bool ok = live && okSv && bc >= 0;
		const bool useB = bc >= 2;
		const bool minus = (bc & 1) != 0;
		double* o = models + 12 * g;
#pragma unroll
		for (int i = 0; i < 3; ++i)
		{
#pragma unroll
			for (int j = 0; j < 3; ++j)
			{
				o[4 * i + j] = ok ? (useB ? Cb.R[i][j] : Ca.R[i][j]) : 0.0;
			}
			o[4 * i + 3] = ok ? (minus ? -u2[i] : u2[i]) : 0.0;
		}
		valid[g] = ok ? 1 : 0;
	}
}

// one lane per correspondence, a pose pair per point: world point = pose1 * triangulate2(pose1^-1 * pose2, f1, f2)
// with inverse(R, t) = (R^T, -(R^T t)) and (Ra, ta)(Rb, tb) = (Ra Rb, Ra tb + ta).  A pose index outside
// [0, nPoses) gives a NaN point, never a read out of bounds.
__global__ void __launch_bounds__(256) k_tv_triangulate(int nPoses, const double* __restrict__ poses, int n,
														const int* __restrict__ posePair, const double* __restrict__ f1,
														const double* __restrict__ f2, double* __restrict__ points)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
	{
		return;
	}
	const size_t o = 3 * static_cast<size_t>(i);
	const int i1 = posePair[2 * static_cast<size_t>(i)], i2 = posePair[2 * static_cast<size_t>(i) + 1];
	if (i1 < 0 || i1 >= nPoses || i2 < 0 || i2 >= nPoses)
	{
		points[o] = points[o + 1] = points[o + 2] = __builtin_nan("");
		return;
	}
	const TvPoseRT P1 = tv_load_pose(poses + 12 * static_cast<size_t>(i1));
	const TvPoseRT P2 = tv_load_pose(poses + 12 * static_cast<size_t>(i2));
	TvPoseRT T;  // pose1^-1 * pose2
#pragma unroll
	for (int r = 0; r < 3; ++r)
	{
		const double it = -tv_dot3(P1.R[0][r], P1.R[1][r], P1.R[2][r], P1.t[0], P1.t[1], P1.t[2]);
#pragma unroll
		for (int c = 0; c < 3; ++c)
		{
			T.R[r][c] = tv_dot3(P1.R[0][r], P1.R[1][r], P1.R[2][r], P2.R[0][c], P2.R[1][c], P2.R[2][c]);
		}
		T.t[r] = __dadd_rn(tv_dot3(P1.R[0][r], P1.R[1][r], P1.R[2][r], P2.t[0], P2.t[1], P2.t[2]), it);
	}
	const double a1[3] = {f1[o], f1[o + 1], f1[o + 2]};
	const double a2[3] = {f2[o], f2[o + 1], f2[o + 2]};
	double p[3];
	tv_triangulate2(T, a1, a2, p);
#pragma unroll
	for (int r = 0; r < 3; ++r)
	{
		points[o + r] = __dadd_rn(tv_dot3(P1.R[r][0], P1.R[r][1], P1.R[r][2], p[0], p[1], p[2]), P1.t[r]);
	}
}

// rule 7: E = hat(t / |t|) R, flag = |f1^T E f2| < threshold
__global__ void __launch_bounds__(256) k_tv_epipolar(TvModelArg model, int n, const double* __restrict__ f1,
													 const double* __restrict__ f2, double threshold,
													 unsigned char* __restrict__ flags)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
	{
		return;
	}
	const TvPoseRT T = tv_pose_of(model);
	const double nt = __dsqrt_rn(tv_dot3(T.t[0], T.t[1], T.t[2], T.t[0], T.t[1], T.t[2]));
	const double tx = __ddiv_rn(T.t[0], nt), ty = __ddiv_rn(T.t[1], nt), tz = __ddiv_rn(T.t[2], nt);
	const size_t o = 3 * static_cast<size_t>(i);
	double E[3][3];
#pragma unroll
	for (int j = 0; j < 3; ++j)
	{
		E[0][j] = __dsub_rn(__dmul_rn(ty, T.R[2][j]), __dmul_rn(tz, T.R[1][j]));
		E[1][j] = __dsub_rn(__dmul_rn(tz, T.R[0][j]), __dmul_rn(tx, T.R[2][j]));
		E[2][j] = __dsub_rn(__dmul_rn(tx, T.R[1][j]), __dmul_rn(ty, T.R[0][j]));
	}
	const double w0 = tv_dot3(E[0][0], E[0][1], E[0][2], f2[o], f2[o + 1], f2[o + 2]);
	const double w1 = tv_dot3(E[1][0], E[1][1], E[1][2], f2[o], f2[o + 1], f2[o + 2]);
	const double w2 = tv_dot3(E[2][0], E[2][1], E[2][2], f2[o], f2[o + 1], f2[o + 2]);
	const double v = tv_dot3(f1[o], f1[o + 1], f1[o + 2], w0, w1, w2);
	flags[i] = fabs(v) < threshold ? 1 : 0;
}

#endif  // EBO_TWOVIEW_RULES_ONLY
