// ebo_abspose.inc — absolute pose on the device: three-point RANSAC hypotheses over (bearing vector, landmark) pairs
// and the per-point score for a given pose; the kernels that count and list a hypothesis's inliers are
// ebo_ransac.inc's.  Replaces what the reference does serially through OpenGV in
// VisualOdometryFrontEnd::localizeCamera (visual_odometry.cpp:212-286).  Included inside ebo_kernels.hip's anonymous
// namespace, after ebo_twoview.inc, whose dot, cross, mix, rotation and 3 x 3 Jacobi rotation it reuses (and through
// which ebo_ransac.inc comes in).
// The rules are written out in include/ebo.h ("absolute pose", A1-A5); tests/abspose_ref.py restates them in numpy.
// Every float64 operation is rounded on its own (__dadd_rn / __dsub_rn / __dmul_rn / __ddiv_rn / __dsqrt_rn).

constexpr int kApNewton = 32;        // Newton steps on the cubic (A3)
constexpr int kApPolish = 3;         // Gauss-Newton steps on the three distance equations (A3)
constexpr int kApSweeps = 8;         // jacobi(D0, 8)
constexpr int kApBlock = 64;         // hypotheses per workgroup of the hypothesis kernel: one lane each

// A1: the bearing-vector reprojection score of one (bearing, landmark) pair under a camera-to-world pose
__device__ __forceinline__ double ap_score(const TvPoseRT& T, const double (&f)[3], const double (&p)[3])
{
	const double d0 = __dsub_rn(p[0], T.t[0]), d1 = __dsub_rn(p[1], T.t[1]), d2 = __dsub_rn(p[2], T.t[2]);
	double q[3];
#pragma unroll
	for (int j = 0; j < 3; ++j)
	{
		q[j] = tv_dot3(T.R[0][j], T.R[1][j], T.R[2][j], d0, d1, d2);
	}
	const double n = __dsqrt_rn(tv_dot3(q[0], q[1], q[2], q[0], q[1], q[2]));
	const double r0 = __ddiv_rn(q[0], n), r1 = __ddiv_rn(q[1], n), r2 = __ddiv_rn(q[2], n);
	return __dsub_rn(1.0, tv_dot3(f[0], f[1], f[2], r0, r1, r2));
}

// A2: rule 3 with four draws is ransac_sample<4> (ebo_ransac.inc)

// cofactors with cyclic indices, C[i][j] = M[i+1][j+1] * M[i+2][j+2] - M[i+1][j+2] * M[i+2][j+1]; returns dot(M[0], C[0])
__device__ __forceinline__ double ap_cof(const double (&M)[3][3], double (&C)[3][3])
{
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
#pragma unroll
		for (int j = 0; j < 3; ++j)
		{
			C[i][j] = __dsub_rn(__dmul_rn(M[(i + 1) % 3][(j + 1) % 3], M[(i + 2) % 3][(j + 2) % 3]),
								__dmul_rn(M[(i + 1) % 3][(j + 2) % 3], M[(i + 2) % 3][(j + 1) % 3]));
		}
	}
	return tv_dot3(M[0][0], M[0][1], M[0][2], C[0][0], C[0][1], C[0][2]);
}

__device__ __forceinline__ double ap_rows_dot(const double (&A)[3][3], const double (&B)[3][3])
{
	const double r0 = tv_dot3(A[0][0], A[0][1], A[0][2], B[0][0], B[0][1], B[0][2]);
	const double r1 = tv_dot3(A[1][0], A[1][1], A[1][2], B[1][0], B[1][1], B[1][2]);
	const double r2 = tv_dot3(A[2][0], A[2][1], A[2][2], B[2][0], B[2][1], B[2][2]);
	return __dadd_rn(__dadd_rn(r0, r1), r2);
}

__device__ __forceinline__ double ap_cubic(double r, double b, double c, double d)
{
	return __dadd_rn(__dmul_rn(__dadd_rn(__dmul_rn(__dadd_rn(r, b), r), c), r), d);
}

// one real root of x^3 + b x^2 + c x + d: kApNewton Newton steps from outside the outer stationary point on the side
// where the iteration is monotone, or from the inflection point when the derivative has no two real roots
__device__ __forceinline__ double ap_cubic_root(double b, double c, double d)
{
	const double q = __dsub_rn(__dmul_rn(b, b), __dmul_rn(3.0, c));
	const double v = __dsqrt_rn(q);
	const double nb = -b;
	const double t1 = __ddiv_rn(__dsub_rn(nb, v), 3.0);
	const double k1 = ap_cubic(t1, b, c, d);
	const double t2 = __ddiv_rn(__dadd_rn(nb, v), 3.0);
	const double k2 = ap_cubic(t2, b, c, d);
	const double rl = __dsub_rn(t1, __dsqrt_rn(__ddiv_rn(k1, v)));
	const double rr = __dadd_rn(t2, __dsqrt_rn(__ddiv_rn(fabs(k2), v)));
	const double ri = __ddiv_rn(nb, 3.0);
	double r = (q > 0.0) ? ((k1 > 0.0) ? rl : rr) : ri;
	const double tb = __dmul_rn(2.0, b);
	for (int it = 0; it < kApNewton; ++it)
	{
		const double fx = ap_cubic(r, b, c, d);
		const double fp = __dadd_rn(__dmul_rn(__dadd_rn(__dmul_rn(3.0, r), tb), r), c);
		const double nr = __dsub_rn(r, __ddiv_rn(fx, fp));
		r = (fp != 0.0) ? nr : r;
	}
	return r;
}

// A3 + A4: the pose of three (bearing, landmark) pairs that the fourth agrees with best.  f, p: [4][3] in sample
// order.  False (and T untouched) when the hypothesis has no model.
__device__ __forceinline__ bool ap_solve(const double (&f)[4][3], const double (&p)[4][3], TvPoseRT& T)
{
	const double inf = __builtin_inf();
	const double b12 = tv_dot3(f[0][0], f[0][1], f[0][2], f[1][0], f[1][1], f[1][2]);
	const double b13 = tv_dot3(f[0][0], f[0][1], f[0][2], f[2][0], f[2][1], f[2][2]);
	const double b23 = tv_dot3(f[1][0], f[1][1], f[1][2], f[2][0], f[2][1], f[2][2]);
	double d12[3], d13[3], d23[3], ww[3];
#pragma unroll
	for (int k = 0; k < 3; ++k)
	{
		d12[k] = __dsub_rn(p[0][k], p[1][k]);
		d13[k] = __dsub_rn(p[0][k], p[2][k]);
		d23[k] = __dsub_rn(p[1][k], p[2][k]);
	}
	const double a12 = tv_dot3(d12[0], d12[1], d12[2], d12[0], d12[1], d12[2]);
	const double a13 = tv_dot3(d13[0], d13[1], d13[2], d13[0], d13[1], d13[2]);
	const double a23 = tv_dot3(d23[0], d23[1], d23[2], d23[0], d23[1], d23[2]);
	tv_cross(d12, d13, ww);
	bool ok = tv_dot3(ww[0], ww[1], ww[2], ww[0], ww[1], ww[2]) > 0.0;
#pragma unroll
	for (int i = 0; i < 4; ++i)
	{
		ok = ok && (tv_dot3(f[i][0], f[i][1], f[i][2], f[i][0], f[i][1], f[i][2]) > 0.0);
	}
	const double m12 = -__dmul_rn(b12, a23), m13 = -__dmul_rn(b13, a23);
	const double x1 = __dmul_rn(b23, a12), x2 = __dmul_rn(b23, a13);
	const double D1[3][3] = {{a23, m12, 0.0}, {m12, __dsub_rn(a23, a12), x1}, {0.0, x1, -a12}};
	const double D2[3][3] = {{a23, 0.0, m13}, {0.0, -a13, x2}, {m13, x2, __dsub_rn(a23, a13)}};
	double gam;
	{
		double C1[3][3], C2[3][3];
		const double c0 = ap_cof(D1, C1);
		const double c3 = ap_cof(D2, C2);
		const double c1 = ap_rows_dot(C1, D2);
		const double c2 = ap_rows_dot(C2, D1);
		ok = ok && (c3 != 0.0);
		gam = ap_cubic_root(__ddiv_rn(c2, c3), __ddiv_rn(c1, c3), __ddiv_rn(c0, c3));
	}
	double M[3][3], V[3][3];
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
#pragma unroll
		for (int j = 0; j < 3; ++j)
		{
			M[i][j] = __dadd_rn(D1[i][j], __dmul_rn(gam, D2[i][j]));
			V[i][j] = (i == j) ? 1.0 : 0.0;
		}
	}
	for (int sweep = 0; sweep < kApSweeps; ++sweep)
	{
		tv_rot3<0, 1>(M, V);
		tv_rot3<0, 2>(M, V);
		tv_rot3<1, 2>(M, V);
	}
	// drop the eigenvalue of smallest magnitude (the first of equals); the other two in index order
	const double e0 = M[0][0], e1 = M[1][1], e2 = M[2][2];
	int m = 0;
	double am = fabs(e0);
	if (fabs(e1) < am)
	{
		am = fabs(e1);
		m = 1;
	}
	if (fabs(e2) < am)
	{
		m = 2;
	}
	const double ea = (m == 0) ? e1 : e0, eb = (m == 2) ? e1 : e2;
	double va[3], vb[3];
#pragma unroll
	for (int k = 0; k < 3; ++k)
	{
		va[k] = (m == 0) ? V[k][1] : V[k][0];
		vb[k] = (m == 2) ? V[k][1] : V[k][2];
	}
	ok = ok && ((ea > 0.0 && eb < 0.0) || (ea < 0.0 && eb > 0.0));
	const double s = __dsqrt_rn(__ddiv_rn(-eb, ea));
	const double tb12 = __dmul_rn(2.0, b12), tb13 = __dmul_rn(2.0, b13), tb23 = __dmul_rn(2.0, b23);
	double best = inf;
	bool have = false;
	for (int plane = 0; plane < 2; ++plane)
	{
		const double sg = plane ? -s : s;
		const double n0 = __dsub_rn(va[0], __dmul_rn(sg, vb[0]));
		const double n1 = __dsub_rn(va[1], __dmul_rn(sg, vb[1]));
		const double n2 = __dsub_rn(va[2], __dmul_rn(sg, vb[2]));
		bool okp = ok && (n0 != 0.0);
		const double w0 = __ddiv_rn(-n1, n0), w1 = __ddiv_rn(-n2, n0);
		const double qa = __dsub_rn(__dmul_rn(a23, __dmul_rn(w1, w1)), a12);
		const double qb = __dadd_rn(__dmul_rn(a23, __dsub_rn(__dmul_rn(__dmul_rn(2.0, w0), w1), __dmul_rn(tb12, w1))),
									__dmul_rn(__dmul_rn(2.0, a12), b23));
		const double qc = __dsub_rn(__dmul_rn(a23, __dsub_rn(__dadd_rn(__dmul_rn(w0, w0), 1.0), __dmul_rn(tb12, w0))), a12);
		okp = okp && (qa != 0.0);
		const double disc = __dsub_rn(__dmul_rn(qb, qb), __dmul_rn(__dmul_rn(4.0, qa), qc));
		okp = okp && (disc >= 0.0);
		const double sq = __dsqrt_rn(disc);
		const double nqb = -qb, ta = __dmul_rn(2.0, qa);
		for (int root = 0; root < 2; ++root)
		{
			const double num = root ? __dsub_rn(nqb, sq) : __dadd_rn(nqb, sq);
			const double tau = __ddiv_rn(num, ta);
			bool okc = okp && (tau > 0.0);
			const double den = __dsub_rn(__dadd_rn(1.0, __dmul_rn(tau, tau)), __dmul_rn(tb23, tau));
			okc = okc && (den > 0.0);
			double l2 = __dsqrt_rn(__ddiv_rn(a23, den));
			double l3 = __dmul_rn(tau, l2);
			double l1 = __dadd_rn(__dmul_rn(w0, l2), __dmul_rn(w1, l3));
			okc = okc && (l1 > 0.0);
			for (int it = 0; it < kApPolish; ++it)
			{
				const double r0 = __dsub_rn(__dsub_rn(__dadd_rn(__dmul_rn(l1, l1), __dmul_rn(l2, l2)), __dmul_rn(__dmul_rn(tb12, l1), l2)), a12);
				const double r1 = __dsub_rn(__dsub_rn(__dadd_rn(__dmul_rn(l1, l1), __dmul_rn(l3, l3)), __dmul_rn(__dmul_rn(tb13, l1), l3)), a13);
				const double r2 = __dsub_rn(__dsub_rn(__dadd_rn(__dmul_rn(l2, l2), __dmul_rn(l3, l3)), __dmul_rn(__dmul_rn(tb23, l2), l3)), a23);
				const double J[3][3] = {
					{__dsub_rn(__dmul_rn(2.0, l1), __dmul_rn(tb12, l2)), __dsub_rn(__dmul_rn(2.0, l2), __dmul_rn(tb12, l1)), 0.0},
					{__dsub_rn(__dmul_rn(2.0, l1), __dmul_rn(tb13, l3)), 0.0, __dsub_rn(__dmul_rn(2.0, l3), __dmul_rn(tb13, l1))},
					{0.0, __dsub_rn(__dmul_rn(2.0, l2), __dmul_rn(tb23, l3)), __dsub_rn(__dmul_rn(2.0, l3), __dmul_rn(tb23, l2))}};
				double Cj[3][3];
				const double dj = ap_cof(J, Cj);
				const bool go = dj != 0.0;
				const double s1 = __dsub_rn(l1, __ddiv_rn(tv_dot3(Cj[0][0], Cj[1][0], Cj[2][0], r0, r1, r2), dj));
				const double s2 = __dsub_rn(l2, __ddiv_rn(tv_dot3(Cj[0][1], Cj[1][1], Cj[2][1], r0, r1, r2), dj));
				const double s3 = __dsub_rn(l3, __ddiv_rn(tv_dot3(Cj[0][2], Cj[1][2], Cj[2][2], r0, r1, r2), dj));
				l1 = go ? s1 : l1;
				l2 = go ? s2 : l2;
				l3 = go ? s3 : l3;
			}
			double X1[3], u[3], v[3], w[3];
#pragma unroll
			for (int k = 0; k < 3; ++k)
			{
				X1[k] = __dmul_rn(l1, f[0][k]);
				u[k] = __dsub_rn(X1[k], __dmul_rn(l2, f[1][k]));
				v[k] = __dsub_rn(X1[k], __dmul_rn(l3, f[2][k]));
			}
			tv_cross(u, v, w);
			const double Bc[3][3] = {{u[0], v[0], w[0]}, {u[1], v[1], w[1]}, {u[2], v[2], w[2]}};
			double Cc[3][3];
			const double dc = ap_cof(Bc, Cc);
			okc = okc && (dc != 0.0);
			TvPoseRT Cn;
#pragma unroll
			for (int j = 0; j < 3; ++j)
			{
				const double i0 = __ddiv_rn(Cc[j][0], dc), i1 = __ddiv_rn(Cc[j][1], dc), i2 = __ddiv_rn(Cc[j][2], dc);
#pragma unroll
				for (int i = 0; i < 3; ++i)
				{
					Cn.R[i][j] = tv_dot3(d12[i], d13[i], ww[i], i0, i1, i2);
				}
			}
#pragma unroll
			for (int i = 0; i < 3; ++i)
			{
				Cn.t[i] = __dsub_rn(p[0][i], tv_dot3(Cn.R[i][0], Cn.R[i][1], Cn.R[i][2], X1[0], X1[1], X1[2]));
			}
			// A4: the first candidate with the smallest score of the fourth point; not finite counts as +infinity
			const double sc = ap_score(Cn, f[3], p[3]);
			const bool take = okc && (fabs(sc) < inf) && (sc < best);
			if (take)
			{
				best = sc;
				T = Cn;
				have = true;
			}
		}
	}
	return have;
}

#ifndef EBO_ABSPOSE_RULES_ONLY  // tools/abs_pose_serial.cpp compiles the rules above for the host and stops here

// Hypothesis kernel: one lane per (frame, hypothesis); sample, solve and choose (A2-A4) entirely in registers.
// models: [nFrames * H][3][4], all zero where valid[] is 0;  samplesOut: [nFrames * H][4] or null.
__global__ void __launch_bounds__(kApBlock) k_ap_hypotheses(int nFrames, int H, const int* __restrict__ offsets,
															const double* __restrict__ f, const double* __restrict__ pts,
															unsigned long long seed, double* __restrict__ models,
															int* __restrict__ valid, int* __restrict__ samplesOut)
{
	const long long g = static_cast<long long>(blockIdx.x) * kApBlock + threadIdx.x;
	if (g >= static_cast<long long>(nFrames) * H)
	{
		return;
	}
	const int frame = static_cast<int>(g / H), h = static_cast<int>(g % H);
	const long long base = offsets[frame];
	const int n = offsets[frame + 1] - offsets[frame];
	TvPoseRT T;
	bool ok = false;
	if (n >= 4)
	{
		int smp[4];
		ransac_sample<4>(seed, frame, h, n, smp);
		double sf[4][3], sp[4][3];
#pragma unroll
		for (int i = 0; i < 4; ++i)
		{
#pragma unroll
			for (int k = 0; k < 3; ++k)
			{
				sf[i][k] = f[3 * (base + smp[i]) + k];
				sp[i][k] = pts[3 * (base + smp[i]) + k];
			}
			if (samplesOut)
			{
				samplesOut[4 * g + i] = smp[i];
			}
		}
		ok = ap_solve(sf, sp, T);
	}
	double* o = models + 12 * g;
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
#pragma unroll
		for (int j = 0; j < 3; ++j)
		{
			o[4 * i + j] = ok ? T.R[i][j] : 0.0;
		}
		o[4 * i + 3] = ok ? T.t[i] : 0.0;
	}
	valid[g] = ok ? 1 : 0;
}

// what ebo_ransac.inc's kernels need to know of this path
struct ApProblem
{
	static constexpr int kSample = 4;
	static __device__ __forceinline__ double score(const TvPoseRT& T, const double (&f)[3], const double (&p)[3])
	{
		return ap_score(T, f, p);
	}
};

#endif  // EBO_ABSPOSE_RULES_ONLY
