// ebo_rpe.inc — relative pose error on the device: the translational and rotational drift of an estimated trajectory
// over steps of `delta` poses against the ground truth's, one wave per (segment, delta) unit, the whole batch in one
// launch.  The reference has no counterpart: it judges a trajectory by the absolute trajectory error alone
// (aligner.cpp:27-114).  Included inside ebo_kernels.hip's anonymous namespace, after ebo_relpose.inc, whose RP_FN /
// rp_reduce / rp_dot3 / rp_finite it uses: the tree of its sums is R6's.  The rules are written out in include/ebo.h
// ("trajectory evaluation: relative pose error", T1-T7); tests/rpe_ref.py restates them in numpy.  Float64, one
// rounding per operation in the association written here: the library is compiled with -ffp-contract=off, so the plain
// operators below are the rules' operations.
//
// Only the bodies handed to rp_reduce / rpe_reduce depend on the lane: lane l takes the segment's poses (T1) or the
// unit's pairs (T2-T6) l, l + 64, ..  Everything else is scalar state that every lane carries alike: no LDS, no
// barrier, no atomics.  A host build (EBO_RELPOSE_RULES_ONLY, tools/rpe_serial.cpp) runs the lanes of a reduction one
// after the other.

// one unit: the segment's first pose in each array, its length, the step and the scale
struct RpeView
{
	int n;             // poses of the segment
	int delta;         // >= 1
	double s;          // scale of the estimate's translations
	const double* gt;  // [n][12]: the ground truth Q_i = [G_i | g_i]
	const double* est; // [n][12]: the estimate P_i = [R_i | p_i]
};

// T6's eight results at once: slots 0-3 are sums in R6's tree (q, e, theta * theta, theta), slots 4 and 6 minima and
// slots 5 and 7 maxima over the same tree (partial[i] takes partial[i + s] when that is strictly smaller / larger)
constexpr int kRpeSlots = 8;
RP_FN void rpe_merge(double (&a)[kRpeSlots], const double (&b)[kRpeSlots])
{
#pragma unroll
	for (int k = 0; k < 4; ++k)
	{
		a[k] = a[k] + b[k];
	}
	a[4] = b[4] < a[4] ? b[4] : a[4];
	a[5] = b[5] > a[5] ? b[5] : a[5];
	a[6] = b[6] < a[6] ? b[6] : a[6];
	a[7] = b[7] > a[7] ? b[7] : a[7];
}
#ifdef EBO_RELPOSE_RULES_ONLY
template <class F>
inline void rpe_reduce(F&& body, double (&out)[kRpeSlots])
{
	double part[kRpLanes][kRpeSlots];
	for (int lane = 0; lane < kRpLanes; ++lane)
	{
		body(lane, part[lane]);
	}
	for (int s = kRpLanes / 2; s > 0; s /= 2)
	{
		for (int i = 0; i < s; ++i)
		{
			rpe_merge(part[i], part[i + s]);
		}
	}
	for (int k = 0; k < kRpeSlots; ++k)
	{
		out[k] = part[0][k];
	}
}
#else
template <class F>
__device__ __forceinline__ void rpe_reduce(F&& body, double (&out)[kRpeSlots])
{
	double acc[kRpeSlots];
	body(static_cast<int>(threadIdx.x) & (kRpLanes - 1), acc);
#pragma unroll
	for (int s = kRpLanes / 2; s > 0; s /= 2)
	{
		double other[kRpeSlots];
#pragma unroll
		for (int k = 0; k < kRpeSlots; ++k)
		{
			other[k] = __shfl_down(acc[k], s, kRpLanes);  // lanes >= s merge what no later step reads
		}
		rpe_merge(acc, other);
	}
#pragma unroll
	for (int k = 0; k < kRpeSlots; ++k)
	{
		out[k] = __shfl(acc[k], 0, kRpLanes);
	}
}
#endif

// T5: the angle in [0, pi] whose sine and cosine are in the ratio sn : cs (sn >= 0), from + - * / sqrt alone.  The
// tangent of the half angle of the fold onto [0, pi / 2], halved twice more, then thirteen terms of the arctangent's
// series at u <= tan(pi / 16): the first term left out is below 2^-63 of the sum
RP_FN double rpe_angle(double sn, double cs)
{
	const double h = sqrt(sn * sn + cs * cs);
	if (!(h > 0.0))
	{
		return 0.0;
	}
	double u = sn / (h + fabs(cs));
#pragma unroll
	for (int k = 0; k < kRpeHalvings; ++k)
	{
		u = u / (1.0 + sqrt(1.0 + u * u));
	}
	const double z = u * u;
	double p = 1.0 / static_cast<double>(2 * (kRpeTerms - 1) + 1);  // k = 12 is even
#pragma unroll
	for (int k = kRpeTerms - 2; k >= 0; --k)
	{
		p = p * z + ((k % 2) ? -1.0 : 1.0) / static_cast<double>(2 * k + 1);
	}
	const double phi = 8.0 * (u * p);
	return cs >= 0.0 ? phi : kRpePi - phi;
}

// column k of A's rotation block against the vector d
RP_FN double rpe_colDot(const double* A, int k, double d0, double d1, double d2)
{
	return rp_dot3(A[k], A[4 + k], A[8 + k], d0, d1, d2);
}

// M = X_i^T X_j on the rotation blocks of two poses: M[r][c] = dot(column r of X_i, column c of X_j)
RP_FN void rpe_relRot(const double* Xi, const double* Xj, double (&M)[3][3])
{
#pragma unroll
	for (int r = 0; r < 3; ++r)
	{
#pragma unroll
		for (int c = 0; c < 3; ++c)
		{
			M[r][c] = rp_dot3(Xi[r], Xi[4 + r], Xi[8 + r], Xj[c], Xj[4 + c], Xj[8 + c]);
		}
	}
}

// what a unit without statistics returns (T1): zeros, with the count its status calls for
RP_FN void rpe_none(ebo_rpe_result* out, int status, int count)
{
	if (RP_FIRST_LANE())
	{
		out->trans_rmse = out->trans_mean = out->trans_min = out->trans_max = 0.0;
		out->rot_rmse = out->rot_mean = out->rot_min = out->rot_max = 0.0;
		out->count = count;
		out->status = status;
	}
}

RP_FN void rpe_unit(const RpeView& v, ebo_rpe_result* out)
{
	// T1: no pair; then one pass over the segment's poses for the count of those with a non-finite entry
	if (v.n <= v.delta)
	{
		rpe_none(out, 1, 0);
		return;
	}
	const int pairs = v.n - v.delta;
	double bad[1];
	rp_reduce<1>(
		[&](int lane, double(&acc)[1]) RP_BODY {
			acc[0] = 0.0;
			for (int i = lane; i < v.n; i += kRpLanes)
			{
				const double* q = v.gt + kRpePoseDoubles * static_cast<size_t>(i);
				const double* p = v.est + kRpePoseDoubles * static_cast<size_t>(i);
				bool ok = true;
#pragma unroll
				for (int k = 0; k < kRpePoseDoubles; ++k)
				{
					ok = ok && rp_finite(q[k]) && rp_finite(p[k]);
				}
				acc[0] = acc[0] + (ok ? 0.0 : 1.0);
			}
		},
		bad);
	if (RP_UNIFORM(static_cast<int>(bad[0] != 0.0 || !rp_finite(v.s))))
	{
		rpe_none(out, 2, pairs);
		return;
	}
	// T2-T6: one pass over the pairs
	const double s = v.s;
	double st[kRpeSlots];
	rpe_reduce(
		[&](int lane, double(&acc)[kRpeSlots]) RP_BODY {
			acc[0] = acc[1] = acc[2] = acc[3] = 0.0;
			acc[4] = acc[6] = 1.7976931348623157e308;
			acc[5] = acc[7] = 0.0;
			for (int i = lane; i < pairs; i += kRpLanes)
			{
				const double* Qi = v.gt + kRpePoseDoubles * static_cast<size_t>(i);
				const double* Qj = Qi + kRpePoseDoubles * static_cast<size_t>(v.delta);
				const double* Pi = v.est + kRpePoseDoubles * static_cast<size_t>(i);
				const double* Pj = Pi + kRpePoseDoubles * static_cast<size_t>(v.delta);
				// T2
				const double dp[3] = {Pj[3] - Pi[3], Pj[7] - Pi[7], Pj[11] - Pi[11]};
				const double dg[3] = {Qj[3] - Qi[3], Qj[7] - Qi[7], Qj[11] - Qi[11]};
				double r[3];
#pragma unroll
				for (int k = 0; k < 3; ++k)
				{
					const double a = s * rpe_colDot(Pi, k, dp[0], dp[1], dp[2]);
					const double b = rpe_colDot(Qi, k, dg[0], dg[1], dg[2]);
					r[k] = a - b;
				}
				const double q = rp_dot3(r[0], r[1], r[2], r[0], r[1], r[2]);
				const double e = sqrt(q);
				// T3
				double A[3][3], B[3][3], E[3][3];
				rpe_relRot(Pi, Pj, A);
				rpe_relRot(Qi, Qj, B);
#pragma unroll
				for (int a = 0; a < 3; ++a)
				{
#pragma unroll
					for (int c = 0; c < 3; ++c)
					{
						E[a][c] = rp_dot3(B[0][a], B[1][a], B[2][a], A[0][c], A[1][c], A[2][c]);
					}
				}
				// T4, T5
				const double w[3] = {0.5 * (E[2][1] - E[1][2]), 0.5 * (E[0][2] - E[2][0]), 0.5 * (E[1][0] - E[0][1])};
				const double sn = sqrt(rp_dot3(w[0], w[1], w[2], w[0], w[1], w[2]));
				const double cs = (((E[0][0] + E[1][1]) + E[2][2]) - 1.0) / 2.0;
				const double th = rpe_angle(sn, cs);
				// T6
				acc[0] = acc[0] + q;
				acc[1] = acc[1] + e;
				acc[2] = acc[2] + th * th;
				acc[3] = acc[3] + th;
				acc[4] = e < acc[4] ? e : acc[4];
				acc[5] = e > acc[5] ? e : acc[5];
				acc[6] = th < acc[6] ? th : acc[6];
				acc[7] = th > acc[7] ? th : acc[7];
			}
		},
		st);
	if (RP_FIRST_LANE())
	{
		const double nd = static_cast<double>(pairs);
		out->trans_rmse = sqrt(st[0] / nd);
		out->trans_mean = st[1] / nd;
		out->trans_min = st[4];
		out->trans_max = st[5];
		out->rot_rmse = sqrt(st[2] / nd);
		out->rot_mean = st[3] / nd;
		out->rot_min = st[6];
		out->rot_max = st[7];
		out->count = pairs;
		out->status = 0;
	}
}

#ifndef EBO_RELPOSE_RULES_ONLY
// one wave per unit.  Unit u = g * nDeltas + k is segment g, poses segBegin[g] .. segEnd[g] - 1 of gt and est, at
// step deltas[k]; segScale may be null (scale 1)
__global__ void __launch_bounds__(kRpLanes) k_trajectory_rpe(int nPoses, const double* __restrict__ gt, const double* __restrict__ est,
															   const int* __restrict__ segBegin, const int* __restrict__ segEnd,
															   const double* __restrict__ segScale, int nDeltas,
															   const int* __restrict__ deltas, ebo_rpe_result* __restrict__ results)
{
	const int u = static_cast<int>(blockIdx.x);
	const int g = u / nDeltas, k = u - g * nDeltas;
	int b = segBegin[g], e = segEnd[g];
	// the entry has refused such a segment or step; never past the arrays
	b = b < 0 ? 0 : (b > nPoses ? nPoses : b);
	e = e < b ? b : (e > nPoses ? nPoses : e);
	const int d = deltas[k];
	RpeView v;
	v.n = e - b;
	v.delta = d < 1 ? 1 : d;
	v.s = segScale ? segScale[g] : 1.0;
	v.gt = gt + kRpePoseDoubles * static_cast<size_t>(b);
	v.est = est + kRpePoseDoubles * static_cast<size_t>(b);
	rpe_unit(v, results + u);
}
#endif
