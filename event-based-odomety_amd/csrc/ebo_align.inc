// ebo_align.inc — trajectory alignment on the device: the similarity (or rigid) transform that takes the estimated
// camera centres of a trajectory segment onto the ground truth's in the least-squares sense, and the absolute
// trajectory error it leaves, one wave per segment, the whole batch in one launch.  Takes the place of what the
// reference does through align_points_sim3 (aligner.cpp:27-88) once per new keyframe.  Included inside
// ebo_kernels.hip's anonymous namespace, after ebo_relpose.inc, whose RP_FN / rp_reduce / rp_dot3 / rp_finite it uses:
// the tree of its sums is R6's.  The rules are written out in include/ebo.h ("trajectory alignment", S1-S7);
// tests/align_ref.py restates them in numpy.  Float64, one rounding per operation in the association written here: the
// library is compiled with -ffp-contract=off, so the plain operators below are the rules' operations.
//
// Only the bodies handed to rp_reduce / al_reduce_errors depend on the lane: lane l takes the segment's points l,
// l + 64, ..  Everything else is scalar state that every lane carries alike: no LDS, no barrier, no atomics.  A host
// build (EBO_RELPOSE_RULES_ONLY, tools/align_sim3_serial.cpp) runs the lanes of a reduction one after the other.

// one segment: its first point in each array and its length
struct AlView
{
	int n;
	const double* d;  // data  [n][3]: the ground-truth centres
	const double* m;  // model [n][3]: the estimated centres
};

// S7's four results at once: slots 0 and 1 are sums in R6's tree, slot 2 a minimum and slot 3 a maximum over the same
// tree (partial[i] takes partial[i + s] when that is strictly smaller / larger)
RP_FN void al_merge_errors(double (&a)[4], const double (&b)[4])
{
	a[0] = a[0] + b[0];
	a[1] = a[1] + b[1];
	a[2] = b[2] < a[2] ? b[2] : a[2];
	a[3] = b[3] > a[3] ? b[3] : a[3];
}
#ifdef EBO_RELPOSE_RULES_ONLY
template <class F>
inline void al_reduce_errors(F&& body, double (&out)[4])
{
	double part[kRpLanes][4];
	for (int lane = 0; lane < kRpLanes; ++lane)
	{
		body(lane, part[lane]);
	}
	for (int s = kRpLanes / 2; s > 0; s /= 2)
	{
		for (int i = 0; i < s; ++i)
		{
			al_merge_errors(part[i], part[i + s]);
		}
	}
	for (int k = 0; k < 4; ++k)
	{
		out[k] = part[0][k];
	}
}
#else
template <class F>
__device__ __forceinline__ void al_reduce_errors(F&& body, double (&out)[4])
{
	double acc[4];
	body(static_cast<int>(threadIdx.x) & (kRpLanes - 1), acc);
#pragma unroll
	for (int s = kRpLanes / 2; s > 0; s /= 2)
	{
		double other[4];
#pragma unroll
		for (int k = 0; k < 4; ++k)
		{
			other[k] = __shfl_down(acc[k], s, kRpLanes);  // lanes >= s merge what no later step reads
		}
		al_merge_errors(acc, other);
	}
#pragma unroll
	for (int k = 0; k < 4; ++k)
	{
		out[k] = __shfl(acc[k], 0, kRpLanes);
	}
}
#endif

// one rotation of jacobi(G, 8) (rule 4 of the two-view section), in registers: P, Q are compile-time, so every index is
template <int P, int Q>
RP_FN void al_rot3(double (&M)[3][3], double (&V)[3][3])
{
	const double apq = M[P][Q];
	if (apq != 0.0)
	{
		const double app = M[P][P], aqq = M[Q][Q];
		const double th = (aqq - app) / (2.0 * apq);
		const double den = fabs(th) + sqrt(th * th + 1.0);
		const double t = (th < 0.0 ? -1.0 : 1.0) / den;
		const double c = 1.0 / sqrt(t * t + 1.0);
		const double s = t * c;
		constexpr int K = 3 - P - Q;
		const double mkp = c * M[K][P] - s * M[K][Q];
		const double mkq = s * M[K][P] + c * M[K][Q];
		M[K][P] = M[P][K] = mkp;
		M[K][Q] = M[Q][K] = mkq;
		const double tapq = t * apq;
		M[P][P] = app - tapq;
		M[Q][Q] = aqq + tapq;
		M[P][Q] = M[Q][P] = 0.0;
#pragma unroll
		for (int k = 0; k < 3; ++k)
		{
			const double vkp = c * V[k][P] - s * V[k][Q];
			const double vkq = s * V[k][P] + c * V[k][Q];
			V[k][P] = vkp;
			V[k][Q] = vkq;
		}
	}
}

// the compare-exchange of S4's descending order: swaps only when strictly smaller
RP_FN void al_cswap(double& da, double& db, double (&va)[3], double (&vb)[3])
{
	const bool sw = da < db;
	const double a = da, b = db;
	da = sw ? b : a;
	db = sw ? a : b;
#pragma unroll
	for (int r = 0; r < 3; ++r)
	{
		const double xa = va[r], xb = vb[r];
		va[r] = sw ? xb : xa;
		vb[r] = sw ? xa : xb;
	}
}

RP_FN void al_cross(const double (&a)[3], const double (&b)[3], double (&o)[3])
{
	o[0] = a[1] * b[2] - a[2] * b[1];
	o[1] = a[2] * b[0] - a[0] * b[2];
	o[2] = a[0] * b[1] - a[1] * b[0];
}

// what a segment that is not aligned returns (S1): scale 1, identity, zero translation, zero metrics
RP_FN void al_not_aligned(ebo_align_result* out, int status, int n)
{
	if (RP_FIRST_LANE())
	{
		out->scale = 1.0;
#pragma unroll
		for (int k = 0; k < 9; ++k)
		{
			out->R[k] = (k % 4 == 0) ? 1.0 : 0.0;
		}
		out->t[0] = out->t[1] = out->t[2] = 0.0;
		out->rmse = out->mean = out->min = out->max = 0.0;
		out->count = n;
		out->status = status;
	}
}

RP_FN void al_solve(const AlView& v, int fixScale, ebo_align_result* out)
{
	// S1, S2: one pass for the six coordinate sums and the count of points with a non-finite coordinate
	if (v.n < kAlMinPoints)
	{
		al_not_aligned(out, 1, v.n);
		return;
	}
	const double nd = static_cast<double>(v.n);
	double s1[7];
	rp_reduce<7>(
		[&](int lane, double(&acc)[7]) RP_BODY {
#pragma unroll
			for (int k = 0; k < 7; ++k)
			{
				acc[k] = 0.0;
			}
			for (int i = lane; i < v.n; i += kRpLanes)
			{
				const double* d = v.d + 3 * static_cast<size_t>(i);
				const double* m = v.m + 3 * static_cast<size_t>(i);
				bool ok = true;
#pragma unroll
				for (int k = 0; k < 3; ++k)
				{
					ok = ok && rp_finite(d[k]) && rp_finite(m[k]);
					acc[k] = acc[k] + d[k];
					acc[3 + k] = acc[3 + k] + m[k];
				}
				acc[6] = acc[6] + (ok ? 0.0 : 1.0);
			}
		},
		s1);
	if (RP_UNIFORM(static_cast<int>(s1[6] != 0.0)))
	{
		al_not_aligned(out, 2, v.n);
		return;
	}
	const double cd[3] = {s1[0] / nd, s1[1] / nd, s1[2] / nd};
	const double cm[3] = {s1[3] / nd, s1[4] / nd, s1[5] / nd};
	// S3: the centred second moments
	double s2[10];
	rp_reduce<10>(
		[&](int lane, double(&acc)[10]) RP_BODY {
#pragma unroll
			for (int k = 0; k < 10; ++k)
			{
				acc[k] = 0.0;
			}
			for (int i = lane; i < v.n; i += kRpLanes)
			{
				const double* d = v.d + 3 * static_cast<size_t>(i);
				const double* m = v.m + 3 * static_cast<size_t>(i);
				const double dc[3] = {d[0] - cd[0], d[1] - cd[1], d[2] - cd[2]};
				const double mc[3] = {m[0] - cm[0], m[1] - cm[1], m[2] - cm[2]};
#pragma unroll
				for (int a = 0; a < 3; ++a)
				{
#pragma unroll
					for (int b = 0; b < 3; ++b)
					{
						acc[3 * a + b] = acc[3 * a + b] + dc[a] * mc[b];
					}
				}
				acc[9] = acc[9] + ((mc[0] * mc[0] + mc[1] * mc[1]) + mc[2] * mc[2]);
			}
		},
		s2);
	double W[3][3];
#pragma unroll
	for (int a = 0; a < 3; ++a)
	{
#pragma unroll
		for (int b = 0; b < 3; ++b)
		{
			W[a][b] = s2[3 * a + b];
		}
	}
	const double nm = s2[9];
	// S4: the right singular vectors of W from Jacobi on W^T W
	double G[3][3], V[3][3];
#pragma unroll
	for (int j = 0; j < 3; ++j)
	{
#pragma unroll
		for (int k = 0; k < 3; ++k)
		{
			G[j][k] = rp_dot3(W[0][j], W[1][j], W[2][j], W[0][k], W[1][k], W[2][k]);
			V[j][k] = (j == k) ? 1.0 : 0.0;
		}
	}
	for (int sweep = 0; sweep < kAlSweeps; ++sweep)
	{
		al_rot3<0, 1>(G, V);
		al_rot3<0, 2>(G, V);
		al_rot3<1, 2>(G, V);
	}
	double dd[3] = {G[0][0], G[1][1], G[2][2]};
	double vc[3][3];  // vc[c] = column c of V
#pragma unroll
	for (int c = 0; c < 3; ++c)
	{
#pragma unroll
		for (int r = 0; r < 3; ++r)
		{
			vc[c][r] = V[r][c];
		}
	}
	al_cswap(dd[0], dd[1], vc[0], vc[1]);
	al_cswap(dd[1], dd[2], vc[1], vc[2]);
	al_cswap(dd[0], dd[1], vc[0], vc[1]);
	// 2^-46 of the largest (128 ulps of it): a second singular value below 2^-23 of the first is a line to the digits G carries
	bool ok = dd[1] > 0.0 && rp_finite(dd[1]) && dd[1] > dd[0] * 1.4210854715202004e-14 && nm > 0.0 && rp_finite(nm);
	// S5: the rotation from the top two singular pairs only
	double u0[3], u1[3], u2[3], v2[3];
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		u0[i] = rp_dot3(W[i][0], W[i][1], W[i][2], vc[0][0], vc[0][1], vc[0][2]);
		u1[i] = rp_dot3(W[i][0], W[i][1], W[i][2], vc[1][0], vc[1][1], vc[1][2]);
	}
	const double n0 = sqrt(rp_dot3(u0[0], u0[1], u0[2], u0[0], u0[1], u0[2]));
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		u0[i] = u0[i] / n0;
	}
	const double h = rp_dot3(u0[0], u0[1], u0[2], u1[0], u1[1], u1[2]);
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		u1[i] = u1[i] - h * u0[i];
	}
	const double n1 = sqrt(rp_dot3(u1[0], u1[1], u1[2], u1[0], u1[1], u1[2]));
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		u1[i] = u1[i] / n1;
	}
	ok = ok && n0 > 0.0 && rp_finite(n0) && n1 > 0.0 && rp_finite(n1);
	if (RP_UNIFORM(static_cast<int>(!ok)))
	{
		al_not_aligned(out, 3, v.n);
		return;
	}
	al_cross(u0, u1, u2);
	al_cross(vc[0], vc[1], v2);
	double R[3][3];
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
#pragma unroll
		for (int j = 0; j < 3; ++j)
		{
			R[i][j] = (u0[i] * vc[0][j] + u1[i] * vc[1][j]) + u2[i] * v2[j];
		}
	}
	// S6: the scale from the sums S3 left (sum of dot(dc, R mc) = sum over a, b of R[a][b] W[a][b]), the translation
	double s = 1.0;
	if (!fixScale)
	{
		double dots = 0.0;
#pragma unroll
		for (int a = 0; a < 3; ++a)
		{
#pragma unroll
			for (int b = 0; b < 3; ++b)
			{
				dots = dots + R[a][b] * W[a][b];
			}
		}
		s = dots / nm;
	}
	double t[3];
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		t[i] = cd[i] - s * rp_dot3(R[i][0], R[i][1], R[i][2], cm[0], cm[1], cm[2]);
	}
	// S7: the errors
	double err[4];
	al_reduce_errors(
		[&](int lane, double(&acc)[4]) RP_BODY {
			acc[0] = 0.0;
			acc[1] = 0.0;
			acc[2] = 1.7976931348623157e308;
			acc[3] = 0.0;
			for (int i = lane; i < v.n; i += kRpLanes)
			{
				const double* d = v.d + 3 * static_cast<size_t>(i);
				const double* m = v.m + 3 * static_cast<size_t>(i);
				double r[3];
#pragma unroll
				for (int k = 0; k < 3; ++k)
				{
					r[k] = d[k] - (s * rp_dot3(R[k][0], R[k][1], R[k][2], m[0], m[1], m[2]) + t[k]);
				}
				const double q = rp_dot3(r[0], r[1], r[2], r[0], r[1], r[2]);
				const double e = sqrt(q);
				acc[0] = acc[0] + q;
				acc[1] = acc[1] + e;
				acc[2] = e < acc[2] ? e : acc[2];
				acc[3] = e > acc[3] ? e : acc[3];
			}
		},
		err);
	if (RP_FIRST_LANE())
	{
		out->scale = s;
#pragma unroll
		for (int i = 0; i < 3; ++i)
		{
#pragma unroll
			for (int j = 0; j < 3; ++j)
			{
				out->R[3 * i + j] = R[i][j];
			}
			out->t[i] = t[i];
		}
		out->rmse = sqrt(err[0] / nd);
		out->mean = err[1] / nd;
		out->min = err[2];
		out->max = err[3];
		out->count = v.n;
		out->status = 0;
	}
}

#ifndef EBO_RELPOSE_RULES_ONLY
// one wave per segment.  Segment g covers points segBegin[g] .. segEnd[g] - 1 of data and model
__global__ void __launch_bounds__(kRpLanes) k_align_sim3(int nPoints, const double* __restrict__ data, const double* __restrict__ model,
														   const int* __restrict__ segBegin, const int* __restrict__ segEnd, int fixScale,
														   ebo_align_result* __restrict__ results)
{
	const int g = static_cast<int>(blockIdx.x);
	int b = segBegin[g], e = segEnd[g];
	// the entry has refused such a segment; never past the arrays
	b = b < 0 ? 0 : (b > nPoints ? nPoints : b);
	e = e < b ? b : (e > nPoints ? nPoints : e);
	AlView v;
	v.n = e - b;
	v.d = data + 3 * static_cast<size_t>(b);
	v.m = model + 3 * static_cast<size_t>(b);
	al_solve(v, fixScale, results + g);
}
#endif
