// ebo_relpose.inc — relative-pose refinement on the device: a five-variable trust-region Levenberg-Marquardt on the
// chords of the two-view score over a pair's RANSAC inliers, one wave per keyframe pair, the whole solve in one launch.
// Takes the place of what the reference does through relative_pose::optimize_nonlinear after findInliersRansac's
// RANSAC (visual_odometry.cpp:316-330).  Included inside ebo_kernels.hip's anonymous namespace.  The rules are written
// out in include/ebo.h ("relative-pose refinement", R1-R8); tests/relpose_ref.py restates them in numpy.  Float64, one
// rounding per operation in the association written here: the library is compiled with -ffp-contract=off, so the plain
// operators below are the rules' operations.
//
// Only the bodies handed to rp_reduce depend on the lane: lane l takes the listed inliers l, l + 64, .. and the 64
// partial sums meet in R6's tree, on the device by wave shuffles.  Everything else is the solver's scalar state, which
// every lane carries and advances alike: no LDS, no barrier, no atomics, uniform loop counts.  A host build
// (EBO_RELPOSE_RULES_ONLY, tools/relpose_refine_serial.cpp) runs the lanes of a reduction one after the other.

// The lane count, the limits and the work size are csrc/ebo_relpose.h's, which every build includes before this file.

#ifdef EBO_RELPOSE_RULES_ONLY
#define RP_FN inline
#define RP_UNIFORM(x) (x)
#define RP_FIRST_LANE() true
#else
#define RP_FN __device__ __forceinline__
// an integer of the scalar state that decides where the wave goes next: equal in every lane, and said so
#define RP_UNIFORM(x) __builtin_amdgcn_readfirstlane(x)
#define RP_FIRST_LANE() ((threadIdx.x & (kRpLanes - 1)) == 0)
#endif
#define RP_BODY __attribute__((always_inline))

// R6: K sums at once.  body(lane, acc) leaves lane's partial sums in acc; partial[i] = partial[i] + partial[i + s] for
// i < s, s = 32, 16, .., 1; out = partial[0], in every lane.
#ifdef EBO_RELPOSE_RULES_ONLY
template <int K, class F>
inline void rp_reduce(F&& body, double (&out)[K])
{
	double part[kRpLanes][K];
	for (int lane = 0; lane < kRpLanes; ++lane)
	{
		body(lane, part[lane]);
	}
	for (int s = kRpLanes / 2; s > 0; s /= 2)
	{
		for (int i = 0; i < s; ++i)
		{
			for (int k = 0; k < K; ++k)
			{
				part[i][k] = part[i][k] + part[i + s][k];
			}
		}
	}
	for (int k = 0; k < K; ++k)
	{
		out[k] = part[0][k];
	}
}
template <class F>
inline void rp_for_lanes(F&& body)
{
	for (int lane = 0; lane < kRpLanes; ++lane)
	{
		body(lane);
	}
}
#else
template <int K, class F>
__device__ __forceinline__ void rp_reduce(F&& body, double (&out)[K])
{
	double acc[K];
	body(static_cast<int>(threadIdx.x) & (kRpLanes - 1), acc);
#pragma unroll
	for (int k = 0; k < K; ++k)
	{
		double v = acc[k];
#pragma unroll
		for (int s = kRpLanes / 2; s > 0; s /= 2)
		{
			v = v + __shfl_down(v, s, kRpLanes);  // lanes >= s add what no later step reads
		}
		out[k] = __shfl(v, 0, kRpLanes);
	}
}
template <class F>
__device__ __forceinline__ void rp_for_lanes(F&& body)
{
	body(static_cast<int>(threadIdx.x) & (kRpLanes - 1));
}
#endif

// one pair: the caller's arrays and the pair's slice of the work memory
struct RpView
{
	int n;             // correspondences of the pair
	int m;             // listed inliers
	const double* f1;  // [n][3]
	const double* f2;  // [n][3]
	const int* idx;    // [m] indices within the pair
	double* work;      // [kRpRowDoubles][m]: component c of listed inlier i at work[c * m + i]
};

// a quantity with one derivative slot (R4)
struct RpDual
{
	double v, d;
};

// a quantity without a slot: the same operations on the value alone, for the evaluations that need no Jacobian.  A value
// never reads a slot, so rp_chords gives the same chords with either type
struct RpValue
{
	double v;
};
RP_FN RpValue rp_add(RpValue x, RpValue y)
{
	return {x.v + y.v};
}
RP_FN RpValue rp_sub(RpValue x, RpValue y)
{
	return {x.v - y.v};
}
RP_FN RpValue rp_neg(RpValue x)
{
	return {-x.v};
}
RP_FN RpValue rp_mul(RpValue x, RpValue y)
{
	return {x.v * y.v};
}
RP_FN RpValue rp_mulc(double c, RpValue x)
{
	return {c * x.v};
}
RP_FN RpValue rp_div(RpValue x, RpValue y)
{
	return {x.v / y.v};
}
RP_FN RpValue rp_divc(RpValue x, double c)
{
	return {x.v / c};
}
RP_FN RpValue rp_sqrt(RpValue x)
{
	return {sqrt(x.v)};
}
RP_FN void rp_make(double v, double, RpValue& out)
{
	out = {v};
}
RP_FN double rp_slot(RpValue)
{
	return 0.0;
}
RP_FN void rp_make(double v, double d, RpDual& out)
{
	out = {v, d};
}
RP_FN double rp_slot(RpDual x)
{
	return x.d;
}

RP_FN RpDual rp_add(RpDual x, RpDual y)
{
	return {x.v + y.v, x.d + y.d};
}
RP_FN RpDual rp_sub(RpDual x, RpDual y)
{
	return {x.v - y.v, x.d - y.d};
}
RP_FN RpDual rp_neg(RpDual x)
{
	return {-x.v, -x.d};
}
RP_FN RpDual rp_mul(RpDual x, RpDual y)
{
	return {x.v * y.v, x.v * y.d + y.v * x.d};
}
RP_FN RpDual rp_mulc(double c, RpDual x)
{
	return {c * x.v, c * x.d};
}
RP_FN RpDual rp_div(RpDual x, RpDual y)
{
	const double c = x.v / y.v;
	return {c, (x.d - c * y.d) / y.v};
}
RP_FN RpDual rp_divc(RpDual x, double c)
{
	return {x.v / c, x.d / c};
}
RP_FN RpDual rp_sqrt(RpDual x)
{
	const double s = sqrt(x.v);
	return {s, x.d / (2.0 * s)};
}
template <class N>
RP_FN N rp_dot(const N (&a)[3], const N (&b)[3])
{
	return rp_add(rp_add(rp_mul(a[0], b[0]), rp_mul(a[1], b[1])), rp_mul(a[2], b[2]));
}
template <class N>
RP_FN N rp_dotc(const N (&a)[3], const double (&c)[3])
{
	return rp_add(rp_add(rp_mulc(c[0], a[0]), rp_mulc(c[1], a[1])), rp_mulc(c[2], a[2]));
}

RP_FN double rp_dot3(double a0, double a1, double a2, double b0, double b1, double b2)
{
	return (a0 * b0 + a1 * b1) + a2 * b2;
}

RP_FN bool rp_finite(double v)
{
	return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308;
}

// packed lower triangle: entry (i, j), j <= i
RP_FN constexpr int rp_tri(int i, int j)
{
	return i * (i + 1) / 2 + j;
}

// R3, R4: the six chords of one correspondence at the model M = [R | t] and, with N = RpDual, their derivatives along the
// seed dM (with N = RpValue neither dM nor dc is touched)
template <class N>
RP_FN void rp_chords(const double (&M)[12], const double (&dM)[12], const double (&f1)[3], const double (&f2)[3], double (&c)[6],
					 double (&dc)[6])
{
	N R[3][3], t[3];
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
#pragma unroll
		for (int j = 0; j < 3; ++j)
		{
			rp_make(M[4 * i + j], dM[4 * i + j], R[i][j]);
		}
		rp_make(M[4 * i + 3], dM[4 * i + 3], t[i]);
	}
	// rule 1 of the two-view section
	N g[3];
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		g[i] = rp_dotc(R[i], f2);
	}
	const N b0 = rp_dotc(t, f1);
	const N b1 = rp_dot(t, g);
	const double a00 = rp_dot3(f1[0], f1[1], f1[2], f1[0], f1[1], f1[2]);
	const N fg = rp_dotc(g, f1);
	const N a01 = rp_neg(fg), a10 = fg;
	const N a11 = rp_neg(rp_dot(g, g));
	const N det = rp_sub(rp_mulc(a00, a11), rp_mul(a01, a10));
	const N l0 = rp_div(rp_sub(rp_mul(a11, b0), rp_mul(a01, b1)), det);
	const N l1 = rp_div(rp_sub(rp_mulc(a00, b1), rp_mul(a10, b0)), det);
	N p[3];
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		const N x = rp_mulc(f1[i], l0);
		const N z = rp_add(t[i], rp_mul(l1, g[i]));
		p[i] = rp_divc(rp_add(x, z), 2.0);
	}
	// rule 2 up to r1, r2
	const N n1 = rp_sqrt(rp_dot(p, p));
	N d[3], q[3];
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		d[i] = rp_sub(p[i], t[i]);
	}
#pragma unroll
	for (int j = 0; j < 3; ++j)
	{
		q[j] = rp_add(rp_add(rp_mul(R[0][j], d[0]), rp_mul(R[1][j], d[1])), rp_mul(R[2][j], d[2]));
	}
	const N n2 = rp_sqrt(rp_dot(q, q));
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		const N r1 = rp_div(p[i], n1), r2 = rp_div(q[i], n2);
		c[i] = f1[i] - r1.v;
		dc[i] = -rp_slot(r1);
		c[3 + i] = f2[i] - r2.v;
		dc[3 + i] = -rp_slot(r2);
	}
}

// R4: the seed of variable s at the model M with the tangent basis (e1, e2)
RP_FN void rp_seed(const double (&M)[12], const double (&e1)[3], const double (&e2)[3], int s, double (&dM)[12])
{
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		const double r0 = M[4 * i], r1 = M[4 * i + 1], r2 = M[4 * i + 2];
		dM[4 * i] = s == 3 ? -r2 : (s == 4 ? r1 : 0.0);
		dM[4 * i + 1] = s == 2 ? r2 : (s == 4 ? -r0 : 0.0);
		dM[4 * i + 2] = s == 2 ? -r1 : (s == 3 ? r0 : 0.0);
		dM[4 * i + 3] = s == 0 ? e1[i] : (s == 1 ? e2[i] : 0.0);
	}
}

// R2: the tangent basis at the unit vector t
RP_FN void rp_basis(const double (&M)[12], double (&e1)[3], double (&e2)[3])
{
	const double t0 = M[3], t1 = M[7], t2 = M[11];
	int k = 0;
	double least = fabs(t0);
	if (fabs(t1) < least)
	{
		k = 1;
		least = fabs(t1);
	}
	if (fabs(t2) < least)
	{
		k = 2;
	}
	const double w0 = k == 0 ? 0.0 : (k == 1 ? -t2 : t1);
	const double w1 = k == 0 ? t2 : (k == 1 ? 0.0 : -t0);
	const double w2 = k == 0 ? -t1 : (k == 1 ? t0 : 0.0);
	const double n = sqrt(rp_dot3(w0, w1, w2, w0, w1, w2));
	e1[0] = w0 / n;
	e1[1] = w1 / n;
	e1[2] = w2 / n;
	e2[0] = t1 * e1[2] - t2 * e1[1];
	e2[1] = t2 * e1[0] - t0 * e1[2];
	e2[2] = t0 * e1[1] - t1 * e1[0];
}

// R5: the candidate M (+) step, the step already multiplied by the scales
RP_FN void rp_retract(const double (&M)[12], const double (&e1)[3], const double (&e2)[3], const double (&s)[5], double (&out)[12])
{
	const double a = s[0], b = s[1];
	const double nt = sqrt(1.0 + (a * a + b * b));
	const double hx = s[2] * 0.5, hy = s[3] * 0.5, hz = s[4] * 0.5;
	const double n = sqrt(1.0 + ((hx * hx + hy * hy) + hz * hz));
	const double x = hx / n, y = hy / n, z = hz / n, w = 1.0 / n;
	const double x2 = 2.0 * x, y2 = 2.0 * y, z2 = 2.0 * z;
	const double twx = x2 * w, twy = y2 * w, twz = z2 * w;
	const double txx = x2 * x, txy = y2 * x, txz = z2 * x;
	const double tyy = y2 * y, tyz = z2 * y, tzz = z2 * z;
	const double C[3][3] = {{1.0 - (tyy + tzz), txy - twz, txz + twy}, {txy + twz, 1.0 - (txx + tzz), tyz - twx}, {txz - twy, tyz + twx, 1.0 - (txx + tyy)}};
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
#pragma unroll
		for (int j = 0; j < 3; ++j)
		{
			out[4 * i + j] = rp_dot3(M[4 * i], M[4 * i + 1], M[4 * i + 2], C[0][j], C[1][j], C[2][j]);
		}
		out[4 * i + 3] = (M[4 * i + 3] + (a * e1[i] + b * e2[i])) / nt;
	}
}

RP_FN void rp_load_pair(const RpView& v, int i, double (&f1)[3], double (&f2)[3])
{
	const size_t at = 3 * static_cast<size_t>(v.idx[i]);
#pragma unroll
	for (int k = 0; k < 3; ++k)
	{
		f1[k] = v.f1[at + k];
		f2[k] = v.f2[at + k];
	}
}

// value + Jacobian at M: the scaled Jacobian and the chords of every listed inlier into the work memory, and R6's 21 sums:
// the packed lower triangle of J^T J [0, 15), J^T c [15, 20), the squared chords [20]
RP_FN void rp_eval_jac(const RpView& v, const double (&M)[12], const double (&e1)[3], const double (&e2)[3], const double (&scale)[5],
					   double (&sums)[21])
{
	rp_reduce<21>(
		[&](int lane, double(&acc)[21]) RP_BODY {
#pragma unroll
			for (int k = 0; k < 21; ++k)
			{
				acc[k] = 0.0;
			}
			for (int i = lane; i < v.m; i += kRpLanes)
			{
				double f1[3], f2[3], c[6];
				rp_load_pair(v, i, f1, f2);
				// one derivative slot at a time (by R4 the slots do not meet, so the bits are those of five at once): the
				// column goes to the work memory, which the model cost change reads again, and comes back below
#pragma unroll 1
				for (int s = 0; s < 5; ++s)
				{
					double dM[12], dc[6];
					rp_seed(M, e1, e2, s, dM);
					rp_chords<RpDual>(M, dM, f1, f2, c, dc);
					const double sc = s == 0 ? scale[0] : (s == 1 ? scale[1] : (s == 2 ? scale[2] : (s == 3 ? scale[3] : scale[4])));
#pragma unroll
					for (int k = 0; k < 6; ++k)
					{
						v.work[static_cast<size_t>(5 * k + s) * v.m + i] = dc[k] * sc;
					}
				}
#pragma unroll
				for (int k = 0; k < 6; ++k)
				{
					double J[5];
#pragma unroll
					for (int a = 0; a < 5; ++a)
					{
						J[a] = v.work[static_cast<size_t>(5 * k + a) * v.m + i];
					}
#pragma unroll
					for (int a = 0; a < 5; ++a)
					{
#pragma unroll
						for (int b = 0; b <= a; ++b)
						{
							acc[rp_tri(a, b)] = acc[rp_tri(a, b)] + J[a] * J[b];
						}
					}
#pragma unroll
					for (int a = 0; a < 5; ++a)
					{
						acc[15 + a] = acc[15 + a] + J[a] * c[k];
					}
					v.work[static_cast<size_t>(30 + k) * v.m + i] = c[k];
					acc[20] = acc[20] + c[k] * c[k];
				}
			}
		},
		sums);
}

// the cost at M: 0.5 * tree(squared chords)
RP_FN double rp_cost(const RpView& v, const double (&M)[12])
{
	double sum[1];
	rp_reduce<1>(
		[&](int lane, double(&acc)[1]) RP_BODY {
			acc[0] = 0.0;
			for (int i = lane; i < v.m; i += kRpLanes)
			{
				double f1[3], f2[3], c[6], dc[6];
				const double dM[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
				rp_load_pair(v, i, f1, f2);
				rp_chords<RpValue>(M, dM, f1, f2, c, dc);
#pragma unroll
				for (int k = 0; k < 6; ++k)
				{
					acc[0] = acc[0] + c[k] * c[k];
				}
			}
		},
		sum);
	return 0.5 * sum[0];
}

// R8: minus the model cost change of `step` from the rows the last rp_eval_jac left in the work memory
RP_FN double rp_model_sum(const RpView& v, const double (&step)[5])
{
	double sum[1];
	rp_reduce<1>(
		[&](int lane, double(&acc)[1]) RP_BODY {
			acc[0] = 0.0;
			for (int i = lane; i < v.m; i += kRpLanes)
			{
#pragma unroll
				for (int k = 0; k < 6; ++k)
				{
					const double* J = v.work + static_cast<size_t>(5 * k) * v.m + i;
					double mr = J[0] * step[0] + J[v.m] * step[1];
					mr = mr + J[2 * static_cast<size_t>(v.m)] * step[2];
					mr = mr + J[3 * static_cast<size_t>(v.m)] * step[3];
					mr = mr + J[4 * static_cast<size_t>(v.m)] * step[4];
					const double c = v.work[static_cast<size_t>(30 + k) * v.m + i];
					acc[0] = acc[0] + mr * (c + mr / 2.0);
				}
			}
		},
		sum);
	return sum[0];
}

// R8: R6's tree over 12 squares: partial i is entry i and the others are 0, and adding +0 to a square (which is never
// -0) changes nothing, so only these additions of the tree are left
RP_FN double rp_tree12(const double (&e)[12])
{
	double p[8];
#pragma unroll
	for (int i = 0; i < 8; ++i)
	{
		p[i] = e[i];
	}
#pragma unroll
	for (int i = 0; i < 4; ++i)
	{
		p[i] = p[i] + e[8 + i];
	}
#pragma unroll
	for (int i = 0; i < 4; ++i)
	{
		p[i] = p[i] + p[4 + i];
	}
	p[0] = p[0] + p[2];
	p[1] = p[1] + p[3];
	return p[0] + p[1];
}

// |a - b| over the 12 entries (b == null: |a|)
RP_FN double rp_norm12(const double (&a)[12], const double* b)
{
	double e[12];
#pragma unroll
	for (int i = 0; i < 12; ++i)
	{
		const double d = b ? a[i] - b[i] : a[i];
		e[i] = d * d;
	}
	return sqrt(rp_tree12(e));
}

RP_FN double rp_damp(const ebo_solver_opts& o, double diag, double radius)
{
	double d = diag > o.min_lm_diagonal ? diag : o.min_lm_diagonal;
	d = d < o.max_lm_diagonal ? d : o.max_lm_diagonal;
	const double l = sqrt(d / radius);
	return l * l;
}

// R7: the damped 5 x 5 system by Cholesky and two substitutions; false for an invalid step
RP_FN bool rp_step(const ebo_solver_opts& o, const double (&sums)[21], double radius, double (&step)[5])
{
	double L[5][5], vec[5], sol[5];
	bool ok = true;
#pragma unroll
	for (int i = 0; i < 5; ++i)
	{
#pragma unroll
		for (int j = 0; j <= i; ++j)
		{
			L[i][j] = sums[rp_tri(i, j)];
		}
		L[i][i] = L[i][i] + rp_damp(o, L[i][i], radius);
		vec[i] = sums[15 + i];
	}
#pragma unroll
	for (int k = 0; k < 5; ++k)
	{
		const double d = L[k][k];
		ok = ok && d > 0.0 && rp_finite(d);
		L[k][k] = sqrt(d);
#pragma unroll
		for (int i = k + 1; i < 5; ++i)
		{
			L[i][k] = L[i][k] / L[k][k];
		}
#pragma unroll
		for (int i = k + 1; i < 5; ++i)
		{
#pragma unroll
			for (int j = k + 1; j <= i; ++j)
			{
				L[i][j] = L[i][j] - L[i][k] * L[j][k];
			}
		}
	}
#pragma unroll
	for (int k = 0; k < 5; ++k)
	{
		const double y = vec[k] / L[k][k];
#pragma unroll
		for (int i = k + 1; i < 5; ++i)
		{
			vec[i] = vec[i] - L[i][k] * y;
		}
		sol[k] = y;
	}
#pragma unroll
	for (int k = 4; k >= 0; --k)
	{
		const double x = sol[k] / L[k][k];
#pragma unroll
		for (int i = 0; i < k; ++i)
		{
			sol[i] = sol[i] - L[k][i] * x;
		}
		step[k] = -x;
		ok = ok && rp_finite(step[k]);
	}
	return ok;
}

RP_FN void rp_trace(double* trace, int row, double cost, double radius, double quality, double flag)
{
	if (trace && RP_FIRST_LANE())
	{
		trace[4 * row] = cost;
		trace[4 * row + 1] = radius;
		trace[4 * row + 2] = quality;
		trace[4 * row + 3] = flag;
	}
}

// what a solve leaves behind: the summary, the trace rows it never reached set to zero, and with `best` the model
RP_FN void rp_finish(double* model, const double* best, ebo_summary* summary, double* trace, size_t traceRows, int iterations, int evalsCost,
					 int evalsJac, int termination, double initialCost, double finalCost, int rowsWritten)
{
	if (trace)
	{
		rp_for_lanes([&](int lane) RP_BODY {
			for (size_t i = 4 * static_cast<size_t>(rowsWritten) + lane; i < 4 * traceRows; i += kRpLanes)
			{
				trace[i] = 0.0;
			}
		});
	}
	if (RP_FIRST_LANE())
	{
		if (best)
		{
#pragma unroll
			for (int i = 0; i < 12; ++i)
			{
				model[i] = best[i];
			}
		}
		ebo_summary s;
		s.iterations = iterations;
		s.num_evals_cost = evalsCost;
		s.num_evals_jac = evalsJac;
		s.termination = termination;
		s.initial_cost = initialCost;
		s.final_cost = finalCost;
		*summary = s;
	}
}

// R1-R8: the whole solve of one pair.  model: double [12], in the start, out the lowest-cost point visited.
RP_FN void rp_solve(const RpView& v, const ebo_solver_opts& o, double* model, ebo_summary* summary, double* trace)
{
	const size_t traceRows = static_cast<size_t>(o.max_num_iterations) + 1;
	if (v.m < kRpMinInliers)
	{
		rp_finish(model, nullptr, summary, trace, traceRows, 0, 0, 0, 1, 0.0, 0.0, 0);
		return;
	}
	// R1: what the solve cannot start from
	double x[12];
	bool modelOk = true;
#pragma unroll
	for (int i = 0; i < 12; ++i)
	{
		x[i] = model[i];
		modelOk = modelOk && rp_finite(x[i]);
	}
	const double tn = sqrt(rp_dot3(x[3], x[7], x[11], x[3], x[7], x[11]));
	modelOk = modelOk && tn > 0.0 && rp_finite(tn);
	double bad[1];
	rp_reduce<1>(
		[&](int lane, double(&acc)[1]) RP_BODY {
			acc[0] = 0.0;
			for (int i = lane; i < v.n; i += kRpLanes)
			{
				bool ok = true;
#pragma unroll
				for (int k = 0; k < 3; ++k)
				{
					ok = ok && rp_finite(v.f1[3 * static_cast<size_t>(i) + k]) && rp_finite(v.f2[3 * static_cast<size_t>(i) + k]);
				}
				acc[0] = acc[0] + (ok ? 0.0 : 1.0);
			}
			for (int i = lane; i < v.m; i += kRpLanes)
			{
				acc[0] = acc[0] + ((v.idx[i] >= 0 && v.idx[i] < v.n) ? 0.0 : 1.0);
			}
		},
		bad);
	if (RP_UNIFORM(static_cast<int>(!modelOk || bad[0] > 0.0)))
	{
		rp_finish(model, nullptr, summary, trace, traceRows, 0, 0, 0, 2, 0.0, 0.0, 0);
		return;
	}
	x[3] = x[3] / tn;
	x[7] = x[7] / tn;
	x[11] = x[11] / tn;

	double scale[5] = {1.0, 1.0, 1.0, 1.0, 1.0};
	double e1[3], e2[3], sums[21], best[12], cand[12], step[5];
	int iterations = 0, evalsCost = 0, evalsJac = 1, termination = 1;
	double radius = o.initial_radius, decrease = 2.0;
	const int maxNonmono = o.use_nonmonotonic ? o.max_consecutive_nonmonotonic : 0;
	rp_basis(x, e1, e2);
	rp_eval_jac(v, x, e1, e2, scale, sums);
	double xCost = 0.5 * sums[20];
	const double initialCost = xCost;
	double minCost = xCost;
	rp_trace(trace, 0, xCost, radius, 0.0, 1.0);
	if (RP_UNIFORM(static_cast<int>(!rp_finite(xCost))))
	{
		rp_finish(model, nullptr, summary, trace, traceRows, 0, 0, 1, 2, initialCost, minCost, 1);
		return;
	}
#pragma unroll
	for (int i = 0; i < 12; ++i)
	{
		best[i] = x[i];
	}
	if (o.jacobi_scaling)
	{
#pragma unroll
		for (int a = 0; a < 5; ++a)
		{
			scale[a] = 1.0 / (1.0 + sqrt(sums[rp_tri(a, a)]));
		}
		rp_eval_jac(v, x, e1, e2, scale, sums);
		xCost = 0.5 * sums[20];
	}
	double gradMax = 0.0;
#pragma unroll
	for (int a = 0; a < 5; ++a)
	{
		const double g = fabs(sums[15 + a] / scale[a]);
		gradMax = g > gradMax ? g : gradMax;
	}
	double xNorm = rp_norm12(x, nullptr);
	double seMin = xCost, seCur = xCost, seRef = xCost, seCand = xCost, seAccRef = 0.0, seAccCand = 0.0;
	int seNonmono = 0, numInvalid = 0, lastSuccessful = 1;

	for (;;)
	{
		if (lastSuccessful && xCost < minCost)
		{
			minCost = xCost;
#pragma unroll
			for (int i = 0; i < 12; ++i)
			{
				best[i] = x[i];
			}
		}
		int done = 0;
		if (iterations >= o.max_num_iterations)
		{
			termination = 1;
			done = 1;
		}
		else if (lastSuccessful && gradMax <= o.gradient_tolerance)
		{
			termination = 0;
			done = 1;
		}
		else if (radius < o.min_radius)
		{
			termination = 0;
			done = 1;
		}
		if (RP_UNIFORM(done))
		{
			break;
		}
		iterations++;
		lastSuccessful = 0;
		// the step and the model cost change
		int valid = rp_step(o, sums, radius, step) ? 1 : 0;
		double mcc = 0.0;
		if (RP_UNIFORM(valid))
		{
			mcc = -rp_model_sum(v, step);
			valid = mcc > 0.0 ? 1 : 0;
		}
		if (!RP_UNIFORM(valid))
		{
			numInvalid++;
			radius = radius * 0.5;
			rp_trace(trace, iterations, xCost, radius, 0.0, -1.0);
			if (numInvalid >= o.max_consecutive_invalid)
			{
				termination = 2;
				break;
			}
			continue;
		}
		// the candidate and its cost
		numInvalid = 0;
		double scaled[5];
#pragma unroll
		for (int a = 0; a < 5; ++a)
		{
			scaled[a] = step[a] * scale[a];
		}
		rp_retract(x, e1, e2, scaled, cand);
		evalsCost++;
		double candCost = rp_cost(v, cand);
		if (!rp_finite(candCost))
		{
			candCost = 1.7976931348623157e308;
		}
		const double stepNorm = rp_norm12(x, cand);
		int accepted = 0;
		if (stepNorm <= o.parameter_tolerance * (xNorm + o.parameter_tolerance) || fabs(xCost - candCost) <= o.function_tolerance * xCost)
		{
			termination = 0;
			done = 1;
			rp_trace(trace, iterations, candCost, radius, 0.0, 2.0);
		}
		else
		{
			const double rel = (seCur - candCost) / mcc;
			const double hist = (seRef - candCost) / (seAccRef + mcc);
			const double quality = rel > hist ? rel : hist;
			if (quality > o.min_relative_decrease)
			{
				accepted = 1;
				const double q = 2.0 * quality - 1.0;
				const double den = 1.0 - (q * q) * q;
				radius = radius / (den > 1.0 / 3.0 ? den : 1.0 / 3.0);
				radius = radius < o.max_radius ? radius : o.max_radius;
				decrease = 2.0;
				seCur = candCost;
				seAccCand = seAccCand + mcc;
				seAccRef = seAccRef + mcc;
				if (seCur < seMin)
				{
					seMin = seCur;
					seNonmono = 0;
					seCand = seCur;
					seAccCand = 0.0;
				}
				else
				{
					++seNonmono;
					if (seCur > seCand)
					{
						seCand = seCur;
						seAccCand = 0.0;
					}
				}
				if (seNonmono == maxNonmono)
				{
					seRef = seCand;
					seAccRef = seAccCand;
				}
			}
			else
			{
				radius = radius / decrease;
				decrease = decrease * 2.0;
			}
			rp_trace(trace, iterations, candCost, radius, quality, accepted ? 1.0 : 0.0);
		}
		if (RP_UNIFORM(done))
		{
			break;
		}
		if (!RP_UNIFORM(accepted))
		{
			continue;
		}
#pragma unroll
		for (int i = 0; i < 12; ++i)
		{
			x[i] = cand[i];
		}
		xNorm = rp_norm12(x, nullptr);
		rp_basis(x, e1, e2);
		rp_eval_jac(v, x, e1, e2, scale, sums);
		xCost = 0.5 * sums[20];
		gradMax = 0.0;
#pragma unroll
		for (int a = 0; a < 5; ++a)
		{
			const double g = fabs(sums[15 + a] / scale[a]);
			gradMax = g > gradMax ? g : gradMax;
		}
		evalsJac++;
		lastSuccessful = 1;
		if (RP_UNIFORM(static_cast<int>(!rp_finite(xCost))))
		{
			termination = 2;
			break;
		}
	}
	rp_finish(model, best, summary, trace, traceRows, iterations, evalsCost, evalsJac, termination, initialCost, minCost, iterations + 1);
}

#ifndef EBO_RELPOSE_RULES_ONLY
// one wave per pair.  offsets [n_pairs + 1]: pair p owns correspondences offsets[p] .. offsets[p + 1] - 1 of f1 / f2, and its
// inlier list and its slice of the work memory start at offsets[p] too
__global__ void __launch_bounds__(kRpLanes) k_relpose_refine(const int* __restrict__ offsets, const int* __restrict__ nInliers, const double* f1,
															   const double* f2, const int* idx, double* models, double* work, ebo_solver_opts o,
															   ebo_summary* summaries, double* trace)
{
	const int p = static_cast<int>(blockIdx.x);
	const size_t at = static_cast<size_t>(offsets[p]);
	RpView v;
	v.n = offsets[p + 1] - offsets[p];
	v.m = nInliers[p];
	v.m = v.m < 0 ? 0 : (v.m > v.n ? v.n : v.m);  // the entry has refused such a list; never past the pair's slice
	v.f1 = f1 + 3 * at;
	v.f2 = f2 + 3 * at;
	v.idx = idx + at;
	v.work = work + kRpRowDoubles * at;
	double* tr = trace ? trace + 4 * (static_cast<size_t>(o.max_num_iterations) + 1) * p : nullptr;
	rp_solve(v, o, models + 12 * static_cast<size_t>(p), summaries + p, tr);
}
#endif
