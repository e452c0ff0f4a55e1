// ebo_maptrack.inc — camera pose from events against a map: the six-degree-of-freedom pose that lays a list of world
// points onto an image (in use the blurred event image of a window), by a trust-region Levenberg-Marquardt over a dense,
// image-sampling residual.  One 256-lane workgroup per unit (an image and a start pose), the whole solve in one launch.
// Included inside ebo_kernels.hip's anonymous namespace.  The rules are written out in include/ebo.h ("pose from events
// against a map", E1-E9); tests/maptrack_ref.py restates them in numpy.  Float64, one rounding per operation in the
// association written here: the library is compiled with -ffp-contract=off, so the plain operators below are the rules'
// operations.
//
// The damping, the 6 x 6 Cholesky, the substitutions and the trust region are those of ebo_bundle.inc (B7-B9) for one free
// frame and constant points, RESTATED here and not shared with it: there they are spread over the lanes of a phase and
// read the work tables of a problem, here one lane advances a state of a few dozen doubles in LDS between the sums, and
// k_bundle_adjust's text stays as it is.
//
// A host build (EBO_MAPTRACK_RULES_ONLY, tools/map_track_serial.cpp) runs the lanes of a sum one after the other and
// folds their 256 partial sums in the same pairs.

// The limits, the lane count and the call's constants are csrc/ebo_maptrack.h's, which every build includes before this file.

#ifdef EBO_MAPTRACK_RULES_ONLY
#define MT_FN inline
#define MT_LANE0_BEGIN {
#define MT_LANE0_END }
#define MT_SHARED(x) (x)
constexpr int kMtFoldDoubles = (kMtSums + 1) * kMtLanes;
#else
#define MT_FN __device__ __forceinline__
#define MT_LANE0_BEGIN if (threadIdx.x == 0) {
#define MT_LANE0_END } __syncthreads();
// a read of the shared state that decides where the lanes go next: the barrier keeps lane 0's next writes to the state
// away from lanes that have not read it yet
__device__ __forceinline__ int mt_shared(int x)
{
	const int t = x;
	__syncthreads();
	return t;
}
#define MT_SHARED(x) mt_shared(x)
constexpr int kMtFoldDoubles = (kMtSums + 1) * (kMtLanes / 2);
#endif

struct MtState
{
	int iterations, evalsCost, evalsJac, termination;
	int visStart, visX, visBest, solved;
	double bmax, s;
	double initialCost, xCost, candCost, minCost, radius, decrease, gradMax, xNorm, mcc;
	double seMin, seCur, seRef, seCand, seAccRef, seAccCand;
	int seNonmono, maxNonmono, numInvalid, lastSuccessful;
	int invalid, done, accepted;
};

// what the lanes of a unit share (LDS on the device)
struct MtShared
{
	MtState st;
	double x[12], c[12];  // the current point and the candidate
	double scale[6], step[6];
	double sums[kMtSums + 1];  // E7's sums and the number of visible points at x: the step of every radius is taken from them
	double aux[2];             // a candidate's r r and visible count, or the model's sum
	double fold[kMtFoldDoubles];
};

enum
{
	kMtValue = 0,  // r r and the visible count
	kMtJacobian = 1,  // E7's 28 sums and the visible count
	kMtModel = 2  // B9's model cost change
};

constexpr int mt_ns(int mode)
{
	return mode == kMtJacobian ? kMtSums + 1 : mode == kMtValue ? 2 : 1;
}

MT_FN double mt_dot3(double a0, double a1, double a2, double b0, double b1, double b2)
{
	return (a0 * b0 + a1 * b1) + a2 * b2;
}

MT_FN bool mt_finite(double v)
{
	return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308;
}

// packed lower triangle: entry (i, j), j <= i
constexpr int mt_tri(int i, int j)
{
	return i * (i + 1) / 2 + j;
}

// E2-E5 of one point: the residual and, with WANT_J, the scaled Jacobian row.  Returns whether the point is visible; one
// that is not has r = 1 and a zero row, and nothing of the image is read for it.
template <bool WANT_J>
MT_FN bool mt_point(const MtCall& k, const double* __restrict__ img, double s, const double (&T)[12], const double* __restrict__ X,
					const double* scale, double& r, double (&J)[6])
{
	r = 1.0;
#pragma unroll
	for (int a = 0; a < 6; ++a)
	{
		J[a] = 0.0;
	}
	// a pose is R row-major, then t
	const double d0 = X[0] - T[9], d1 = X[1] - T[10], d2 = X[2] - T[11];
	const double q0 = mt_dot3(T[0], T[3], T[6], d0, d1, d2);
	const double q1 = mt_dot3(T[1], T[4], T[7], d0, d1, d2);
	const double q2 = mt_dot3(T[2], T[5], T[8], d0, d1, d2);
	const double iz = 1.0 / q2;
	const double xP = q0 * iz, yP = q1 * iz;
	const double u = k.fx * xP + k.cx, v = k.fy * yP + k.cy;
	// every test in double before any conversion: all four taps are inside the image, a NaN fails a test
	if (!(q2 > k.z_min && u >= 0.0 && u < static_cast<double>(k.w - 1) && v >= 0.0 && v < static_cast<double>(k.h - 1)))
	{
		return false;
	}
	const double x0 = floor(u), y0 = floor(v);
	const double al = u - x0, be = v - y0, ial = 1.0 - al, ibe = 1.0 - be;
	const double* __restrict__ tap = img + static_cast<size_t>(static_cast<int>(y0)) * k.w + static_cast<int>(x0);
	const double b00 = tap[0], b10 = tap[1], b01 = tap[k.w], b11 = tap[k.w + 1];
	const double b = ibe * (ial * b00 + al * b10) + be * (ial * b01 + al * b11);
	r = 1.0 - s * b;
	if (WANT_J)
	{
		const double Du = ibe * (b10 - b00) + be * (b11 - b01);
		const double Dv = ial * (b01 - b00) + al * (b11 - b10);
		const double au = Du * k.fx, av = Dv * k.fy;
		const double A0 = -(s * (au * iz));
		const double A1 = -(s * (av * iz));
		const double A2 = s * ((au * xP + av * yP) * iz);
		J[0] = (-A0) * scale[0];
		J[1] = (-A1) * scale[1];
		J[2] = (-A2) * scale[2];
		J[3] = (A1 * q2 - A2 * q1) * scale[3];
		J[4] = (A2 * q0 - A0 * q2) * scale[4];
		J[5] = (A0 * q1 - A1 * q0) * scale[5];
	}
	return true;
}

// one lane's partial sums: its points lane, lane + 256, .. in that order from 0
template <int MODE>
MT_FN void mt_lane(const MtCall& k, const double* __restrict__ img, double s, const double* pose, const double* scale, const double* step,
				   int lane, double (&acc)[mt_ns(MODE)])
{
	double T[12], sc[6], st[6];
#pragma unroll
	for (int i = 0; i < 12; ++i)
	{
		T[i] = pose[i];
	}
#pragma unroll
	for (int a = 0; a < 6; ++a)
	{
		sc[a] = scale[a];
		st[a] = step[a];
	}
#pragma unroll
	for (int e = 0; e < mt_ns(MODE); ++e)
	{
		acc[e] = 0.0;
	}
	for (int i = lane; i < k.n_points; i += kMtLanes)
	{
		double r, J[6];
		const bool vis = mt_point<MODE != kMtValue>(k, img, s, T, k.points + 3 * static_cast<size_t>(i), sc, r, J);
		if (MODE == kMtValue)
		{
			acc[0] = acc[0] + r * r;
			acc[1] = acc[1] + (vis ? 1.0 : 0.0);
		}
		else if (MODE == kMtJacobian)
		{
#pragma unroll
			for (int a = 0; a < 6; ++a)
			{
#pragma unroll
				for (int b = 0; b <= a; ++b)
				{
					acc[mt_tri(a, b)] = acc[mt_tri(a, b)] + J[a] * J[b];
				}
				acc[21 + a] = acc[21 + a] + J[a] * r;
			}
			acc[27] = acc[27] + r * r;
			acc[28] = acc[28] + (vis ? 1.0 : 0.0);
		}
		else
		{
			double m = 0.0;
			if (vis)
			{
				double mr = J[0] * st[0] + J[1] * st[1];
				mr = mr + J[2] * st[2];
				mr = mr + J[3] * st[3];
				mr = mr + J[4] * st[4];
				mr = mr + J[5] * st[5];
				m = mr * (r + mr / 2.0);
			}
			acc[0] = acc[0] + m;
		}
	}
}

// B9's tree over the points of every sum of MODE at `pose`, into dst: the lanes' partial sums are the tree's 256,
// folded part[i] = part[i] + part[i + s] for s = 128, 64 (across waves, through LDS) and 32 .. 1 (inside wave 0, by
// shuffles that pair the same lanes).  Ends with the sums visible to every lane.
template <int MODE>
MT_FN void mt_sums(const MtCall& k, const double* __restrict__ img, MtShared& sh, const double* pose, double* dst)
{
	constexpr int NS = mt_ns(MODE);
#ifdef EBO_MAPTRACK_RULES_ONLY
	for (int lane = 0; lane < kMtLanes; ++lane)
	{
		double acc[NS];
		mt_lane<MODE>(k, img, sh.st.s, pose, sh.scale, sh.step, lane, acc);
		for (int e = 0; e < NS; ++e)
		{
			sh.fold[e * kMtLanes + lane] = acc[e];
		}
	}
	for (int e = 0; e < NS; ++e)
	{
		double* part = sh.fold + e * kMtLanes;
		for (int s = kMtLanes / 2; s > 0; s /= 2)
		{
			for (int i = 0; i < s; ++i)
			{
				part[i] = part[i] + part[i + s];
			}
		}
		dst[e] = part[0];
	}
#else
	constexpr int H = kMtLanes / 2;
	const int lane = static_cast<int>(threadIdx.x);
	double acc[NS];
	mt_lane<MODE>(k, img, sh.st.s, pose, sh.scale, sh.step, lane, acc);
	if (lane >= H)
	{
#pragma unroll
		for (int e = 0; e < NS; ++e)
		{
			sh.fold[e * H + (lane - H)] = acc[e];
		}
	}
	__syncthreads();
	if (lane < H)
	{
#pragma unroll
		for (int e = 0; e < NS; ++e)
		{
			acc[e] = acc[e] + sh.fold[e * H + lane];
		}
	}
	__syncthreads();
	if (lane >= 64 && lane < H)
	{
#pragma unroll
		for (int e = 0; e < NS; ++e)
		{
			sh.fold[e * H + (lane - 64)] = acc[e];
		}
	}
	__syncthreads();
	if (lane < 64)
	{
#pragma unroll
		for (int e = 0; e < NS; ++e)
		{
			double a = acc[e] + sh.fold[e * H + lane];
#pragma unroll
			for (int d = 32; d > 0; d /= 2)
			{
				a = a + __shfl_down(a, d, 64);
			}
			if (lane == 0)
			{
				dst[e] = a;
			}
		}
	}
	__syncthreads();
#endif
}

// E1: the largest pixel that is > 0, 0 when there is none; a NaN is never taken, so the order does not matter
MT_FN void mt_image_max(const MtCall& k, const double* __restrict__ img, MtShared& sh)
{
	const int np = k.w * k.h;
#ifdef EBO_MAPTRACK_RULES_ONLY
	double m = 0.0;
	for (int i = 0; i < np; ++i)
	{
		m = img[i] > m ? img[i] : m;
	}
	sh.st.bmax = m;
#else
	const int lane = static_cast<int>(threadIdx.x);
	double m = 0.0;
	for (int i = lane; i < np; i += kMtLanes)
	{
		const double v = img[i];
		m = v > m ? v : m;
	}
#pragma unroll
	for (int d = 32; d > 0; d /= 2)
	{
		const double t = __shfl_down(m, d, 64);
		m = t > m ? t : m;
	}
	if (lane % 64 == 0)
	{
		sh.fold[lane / 64] = m;
	}
	__syncthreads();
	if (lane == 0)
	{
#pragma unroll
		for (int w = 1; w < kMtLanes / 64; ++w)
		{
			m = sh.fold[w] > m ? sh.fold[w] : m;
		}
		sh.st.bmax = m;
	}
	__syncthreads();
#endif
}

// B4: T <- T * retract(ups, om)
MT_FN void mt_retract(const double* T, const double (&ups)[3], const double (&om)[3], double* out)
{
	const double hx = om[0] * 0.5, hy = om[1] * 0.5, hz = om[2] * 0.5;
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
			out[3 * i + j] = mt_dot3(T[3 * i], T[3 * i + 1], T[3 * i + 2], C[0][j], C[1][j], C[2][j]);
		}
		out[9 + i] = T[9 + i] + mt_dot3(T[3 * i], T[3 * i + 1], T[3 * i + 2], ups[0], ups[1], ups[2]);
	}
}

// B9's tree of 12 entries: partial i = 0 + v[i], the folds 128 .. 16 add zeros, then 8, 4, 2, 1
MT_FN double mt_tree12(const double (&v)[12])
{
	double p[16];
#pragma unroll
	for (int i = 0; i < 16; ++i)
	{
		p[i] = i < 12 ? 0.0 + v[i] : 0.0;
	}
#pragma unroll
	for (int s = 8; s > 0; s /= 2)
	{
#pragma unroll
		for (int i = 0; i < s; ++i)
		{
			p[i] = p[i] + p[i + s];
		}
	}
	return p[0];
}

// |a - b| over the 12 pose entries (b == null: |a|)
MT_FN double mt_norm(const double* a, const double* b)
{
	double v[12];
#pragma unroll
	for (int i = 0; i < 12; ++i)
	{
		const double d = b ? a[i] - b[i] : a[i];
		v[i] = d * d;
	}
	return sqrt(mt_tree12(v));
}

MT_FN double mt_damp(const ebo_solver_opts& o, double diag, double radius)
{
	double d = diag > o.min_lm_diagonal ? diag : o.min_lm_diagonal;
	d = d < o.max_lm_diagonal ? d : o.max_lm_diagonal;
	const double l = sqrt(d / radius);
	return l * l;
}

// B7, B8 for the one 6 x 6 block: damping, Cholesky by columns, the two substitutions, step = minus the solution.
// Returns false for an invalid step.
MT_FN bool mt_step(const ebo_solver_opts& o, const double* sums, double radius, double* step)
{
	double S[21], vec[6], sol[6];
#pragma unroll
	for (int e = 0; e < 21; ++e)
	{
		S[e] = sums[e];
	}
#pragma unroll
	for (int a = 0; a < 6; ++a)
	{
		S[mt_tri(a, a)] = S[mt_tri(a, a)] + mt_damp(o, S[mt_tri(a, a)], radius);
		vec[a] = sums[21 + a];
	}
	bool ok = true;
#pragma unroll
	for (int c = 0; c < 6; ++c)
	{
		const double d = S[mt_tri(c, c)];
		if (ok && d > 0.0 && mt_finite(d))
		{
			S[mt_tri(c, c)] = sqrt(d);
#pragma unroll
			for (int i = c + 1; i < 6; ++i)
			{
				S[mt_tri(i, c)] = S[mt_tri(i, c)] / S[mt_tri(c, c)];
			}
#pragma unroll
			for (int i = c + 1; i < 6; ++i)
			{
#pragma unroll
				for (int j = c + 1; j <= i; ++j)
				{
					S[mt_tri(i, j)] = S[mt_tri(i, j)] - S[mt_tri(i, c)] * S[mt_tri(j, c)];
				}
			}
		}
		else
		{
			ok = false;
		}
	}
	if (!ok)
	{
		return false;
	}
#pragma unroll
	for (int c = 0; c < 6; ++c)
	{
		const double y = vec[c] / S[mt_tri(c, c)];
#pragma unroll
		for (int i = c + 1; i < 6; ++i)
		{
			vec[i] = vec[i] - S[mt_tri(i, c)] * y;
		}
		sol[c] = y;
	}
#pragma unroll
	for (int c = 5; c >= 0; --c)
	{
		const double x = sol[c] / S[mt_tri(c, c)];
#pragma unroll
		for (int i = 0; i < c; ++i)
		{
			sol[i] = sol[i] - S[mt_tri(c, i)] * x;
		}
		vec[c] = x;
	}
#pragma unroll
	for (int a = 0; a < 6; ++a)
	{
		step[a] = -vec[a];
		ok = ok && mt_finite(step[a]);
	}
	return ok;
}

MT_FN void mt_trace(double* trace, int row, double cost, double radius, double quality, double flag)
{
	if (trace)
	{
		double* t = trace + 4 * static_cast<size_t>(row);
		t[0] = cost;
		t[1] = radius;
		t[2] = quality;
		t[3] = flag;
	}
}

// lane 0 after a Jacobian evaluation at x: the cost, the visible count and B9's gradient norm
MT_FN void mt_take_jacobian(MtShared& sh)
{
	MtState& st = sh.st;
	st.xCost = 0.5 * sh.sums[27];
	st.visX = static_cast<int>(sh.sums[28]);
	double g = 0.0;
#pragma unroll
	for (int a = 0; a < 6; ++a)
	{
		const double t = fabs(sh.sums[21 + a] / sh.scale[a]);
		g = t > g ? t : g;
	}
	st.gradMax = g;
}

// E1-E9: the whole solve of one unit.  image < 0 or >= n_images: the unit is not solved (only the _device form can get
// there).  outPose: in the start, out the lowest-cost point visited.
MT_FN void mt_solve(const MtCall& k, int image, double* outPose, const ebo_solver_opts& o, MtShared& sh, double* trace)
{
	MtState& st = sh.st;
	const bool imageOk = image >= 0 && image < k.n_images;
	const double* __restrict__ img = k.images + static_cast<size_t>(imageOk ? image : 0) * k.w * k.h;
#ifdef EBO_MAPTRACK_RULES_ONLY
	if (trace)
	{
		for (size_t i = 0; i < 4 * (static_cast<size_t>(o.max_num_iterations) + 1); ++i)
		{
			trace[i] = 0.0;
		}
	}
#else
	if (trace)
	{
		for (size_t i = threadIdx.x; i < 4 * (static_cast<size_t>(o.max_num_iterations) + 1); i += kMtLanes)
		{
			trace[i] = 0.0;
		}
	}
#endif
	MT_LANE0_BEGIN
	st = MtState{};
	st.termination = 2;
	st.radius = o.initial_radius;
	st.decrease = 2.0;
	st.maxNonmono = o.use_nonmonotonic ? o.max_consecutive_nonmonotonic : 0;
	for (int i = 0; i < 12; ++i)
	{
		sh.x[i] = outPose[i];
		sh.c[i] = outPose[i];
	}
	for (int a = 0; a < 6; ++a)
	{
		sh.scale[a] = 1.0;
		sh.step[a] = 0.0;
	}
	MT_LANE0_END
	if (!imageOk)
	{
		return;
	}
	mt_image_max(k, img, sh);
	MT_LANE0_BEGIN
	if (st.bmax > 0.0 && mt_finite(st.bmax))
	{
		st.s = 1.0 / st.bmax;
		st.solved = 1;
	}
	MT_LANE0_END
	if (!MT_SHARED(st.solved))
	{
		return;
	}
	mt_sums<kMtJacobian>(k, img, sh, sh.x, sh.sums);
	MT_LANE0_BEGIN
	mt_take_jacobian(sh);
	st.termination = 1;
	st.evalsJac = 1;
	st.visStart = st.visBest = st.visX;
	st.initialCost = st.minCost = st.xCost;
	mt_trace(trace, 0, st.xCost, st.radius, 0.0, 1.0);
	if (!mt_finite(st.xCost))
	{
		st.termination = 2;
		st.done = 1;
	}
	else if (o.jacobi_scaling)
	{
		// B6: from the column norms of the first Jacobian, which the sums with scale 1 left on the diagonal
		for (int a = 0; a < 6; ++a)
		{
			sh.scale[a] = 1.0 / (1.0 + sqrt(sh.sums[mt_tri(a, a)]));
		}
	}
	MT_LANE0_END
	if (MT_SHARED(st.done))
	{
		return;
	}
	if (o.jacobi_scaling)
	{
		mt_sums<kMtJacobian>(k, img, sh, sh.x, sh.sums);
	}
	MT_LANE0_BEGIN
	mt_take_jacobian(sh);
	st.xNorm = mt_norm(sh.x, nullptr);
	st.seMin = st.seCur = st.seRef = st.seCand = st.xCost;
	st.lastSuccessful = 1;
	MT_LANE0_END

	for (;;)
	{
		MT_LANE0_BEGIN
		if (st.lastSuccessful && st.xCost < st.minCost)
		{
			st.minCost = st.xCost;
			st.visBest = st.visX;
			for (int i = 0; i < 12; ++i)
			{
				outPose[i] = sh.x[i];
			}
		}
		if (st.iterations >= o.max_num_iterations)
		{
			st.termination = 1;
			st.done = 1;
		}
		else if (st.lastSuccessful && st.gradMax <= o.gradient_tolerance)
		{
			st.termination = 0;
			st.done = 1;
		}
		else if (st.radius < o.min_radius)
		{
			st.termination = 0;
			st.done = 1;
		}
		else
		{
			st.iterations++;
			st.lastSuccessful = 0;
			st.invalid = mt_step(o, sh.sums, st.radius, sh.step) ? 0 : 1;
		}
		MT_LANE0_END
		// one read of both flags behind one barrier
		const int top = MT_SHARED(st.done | (st.invalid << 1));
		if (top & 1)
		{
			break;
		}
		if (!(top & 2))
		{
			mt_sums<kMtModel>(k, img, sh, sh.x, sh.aux);
			MT_LANE0_BEGIN
			st.mcc = -sh.aux[0];
			if (!(st.mcc > 0.0))
			{
				st.invalid = 1;
			}
			MT_LANE0_END
		}
		if (MT_SHARED(st.invalid))
		{
			MT_LANE0_BEGIN
			st.numInvalid++;
			if (st.numInvalid >= o.max_consecutive_invalid)
			{
				st.termination = 2;
				st.done = 1;
			}
			st.radius = st.radius * 0.5;
			mt_trace(trace, st.iterations, st.xCost, st.radius, 0.0, -1.0);
			MT_LANE0_END
			if (MT_SHARED(st.done))
			{
				break;
			}
			continue;
		}
		// the candidate and its cost
		MT_LANE0_BEGIN
		double ups[3], om[3];
		for (int a = 0; a < 3; ++a)
		{
			ups[a] = sh.step[a] * sh.scale[a];
			om[a] = sh.step[3 + a] * sh.scale[3 + a];
		}
		mt_retract(sh.x, ups, om, sh.c);
		MT_LANE0_END
		mt_sums<kMtValue>(k, img, sh, sh.c, sh.aux);
		MT_LANE0_BEGIN
		st.numInvalid = 0;
		st.evalsCost++;
		st.candCost = 0.5 * sh.aux[0];
		const int visC = static_cast<int>(sh.aux[1]);
		if (!mt_finite(st.candCost))
		{
			st.candCost = 1.7976931348623157e308;
		}
		const double stepNorm = mt_norm(sh.x, sh.c);
		st.accepted = 0;
		if (stepNorm <= o.parameter_tolerance * (st.xNorm + o.parameter_tolerance) ||
			fabs(st.xCost - st.candCost) <= o.function_tolerance * st.xCost)
		{
			st.termination = 0;
			st.done = 1;
			mt_trace(trace, st.iterations, st.candCost, st.radius, 0.0, 2.0);
		}
		else
		{
			const double rel = (st.seCur - st.candCost) / st.mcc;
			const double hist = (st.seRef - st.candCost) / (st.seAccRef + st.mcc);
			const double quality = rel > hist ? rel : hist;
			if (quality > o.min_relative_decrease)
			{
				st.accepted = 1;
				const double q = 2.0 * quality - 1.0;
				const double den = 1.0 - (q * q) * q;
				st.radius = st.radius / (den > 1.0 / 3.0 ? den : 1.0 / 3.0);
				st.radius = st.radius < o.max_radius ? st.radius : o.max_radius;
				st.decrease = 2.0;
				st.seCur = st.candCost;
				st.seAccCand = st.seAccCand + st.mcc;
				st.seAccRef = st.seAccRef + st.mcc;
				if (st.seCur < st.seMin)
				{
					st.seMin = st.seCur;
					st.seNonmono = 0;
					st.seCand = st.seCur;
					st.seAccCand = 0.0;
				}
				else
				{
					++st.seNonmono;
					if (st.seCur > st.seCand)
					{
						st.seCand = st.seCur;
						st.seAccCand = 0.0;
					}
				}
				if (st.seNonmono == st.maxNonmono)
				{
					st.seRef = st.seCand;
					st.seAccRef = st.seAccCand;
				}
				for (int i = 0; i < 12; ++i)
				{
					sh.x[i] = sh.c[i];
				}
				st.xNorm = mt_norm(sh.x, nullptr);
				st.visX = visC;
			}
			else
			{
				st.radius = st.radius / st.decrease;
				st.decrease = st.decrease * 2.0;
			}
			mt_trace(trace, st.iterations, st.candCost, st.radius, quality, st.accepted ? 1.0 : 0.0);
		}
		MT_LANE0_END
		const int after = MT_SHARED(st.done | (st.accepted << 1));
		if (after & 1)
		{
			break;
		}
		if (!(after & 2))
		{
			continue;
		}
		// at x, which the taken step has moved: cost, sums and gradient norm
		mt_sums<kMtJacobian>(k, img, sh, sh.x, sh.sums);
		MT_LANE0_BEGIN
		mt_take_jacobian(sh);
		st.evalsJac++;
		st.lastSuccessful = 1;
		if (!mt_finite(st.xCost))
		{
			st.termination = 2;
			st.done = 1;
		}
		MT_LANE0_END
		if (MT_SHARED(st.done))
		{
			break;
		}
	}
}

MT_FN void mt_result(const MtState& st, ebo_map_track_result& r)
{
	r.termination = st.termination;
	r.iterations = st.iterations;
	r.num_evals_jac = st.evalsJac;
	r.num_evals_cost = st.evalsCost;
	r.visible_start = st.visStart;
	r.visible_final = st.visBest;
	r.reserved0 = 0;
	r.reserved1 = 0;
	r.initial_cost = st.initialCost;
	r.final_cost = st.minCost;
	r.scale = st.s;
	r.reserved2 = 0.0;
}

#ifndef EBO_MAPTRACK_RULES_ONLY
__global__ void __launch_bounds__(kMtLanes) k_map_track(MtCall k, const int* __restrict__ unit_image, double* poses, ebo_solver_opts o,
													   ebo_map_track_result* results, double* trace)
{
	__shared__ MtShared sh;
	const int u = static_cast<int>(blockIdx.x);
	double* tr = trace ? trace + 4 * (static_cast<size_t>(o.max_num_iterations) + 1) * u : nullptr;
	mt_solve(k, unit_image[u], poses + 12 * static_cast<size_t>(u), o, sh, tr);
	__syncthreads();
	if (threadIdx.x == 0)
	{
		ebo_map_track_result r;
		mt_result(sh.st, r);
		results[u] = r;
	}
}
#endif
