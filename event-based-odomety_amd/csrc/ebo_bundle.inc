// ebo_bundle.inc — windowed bundle adjustment on the device: a trust-region Levenberg-Marquardt over camera poses and
// landmarks whose normal equations are reduced by the Schur complement, one 256-lane workgroup per problem, the whole
// solve in one launch.  Replaces what VisualOdometryFrontEnd::optimize (visual_odometry.cpp:416-497) does through
// Ceres, and with the points held constant the refinement after localizeCamera's RANSAC (:262).  Included inside
// ebo_kernels.hip's anonymous namespace.  The rules are written out in include/ebo.h ("bundle adjustment", B1-B9);
// tests/bundle_ref.py restates them in numpy.  Float64, one rounding per operation in the association written here:
// the library is compiled with -ffp-contract=off, so the plain operators below are the rules' operations.
//
// The text between the two lane macros is one PHASE: on the device every lane runs it once and a barrier follows; a
// host build (EBO_BUNDLE_RULES_ONLY, tools/bundle_adjust_serial.cpp) runs the lanes one after the other.  Control flow
// between phases reads only the shared state, so it is uniform and every barrier is reached by every lane.

// The limits, the lane count and the work sizes are csrc/ebo_bundle.h's, which every build includes before this file.

#ifdef EBO_BUNDLE_RULES_ONLY
#define BA_FN inline
#define BA_LANES_BEGIN for (int lane = 0; lane < kBaLanes; ++lane) {
#define BA_LANES_END }
#define BA_SHARED(x) (x)
#else
#define BA_FN __device__ __forceinline__
#define BA_LANES_BEGIN { const int lane = static_cast<int>(threadIdx.x);
#define BA_LANES_END } __syncthreads();
// a read of the shared state that decides where the lanes go next: the barrier keeps the next phase's writes to the
// state away from lanes that have not read it yet
template <class T>
__device__ __forceinline__ T ba_shared(const T& x)
{
	const T t = x;
	__syncthreads();
	return t;
}
#define BA_SHARED(x) ba_shared(x)
#endif

// one problem: the caller's arrays and the problem's slices of the work tables
struct BaView
{
	int F, P, N, fixPoints;
	const unsigned char* fixed;  // [F]
	const int* of;               // [N] frame of an observation
	const int* op;               // [N] point of an observation
	const double* uv;            // [N][2]
	double* outPose;             // [F][12] in: start, out: the best point
	double* outPt;               // [P][3]
	double* xPose;               // current point
	double* xPt;
	double* cPose;               // candidate
	double* cPt;
	int* table;                  // [P][F] observation of (point, frame) or -1
	int* pstart;                 // [P + 1]
	int* fslot;                  // [F] index among the free frames or -1
	int* flist;                  // [F] frame of a free slot
	double* res;                 // [N][2] corrected residual at the current point
	double* Jc;                  // [N][2][6]
	double* Jp;                  // [N][2][3]
	double* W;                   // [N][6][3]
	double* Y;                   // [N][6][3]
	double* U;                   // [F][42] = U_k [6][6], g_k [6]
	double* V;                   // [P][12] = V_l [3][3], g_l [3]
	double* Vinv;                // [P][9]
	double* scale;               // [6 F + 3 P]
	double* step;                // [6 F + 3 P]
	double* red;                 // [max(N, 12 F + 3 P)] values on their way into a tree
};

struct BaState
{
	int iterations, evalsCost, evalsJac, termination;
	double initialCost, xCost, candCost, minCost, radius, decrease, gradMax, xNorm, mcc;
	double seMin, seCur, seRef, seCand, seAccRef, seAccCand;
	int seNonmono, maxNonmono, numInvalid, lastSuccessful;
	int invalid, bad, done, copyBest, accepted, nFree, dim;
};

BA_FN double ba_dot3(double a0, double a1, double a2, double b0, double b1, double b2)
{
	return (a0 * b0 + a1 * b1) + a2 * b2;
}

BA_FN bool ba_finite(double v)
{
	return v >= -1.7976931348623157e308 && v <= 1.7976931348623157e308;
}

// B1-B3: residual, rho and, with wantJac, A = sqrt(rho') d(project)/dq, q and sqrt(rho') of one observation
BA_FN void ba_observe(const ebo_camera& c, const double (&T)[12], const double (&X)[3], double u, double v, double huber, bool wantJac,
					  double (&r)[2], double& rho, double (&A)[2][3], double (&q)[3])
{
	const double d0 = X[0] - T[3], d1 = X[1] - T[7], d2 = X[2] - T[11];
#pragma unroll
	for (int j = 0; j < 3; ++j)
	{
		q[j] = ba_dot3(T[j], T[4 + j], T[8 + j], d0, d1, d2);
	}
	const double xP = q[0] / q[2], yP = q[1] / q[2];
	const double r2 = xP * xP + yP * yP;
	const double rad = (1.0 + c.k1 * r2) + (c.k2 * r2) * r2;
	const double tx = ((2.0 * c.p1) * xP) * yP + c.p2 * (r2 + (2.0 * xP) * xP);
	const double ty = ((2.0 * c.p2) * yP) * xP + c.p1 * (r2 + (2.0 * yP) * yP);
	const double xD = xP * rad + tx, yD = yP * rad + ty;
	r[0] = u - (c.fx * xD + c.cx);
	r[1] = v - (c.fy * yD + c.cy);
	const double s = r[0] * r[0] + r[1] * r[1];
	const double b = huber * huber;
	double rho1 = 1.0;
	rho = s;
	if (s > b)
	{
		const double root = sqrt(s);
		rho = (2.0 * huber) * root - b;
		rho1 = huber / root;
		rho1 = rho1 > 2.2250738585072014e-308 ? rho1 : 2.2250738585072014e-308;
	}
	if (!wantJac)
	{
		return;
	}
	const double sr = sqrt(rho1);
	r[0] = r[0] * sr;
	r[1] = r[1] * sr;
	const double dr = c.k1 + (2.0 * c.k2) * r2;
	const double xx2 = (2.0 * xP) * xP, yy2 = (2.0 * yP) * yP, xy2 = (2.0 * xP) * yP;
	const double dxx = ((rad + xx2 * dr) + (2.0 * c.p1) * yP) + (6.0 * c.p2) * xP;
	const double dxy = (xy2 * dr + (2.0 * c.p1) * xP) + (2.0 * c.p2) * yP;
	const double dyy = ((rad + yy2 * dr) + (2.0 * c.p2) * xP) + (6.0 * c.p1) * yP;
	const double iz = 1.0 / q[2];
	A[0][0] = (c.fx * (dxx * iz)) * sr;
	A[0][1] = (c.fx * (dxy * iz)) * sr;
	A[0][2] = (c.fx * (-((dxx * xP + dxy * yP) * iz))) * sr;
	A[1][0] = (c.fy * (dxy * iz)) * sr;
	A[1][1] = (c.fy * (dyy * iz)) * sr;
	A[1][2] = (c.fy * (-((dxy * xP + dyy * yP) * iz))) * sr;
}

// B4: T <- T * retract(ups, om)
BA_FN void ba_retract(const double (&T)[12], const double (&ups)[3], const double (&om)[3], double (&out)[12])
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
			out[4 * i + j] = ba_dot3(T[4 * i], T[4 * i + 1], T[4 * i + 2], C[0][j], C[1][j], C[2][j]);
		}
		out[4 * i + 3] = T[4 * i + 3] + ba_dot3(T[4 * i], T[4 * i + 1], T[4 * i + 2], ups[0], ups[1], ups[2]);
	}
}

BA_FN bool ba_point_active(const BaView& v, int l)
{
	return v.fixPoints || v.pstart[l + 1] - v.pstart[l] >= 2;
}

// packed lower triangle: entry (i, j), j <= i
BA_FN int ba_tri(int i, int j)
{
	return i * (i + 1) / 2 + j;
}

// ---- phases (one lane's share of each) ---------------------------------------------------------------------------

BA_FN void ba_ph_clear(const BaView& v, double* trace, int traceRows, int lane)
{
	for (int i = lane; i < v.P * v.F; i += kBaLanes)
	{
		v.table[i] = -1;
	}
	for (int i = lane; i < 12 * v.F; i += kBaLanes)
	{
		v.xPose[i] = v.outPose[i];
	}
	for (int i = lane; i < 3 * v.P; i += kBaLanes)
	{
		v.xPt[i] = v.outPt[i];
	}
	if (trace)
	{
		for (int i = lane; i < 4 * traceRows; i += kBaLanes)
		{
			trace[i] = 0.0;
		}
	}
}

// the observation table and the check of what the host entry guarantees: indices in range, (point, frame) ascending
BA_FN void ba_ph_table(const BaView& v, BaState& st, int lane)
{
	for (int i = lane; i < v.N; i += kBaLanes)
	{
		const int f = v.of[i], l = v.op[i];
		bool ok = f >= 0 && f < v.F && l >= 0 && l < v.P;
		if (i > 0)
		{
			const long long k0 = static_cast<long long>(v.op[i - 1]) * v.F + v.of[i - 1], k1 = static_cast<long long>(l) * v.F + f;
			ok = ok && k0 < k1;
		}
		if (ok)
		{
			v.table[l * v.F + f] = i;
		}
		else
		{
			st.bad = 1;
		}
	}
	for (int l = lane; l <= v.P; l += kBaLanes)
	{
		int lo = 0, hi = v.N;  // first observation whose point is >= l
		while (lo < hi)
		{
			const int mid = (lo + hi) / 2;
			if (v.op[mid] < l)
			{
				lo = mid + 1;
			}
			else
			{
				hi = mid;
			}
		}
		v.pstart[l] = lo;
	}
	for (int c = lane; c < 6 * v.F + 3 * v.P; c += kBaLanes)
	{
		v.scale[c] = 1.0;
	}
}

BA_FN void ba_load_pose(const double* p, double (&T)[12])
{
#pragma unroll
	for (int i = 0; i < 12; ++i)
	{
		T[i] = p[i];
	}
}

// B1-B3 for every observation at (pose, pt): rho into the tree's input, and with wantJac the corrected residual and the
// scaled Jacobian blocks
BA_FN void ba_ph_observe(const BaView& v, const ebo_camera& cam, double huber, const double* pose, const double* pt, bool wantJac, int lane)
{
	for (int i = lane; i < v.N; i += kBaLanes)
	{
		const int f = v.of[i], l = v.op[i];
		if (!ba_point_active(v, l))
		{
			v.red[i] = 0.0;
			continue;
		}
		double T[12], r[2], rho, A[2][3], q[3];
		ba_load_pose(pose + 12 * f, T);
		const double X[3] = {pt[3 * l], pt[3 * l + 1], pt[3 * l + 2]};
		ba_observe(cam, T, X, v.uv[2 * i], v.uv[2 * i + 1], huber, wantJac, r, rho, A, q);
		v.red[i] = rho;
		if (!wantJac)
		{
			continue;
		}
		v.res[2 * i] = r[0];
		v.res[2 * i + 1] = r[1];
		const bool freeFrame = v.fslot[f] >= 0;
		double jc[2][6], jp[2][3];
#pragma unroll
		for (int k = 0; k < 2; ++k)
		{
			jc[k][0] = A[k][0];
			jc[k][1] = A[k][1];
			jc[k][2] = A[k][2];
			jc[k][3] = A[k][2] * q[1] - A[k][1] * q[2];
			jc[k][4] = A[k][0] * q[2] - A[k][2] * q[0];
			jc[k][5] = A[k][1] * q[0] - A[k][0] * q[1];
#pragma unroll
			for (int j = 0; j < 3; ++j)
			{
				jp[k][j] = -ba_dot3(A[k][0], A[k][1], A[k][2], T[4 * j], T[4 * j + 1], T[4 * j + 2]);
			}
		}
		if (freeFrame)
		{
#pragma unroll
			for (int k = 0; k < 2; ++k)
			{
#pragma unroll
				for (int a = 0; a < 6; ++a)
				{
					jc[k][a] = jc[k][a] * v.scale[6 * f + a];
					v.Jc[12 * static_cast<size_t>(i) + 6 * k + a] = jc[k][a];
				}
			}
		}
		if (!v.fixPoints)
		{
#pragma unroll
			for (int k = 0; k < 2; ++k)
			{
#pragma unroll
				for (int b = 0; b < 3; ++b)
				{
					jp[k][b] = jp[k][b] * v.scale[6 * v.F + 3 * l + b];
					v.Jp[6 * static_cast<size_t>(i) + 3 * k + b] = jp[k][b];
				}
			}
		}
		if (freeFrame && !v.fixPoints)
		{
#pragma unroll
			for (int a = 0; a < 6; ++a)
			{
#pragma unroll
				for (int b = 0; b < 3; ++b)
				{
					v.W[18 * static_cast<size_t>(i) + 3 * a + b] = jc[0][a] * jp[0][b] + jc[1][a] * jp[1][b];
				}
			}
		}
	}
}

// B5: U_k, g_k over a frame's observations in ascending point order; V_l, g_l over a point's in ascending frame order
BA_FN void ba_ph_sums(const BaView& v, int lane)
{
	for (int e = lane; e < 42 * v.F; e += kBaLanes)
	{
		const int k = e / 42, c = e % 42;
		if (v.fslot[k] < 0)
		{
			continue;
		}
		const int a = c < 36 ? c / 6 : c - 36, b = c % 6;
		double acc = 0.0;
		for (int l = 0; l < v.P; ++l)
		{
			const int o = v.table[l * v.F + k];
			if (o < 0 || !ba_point_active(v, l))
			{
				continue;
			}
			const double* J = v.Jc + 12 * static_cast<size_t>(o);
			if (c < 36)
			{
				acc = acc + (J[a] * J[b] + J[6 + a] * J[6 + b]);
			}
			else
			{
				acc = acc + (J[a] * v.res[2 * o] + J[6 + a] * v.res[2 * o + 1]);
			}
		}
		v.U[e] = acc;
	}
	if (v.fixPoints)
	{
		return;
	}
	for (int e = lane; e < 12 * v.P; e += kBaLanes)
	{
		const int l = e / 12, c = e % 12;
		if (!ba_point_active(v, l))
		{
			continue;
		}
		const int a = c < 9 ? c / 3 : c - 9, b = c % 3;
		double acc = 0.0;
		for (int o = v.pstart[l]; o < v.pstart[l + 1]; ++o)
		{
			const double* J = v.Jp + 6 * static_cast<size_t>(o);
			if (c < 9)
			{
				acc = acc + (J[a] * J[b] + J[3 + a] * J[3 + b]);
			}
			else
			{
				acc = acc + (J[a] * v.res[2 * o] + J[3 + a] * v.res[2 * o + 1]);
			}
		}
		v.V[e] = acc;
	}
}

// is parameter c (6 per frame, then 3 per point) a variable of the problem
BA_FN bool ba_param_free(const BaView& v, int c)
{
	if (c < 6 * v.F)
	{
		return v.fslot[c / 6] >= 0;
	}
	return !v.fixPoints && ba_point_active(v, (c - 6 * v.F) / 3);
}

BA_FN double ba_param_diag(const BaView& v, int c)
{
	if (c < 6 * v.F)
	{
		return v.U[42 * (c / 6) + 7 * (c % 6)];
	}
	const int d = c - 6 * v.F;
	return v.V[12 * (d / 3) + 4 * (d % 3)];
}

BA_FN double ba_param_grad(const BaView& v, int c)
{
	if (c < 6 * v.F)
	{
		return v.U[42 * (c / 6) + 36 + c % 6];
	}
	const int d = c - 6 * v.F;
	return v.V[12 * (d / 3) + 9 + d % 3];
}

// B6: Jacobi scaling from the column norms of the first Jacobian, which the sums with scale 1 left on the diagonals
BA_FN void ba_ph_scale(const BaView& v, int lane)
{
	for (int c = lane; c < 6 * v.F + 3 * v.P; c += kBaLanes)
	{
		if (ba_param_free(v, c))
		{
			v.scale[c] = 1.0 / (1.0 + sqrt(ba_param_diag(v, c)));
		}
	}
}

BA_FN void ba_ph_grad(const BaView& v, int lane)
{
	for (int c = lane; c < 6 * v.F + 3 * v.P; c += kBaLanes)
	{
		v.red[c] = ba_param_free(v, c) ? fabs(ba_param_grad(v, c) / v.scale[c]) : 0.0;
	}
}

BA_FN double ba_damp(const ebo_solver_opts& o, double diag, double radius)
{
	double d = diag > o.min_lm_diagonal ? diag : o.min_lm_diagonal;
	d = d < o.max_lm_diagonal ? d : o.max_lm_diagonal;
	const double l = sqrt(d / radius);
	return l * l;
}

// B7: the damped point blocks inverted by cofactors
BA_FN void ba_ph_points(const BaView& v, BaState& st, const ebo_solver_opts& o, int lane)
{
	for (int l = lane; l < v.P; l += kBaLanes)
	{
		if (!ba_point_active(v, l))
		{
			continue;
		}
		double M[3][3], C[3][3];
#pragma unroll
		for (int i = 0; i < 3; ++i)
		{
#pragma unroll
			for (int j = 0; j < 3; ++j)
			{
				M[i][j] = v.V[12 * l + 3 * i + j];
			}
		}
#pragma unroll
		for (int i = 0; i < 3; ++i)
		{
			M[i][i] = M[i][i] + ba_damp(o, M[i][i], st.radius);
		}
#pragma unroll
		for (int i = 0; i < 3; ++i)
		{
#pragma unroll
			for (int j = 0; j < 3; ++j)
			{
				C[i][j] = M[(i + 1) % 3][(j + 1) % 3] * M[(i + 2) % 3][(j + 2) % 3] - M[(i + 1) % 3][(j + 2) % 3] * M[(i + 2) % 3][(j + 1) % 3];
			}
		}
		const double det = ba_dot3(M[0][0], M[0][1], M[0][2], C[0][0], C[0][1], C[0][2]);
		if (!(det > 0.0))
		{
			st.invalid = 1;
		}
#pragma unroll
		for (int i = 0; i < 3; ++i)
		{
#pragma unroll
			for (int j = 0; j < 3; ++j)
			{
				v.Vinv[9 * l + 3 * i + j] = C[j][i] / det;
			}
		}
	}
}

// Y = W V^-1 for every observation of a free frame
BA_FN void ba_ph_y(const BaView& v, int lane)
{
	for (int e = lane; e < 6 * v.N; e += kBaLanes)
	{
		const int i = e / 6, a = e % 6;
		const int l = v.op[i];
		if (v.fslot[v.of[i]] < 0 || !ba_point_active(v, l))
		{
			continue;
		}
		const double* w = v.W + 18 * static_cast<size_t>(i) + 3 * a;
		const double* iv = v.Vinv + 9 * l;
#pragma unroll
		for (int b = 0; b < 3; ++b)
		{
			v.Y[18 * static_cast<size_t>(i) + 3 * a + b] = ba_dot3(w[0], w[1], w[2], iv[b], iv[3 + b], iv[6 + b]);
		}
	}
}

// B8: the reduced system, one lane per entry of the packed lower triangle, and its right-hand side
BA_FN void ba_ph_schur(const BaView& v, const BaState& st, const ebo_solver_opts& o, double* S, double* vec, int lane)
{
	const int n = st.dim;
	for (int i = lane / 16; i < n; i += 16)
	{
		const int fi = v.flist[i / 6], a = i % 6;
		for (int j = lane % 16; j <= i; j += 16)
		{
			const int fj = v.flist[j / 6], b = j % 6;
			double acc = 0.0;
			if (fi == fj)
			{
				acc = v.U[42 * fi + 6 * a + b];
				if (a == b)
				{
					acc = acc + ba_damp(o, acc, st.radius);
				}
			}
			if (!v.fixPoints)
			{
				for (int l = 0; l < v.P; ++l)
				{
					const int oi = v.table[l * v.F + fi], oj = v.table[l * v.F + fj];
					if (oi < 0 || oj < 0 || !ba_point_active(v, l))
					{
						continue;
					}
					const double* y = v.Y + 18 * static_cast<size_t>(oi) + 3 * a;
					const double* w = v.W + 18 * static_cast<size_t>(oj) + 3 * b;
					acc = acc - ba_dot3(y[0], y[1], y[2], w[0], w[1], w[2]);
				}
			}
			S[ba_tri(i, j)] = acc;
		}
	}
	for (int i = lane; i < n; i += kBaLanes)
	{
		const int fi = v.flist[i / 6], a = i % 6;
		double acc = v.U[42 * fi + 36 + a];
		if (!v.fixPoints)
		{
			for (int l = 0; l < v.P; ++l)
			{
				const int oi = v.table[l * v.F + fi];
				if (oi < 0 || !ba_point_active(v, l))
				{
					continue;
				}
				const double* y = v.Y + 18 * static_cast<size_t>(oi) + 3 * a;
				const double* g = v.V + 12 * l + 9;
				acc = acc - ba_dot3(y[0], y[1], y[2], g[0], g[1], g[2]);
			}
		}
		vec[i] = acc;
	}
}

// B8: the points' share of the solution, and the step = minus the solution
BA_FN void ba_ph_backsub(const BaView& v, BaState& st, const double* vec, int lane)
{
	for (int i = lane; i < st.dim; i += kBaLanes)
	{
		const double s = -vec[i];
		if (!ba_finite(s))
		{
			st.invalid = 1;
		}
		v.step[6 * v.flist[i / 6] + i % 6] = s;
	}
	if (v.fixPoints)
	{
		return;
	}
	for (int l = lane; l < v.P; l += kBaLanes)
	{
		if (!ba_point_active(v, l))
		{
			continue;
		}
		double e[3] = {v.V[12 * l + 9], v.V[12 * l + 10], v.V[12 * l + 11]};
		for (int o = v.pstart[l]; o < v.pstart[l + 1]; ++o)
		{
			const int k = v.fslot[v.of[o]];
			if (k < 0)
			{
				continue;
			}
			const double* w = v.W + 18 * static_cast<size_t>(o);
			const double* d = vec + 6 * k;
#pragma unroll
			for (int b = 0; b < 3; ++b)
			{
				double t = w[b] * d[0] + w[3 + b] * d[1];
				t = t + w[6 + b] * d[2];
				t = t + w[9 + b] * d[3];
				t = t + w[12 + b] * d[4];
				t = t + w[15 + b] * d[5];
				e[b] = e[b] - t;
			}
		}
		const double* iv = v.Vinv + 9 * l;
#pragma unroll
		for (int a = 0; a < 3; ++a)
		{
			const double s = -ba_dot3(iv[3 * a], iv[3 * a + 1], iv[3 * a + 2], e[0], e[1], e[2]);
			if (!ba_finite(s))
			{
				st.invalid = 1;
			}
			v.step[6 * v.F + 3 * l + a] = s;
		}
	}
}

// B9: one observation's term of the model cost change
BA_FN void ba_ph_model(const BaView& v, int lane)
{
	for (int i = lane; i < v.N; i += kBaLanes)
	{
		const int f = v.of[i], l = v.op[i];
		if (!ba_point_active(v, l))
		{
			v.red[i] = 0.0;
			continue;
		}
		double term[2];
#pragma unroll
		for (int k = 0; k < 2; ++k)
		{
			double mc = 0.0, mp = 0.0;
			if (v.fslot[f] >= 0)
			{
				const double* J = v.Jc + 12 * static_cast<size_t>(i) + 6 * k;
				const double* s = v.step + 6 * f;
				mc = J[0] * s[0] + J[1] * s[1];
				mc = mc + J[2] * s[2];
				mc = mc + J[3] * s[3];
				mc = mc + J[4] * s[4];
				mc = mc + J[5] * s[5];
			}
			if (!v.fixPoints)
			{
				const double* J = v.Jp + 6 * static_cast<size_t>(i) + 3 * k;
				const double* s = v.step + 6 * v.F + 3 * l;
				mp = ba_dot3(J[0], J[1], J[2], s[0], s[1], s[2]);
			}
			const double mr = mc + mp;
			term[k] = mr * (v.res[2 * i + k] + mr / 2.0);
		}
		v.red[i] = term[0] + term[1];
	}
}

// the candidate x (+) step, and the squared differences for the step norm
BA_FN void ba_ph_candidate(const BaView& v, int lane)
{
	for (int k = lane; k < v.F; k += kBaLanes)
	{
		double T[12], out[12];
		ba_load_pose(v.xPose + 12 * k, T);
		if (v.fslot[k] >= 0)
		{
			double ups[3], om[3];
#pragma unroll
			for (int a = 0; a < 3; ++a)
			{
				ups[a] = v.step[6 * k + a] * v.scale[6 * k + a];
				om[a] = v.step[6 * k + 3 + a] * v.scale[6 * k + 3 + a];
			}
			ba_retract(T, ups, om, out);
		}
#pragma unroll
		for (int i = 0; i < 12; ++i)
		{
			const double c = v.fslot[k] >= 0 ? out[i] : T[i];
			v.cPose[12 * k + i] = c;
		}
	}
	for (int l = lane; l < v.P; l += kBaLanes)
	{
		const bool moves = !v.fixPoints && ba_point_active(v, l);
#pragma unroll
		for (int b = 0; b < 3; ++b)
		{
			const int c = 6 * v.F + 3 * l + b;
			const double x = v.xPt[3 * l + b];
			v.cPt[3 * l + b] = moves ? x + v.step[c] * v.scale[c] : x;
		}
	}
}

// squared entries of (a - b) over the free frames' poses and the moving points (b == null: of a itself)
BA_FN void ba_ph_norm(const BaView& v, const double* aPose, const double* aPt, const double* bPose, const double* bPt, int lane)
{
	for (int i = lane; i < 12 * v.F; i += kBaLanes)
	{
		const double d = bPose ? aPose[i] - bPose[i] : aPose[i];
		v.red[i] = v.fslot[i / 12] >= 0 ? d * d : 0.0;
	}
	for (int i = lane; i < 3 * v.P; i += kBaLanes)
	{
		const double d = bPt ? aPt[i] - bPt[i] : aPt[i];
		v.red[12 * v.F + i] = (!v.fixPoints && ba_point_active(v, i / 3)) ? d * d : 0.0;
	}
}

BA_FN void ba_ph_copy(const BaView& v, const double* fromPose, const double* fromPt, double* toPose, double* toPt, int lane)
{
	for (int i = lane; i < 12 * v.F; i += kBaLanes)
	{
		toPose[i] = fromPose[i];
	}
	for (int i = lane; i < 3 * v.P; i += kBaLanes)
	{
		toPt[i] = fromPt[i];
	}
}

// The tree of the rules: lane i adds entries i, i + 256, i + 512, .. in that order from 0; the 256 partial sums are
// folded in halves, part[i] = part[i] + part[i + s] for s = 128, 64, .., 1.  BA_MAX takes the larger instead (a NaN
// is never taken).  The result is part[0].
#define BA_TREE(count, IS_MAX)                                                                        \
	BA_LANES_BEGIN                                                                                    \
	double acc = 0.0;                                                                                 \
	for (int i_ = lane; i_ < (count); i_ += kBaLanes)                                                 \
	{                                                                                                 \
		const double t_ = v.red[i_];                                                                  \
		acc = (IS_MAX) ? (t_ > acc ? t_ : acc) : acc + t_;                                            \
	}                                                                                                 \
	part[lane] = acc;                                                                                 \
	BA_LANES_END                                                                                      \
	for (int s_ = kBaLanes / 2; s_ > 0; s_ /= 2)                                                      \
	{                                                                                                 \
		BA_LANES_BEGIN                                                                                \
		if (lane < s_)                                                                                \
		{                                                                                             \
			const double a_ = part[lane], b_ = part[lane + s_];                                       \
			part[lane] = (IS_MAX) ? (b_ > a_ ? b_ : a_) : a_ + b_;                                    \
		}                                                                                             \
		BA_LANES_END                                                                                  \
	}

// value + Jacobian at the current point: cost, sums, gradient norm
#define BA_EVAL_JAC()                                                              \
	BA_LANES_BEGIN                                                                 \
	ba_ph_observe(v, cam, huber, v.xPose, v.xPt, true, lane);                      \
	BA_LANES_END                                                                   \
	BA_TREE(v.N, false)                                                            \
	BA_LANES_BEGIN                                                                 \
	if (lane == 0)                                                                 \
	{                                                                              \
		st.xCost = 0.5 * part[0];                                                  \
	}                                                                              \
	ba_ph_sums(v, lane);                                                           \
	BA_LANES_END

#define BA_GRAD()                                                                  \
	BA_LANES_BEGIN                                                                 \
	ba_ph_grad(v, lane);                                                           \
	BA_LANES_END                                                                   \
	BA_TREE(6 * v.F + 3 * v.P, true)                                               \
	BA_LANES_BEGIN                                                                 \
	if (lane == 0)                                                                 \
	{                                                                              \
		st.gradMax = part[0];                                                      \
	}                                                                              \
	BA_LANES_END

BA_FN void ba_trace(double* trace, int row, double cost, double radius, double quality, double flag)
{
	if (trace)
	{
		trace[4 * row] = cost;
		trace[4 * row + 1] = radius;
		trace[4 * row + 2] = quality;
		trace[4 * row + 3] = flag;
	}
}

// B9: the whole solve of one problem.  S: dim (dim + 1) / 2 doubles, vec and sol: kBaMaxDim, part: kBaLanes; st, S, vec,
// sol and part are shared by the lanes (LDS on the device).
BA_FN void ba_solve(const BaView& v, const ebo_camera& cam, double huber, const ebo_solver_opts& o, BaState& st, double* S, double* vec,
					double* sol, double* part, double* trace)
{
	BA_LANES_BEGIN
	if (lane == 0)
	{
		st = BaState{};
		st.termination = 1;
		st.radius = o.initial_radius;
		st.decrease = 2.0;
		st.maxNonmono = o.use_nonmonotonic ? o.max_consecutive_nonmonotonic : 0;
		for (int k = 0; k < v.F; ++k)
		{
			v.fslot[k] = v.fixed[k] ? -1 : st.nFree;
			if (!v.fixed[k])
			{
				v.flist[st.nFree++] = k;
			}
		}
		st.dim = 6 * st.nFree;
	}
	ba_ph_clear(v, trace, o.max_num_iterations + 1, lane);
	BA_LANES_END
	BA_LANES_BEGIN
	ba_ph_table(v, st, lane);
	BA_LANES_END
	if (BA_SHARED(st.bad))
	{
		// only the _device form can get here: the host entry has checked and sorted
		BA_LANES_BEGIN
		if (lane == 0)
		{
			st.termination = 2;
		}
		BA_LANES_END
		return;
	}
	BA_EVAL_JAC()
	BA_LANES_BEGIN
	if (lane == 0)
	{
		st.evalsJac = 1;
		st.initialCost = st.minCost = st.xCost;
		ba_trace(trace, 0, st.xCost, st.radius, 0.0, 1.0);
		if (!ba_finite(st.xCost))
		{
			st.termination = 2;
			st.done = 1;
		}
	}
	BA_LANES_END
	if (BA_SHARED(st.done))
	{
		return;
	}
	if (o.jacobi_scaling)
	{
		BA_LANES_BEGIN
		ba_ph_scale(v, lane);
		BA_LANES_END
		BA_EVAL_JAC()
	}
	BA_GRAD()
	BA_LANES_BEGIN
	ba_ph_norm(v, v.xPose, v.xPt, nullptr, nullptr, lane);
	BA_LANES_END
	BA_TREE(12 * v.F + 3 * v.P, false)
	BA_LANES_BEGIN
	if (lane == 0)
	{
		st.xNorm = sqrt(part[0]);
		st.seMin = st.seCur = st.seRef = st.seCand = st.xCost;
		st.lastSuccessful = 1;
	}
	BA_LANES_END

	for (;;)
	{
		BA_LANES_BEGIN
		if (lane == 0)
		{
			st.copyBest = 0;
			if (st.lastSuccessful && st.xCost < st.minCost)
			{
				st.minCost = st.xCost;
				st.copyBest = 1;
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
				st.invalid = 0;
			}
		}
		BA_LANES_END
		if (BA_SHARED(st.copyBest))
		{
			BA_LANES_BEGIN
			ba_ph_copy(v, v.xPose, v.xPt, v.outPose, v.outPt, lane);
			BA_LANES_END
		}
		if (BA_SHARED(st.done))
		{
			break;
		}
		// the step
		if (!v.fixPoints)
		{
			BA_LANES_BEGIN
			ba_ph_points(v, st, o, lane);
			BA_LANES_END
			BA_LANES_BEGIN
			ba_ph_y(v, lane);
			BA_LANES_END
		}
		BA_LANES_BEGIN
		ba_ph_schur(v, st, o, S, vec, lane);
		BA_LANES_END
		const int n = BA_SHARED(st.dim);
		// Cholesky, lower, column by column; every entry loses its products in ascending column order
		for (int k = 0; k < n; ++k)
		{
			BA_LANES_BEGIN
			if (lane == 0)
			{
				const double d = S[ba_tri(k, k)];
				if (d > 0.0 && ba_finite(d))
				{
					S[ba_tri(k, k)] = sqrt(d);
				}
				else
				{
					st.invalid = 1;
				}
			}
			BA_LANES_END
			if (BA_SHARED(st.invalid))
			{
				break;
			}
			BA_LANES_BEGIN
			for (int i = k + 1 + lane; i < n; i += kBaLanes)
			{
				S[ba_tri(i, k)] = S[ba_tri(i, k)] / S[ba_tri(k, k)];
			}
			BA_LANES_END
			BA_LANES_BEGIN
			for (int i = k + 1 + lane / 16; i < n; i += 16)
			{
				for (int j = k + 1 + lane % 16; j <= i; j += 16)
				{
					S[ba_tri(i, j)] = S[ba_tri(i, j)] - S[ba_tri(i, k)] * S[ba_tri(j, k)];
				}
			}
			BA_LANES_END
		}
		if (!BA_SHARED(st.invalid))
		{
			// L y = b by columns, then L' x = y by columns from the last
			for (int k = 0; k < n; ++k)
			{
				BA_LANES_BEGIN
				const double y = vec[k] / S[ba_tri(k, k)];
				for (int i = k + 1 + lane; i < n; i += kBaLanes)
				{
					vec[i] = vec[i] - S[ba_tri(i, k)] * y;
				}
				if (lane == 0)
				{
					sol[k] = y;
				}
				BA_LANES_END
			}
			for (int k = n - 1; k >= 0; --k)
			{
				BA_LANES_BEGIN
				const double x = sol[k] / S[ba_tri(k, k)];
				for (int i = lane; i < k; i += kBaLanes)
				{
					sol[i] = sol[i] - S[ba_tri(k, i)] * x;
				}
				if (lane == 0)
				{
					vec[k] = x;
				}
				BA_LANES_END
			}
			BA_LANES_BEGIN
			ba_ph_backsub(v, st, vec, lane);
			BA_LANES_END
		}
		if (!BA_SHARED(st.invalid))
		{
			BA_LANES_BEGIN
			ba_ph_model(v, lane);
			BA_LANES_END
			BA_TREE(v.N, false)
			BA_LANES_BEGIN
			if (lane == 0)
			{
				st.mcc = -part[0];
				if (!(st.mcc > 0.0))
				{
					st.invalid = 1;
				}
			}
			BA_LANES_END
		}
		if (BA_SHARED(st.invalid))
		{
			BA_LANES_BEGIN
			if (lane == 0)
			{
				st.numInvalid++;
				if (st.numInvalid >= o.max_consecutive_invalid)
				{
					st.termination = 2;
					st.done = 1;
				}
				st.radius = st.radius * 0.5;
				ba_trace(trace, st.iterations, st.xCost, st.radius, 0.0, -1.0);
			}
			BA_LANES_END
			if (BA_SHARED(st.done))
			{
				break;
			}
			continue;
		}
		// the candidate and its cost
		BA_LANES_BEGIN
		ba_ph_candidate(v, lane);
		BA_LANES_END
		BA_LANES_BEGIN
		ba_ph_observe(v, cam, huber, v.cPose, v.cPt, false, lane);
		BA_LANES_END
		BA_TREE(v.N, false)
		BA_LANES_BEGIN
		if (lane == 0)
		{
			st.numInvalid = 0;
			st.evalsCost++;
			st.candCost = 0.5 * part[0];
			if (!ba_finite(st.candCost))
			{
				st.candCost = 1.7976931348623157e308;
			}
		}
		ba_ph_norm(v, v.xPose, v.xPt, v.cPose, v.cPt, lane);
		BA_LANES_END
		BA_TREE(12 * v.F + 3 * v.P, false)
		BA_LANES_BEGIN
		if (lane == 0)
		{
			const double stepNorm = sqrt(part[0]);
			st.accepted = 0;
			if (stepNorm <= o.parameter_tolerance * (st.xNorm + o.parameter_tolerance) ||
				fabs(st.xCost - st.candCost) <= o.function_tolerance * st.xCost)
			{
				st.termination = 0;
				st.done = 1;
				ba_trace(trace, st.iterations, st.candCost, st.radius, 0.0, 2.0);
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
				}
				else
				{
					st.radius = st.radius / st.decrease;
					st.decrease = st.decrease * 2.0;
				}
				ba_trace(trace, st.iterations, st.candCost, st.radius, quality, st.accepted ? 1.0 : 0.0);
			}
		}
		BA_LANES_END
		if (BA_SHARED(st.done))
		{
			break;
		}
		if (!BA_SHARED(st.accepted))
		{
			continue;
		}
		BA_LANES_BEGIN
		ba_ph_copy(v, v.cPose, v.cPt, v.xPose, v.xPt, lane);
		BA_LANES_END
		BA_LANES_BEGIN
		ba_ph_norm(v, v.xPose, v.xPt, nullptr, nullptr, lane);
		BA_LANES_END
		BA_TREE(12 * v.F + 3 * v.P, false)
		BA_LANES_BEGIN
		if (lane == 0)
		{
			st.xNorm = sqrt(part[0]);
		}
		BA_LANES_END
		BA_EVAL_JAC()
		BA_GRAD()
		BA_LANES_BEGIN
		if (lane == 0)
		{
			st.evalsJac++;
			st.lastSuccessful = 1;
			if (!ba_finite(st.xCost))
			{
				st.termination = 2;
				st.done = 1;
			}
		}
		BA_LANES_END
		if (BA_SHARED(st.done))
		{
			break;
		}
	}
}

#ifndef EBO_BUNDLE_RULES_ONLY
__global__ void __launch_bounds__(kBaLanes) k_bundle_adjust(BaTables t, ebo_camera cam, double huber, int fixPoints, ebo_solver_opts o,
															 ebo_summary* summaries, double* trace)
{
	extern __shared__ double baS[];
	__shared__ double vec[kBaMaxDim], sol[kBaMaxDim], part[kBaLanes];
	__shared__ BaState st;
	const int p = static_cast<int>(blockIdx.x);
	const size_t f0 = t.frameOff[p], p0 = t.pointOff[p], n0 = t.obsOff[p];
	BaView v;
	v.F = t.frameOff[p + 1] - t.frameOff[p];
	v.P = t.pointOff[p + 1] - t.pointOff[p];
	v.N = t.obsOff[p + 1] - t.obsOff[p];
	v.fixPoints = fixPoints;
	v.fixed = t.fixed + f0;
	v.of = t.of + n0;
	v.op = t.op + n0;
	v.uv = t.uv + 2 * n0;
	v.outPose = t.poses + 12 * f0;
	v.outPt = t.points + 3 * p0;
	double* w = t.work;
	v.xPose = w + 12 * f0;
	w += 12 * t.totalF;
	v.cPose = w + 12 * f0;
	w += 12 * t.totalF;
	v.xPt = w + 3 * p0;
	w += 3 * t.totalP;
	v.cPt = w + 3 * p0;
	w += 3 * t.totalP;
	v.res = w + 2 * n0;
	w += 2 * t.totalN;
	v.Jc = w + 12 * n0;
	w += 12 * t.totalN;
	v.Jp = w + 6 * n0;
	w += 6 * t.totalN;
	v.W = w + 18 * n0;
	w += 18 * t.totalN;
	v.Y = w + 18 * n0;
	w += 18 * t.totalN;
	v.U = w + 42 * f0;
	w += 42 * t.totalF;
	v.V = w + 12 * p0;
	w += 12 * t.totalP;
	v.Vinv = w + 9 * p0;
	w += 9 * t.totalP;
	v.scale = w + 6 * f0 + 3 * p0;
	w += 6 * t.totalF + 3 * t.totalP;
	v.step = w + 6 * f0 + 3 * p0;
	w += 6 * t.totalF + 3 * t.totalP;
	v.red = w + n0 + 12 * f0 + 3 * p0;
	int* iw = t.iwork;
	v.table = iw + t.tableOff[p];
	iw += t.totalTable;
	v.pstart = iw + p0 + p;
	iw += t.totalP + gridDim.x;
	v.fslot = iw + f0;
	iw += t.totalF;
	v.flist = iw + f0;
	double* tr = trace ? trace + 4 * static_cast<size_t>(o.max_num_iterations + 1) * p : nullptr;
	ba_solve(v, cam, huber, o, st, baS, vec, sol, part, tr);
	if (threadIdx.x == 0)
	{
		ebo_summary s;
		s.iterations = st.iterations;
		s.num_evals_cost = st.evalsCost;
		s.num_evals_jac = st.evalsJac;
		s.termination = st.termination;
		s.initial_cost = st.initialCost;
		s.final_cost = st.minCost;
		summaries[p] = s;
	}
}
#endif
