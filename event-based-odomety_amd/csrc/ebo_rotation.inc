// ebo_rotation.inc — rotational contrast maximisation on the device (include/ebo.h, "angular velocity from events",
// rules V1-V9): the whole-sensor vote image of events warped by one angular velocity per window, its blur, the variance
// and the exact gradient.  Included inside ebo_kernels.hip's anonymous namespace, after ebo_landmark.inc.
// tests/rotation_ref.py restates the rules in numpy.  The rule functions (rot_warp, rot_weights, rot_terms) round every
// float64 operation of V2 and V3 on its own; tools/rotation_serial.cpp compiles them for the host behind
// EBO_ROTATION_RULES_ONLY.

struct RotEvent
{
	int x0, y0;            // floor(u), floor(v): in [-1, w - 1] x [-1, h - 1]
	double al, be, ial, ibe;
	double a, b, X, Y, Z;  // V1 / V2, kept for V8
};

// V1 + V2 + the fractions of V3; false: the event is skipped (nothing of `o` may be used)
__device__ __forceinline__ bool rot_warp(const RotConsts& k, int x, int y, double tau, double wx, double wy, double wz, RotEvent& o)
{
	const double a = __ddiv_rn(__dsub_rn(static_cast<double>(x), k.cx), k.fx);
	const double b = __ddiv_rn(__dsub_rn(static_cast<double>(y), k.cy), k.fy);
	const double tx = __dmul_rn(tau, wx), ty = __dmul_rn(tau, wy), tz = __dmul_rn(tau, wz);
	const double X = __dadd_rn(__dsub_rn(a, ty), __dmul_rn(tz, b));
	const double Y = __dadd_rn(__dsub_rn(b, __dmul_rn(tz, a)), tx);
	const double Z = __dadd_rn(__dsub_rn(1.0, __dmul_rn(tx, b)), __dmul_rn(ty, a));
	if (!(Z > 0.0))
	{
		return false;
	}
	const double u = __dadd_rn(__dmul_rn(k.fx, __ddiv_rn(X, Z)), k.cx);
	const double v = __dadd_rn(__dmul_rn(k.fy, __ddiv_rn(Y, Z)), k.cy);
	// in double, before any conversion to an integer; a NaN fails the test
	if (!(u > -1.0 && u < static_cast<double>(k.w) && v > -1.0 && v < static_cast<double>(k.h)))
	{
		return false;
	}
	const double fx0 = floor(u), fy0 = floor(v);
	o.x0 = static_cast<int>(fx0);
	o.y0 = static_cast<int>(fy0);
	o.al = __dsub_rn(u, fx0);
	o.be = __dsub_rn(v, fy0);
	o.ial = __dsub_rn(1.0, o.al);
	o.ibe = __dsub_rn(1.0, o.be);
	o.a = a;
	o.b = b;
	o.X = X;
	o.Y = Y;
	o.Z = Z;
	return true;
}

// V3: the four fixed-point votes, in the order (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1)
__device__ __forceinline__ void rot_weights(const RotEvent& e, long long (&q)[4])
{
	const double s = 1073741824.0;  // 2^30
	q[0] = static_cast<long long>(rint(__dmul_rn(__dmul_rn(e.ial, e.ibe), s)));
	q[1] = static_cast<long long>(rint(__dmul_rn(__dmul_rn(e.al, e.ibe), s)));
	q[2] = static_cast<long long>(rint(__dmul_rn(__dmul_rn(e.ial, e.be), s)));
	q[3] = static_cast<long long>(rint(__dmul_rn(__dmul_rn(e.al, e.be), s)));
}

// V8: one event's three terms tau * (Du * du/dth_i + Dv * dv/dth_i) from C at its four taps
__device__ __forceinline__ void rot_terms(const RotConsts& k, const RotEvent& e, double tau, double c00, double c10, double c01,
										  double c11, double (&t)[3])
{
	const double Du = e.ibe * (c10 - c00) + e.be * (c11 - c01);
	const double Dv = e.ial * (c01 - c00) + e.al * (c11 - c10);
	const double dX[3] = {0.0, -1.0, e.b};
	const double dY[3] = {1.0, 0.0, -e.a};
	const double dZ[3] = {-e.b, e.a, 0.0};
	const double zz = e.Z * e.Z;
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		const double du = k.fx * (dX[i] * e.Z - e.X * dZ[i]) / zz;
		const double dv = k.fy * (dY[i] * e.Z - e.Y * dZ[i]) / zz;
		t[i] = tau * (Du * du + Dv * dv);
	}
}

#ifndef EBO_ROTATION_RULES_ONLY

// V9's fold of a workgroup's 256 values: the wave's shuffle tree, then wave 0 + 1 + 2 + 3; the sum is valid in thread 0
__device__ __forceinline__ double rot_block_sum(double v, double* sRed)
{
#pragma unroll
	for (int s = 32; s > 0; s /= 2)
	{
		v += __shfl_down(v, s, 64);
	}
	__syncthreads();  // sRed may still be read from a previous fold
	if ((threadIdx.x & 63) == 0)
	{
		sRed[threadIdx.x / 64] = v;
	}
	__syncthreads();
	return ((sRed[0] + sRed[1]) + sRed[2]) + sRed[3];
}

// tau of an event of unit `u` against the WINDOW's reference time
__device__ __forceinline__ double rot_tau(const Unit& u, int dt)
{
	const long long dtw = static_cast<long long>(dt) + static_cast<long long>(u.dt_win);
	return __dmul_rn(static_cast<double>(dtw), 1e-6);
}

// The vote (V1-V3).  Grid (patch, chunk slot): a workgroup takes one unit's events.  Their taps land near the unit's
// rect, so the rect grown by kRotMargin pixels (clipped to the image) is accumulated in LDS with 64-bit LDS atomics
// and added to H once; a tap outside that tile goes to H through a global atomic.  A rect too large for the tile
// (kRotTilePx pixels) keeps no margin, and one larger still no tile at all; neither does k.tile == 0, the A/B build's
// plain global-atomic vote (DESIGN.md 4.21).
// H is an integer sum: every split gives the same bits.  Every H access sits behind the tap's own in-image test.
constexpr int kRotMargin = 8;
constexpr int kRotTilePx = 4096;  // 32 KB of int64
__global__ void __launch_bounds__(kRotBlock) k_rot_vote(const uint64_t* __restrict__ events, const Unit* __restrict__ units,
														 RotWindows L, RotConsts k, const double* __restrict__ omegas,
														 unsigned long long* __restrict__ H)
{
	__shared__ unsigned long long sTile[kRotTilePx];
	const int slot = blockIdx.y, win = L.win[slot];
	const Unit u = units[static_cast<size_t>(win) * k.upw + blockIdx.x];
	if (u.n_ev == 0)
	{
		return;
	}
	unsigned long long* __restrict__ Hw = H + static_cast<size_t>(slot) * k.w * k.h;
	const double wx = omegas[3 * win], wy = omegas[3 * win + 1], wz = omegas[3 * win + 2];
	int m = kRotMargin;
	if ((u.rw + 2 * m) * (u.rh + 2 * m) > kRotTilePx)
	{
		m = 0;
	}
	int tx0 = max(u.rx - m, 0), ty0 = max(u.ry - m, 0);
	int tw = min(u.rx + u.rw + m, k.w) - tx0, th = min(u.ry + u.rh + m, k.h) - ty0;
	if (!k.tile || tw <= 0 || th <= 0 || tw * th > kRotTilePx)
	{
		tw = th = 0;
	}
	const int tn = tw * th;
	for (int i = threadIdx.x; i < tn; i += kRotBlock)
	{
		sTile[i] = 0ull;
	}
	__syncthreads();
	const uint64_t* ev = events + u.ev_off;
	for (uint32_t e = threadIdx.x; e < u.n_ev; e += kRotBlock)
	{
		int x, y, pos, dt;
		unpack(ev[e], x, y, pos, dt);
		RotEvent r;
		if (!rot_warp(k, x, y, rot_tau(u, dt), wx, wy, wz, r))
		{
			continue;
		}
		long long q[4];
		rot_weights(r, q);
#pragma unroll
		for (int t = 0; t < 4; ++t)
		{
			const int px = r.x0 + (t & 1), py = r.y0 + (t >> 1);
			if (q[t] == 0 || px < 0 || px >= k.w || py < 0 || py >= k.h)
			{
				continue;
			}
			const int lx = px - tx0, ly = py - ty0;
			if (lx >= 0 && lx < tw && ly >= 0 && ly < th)
			{
				atomicAdd(&sTile[ly * tw + lx], static_cast<unsigned long long>(q[t]));
			}
			else
			{
				atomicAdd(&Hw[static_cast<size_t>(py) * k.w + px], static_cast<unsigned long long>(q[t]));
			}
		}
	}
	__syncthreads();
	for (int i = threadIdx.x; i < tn; i += kRotBlock)
	{
		const unsigned long long v = sTile[i];
		if (v)
		{
			const int px = tx0 + i % tw, py = ty0 + i / tw;
			atomicAdd(&Hw[static_cast<size_t>(py) * k.w + px], v);
		}
	}
}

// V4: F = H * 2^-30 (exact), one lane per pixel; grid (pixel blocks, chunk slot)
__global__ void __launch_bounds__(kRotBlock) k_rot_scale(RotConsts k, const long long* __restrict__ H, double* __restrict__ F)
{
	const int p = blockIdx.x * kRotBlock + threadIdx.x, np = k.w * k.h;
	if (p < np)
	{
		const size_t o = static_cast<size_t>(blockIdx.y) * np + p;
		F[o] = static_cast<double>(H[o]) * 0x1p-30;
	}
}

// The horizontal pass of V5 / V7, one lane per pixel.  CENTERED == false: the source is H (V4 applied on the way).
// CENTERED == true: the source is B - mu, and the workgroup's fold of (B - mu)^2 goes to partV (V6); WANT_T == false
// then skips the pass itself (the value-only path: the same fold, the same r bits).
template <bool CENTERED, bool WANT_T>
__global__ void __launch_bounds__(kRotBlock) k_rot_hpass(RotConsts k, const void* __restrict__ src, const double* __restrict__ mu,
														  double* __restrict__ T, double* __restrict__ partV)
{
	__shared__ double sRed[kRotBlock / 64];
	const int p = blockIdx.x * kRotBlock + threadIdx.x, np = k.w * k.h;
	const size_t base = static_cast<size_t>(blockIdx.y) * np;
	const double m = CENTERED ? mu[blockIdx.y] : 0.0;
	double sq = 0.0;
	if (p < np)
	{
		const int x = p % k.w;
		if (CENTERED)
		{
			const double d = static_cast<const double*>(src)[base + p] - m;
			sq = d * d;
		}
		if (WANT_T)
		{
			double acc = 0.0;
#pragma unroll
			for (int d = -3; d <= 3; ++d)
			{
				if (x + d >= 0 && x + d < k.w)
				{
					const double val = CENTERED ? static_cast<const double*>(src)[base + p + d] - m
												: static_cast<double>(static_cast<const long long*>(src)[base + p + d]) * 0x1p-30;
					acc = acc + k.g[d + 3] * val;
				}
			}
			T[base + p] = acc;
		}
	}
	if (CENTERED)
	{
		const double s = rot_block_sum(sq, sRed);
		if (threadIdx.x == 0)
		{
			partV[static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x] = s;
		}
	}
}

// The vertical pass, one lane per pixel; SUM: the workgroup's fold of the output goes to partB (V6's mean)
template <bool SUM>
__global__ void __launch_bounds__(kRotBlock) k_rot_vpass(RotConsts k, const double* __restrict__ T, double* __restrict__ out,
														  double* __restrict__ partB)
{
	__shared__ double sRed[kRotBlock / 64];
	const int p = blockIdx.x * kRotBlock + threadIdx.x, np = k.w * k.h;
	const size_t base = static_cast<size_t>(blockIdx.y) * np;
	double acc = 0.0;
	if (p < np)
	{
		const int y = p / k.w;
#pragma unroll
		for (int d = -3; d <= 3; ++d)
		{
			if (y + d >= 0 && y + d < k.h)
			{
				acc = acc + k.g[d + 3] * T[base + p + d * k.w];
			}
		}
		out[base + p] = acc;
	}
	if (SUM)
	{
		const double s = rot_block_sum(acc, sRed);
		if (threadIdx.x == 0)
		{
			partB[static_cast<size_t>(blockIdx.y) * gridDim.x + blockIdx.x] = s;
		}
	}
}

// V9's sum of a window's n folds by one wave: lane l adds folds l, l + 64, .. in ascending order from 0, then the
// wave's shuffle tree; valid in lane 0
__device__ __forceinline__ double rot_wave_sum(const double* __restrict__ v, int n, int stride)
{
	double s = 0.0;
	for (int i = threadIdx.x; i < n; i += 64)
	{
		s = s + v[static_cast<size_t>(i) * stride];
	}
#pragma unroll
	for (int d = 32; d > 0; d /= 2)
	{
		s += __shfl_down(s, d, 64);
	}
	return s;
}

// V6's mean: one wave per chunk slot
__global__ void __launch_bounds__(64) k_rot_mean(RotConsts k, int n_blocks, const double* __restrict__ partB, double* __restrict__ mu)
{
	const double s = rot_wave_sum(partB + static_cast<size_t>(blockIdx.x) * n_blocks, n_blocks, 1);
	if (threadIdx.x == 0)
	{
		mu[blockIdx.x] = s / k.np;
	}
}

// V8's gather.  Grid (patch, chunk slot): lane t of the workgroup takes the unit's events t, t + 256, .. in that order
// and repeats V1-V3 for each (the same text as the vote, hence the same skips); the unit's three sums are V9's fold.
__global__ void __launch_bounds__(kRotBlock) k_rot_gather(const uint64_t* __restrict__ events, const Unit* __restrict__ units,
														   RotWindows L, RotConsts k, const double* __restrict__ omegas,
														   const double* __restrict__ C, double* __restrict__ partG)
{
	__shared__ double sRed[kRotBlock / 64];
	const int slot = blockIdx.y, win = L.win[slot];
	const Unit u = units[static_cast<size_t>(win) * k.upw + blockIdx.x];
	const double* __restrict__ Cw = C + static_cast<size_t>(slot) * k.w * k.h;
	const double wx = omegas[3 * win], wy = omegas[3 * win + 1], wz = omegas[3 * win + 2];
	const uint64_t* ev = events + u.ev_off;
	double acc[3] = {0.0, 0.0, 0.0};
	for (uint32_t e = threadIdx.x; e < u.n_ev; e += kRotBlock)
	{
		int x, y, pos, dt;
		unpack(ev[e], x, y, pos, dt);
		const double tau = rot_tau(u, dt);
		RotEvent r;
		if (!rot_warp(k, x, y, tau, wx, wy, wz, r))
		{
			continue;
		}
		double c[4];
#pragma unroll
		for (int t = 0; t < 4; ++t)
		{
			const int px = r.x0 + (t & 1), py = r.y0 + (t >> 1);
			c[t] = 0.0;
			if (px >= 0 && px < k.w && py >= 0 && py < k.h)
			{
				c[t] = Cw[static_cast<size_t>(py) * k.w + px];
			}
		}
		double t3[3];
		rot_terms(k, r, tau, c[0], c[1], c[2], c[3], t3);
		acc[0] = acc[0] + t3[0];
		acc[1] = acc[1] + t3[1];
		acc[2] = acc[2] + t3[2];
	}
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		const double s = rot_block_sum(acc[i], sRed);
		if (threadIdx.x == 0)
		{
			partG[(static_cast<size_t>(slot) * k.P + blockIdx.x) * 3 + i] = s;
		}
	}
}

// r and g of a chunk slot's window: one wave per slot, V9's sum over the pixel blocks' folds for r and over the patches'
// folds for g.  g_out == null: value only.
__global__ void __launch_bounds__(64) k_rot_finish(RotWindows L, RotConsts k, int n_blocks, const double* __restrict__ partV,
												   const double* __restrict__ partG, double* __restrict__ r_out,
												   double* __restrict__ g_out)
{
	const int slot = blockIdx.x, win = L.win[slot];
	const double s = rot_wave_sum(partV + static_cast<size_t>(slot) * n_blocks, n_blocks, 1);
	if (threadIdx.x == 0)
	{
		r_out[win] = s / k.np;
	}
	if (g_out)
	{
#pragma unroll
		for (int i = 0; i < 3; ++i)
		{
			const double a = rot_wave_sum(partG + static_cast<size_t>(slot) * k.P * 3 + i, k.P, 3);
			if (threadIdx.x == 0)
			{
				g_out[3 * win + i] = k.two_over_np * a;
			}
		}
	}
}

#endif  // EBO_ROTATION_RULES_ONLY
