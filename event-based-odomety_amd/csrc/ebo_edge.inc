// ebo_edge.inc — contrastFunctor::calculateEdgeLoss (contrast_functor.h:152-277), the
// loss the reference's operator() actually calls, on the device.  Included inside
// ebo_kernels.hip's anonymous namespace (uses its helpers).
//
// Forward (value), per unit, everything in one workgroup:
//   I   = image of warped events (same scatter as the variance path, exact fixed point)
//   if mean(I over the 3W x 3H canvas) <= 1e-4: out-of-window penalty (:159-165)
//   g   = forward differences on [0,3H-1) x [0,3W-1)                         (:174-183)
//   E   = first eigenvalue of the 7x7 Gaussian-weighted structure tensor,
//         taps clipped to the same domain, kept where > 0                  (:193-247)
//   r   = 1e3 - sum over 5x5 windows at stride 2 of max(E)/1e3 (max > 0)   (:249-275)
// Jacobian = what Jet<double,2> propagates through that code, computed in reverse
// mode: dr/dE is -1/1e3 at each window's argmax (first strict maximum in scan order,
// as the Jet comparison picks it); back through eigenvalue, tensor and differences to
// an adjoint image A = dr/dI; then J_k = sum_e sum_taps A(px) * d_k(e, tap), the same
// per-event gather pass as the variance path.  NaN semantics follow the reference:
// comparisons are on values, NaN > 0 is false.
//
// Arrays (I, E, A: f64; cnt: int32) cover the bounding box of the event taps grown by
// 8 pixels (stencil 3+1, window 2, slack), clipped to the canvas.  They live in LDS
// when they fit, else in a per-unit slice of a global scratch buffer (rare: wild
// trial flows of the first LM iterations).
// Round 5 (late): I is STORED for the rows that can hold a tap plus one row of zeros on either side only
// (rows iy0 .. iy0 + iRows - 1, same columns and pitch as the box); every read of I clamps its row into that
// range, where the box's rows above and below held the same zeros.  About a quarter of I's storage: with the
// compact layout 95 % instead of 85 % of the reference-default units fit three workgroups per CU at the bench's flows.
// E / A, the claim counters, the direction table and the list's entries are indexed over rows qy0 .. qy0 + qRows - 1
// likewise: the rows the eigenvalue region or a tap can touch plus one row either side -- a row of zeros for the
// window maxima, whose reads clamp into the range, and the row that takes the reverse sweep's terms for pixels beyond
// it (no tap reads them back).

// LDS header of the edge kernel: red[128 doubles] | 64 ints of min/max scratch |
// ints 64..79: argmax list length (64), broken-bound flag (65), max I (66, 67) | 2048 ints: the
// first 1024 are the 8x8-cell occupancy of the forward pass, all of them the argmax list of the
// reverse pass (an LDS-resident box has at most 7900 pixels, i.e. fewer than 2048 windows) | arrays.
constexpr int kEdgeHeader = 168 + 1024;
constexpr int kEdgeCellOff = 80;    // int index of the occupancy cells in the int scratch
constexpr int kEdgeMaxCells = 1024;
constexpr int kEdgeListCap = 2048;
// k_solve_edge keeps its solver state (LmUnit) in the last ints of the list region: a box of n pixels
// has fewer than n / 4 windows and an LDS-resident box fewer than 7800 pixels.
constexpr int kEdgeLmInts = 128;  // 32 ints of EdgeReuse, then the solver state
static_assert(sizeof(LmUnit) <= (kEdgeLmInts - 32) * sizeof(int), "LmUnit must fit its LDS slot");
// What k_solve_edge keeps of an evaluation for the next one (32 ints in front of the solver state).  The
// trust-region loop evaluates the cost at a candidate and, on acceptance, value and Jacobian at the very same point:
// the forward pass of that second evaluation -- bounding box, scatter, conversion, tensor filter and eigenvalues --
// would rebuild, bit for bit, what is still in LDS (I, E, the direction table, the image maximum).  With this record
// it starts behind the window maxima (whose claims the cost evaluation has left in cnt and the list as well).  Valid only
// for a full forward pass on the LDS arrays (no penalty branch, no global slice).
constexpr int kEdgeReuseInts = 32;
struct EdgeReuse
{
	double valid;  // 1.0: the fields below describe what is in LDS
	double m0, m1; // the flow it was built at (compared bit for bit)
	double r;      // the value of that evaluation (its window maxima are taken, the claims are in cnt and the list)
	int bx0, by0, bc, br, x0, x1, y0, y1;
};
static_assert(sizeof(EdgeReuse) <= kEdgeReuseInts * sizeof(int), "EdgeReuse must fit its LDS slot");


// Keeps a wave-uniform constant in a VECTOR register across a hot loop: as a scalar it is
// re-loaded from the kernel arguments wherever the scalar registers run out (an s_load and an
// s_waitcnt lgkmcnt(0), which also drains the LDS queue).
#ifdef EBO_EDGE_NO_INTERIOR
constexpr bool kEdgeInterior = false;  // (A/B: the clipped form for every event, as before round 4's end)
#else
constexpr bool kEdgeInterior = true;
#endif

// The claim counters of the window maxima (how many windows have their argmax at a pixel: at most 9).  Two storage
// forms: one int per pixel, or -- the compact LDS layout of round 5 that lets THREE workgroups share a CU -- one
// 4-bit field per pixel, eight to a word (an atomic add of 1 << 4 k never carries into the next field: 9 < 16).
__device__ __forceinline__ int cnt_claim(int* cnt, int p, bool cnt4)
{
	if (cnt4)
	{
		const int sh = (p & 7) * 4;
		const unsigned int old = atomicAdd(reinterpret_cast<unsigned int*>(cnt) + (p >> 3), 1u << sh);
		return static_cast<int>((old >> sh) & 15u);
	}
	return atomicAdd(&cnt[p], 1);
}
__device__ __forceinline__ int cnt_get(const int* cnt, int p, bool cnt4)
{
	return cnt4 ? static_cast<int>((reinterpret_cast<const unsigned int*>(cnt)[p >> 3] >> ((p & 7) * 4)) & 15u) : cnt[p];
}

// min(max(x, lo), hi) for lo <= hi in ONE instruction (the compiler forms v_med3_i32 only for constant bounds)
__device__ __forceinline__ int clamp_med3(int x, int lo, int hi)
{
	int r;
	asm("v_med3_i32 %0, %1, %2, %3" : "=v"(r) : "v"(x), "v"(lo), "v"(hi));
	return r;
}

__device__ __forceinline__ double vgpr_pin(double x)
{
	asm volatile("" : "+v"(x));
	return x;
}

// Workgroup maximum of a non-negative double (or +inf) into an LDS word: the bit patterns of
// non-negative doubles order like unsigned integers.  One LDS atomic per wave; the caller's next
// barrier publishes the result.
__device__ __forceinline__ void block_umax(double v, unsigned long long* slot)
{
	v = wave_reduce(v, 0.0, [](double a, double b) { return fmax(a, b); });
	if ((threadIdx.x & 63) == kWaveResultLane)
	{
		atomicMax(slot, static_cast<unsigned long long>(__double_as_longlong(v)));
	}
}

// Tensor sums at pixel (y, x) of the box-relative image I (pitch bc), canvas origin
// of the box (bx0, by0); taps clipped to the gradient domain [0,H3-1) x [0,W3-1).
__device__ __forceinline__ void tensor_at(const double* I, int bc, int iRows, int bx0, int iy0, int W3,
										   int H3, int y, int x, const EdgeConsts& ec, double& s00,
										   double& s01, double& s11)
{
	s00 = 0.0;
	s01 = 0.0;
	s11 = 0.0;
	// The 7x7 taps need I on rows y-3..y+4 and columns x-3..x+4.  Two rows of 8 values
	// are kept in registers and shifted down: 64 LDS reads per pixel instead of 147.
	// Addresses are clamped into the box (values read through a clamped address belong to
	// taps that the domain test below rejects).  Tap order (i outer, j inner) and the
	// association of every product are the reference's (contrast_functor.h:209-235).
	int co[8];
#pragma unroll
	for (int k = 0; k < 8; ++k)
	{
		co[k] = min(max(x - 3 + k, bx0), bx0 + bc - 1) - bx0;
	}
	const int rowMax = iy0 + iRows - 1;  // last stored row of I (a row beyond the stored ones reads a row of zeros or meets zero weights)
	double cur[8], nxt[8];
	{
		const double* row = I + (clamp_med3(y - 3, iy0, rowMax) - iy0) * bc;
#pragma unroll
		for (int k = 0; k < 8; ++k)
		{
			cur[k] = row[co[k]];
		}
	}
#pragma unroll
	for (int i = -3; i <= 3; ++i)
	{
		const int yy = y + i;
		{
			const double* row = I + (clamp_med3(yy + 1, iy0, rowMax) - iy0) * bc;
#pragma unroll
			for (int k = 0; k < 8; ++k)
			{
				nxt[k] = row[co[k]];
			}
		}
		if (yy >= 0 && yy < H3 - 1)
		{
#pragma unroll
			for (int j = -3; j <= 3; ++j)
			{
				const int xx = x + j;
				if (xx < 0 || xx >= W3 - 1)
				{
					continue;
				}
				const double c0 = cur[j + 3];
				const double gx = cur[j + 4] - c0;
				const double gy = nxt[j + 3] - c0;
				const double w = ec.w[(i + 3) * 7 + (j + 3)];
				const double wgx = w * gx;
				s00 += wgx * gx;
				s01 += wgx * gy;
				s11 += (w * gy) * gy;
			}
		}
#pragma unroll
		for (int k = 0; k < 8; ++k)
		{
			cur[k] = nxt[k];
		}
	}
}

// Eigenvalue image with the separable tensor filter and NO intermediate arrays: a lane owns a
// vertical run of output pixels of one column and slides down the rows, keeping the last seven
// horizontally filtered rows (3 sums each) and two rows of 8 image values in registers.  Per
// output pixel ~(R+6)/R x 56 + 21 f64 operations against ~390 for the direct 49-tap sum, and
// (R+6)/R x 8 LDS reads against 64; consecutive lanes own consecutive columns, so every read is
// stride-1 across the wave.  Same operation order as the band-buffer version of the 28 B/pixel
// layout (horizontal fma chain j = -3..3, vertical fma chain i = -3..3, then the norm): the two
// produce identical bits.
// cs (or null): the direction of the first eigenvector, c = (s00 - s11)/d and s = 2 s01/d with
// d = sqrt(tr^2 - 4 det), of every pixel that gets a positive eigenvalue -- all the reverse pass
// needs of the tensor at an argmax pixel (d lam/d s00 = (1 + c)/2, d lam/d s11 = (1 - c)/2,
// d lam/d s01 = s) -- written to global memory (16 B per pixel; LDS has no room).
template <int R, bool INTERIOR>
__device__ __forceinline__ void tensor_runs(const double* I, double* E, int bc, int br, int bx0, int by0, int iy0, int iRows, int qy0,
											 int W3, int H3, int ex0, int ex1, int ey0, int ey1,
											 const int* cell, int ncx, bool useCells, const EdgeConsts& ec,
											 double2* __restrict__ cs)
{
	const int ew = ex1 - ex0 + 1, eh = ey1 - ey0 + 1;
	if (ew <= 0 || eh <= 0)
	{
		return;
	}
	const int nSeg = (eh + R - 1) / R;
	// Round 5: the region's rows are dealt out EVENLY over the runs -- rEff = ceil(eh / nSeg) <= R rows each -- and a
	// run stops after rEff + 6 row steps: 41 rows are six runs of seven rows (13 row steps) instead of five of eight
	// and one of one (14 row steps each, the last seven of them for a single row).  A pixel's value does not depend on
	// where its run starts: same bits.
#ifdef EBO_AB
	const int rEff = (ec.ablate & 512) ? R : (eh + nSeg - 1) / nSeg;  // (A/B: runs of R rows, the last one short, as in rounds 2-4)
#else
	const int rEff = (eh + nSeg - 1) / nSeg;
#endif
	const int rowMax = iy0 + iRows - 1;  // I's stored rows: iy0 .. rowMax (the first and the last one hold zeros unless they touch the canvas edge)
	for (int k = threadIdx.x; k < ew * nSeg; k += blockDim.x)
	{
		const int x = ex0 + k % ew;
		const int ya = ey0 + (k / ew) * rEff;
		const int yb = min(ya + rEff - 1, ey1);
		if (useCells)
		{
			const int cx0 = max(x - 3 - bx0, 0) >> 3, cx1 = min(x + 4 - bx0, bc - 1) >> 3;
			const int cy0 = max(ya - 3 - by0, 0) >> 3, cy1 = min(yb + 4 - by0, br - 1) >> 3;
			int any = 0;
			for (int cy = cy0; cy <= cy1; ++cy)
			{
				for (int cx = cx0; cx <= cx1; ++cx)
				{
					any |= cell[cy * ncx + cx];
				}
			}
			if (!any)
			{
				continue;
			}
		}
		// clamped column offsets (a value read through a clamped address only meets a zero weight)
		// and the horizontal weights with the column clipping folded in: a clipped tap adds
		// fma(0, finite, h) = h, the same bits as skipping it
		// INTERIOR (decided per unit): every read of the region's stencils lies inside the box and every
		// tap inside the gradient domain, so the eight columns are c0 .. c0 + 7 (immediate offsets, paired
		// reads), the weights are the scalar constants and no row is clipped; rows past the region's
		// last stencil row (the tail of the last run) are read at a clamped offset and only feed outputs
		// that are not stored.  The general form spends as many instructions on addresses and clipping
		// as on the arithmetic (112 per row step for 56 f64 operations).
		int co[8];
		double gm[7];
#pragma unroll
		for (int j = 0; j < 8; ++j)
		{
			co[j] = INTERIOR ? (x - 3 - bx0) + j : min(max(x - 3 + j, bx0), bx0 + bc - 1) - bx0;
		}
#pragma unroll
		for (int j = 0; j < 7; ++j)
		{
			const int xx = x - 3 + j;
			gm[j] = (INTERIOR || (xx >= 0 && xx < W3 - 1)) ? ec.g[j] : 0.0;
		}
		double cur[8], nxt[8];
		double r00[7], r01[7], r11[7];
#pragma unroll
		for (int i = 0; i < 7; ++i)
		{
			r00[i] = 0.0;
			r01[i] = 0.0;
			r11[i] = 0.0;
		}
		// INTERIOR: offset of (row, first column) in an UNTRIMMED image that starts at row iy0, stepped by bc; the read
		// goes to the offset clamped into the stored rows
		int rowOff = INTERIOR ? (ya - 3 - iy0) * bc + co[0] : 0;
		const int rowOffMin = co[0], rowOffMax = (iRows - 1) * bc + co[0];
		{
			const double* row = INTERIOR ? I + clamp_med3(rowOff, rowOffMin, rowOffMax) : I + (clamp_med3(ya - 3, iy0, rowMax) - iy0) * bc;
#pragma unroll
			for (int j = 0; j < 8; ++j)
			{
				cur[j] = INTERIOR ? lds_ld(row + j) : row[co[j]];
			}
		}
		// R + 6 row steps, fully unrolled: the ring shift and the cur/nxt hand-over are renames
#pragma unroll
		for (int t = 0; t < R + 6; ++t)
		{
			// (a run of rEff rows ends after rEff + 6 steps; uniform, and a guard instead of a break: the loop stays
			// fully unrolled.  No run is shorter than one row: the first seven steps need no test)
			if (t >= 7 && t >= rEff + 6)
			{
				continue;
			}
			const int yy = ya - 3 + t;
			{
				rowOff += bc;
				const double* row = INTERIOR ? I + clamp_med3(rowOff, rowOffMin, rowOffMax) : I + (clamp_med3(yy + 1, iy0, rowMax) - iy0) * bc;
#pragma unroll
				for (int j = 0; j < 8; ++j)
				{
					nxt[j] = INTERIOR ? lds_ld(row + j) : row[co[j]];
				}
			}
			double h00 = 0.0, h01 = 0.0, h11 = 0.0;
#pragma unroll
			for (int j = 0; j < 7; ++j)
			{
				const double c0 = cur[j];
				const double gx = cur[j + 1] - c0;
				const double gy = nxt[j] - c0;
				h00 = fma(gm[j], gx * gx, h00);
				h01 = fma(gm[j], gx * gy, h01);
				h11 = fma(gm[j], gy * gy, h11);
			}
			const bool rowIn = INTERIOR || (yy >= 0 && yy < H3 - 1);  // a clipped row contributes zeros
#pragma unroll
			for (int i = 0; i < 6; ++i)
			{
				r00[i] = r00[i + 1];
				r01[i] = r01[i + 1];
				r11[i] = r11[i + 1];
			}
			r00[6] = rowIn ? h00 : 0.0;
			r01[6] = rowIn ? h01 : 0.0;
			r11[6] = rowIn ? h11 : 0.0;
#pragma unroll
			for (int j = 0; j < 8; ++j)
			{
				cur[j] = nxt[j];
			}
			if (t >= 6)  // the ring holds the filtered rows y-3 .. y+3
			{
				const int y = yy - 3;
				double s00 = 0.0, s01 = 0.0, s11 = 0.0;
#pragma unroll
				for (int i = 0; i < 7; ++i)
				{
					s00 = fma(ec.g[i], r00[i], s00);
					s01 = fma(ec.g[i], r01[i], s01);
					s11 = fma(ec.g[i], r11[i], s11);
				}
				s00 *= ec.norm_st;
				s01 *= ec.norm_st;
				s11 *= ec.norm_st;
				const double tr = s00 + s11;
				const double det = s00 * s11 - s01 * s01;
				const double d = sqrt(tr * tr - 4.0 * det);
				const double lam = 0.5 * (tr + d);
				if (y <= yb && lam > 0.0)
				{
					E[(y - qy0) * bc + (x - bx0)] = lam;
					if (cs)
					{
						// 1/d: the hardware estimate (measured ~2^-30 here) and two Newton steps -- an
						// ulp or two, no division sequence (d = 0 gives inf/NaN: the reverse pass
						// flags the unit, as the Jet's sqrt derivative would)
						double rd = __builtin_amdgcn_rcp(d);
						rd = fma(fma(-d, rd, 1.0), rd, rd);
						rd = fma(fma(-d, rd, 1.0), rd, rd);
						cs[(y - qy0) * bc + (x - bx0)] = make_double2((s00 - s11) * rd, (s01 + s01) * rd);
					}
				}
			}
		}
	}
}

// One unit.  Pointers I/E/A/cnt address LDS or global memory.  Returns r, J0, J1 to every
// thread.  ALIAS (the LDS instantiation): 20 bytes per pixel instead of 28, so that the full
// canvas of a 20x20 patch fits twice into a CU's LDS and two workgroups overlap each other's
// barriers (the kernel is latency/barrier bound: 70 % of the wave time is waiting, LDS 37 %
// busy, VALU 10 %; PMC profile in DESIGN.md) --
//   * A (the adjoint image) lives in E's storage: E is dead once the window maxima are taken;
//   * no band buffers: the tensor is summed in its direct 49-tap form;
//   * the argmax list lives in the storage of the dead occupancy cells (the first NMS window to claim a
//     pixel appends it; round 2, (ii)).
template <bool ALIAS, bool JAC, int REVU, bool SOLVE = false>
__device__ __forceinline__ void edge_unit(const uint64_t* __restrict__ ev, const Unit& u,
										   double m0, double m1, bool wantJac, int bx0, int by0,
										   int bc, int br, int iy0, int iRows, int qy0, int qRows, int x0, int x1, int y0, int y1,
										   double* I, double* E, double* A, int* cnt, int* list, int listCap,
										   double* red, int* ired, const EvalConsts& c, const EdgeConsts& ec,
										   double2* __restrict__ cs, uint64_t rec0, bool reuseFwdArg, bool keepFwdArg, bool& fwdDone,
										   double& r, double& j0, double& j1, bool cnt4 EDGE_TICK_ARG)
{
	// (compile-time false outside k_solve_edge: the batched kernels' code is what it was)
	const bool reuseFwd = SOLVE && reuseFwdArg, keepFwd = SOLVE && keepFwdArg;
	// reuseFwd (k_solve_edge): I, E, the directions and the image maximum of THIS point are in LDS already -- start
	// at the window maxima; keepFwd: a Jacobian evaluation of this point may follow -- leave them all behind even
	// if this evaluation wants the value only; fwdDone: the forward pass ran to its end (no penalty branch)
	fwdDone = false;
	const int rx = u.rx, ry = u.ry, rw = u.rw, rh = u.rh;
	const int W3 = 3 * rw, H3 = 3 * rh;
	const uint32_t nEv = u.n_ev;
	double fixBias, fixScale;
	unit_fix_grid(c, nEv, fixBias, fixScale);
	const int npx = bc * br;
	const int nI = bc * iRows;           // I's stored pixels: rows iy0 .. iy1 of the box's columns (nI <= npx)
	const int iy1 = iy0 + iRows - 1;
	const int nE = bc * qRows;           // E / A / cnt: rows qy0 .. qy1 (nI <= nE <= npx)
	const int qy1 = qy0 + qRows - 1;
	unsigned long long* Iq = reinterpret_cast<unsigned long long*>(I);
	// rec0: the lane's first event, loaded once by the bounding-box pass.  The scatter and the gather pass start
	// right behind a barrier, so a fresh load there is an exposed L2 round trip per pass and unit (units of up to
	// blockDim events -- the reference's 139 -- have no other)
	auto event_at = [&](uint32_t e) -> uint64_t { return e == threadIdx.x ? rec0 : ev[e]; };

	if (!reuseFwd)
	{
		for (int p = threadIdx.x; p < nE; p += blockDim.x)
		{
			if (p < nI)
			{
				I[p] = 0.0;
			}
			E[p] = 0.0;
			if (!cnt4)
			{
				cnt[p] = 0;
			}
			else if (p < ((nE + 7) >> 3))
			{
				cnt[p] = 0;  // eight 4-bit counters per word
			}
			if (!ALIAS)
			{
				A[p] = 0.0;
			}
		}
	}
	// ints 66..67 of the scratch: a u64 maximum (bit patterns of non-negative doubles order like
	// integers), the largest image value: it bounds the terms of the reverse pass
	unsigned long long* umax = reinterpret_cast<unsigned long long*>(ired + 66);
	if (threadIdx.x == 0)
	{
		ired[65] = 0;  // an entry of the reverse pass broke the bound of the fixed-point grid
		if (!reuseFwd)
		{
			ired[64] = 0;  // argmax list length
			umax[0] = 0ull;
		}
	}
	// Occupancy of 8x8-pixel cells of the box, marked by the event footprints: a pixel
	// whose whole stencil (rows y-3..y+4, columns x-3..x+4) lies in empty cells reads only
	// zeros, its tensor is identically 0 and E stays 0 -- skipped exactly, not approximately.
	int* cell = ired + kEdgeCellOff;
	const int ncx = (bc + 7) >> 3, ncy = (br + 7) >> 3;
	const bool useCells = ncx * ncy <= min(kEdgeMaxCells, listCap);  // (the cells share the list's storage)
	if (useCells && !reuseFwd)
	{
		for (int k = threadIdx.x; k < ncx * ncy; k += blockDim.x)
		{
			cell[k] = 0;
		}
	}
	__syncthreads();
	EDGE_TICK(1);

	// scatter the value taps (exact fixed point).  Straight-line per event: clipped taps get a ZERO
	// weight and a clamped address (adding the integer 0 changes nothing) instead of a branch.  The
	// branchy form put every tap in its own basic block, and under this kernel's scalar-register
	// pressure the compiler re-loaded the bias from the kernel arguments in each of them: an s_load
	// plus an s_waitcnt lgkmcnt(0) -- which also drains the LDS atomics in flight -- per tap
	// (phase clocks, tools/edge_phase_clock.py: 15.5 k cycles for 139 events per unit).
	// Sharing an event between lanes when a unit has few events (139 on 512 lanes in the reference
	// configuration) was tried twice, here and in the gather pass: seven rows over 2-4 lanes with
	// every lane recomputing the weights (2.13 -> 2.30 ms), and lane pairs that evaluate one axis
	// each and swap the weights by a lane shuffle (2.17 -> 2.16 ms).
#ifdef EBO_AB
	// Diagnostic (A/B build only; EBO_EDGE_ABLATE bit 64, SURVEY section 7's "deterministic variant for debugging"): the
	// image as the REFERENCE builds it -- one rounding per event, in the order of the event list
	// (contrast_functor.h:38-88: img(py,px) += gaussian(c, tap), sequentially), the Gaussian in the reference's own
	// association (:90-99), no factorisation, no fixed point.  A lane owns pixels and walks the unit's events in
	// memory order, so every pixel's sum is the reference's sum.  With the direct tensor form (EBO_EDGE_SEPARABLE=0)
	// the whole forward pass then follows the reference's arithmetic: what decides an exact tie of a window maximum
	// there decides it here (tests/test_gpu_edge_ties.py).  Load the unit in list order (EBO_KEEP_ORDER=1).
	const bool refOrder = (ec.ablate & 64) != 0;
	if (!reuseFwd && refOrder)
	{
		for (int p = threadIdx.x; p < nI; p += blockDim.x)
		{
			const int py = iy0 + p / bc, px = bx0 + p % bc;  // canvas coordinates
			double acc = 0.0;
			if (px >= 0 && px < W3 && py >= 0 && py < H3)
			{
				for (uint32_t e = 0; e < nEv; ++e)
				{
					int x, y, pos, dt;
					unpack(ev[e], x, y, pos, dt);
					const double tau = static_cast<double>(dt) * c.scale;
					const double cx = static_cast<double>(x) + tau * m0;
					const double cy = static_cast<double>(y) + tau * m1;
					if (!convertible(cx) || !convertible(cy))
					{
						continue;
					}
					const int bx = static_cast<int>(cx), by = static_cast<int>(cy);
					const int i = px - (bx - rx + rw), j = py - (by - ry + rh);
					if (i < -3 || i > 3 || j < -3 || j > 3)
					{
						continue;
					}
					const double dx = static_cast<double>(bx + i) - cx, dy = static_cast<double>(by + j) - cy;
					acc += c.norm * exp(c.hs * (dx * dx + dy * dy));
				}
			}
			I[p] = acc;
		}
		for (int k = threadIdx.x; useCells && k < ncx * ncy; k += blockDim.x)
		{
			cell[k] = 1;  // no occupancy shortcut in this mode
		}
	}
	if (!reuseFwd && !refOrder)
#else
	const bool refOrder = false;
	if (!reuseFwd)
#endif
	{
		const double biasV = vgpr_pin(fixBias);  // low dword 0 (1.5 * 2^k): removing it is a 32-bit subtract
		const int biasHi = __double2hiint(fixBias);
		for (uint32_t e = threadIdx.x; e < ((ec.ablate & 16) ? 0u : nEv); e += blockDim.x)
		{
			int pxc, pyc;
			double fx, fy, tau;
			if (!warp_event(event_at(e), rx, ry, rw, rh, m0, m1, c, pxc, pyc, fx, fy, tau))
			{
				continue;
			}
			double wx[7], wy[7];
			axis_taps(fx, c.norm, c, wx);
			axis_taps(fy, 1.0, c, wy);
			if (useCells)
			{
				// a 7-pixel footprint touches at most 2 x 2 cells of 8 x 8: four unconditional stores
				const int cx0 = max(pxc - 3 - bx0, 0) >> 3, cx1 = min(pxc + 3 - bx0, bc - 1) >> 3;
				const int cy0 = max(pyc - 3 - by0, 0) >> 3, cy1 = min(pyc + 3 - by0, br - 1) >> 3;
				cell[cy0 * ncx + cx0] = 1;
				cell[cy0 * ncx + cx1] = 1;
				cell[cy1 * ncx + cx0] = 1;
				cell[cy1 * ncx + cx1] = 1;
			}
			if (kEdgeInterior && pxc >= 3 && pxc + 3 < W3 && pyc >= 3 && pyc + 3 < H3)
			{
				// the footprint lies inside the canvas (almost every event): no clipping, immediate column offsets --
				// the same products, the same sums
				unsigned long long* rowp = Iq + (pyc - 3 - iy0) * bc + (pxc - 3 - bx0);
#pragma unroll
				for (int j = 0; j < 7; ++j)
				{
#pragma unroll
					for (int i = 0; i < 7; ++i)
					{
						const double b = wx[i] * wy[j] + biasV;
						unsigned int hi = static_cast<unsigned int>(__double2hiint(b) - biasHi);
						keep32(hi);
						const unsigned int lo = static_cast<unsigned int>(__double2loint(b));
						atomicAdd(rowp + i, (static_cast<unsigned long long>(hi) << 32) | lo);
					}
					rowp += bc;
				}
				continue;
			}
			int ci[7];
#pragma unroll
			for (int i = 0; i < 7; ++i)
			{
				const int xx = pxc - 3 + i;
				wx[i] = (xx >= 0 && xx < W3) ? wx[i] : 0.0;
				ci[i] = min(max(xx, 0), W3 - 1) - bx0;  // inside the box: it reaches the canvas edge whenever a tap does
			}
#pragma unroll
			for (int j = 0; j < 7; ++j)
			{
				const int yy = pyc - 3 + j;
				const double wyj = (yy >= 0 && yy < H3) ? wy[j] : 0.0;
				unsigned long long* rowp = Iq + (min(max(yy, 0), H3 - 1) - iy0) * bc;  // (a row with a tap: stored)
#pragma unroll
				for (int i = 0; i < 7; ++i)
				{
					const double b = wx[i] * wyj + biasV;
					unsigned int hi = static_cast<unsigned int>(__double2hiint(b) - biasHi);
					keep32(hi);  // ONE 32-bit subtract (ebo_kernels.hip)
					const unsigned int lo = static_cast<unsigned int>(__double2loint(b));
					atomicAdd(rowp + ci[i], (static_cast<unsigned long long>(hi) << 32) | lo);
				}
			}
		}
	}
	__syncthreads();
	EDGE_TICK(2);
	if (!reuseFwd)
	{
		double s1[1] = {0.0};
		double iMax = 0.0;
		for (int p = threadIdx.x; p < nI; p += blockDim.x)
		{
			const double v = refOrder ? I[p] : static_cast<double>(Iq[p]) * fixScale;
			I[p] = v;
			s1[0] += v;
			iMax = fmax(iMax, v);
		}
		if (JAC && (wantJac || keepFwd))
		{
			block_umax(iMax, &umax[0]);  // published by the barriers of block_sum
		}
		block_sum<1>(s1, red);  // includes the barrier that publishes I
		EDGE_TICK(3);
		const double meanAll = s1[0] * (1.0 / static_cast<double>(static_cast<long>(W3) * H3));
		if (meanAll <= ec.mean_threshold)
		{
			r = c.max_res * (1.0 + m0 * m0 + m1 * m1);
			j0 = c.max_res * (m0 + m0);
			j1 = c.max_res * (m1 + m1);
			return;
		}
	}

	// Eigenvalue image on the taps' box grown by the stencil reach, inside the domain.
	// The tensor weights are separable, w(i,j) = N e(i) e(j) with e(k) = exp(hs k^2): rows are
	// filtered horizontally into three band buffers (in A's storage, which the forward pass does
	// not need yet), then vertically: ~90 f64 operations per pixel instead of ~490 for the
	// direct 49-tap sum (the direct form, in the reference's summation order, is kept for the
	// few argmax pixels of the reverse pass).  Same real numbers, last-bit differences only.
	const int ex0 = max(x0 - 4, 0), ex1 = min(x1 + 3, W3 - 2);
	const int ey0 = max(y0 - 4, 0), ey1 = min(y1 + 3, H3 - 2);
	const int ew = ex1 - ex0 + 1, eh = ey1 - ey0 + 1;
	// Under ALIAS there is no room for band buffers (cnt's storage would give bands so short
	// that the halo rows dominate: measured slower than the direct form) and the direct 49-tap
	// form is used; two workgroups per CU more than pay for its extra arithmetic.
	const int band = max(npx / (3 * ew) - 6, 1);  // rows of E per band: 3 (band + 6) ew doubles fit A
	double* H0 = A;
	// (EBO_EDGE_SEPARABLE=0 selects the direct form everywhere, 12 % slower at C2.)  The two forms
	// round differently, which only matters at exact mathematical ties of the window maximum:
	// at zero flow events sit on integer positions, symmetric pixels have EQUAL eigenvalues and
	// the argmax -- hence the Jacobian, not the value -- is decided by rounding noise.  Neither
	// form reproduces the reference there (measured at exactly zero flow: the Jacobians of 0.8 %
	// of the active patches differ from the oracle's with either form), because the image itself
	// is accumulated exactly here and with one rounding per event in the reference.
	const bool runs = (ec.reserved & (ALIAS ? 2 : 4)) != 0 && !(ec.ablate & 32);
	cs = runs ? cs : nullptr;  // only the register-run form writes the directions
	const bool separable = !ALIAS && !runs && (ec.reserved & 1) != 0 && 21 * ew <= npx && !(ec.ablate & 32);
	if (!reuseFwd && runs && !(ec.ablate & 1))
	{
		// (see tensor_runs: all stencil reads inside the box, all taps inside the gradient domain)
		const bool interior = ex0 - 3 >= max(bx0, 0) && ex1 + 4 <= bx0 + bc - 1 && ex1 + 3 <= W3 - 2 &&
							  ey0 - 3 >= max(by0, 0) && ey1 + 4 <= by0 + br - 1 && ey1 + 3 <= H3 - 2;
		if (interior)
		{
			tensor_runs<8, true>(I, E, bc, br, bx0, by0, iy0, iRows, qy0, W3, H3, ex0, ex1, ey0, ey1, cell, ncx, useCells, ec,
								 (JAC && (wantJac || keepFwd)) ? cs : nullptr);
		}
		else
		{
			tensor_runs<8, false>(I, E, bc, br, bx0, by0, iy0, iRows, qy0, W3, H3, ex0, ex1, ey0, ey1, cell, ncx, useCells, ec,
								  (JAC && (wantJac || keepFwd)) ? cs : nullptr);
		}
	}
	if (!reuseFwd && !separable && !runs && !(ec.ablate & 1))
	{
		for (int k = threadIdx.x; k < ew * eh; k += blockDim.x)
		{
			const int y = ey0 + k / ew, x = ex0 + k % ew;
			double s00, s01, s11;
			tensor_at(I, bc, iRows, bx0, iy0, W3, H3, y, x, ec, s00, s01, s11);
			const double tr = s00 + s11;
			const double det = s00 * s11 - s01 * s01;
			const double lam = 0.5 * (tr + sqrt(tr * tr - 4.0 * det));
			if (lam > 0.0)
			{
				E[(y - qy0) * bc + (x - bx0)] = lam;
			}
		}
	}
	for (int r0 = ey0; r0 <= ey1 && separable && !reuseFwd && !(ec.ablate & 1); r0 += band)
	{
		const int r1 = min(r0 + band - 1, ey1);
		const int hy0 = max(r0 - 3, 0), hy1 = min(r1 + 3, H3 - 2);
		const int nh = hy1 - hy0 + 1;
		double* H1 = H0 + nh * ew;
		double* H2 = H1 + nh * ew;
		for (int k = threadIdx.x; k < nh * ew; k += blockDim.x)
		{
			const int yy = hy0 + k / ew, x = ex0 + k % ew;
			// two rows of 8 values: I(yy, x-3..x+4), I(yy+1, x-3..x+4); clamped addresses only
			// feed taps that the domain test rejects
			const double* rowA = I + (clamp_med3(yy, iy0, iy1) - iy0) * bc;
			const double* rowB = I + (clamp_med3(yy + 1, iy0, iy1) - iy0) * bc;  // (yy <= H3-2: row yy+1 is in the canvas)
			double h00 = 0.0, h01 = 0.0, h11 = 0.0;
			double prev = rowA[min(max(x - 3, bx0), bx0 + bc - 1) - bx0];
#pragma unroll
			for (int j = -3; j <= 3; ++j)
			{
				const int xx = x + j;
				const double next = rowA[min(max(xx + 1, bx0), bx0 + bc - 1) - bx0];
				if (xx >= 0 && xx < W3 - 1)
				{
					const double gx = next - prev;
					const double gy = rowB[xx - bx0] - prev;
					const double g = ec.g[j + 3];
					h00 = fma(g, gx * gx, h00);
					h01 = fma(g, gx * gy, h01);
					h11 = fma(g, gy * gy, h11);
				}
				prev = next;
			}
			H0[k] = h00;
			H1[k] = h01;
			H2[k] = h11;
		}
		__syncthreads();
		for (int k = threadIdx.x; k < (r1 - r0 + 1) * ew; k += blockDim.x)
		{
			const int y = r0 + k / ew, x = ex0 + k % ew;
			if (useCells)
			{
				const int cx0 = max(x - 3 - bx0, 0) >> 3, cx1 = min(x + 4 - bx0, bc - 1) >> 3;
				const int cy0 = max(y - 3 - by0, 0) >> 3, cy1 = min(y + 4 - by0, br - 1) >> 3;
				int any = 0;
				for (int cy = cy0; cy <= cy1; ++cy)
				{
					for (int cx = cx0; cx <= cx1; ++cx)
					{
						any |= cell[cy * ncx + cx];
					}
				}
				if (!any)
				{
					continue;
				}
			}
			double s00 = 0.0, s01 = 0.0, s11 = 0.0;
#pragma unroll
			for (int i = -3; i <= 3; ++i)
			{
				const int yy = y + i;
				if (yy < 0 || yy >= H3 - 1)
				{
					continue;
				}
				const int idx = (yy - hy0) * ew + (x - ex0);
				const double g = ec.g[i + 3];
				s00 = fma(g, H0[idx], s00);
				s01 = fma(g, H1[idx], s01);
				s11 = fma(g, H2[idx], s11);
			}
			s00 *= ec.norm_st;
			s01 *= ec.norm_st;
			s11 *= ec.norm_st;
			const double tr = s00 + s11;
			const double det = s00 * s11 - s01 * s01;
			const double lam = 0.5 * (tr + sqrt(tr * tr - 4.0 * det));
			if (lam > 0.0)
			{
				E[(y - qy0) * bc + (x - bx0)] = lam;
			}
		}
		__syncthreads();
	}
	(void)eh;
	if (!ALIAS && JAC && wantJac)
	{
		// the band buffers lived in A: the reverse pass needs it zeroed again
		for (int p = threadIdx.x; p < npx; p += blockDim.x)
		{
			A[p] = 0.0;
		}
	}
	__syncthreads();
	EDGE_TICK(4);
	fwdDone = true;

	// non-maximum suppression windows: centres 2,4,.. < dim-1-2, 5x5, stride 2.  A window with a
	// positive maximum counts itself at its argmax pixel; the first window to claim a pixel also
	// appends the pixel to the entry list of the reverse pass (the occupancy cells are dead by now:
	// the list lives in their storage).  The order of the list depends on the order the atomics
	// retire in; nothing that is computed from it does (every entry's contribution is added in
	// exact fixed point below).
	const int cyLo = max(2, ((ey0 - 2 + 1) / 2) * 2), cxLo = max(2, ((ex0 - 2 + 1) / 2) * 2);
	const int cyHi = min(ey1 + 2, H3 - 4), cxHi = min(ex1 + 2, W3 - 4);  // inclusive, < dim-3
	const int nwy = cyHi >= cyLo ? (cyHi - cyLo) / 2 + 1 : 0;
	const int nwx = cxHi >= cxLo ? (cxHi - cxLo) / 2 + 1 : 0;
	const bool jac = JAC && wantJac;
	EDGE_COUNT(10, npx);
	EDGE_COUNT(11, ew * eh);
	EDGE_COUNT(12, nwy * nwx);
	if (ec.stats && threadIdx.x == 0)  // ebo_edge_work_stats only: the work this unit's evaluation is made of
	{
		atomicAdd(&ec.stats[0], 1ull);
		atomicAdd(&ec.stats[1], static_cast<unsigned long long>(nEv));
		atomicAdd(&ec.stats[2], static_cast<unsigned long long>(npx));
		atomicAdd(&ec.stats[3], static_cast<unsigned long long>(ew * eh));
		atomicAdd(&ec.stats[4], static_cast<unsigned long long>(nwy * nwx));
	}
	const bool claim = JAC && (wantJac || keepFwd);  // keepFwd: for the Jacobian evaluation that may follow at this point
	if (!reuseFwd)  // (reuseFwd: r comes in with the record, the claims are where that evaluation left them)
	{
	double acc[1] = {0.0};
	// (Round 5 measured a separable, sliding form -- a lane owns a column of windows over a run of five window rows:
	// 2 n + 3 rows of 5 reads for n windows, 40 % of the compare / select groups -- and it is SLOWER everywhere,
	// +1.3 % at the reference default, +6 % at C2 and C4: half the instructions, but 13 dependent read -> compare steps
	// per lane instead of 25 reads in flight at once, on half the lanes.  profiles/r05_edge_levers.txt)
	for (int k = threadIdx.x; k < ((ec.ablate & 2) ? 0 : nwy * nwx); k += blockDim.x)
	{
		const int cy = cyLo + 2 * (k / nwx), cx = cxLo + 2 * (k % nwx);
		double best = 0.0;
		int bestP = -1;
#pragma unroll
		for (int i = -2; i <= 2; ++i)
		{
			// (a window row beyond E's stored rows reads the row of zeros at their end)
			const int rowP = (clamp_med3(cy + i, qy0, qy1) - qy0) * bc + (cx - bx0);
#pragma unroll
			for (int j = -2; j <= 2; ++j)
			{
				const int p = rowP + j;
				const double v = lds_ld(E + p);
				if (v > best)
				{
					best = v;
					bestP = p;
				}
			}
		}
		if (best > 0.0)
		{
			acc[0] += best / c.max_res;
			if (claim && cnt_claim(cnt, bestP, cnt4) == 0)
			{
				const int at = atomicAdd(&ired[64], 1);
				if (at < listCap)
				{
					list[at] = bestP;
				}
			}
		}
	}
	block_sum<1>(acc, red);
	EDGE_TICK(5);
	r = c.max_res - acc[0];
	}
	j0 = 0.0;
	j1 = 0.0;
	if (!jac)  // JAC = false: the value-only instantiation carries none of what follows
	{
		return;
	}

	// E is dead (block_sum's barriers are behind every window): under ALIAS its storage becomes
	// the adjoint image A.
	// (only the rows that hold taps, y0 .. y1, are ever read back -- by the gather pass, at the event taps: the rows
	// above and below collect terms nobody asks for, on whatever E left there)
	const int aLo = (y0 - qy0) * bc, aHi = (y1 - qy0 + 1) * bc;
	if (ALIAS)
	{
		for (int p = aLo + threadIdx.x; p < aHi; p += blockDim.x)
		{
			A[p] = 0.0;
		}
	}
	const int nList = min(ired[64], listCap);
	EDGE_COUNT(13, nList);
	if (ec.stats && threadIdx.x == 0)
	{
		atomicAdd(&ec.stats[5], static_cast<unsigned long long>(nList));
	}
	__syncthreads();
	EDGE_TICK(6);
	// reverse through eigenvalue -> tensor -> differences -> A = dr/dI.
	// The three adjoint terms a tap sends to (x+1, y), (x, y+1) and (x, y) are combined per
	// pixel of the entry's 8x8 footprint in registers first: 64 LDS atomics per entry
	// instead of 147; and consecutive lanes take entries a prime stride apart instead of
	// consecutive ones (neighbouring entries have overlapping footprints, and same-address
	// atomics serialise).
	// A is accumulated in EXACT FIXED POINT like the value image: integer adds commute, so the
	// Jacobian is bit-reproducible run to run, and ds_add_u64 is the faster LDS atomic.  The grid
	// follows from a bound that needs no pass over the entries: the partial derivatives of the
	// first eigenvalue are bounded, 0 <= d lam/d s00, d lam/d s11 <= 1 and |d lam/d s01| <= 1
	// (lam = (tr + d)/2, d^2 = (s00 - s11)^2 + 4 s01^2 >= (s00 - s11)^2, 4 s01^2), a pixel is the
	// argmax of at most 9 windows, so |a00|, |a11|, |a01| <= 9 / 1e3 (x 2: rounding slack of the
	// cancelling form the reference's arithmetic takes near d = 0), a gradient is at most max I,
	// and one A pixel of one entry collects 4 terms:
	//     |v| <= 4 wmax maxI (2 |a| + |a|) <= 12 wmax maxI (18 / max_res) =: B.
	// bias = 1.5 * 2^(e+1) with 2^e >= B; a term is added as the mantissa of (v + bias), i.e.
	// rounded once onto the 2^(e-51) grid.  An entry whose adjoints break the bound (d = 0 or
	// denormal: the Jet's sqrt derivative is inf/NaN there as well) makes the Jacobian NaN.
	unsigned int stride = 61;
	if (nList % 61 == 0)
	{
		stride = (nList % 67 == 0) ? 71 : 67;  // a prime that does not divide nList
	}
	const double aMax = 18.0 / c.max_res;
	const double bound = 12.0 * ec.w_max * __longlong_as_double(static_cast<long long>(umax[0])) * aMax;
	long long ebits = (__double_as_longlong(bound) >> 52) + 2;  // exponent of 2^e >= bound, + 1 for the bias
	ebits = ebits < 123 ? 123 : ebits;                          // keep the grid normal
	const double revBias = vgpr_pin(__longlong_as_double((ebits << 52) | 0x0008000000000000ll));  // low dword 0
	const int revBiasHi = static_cast<int>(((ebits << 52) | 0x0008000000000000ll) >> 32);
	const double revScale = __longlong_as_double((ebits - 52) << 52);  // one grid step
	unsigned long long* Aq = reinterpret_cast<unsigned long long*>(A);
	int broken = 0;
	const double negInvMaxRes = -1.0 / c.max_res;
	// Per entry, straight-line code (no branch inside: as in the scatter pass, the branchy form paid a
	// scalar reload and a full LDS drain per tap).  The domain clipping of the taps is folded into
	// the 1-D weights -- the tensor weights are separable, w(i,j) = N g(i) g(j), and a clipped column
	// or row gets g = 0 --, so the sums are the ones tensor_runs forms (same operations, same order:
	// the eigenvalue re-derived here has the bits of E) and no 49-entry table is needed; the
	// adjoint of a tap is  g(j) [gr(i) (...)]  with the row factor hoisted.  All 64 pixels of the
	// 8 x 8 footprint are added unconditionally at clamped addresses: a pixel outside the canvas
	// only ever collects clipped taps, i.e. the integer 0.
	// Whole entries go one per lane and round; the entries of a last, mostly empty round (301 entries on 256
	// lanes leave 45) would keep ONE wave busy for a whole sweep of eight rows while the others wait at the
	// barrier: they are cut into single-row tasks instead (REVTAIL below), spread over every lane.
	const unsigned int nListU = (ec.ablate & 4) ? 0u : static_cast<unsigned int>(nList);
	const unsigned int tailEntries = nListU % blockDim.x;
	// (round 5: also in the rolled, 168-VGPR instantiation when it runs 256-lane workgroups -- the compact layout, three
	// per CU: reference default x 256 windows 1.401 -> 1.350 ms, same bits; at 768 lanes the last round is rarely that empty)
#ifdef EBO_AB
	const bool rowTailOk = (REVU == 8 || blockDim.x <= 256) && !(ec.ablate & 1024);  // (A/B bit 1024: whole entries only)
#else
	const bool rowTailOk = REVU == 8 || blockDim.x <= 256;
#endif
	const bool rowTail = rowTailOk && cs != nullptr && tailEntries != 0 && tailEntries * 8u <= 2u * blockDim.x;
	const unsigned int wholeEntries = rowTail ? nListU - tailEntries : nListU;
	for (unsigned int kk = threadIdx.x; kk < wholeEntries; kk += blockDim.x)
	{
		const unsigned int k = (kk * stride) % static_cast<unsigned int>(nList);  // < 2048 * 71
		int p = list[k];
#ifdef EBO_AB
		if (ec.ablate & 128)  // timing only: entries whose LDS words fall on 32 different bank pairs per half wave
		{
			p = (ey0 + 3 - qy0 + 4 * static_cast<int>(threadIdx.x >> 5)) * bc + (ex0 + 3 - bx0) + static_cast<int>(threadIdx.x & 31);
			p = min(p, nE - 1);
		}
#endif
		const int y = qy0 + p / bc, x = bx0 + p % bc;
		int co[8];
		double gm[7];
#pragma unroll
		for (int j = 0; j < 8; ++j)
		{
			co[j] = min(max(x - 3 + j, 0), W3 - 1) - bx0;
		}
#pragma unroll
		for (int j = 0; j < 7; ++j)
		{
			const int xx = x - 3 + j;
			gm[j] = (xx >= 0 && xx < W3 - 1) ? ec.g[j] : 0.0;
		}
		double cur[8], nxt[8];
		const double lamBar = static_cast<double>(cnt_get(cnt, p, cnt4)) * negInvMaxRes;  // -count / 1e3 to one rounding of the reciprocal
		double a00, a11, a01;
		if (cs)
		{
			// the eigenvalue pass left the eigenvector direction of this pixel: no tensor sums needed
			const double2 dir = cs[p];
			const double h = 0.5 * lamBar;
			a00 = fma(h, dir.x, h);
			a11 = fma(-h, dir.x, h);
			a01 = lamBar * dir.y;
		}
		else
		{
			double s00 = 0.0, s01 = 0.0, s11 = 0.0;
			{
				const double* row = I + (clamp_med3(y - 3, iy0, iy1) - iy0) * bc;
#pragma unroll
				for (int j = 0; j < 8; ++j)
				{
					cur[j] = row[co[j]];
				}
			}
#pragma unroll
			for (int i = -3; i <= 3; ++i)
			{
				const int yy = y + i;
				{
					const double* row = I + (clamp_med3(yy + 1, iy0, iy1) - iy0) * bc;
#pragma unroll
					for (int j = 0; j < 8; ++j)
					{
						nxt[j] = row[co[j]];
					}
				}
				double h00 = 0.0, h01 = 0.0, h11 = 0.0;
#pragma unroll
				for (int j = 0; j < 7; ++j)
				{
					const double c0 = cur[j];
					const double gx = cur[j + 1] - c0;
					const double gy = nxt[j] - c0;
					h00 = fma(gm[j], gx * gx, h00);
					h01 = fma(gm[j], gx * gy, h01);
					h11 = fma(gm[j], gy * gy, h11);
				}
				const double gr = (yy >= 0 && yy < H3 - 1) ? ec.g[i + 3] : 0.0;
				s00 = fma(gr, h00, s00);
				s01 = fma(gr, h01, s01);
				s11 = fma(gr, h11, s11);
#pragma unroll
				for (int j = 0; j < 8; ++j)
				{
					cur[j] = nxt[j];
				}
			}
			s00 *= ec.norm_st;
			s01 *= ec.norm_st;
			s11 *= ec.norm_st;
			const double tr = s00 + s11;
			const double det = s00 * s11 - s01 * s01;
			const double d = sqrt(tr * tr - 4.0 * det);
			const double dBar = 0.5 * lamBar;
			const double discBar = dBar * (1.0 / (2.0 * d));
			const double trBar = 0.5 * lamBar + 2.0 * tr * discBar;
			const double detBar = -4.0 * discBar;
			a00 = s11 * detBar + trBar;
			a11 = s00 * detBar + trBar;
			a01 = -2.0 * s01 * detBar;
		}
		if (!(fmax(fmax(fabs(a00), fabs(a11)), fabs(a01)) <= aMax))  // also catches NaN
		{
			broken = 1;
			a00 = 0.0;  // the unit's Jacobian becomes NaN below; keep this entry's terms finite
			a11 = 0.0;
			a01 = 0.0;
		}
		// second sweep over the rows: the adjoints of the differences, combined per pixel
		double prevGy[7] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
		{
			const double* row = I + (clamp_med3(y - 3, iy0, iy1) - iy0) * bc;
#pragma unroll
			for (int j = 0; j < 8; ++j)
			{
				cur[j] = row[co[j]];
			}
		}
		const double n2a00 = ec.norm_st * (2.0 * a00), n2a11 = ec.norm_st * (2.0 * a11), na01 = ec.norm_st * a01;
		// REVU = 1 (rolled) where the kernel has 128 or 168 VGPRs: fully unrolled, the eight rows cost 265
		// spilled vector registers there, two rows per trip 124 B of scratch per lane (1.58 -> 1.64 ms);
		// REVU = 8 in the 256-lane instantiation, whose 256 VGPRs hold the unrolled sweep (1.61 -> 1.55 ms)
#pragma unroll REVU
		for (int i = -3; i <= 4; ++i)
		{
			const int yy = y + i;
			{
				const double* row = I + (clamp_med3(yy + 1, iy0, iy1) - iy0) * bc;
#pragma unroll
				for (int j = 0; j < 8; ++j)
				{
					nxt[j] = row[co[j]];
				}
			}
			// row factor; 0 for a clipped row and for the extra row i = 4, which only receives
			const double gr = (i <= 3 && yy >= 0 && yy < H3 - 1) ? ec.g[min(i, 3) + 3] : 0.0;
			const double r00 = gr * n2a00, r11 = gr * n2a11, r01 = gr * na01;
			// row yy of A, columns x-3 .. x+4: +gxBar of the tap to the left, +gyBar of the tap
			// above, -(gxBar + gyBar) of the tap at the pixel itself
			unsigned long long* rowq = Aq + (clamp_med3(yy, qy0, qy1) - qy0) * bc;
			double gxLeft = 0.0;
#pragma unroll
			for (int m = 0; m <= 7; ++m)
			{
				double v = gxLeft;
				if (m <= 6)
				{
					const double c0 = cur[m];
					const double gx = cur[m + 1] - c0;
					const double gy = nxt[m] - c0;
					const double gxBar = gm[m] * fma(gx, r00, gy * r01);
					const double gyBar = gm[m] * fma(gy, r11, gx * r01);
					v = (prevGy[m] - (gxBar + gyBar)) + gxLeft;
					prevGy[m] = gyBar;
					gxLeft = gxBar;
				}
				const double b = v + revBias;
				unsigned int hi = static_cast<unsigned int>(__double2hiint(b) - revBiasHi);
				keep32(hi);  // ONE 32-bit subtract (ebo_kernels.hip)
				const unsigned int lo = static_cast<unsigned int>(__double2loint(b));
				atomicAdd(rowq + co[m], (static_cast<unsigned long long>(hi) << 32) | lo);
			}
#pragma unroll
			for (int j = 0; j < 8; ++j)
			{
				cur[j] = nxt[j];
			}
		}
	}
	// REVTAIL: one task = one row (i = -3 .. 4) of one entry of the last round.  The row needs the adjoint
	// gyBar of the row above it, which the sweep carries from row to row; a task re-derives it from the three
	// image rows it reads (24 LDS reads and ~2.2 rows of arithmetic for one row of output).  Every term is
	// formed by the same expressions from the same operands as in the sweep, and the sum is exact fixed point:
	// the adjoint image has the same bits whichever way an entry is processed.
	for (unsigned int t = threadIdx.x; rowTail && t < tailEntries * 8u; t += blockDim.x)
	{
		const unsigned int kk = wholeEntries + (t >> 3);
		const int i = static_cast<int>(t & 7u) - 3;
		const unsigned int k = (kk * stride) % static_cast<unsigned int>(nList);
		const int p = list[k];
		const int y = qy0 + p / bc, x = bx0 + p % bc;
		int co[8];
		double gm[7];
#pragma unroll
		for (int j = 0; j < 8; ++j)
		{
			co[j] = min(max(x - 3 + j, 0), W3 - 1) - bx0;
		}
#pragma unroll
		for (int j = 0; j < 7; ++j)
		{
			const int xx = x - 3 + j;
			gm[j] = (xx >= 0 && xx < W3 - 1) ? ec.g[j] : 0.0;
		}
		const double lamBar = static_cast<double>(cnt_get(cnt, p, cnt4)) * negInvMaxRes;
		const double2 dir = cs[p];
		const double h = 0.5 * lamBar;
		double a00 = fma(h, dir.x, h), a11 = fma(-h, dir.x, h), a01 = lamBar * dir.y;
		if (!(fmax(fmax(fabs(a00), fabs(a11)), fabs(a01)) <= aMax))
		{
			broken = 1;
			a00 = 0.0;
			a11 = 0.0;
			a01 = 0.0;
		}
		const double n2a00 = ec.norm_st * (2.0 * a00), n2a11 = ec.norm_st * (2.0 * a11), na01 = ec.norm_st * a01;
		const int yy = y + i;
		double rp[8], rc[8], rn[8];
		{
			const double* rowP = I + (clamp_med3(yy - 1, iy0, iy1) - iy0) * bc;
			const double* rowC = I + (clamp_med3(yy, iy0, iy1) - iy0) * bc;
			const double* rowN = I + (clamp_med3(yy + 1, iy0, iy1) - iy0) * bc;
#pragma unroll
			for (int j = 0; j < 8; ++j)
			{
				rp[j] = rowP[co[j]];
				rc[j] = rowC[co[j]];
				rn[j] = rowN[co[j]];
			}
		}
		// gyBar of the row above (row i - 1 of the sweep; none above the first row)
		double prevGy[7];
		{
			const int ip = i - 1, yp = yy - 1;
			const double grP = (ip >= -3 && yp >= 0 && yp < H3 - 1) ? ec.g[max(ip, -3) + 3] : 0.0;
			const double r11 = grP * n2a11, r01 = grP * na01;
#pragma unroll
			for (int m = 0; m < 7; ++m)
			{
				const double c0 = rp[m];
				const double gx = rp[m + 1] - c0;
				const double gy = rc[m] - c0;
				prevGy[m] = (ip >= -3) ? gm[m] * fma(gy, r11, gx * r01) : 0.0;
			}
		}
		const double gr = (i <= 3 && yy >= 0 && yy < H3 - 1) ? ec.g[min(i, 3) + 3] : 0.0;
		const double r00 = gr * n2a00, r11 = gr * n2a11, r01 = gr * na01;
		unsigned long long* rowq = Aq + (clamp_med3(yy, qy0, qy1) - qy0) * bc;
		double gxLeft = 0.0;
#pragma unroll
		for (int m = 0; m <= 7; ++m)
		{
			double v = gxLeft;
			if (m <= 6)
			{
				const double c0 = rc[m];
				const double gx = rc[m + 1] - c0;
				const double gy = rn[m] - c0;
				const double gxBar = gm[m] * fma(gx, r00, gy * r01);
				const double gyBar = gm[m] * fma(gy, r11, gx * r01);
				v = (prevGy[m] - (gxBar + gyBar)) + gxLeft;
				gxLeft = gxBar;
			}
			const double b = v + revBias;
			unsigned int hi = static_cast<unsigned int>(__double2hiint(b) - revBiasHi);
			keep32(hi);  // ONE 32-bit subtract (ebo_kernels.hip)
			const unsigned int lo = static_cast<unsigned int>(__double2loint(b));
			atomicAdd(rowq + co[m], (static_cast<unsigned long long>(hi) << 32) | lo);
		}
	}
	if (broken)
	{
		ired[65] = 1;  // cleared with the list length at the start of the unit
	}
	__syncthreads();
	EDGE_TICK(7);
	// fixed point -> double, in place
	for (int p = aLo + threadIdx.x; p < aHi; p += blockDim.x)
	{
		A[p] = static_cast<double>(static_cast<long long>(Aq[p])) * revScale;
	}
	const bool anyBroken = ired[65] != 0 || ired[64] > listCap;
	__syncthreads();
	EDGE_TICK(8);

	// gather: J_k = sum_e sum_taps A(px) * dI_k contribution of that tap
	double S[2] = {0.0, 0.0};
	for (uint32_t e = threadIdx.x; e < ((ec.ablate & 8) ? 0u : nEv); e += blockDim.x)
	{
		int pxc, pyc;
		double fx, fy, tau;
		if (!warp_event(event_at(e), rx, ry, rw, rh, m0, m1, c, pxc, pyc, fx, fy, tau))
		{
			continue;
		}
		double wx[7], wy[7], ax[7];
		int ci[7];
		axis_taps(fx, c.norm, c, wx);
		axis_taps(fy, 1.0, c, wy);
		const double g = tau * c.inv_sigsq;
		if (kEdgeInterior && pxc >= 3 && pxc + 3 < W3 && pyc >= 3 && pyc + 3 < H3)
		{
			// the footprint lies inside the canvas (almost every event): no clipping, immediate column offsets, single
			// 8-byte reads -- the same products and sums as the clipped form below
#pragma unroll
			for (int i = 0; i < 7; ++i)
			{
				ax[i] = wx[i] * (g * (static_cast<double>(i - 3) - fx));
			}
			const double* rowp = A + (pyc - 3 - qy0) * bc + (pxc - 3 - bx0);
			double d2a = 0.0, d2b = 0.0;
#pragma unroll
			for (int j = 0; j < 7; ++j)
			{
				const double ay = wy[j] * (g * (static_cast<double>(j - 3) - fy));
				double ra = 0.0, rb = 0.0;
#pragma unroll
				for (int i = 0; i < 7; ++i)
				{
					const double a = lds_ld(rowp + i);
					ra = fma(ax[i], a, ra);
					rb = fma(wx[i], a, rb);
				}
				d2a = fma(wy[j], ra, d2a);
				d2b = fma(ay, rb, d2b);
				rowp += bc;
			}
			S[0] += d2a;
			S[1] += d2b;
			continue;
		}
#pragma unroll
		for (int i = 0; i < 7; ++i)
		{
			const int xx = pxc - 3 + i;
			const bool ok = xx >= 0 && xx < W3;
			wx[i] = ok ? wx[i] : 0.0;
			ax[i] = wx[i] * (g * (static_cast<double>(i - 3) - fx));
			ci[i] = min(max(xx, 0), W3 - 1) - bx0;
		}
		// straight-line rows: a clipped row gets zero weights and a clamped address
		double d2a = 0.0, d2b = 0.0;
#pragma unroll
		for (int j = 0; j < 7; ++j)
		{
			const int yy = pyc - 3 + j;
			const double wyj = (yy >= 0 && yy < H3) ? wy[j] : 0.0;
			const double ay = wyj * (g * (static_cast<double>(j - 3) - fy));
			const double* rowp = A + (min(max(yy, 0), H3 - 1) - qy0) * bc;  // (a row with a tap: stored)
			double ra = 0.0, rb = 0.0;
#pragma unroll
			for (int i = 0; i < 7; ++i)
			{
				const double a = rowp[ci[i]];
				ra = fma(ax[i], a, ra);
				rb = fma(wx[i], a, rb);
			}
			d2a = fma(wyj, ra, d2a);
			d2b = fma(ay, rb, d2b);
		}
		S[0] += d2a;
		S[1] += d2b;
	}
	block_sum<2>(S, red);
	EDGE_TICK(9);
	j0 = S[0];
	j1 = S[1];
	if (anyBroken)
	{
		j0 = __longlong_as_double(0x7ff8000000000000ll);
		j1 = j0;
	}
}

// The geometry that follows from the bounding box of a unit's centre taps (xmin .. ymax, canvas coordinates): the taps'
// box, the arrays' box (grown by 8, inside the canvas), the rows I and E / A are stored for -- and whether the arrays fit
// an aliased LDS layout of capPx nominal pixels (see edge_eval_point).  One function for the kernels that evaluate and
// for k_edge_classify, which decides BEFORE the launches which of them evaluates a unit.
struct EdgeBox
{
	int x0, x1, y0, y1;      // the taps
	int bx0, by0, bc, br;    // the arrays' box: origin, columns (= pitch), rows
	int iy0, iRows;          // I's stored rows
	int qy0, qRows;          // E / A / counters' stored rows
};
__device__ __forceinline__ EdgeBox edge_box_of(int xmin, int xmax, int ymin, int ymax, int W3, int H3)
{
	EdgeBox b;
	b.x0 = max(xmin - 3, 0);
	b.x1 = min(xmax + 3, W3 - 1);
	b.y0 = max(ymin - 3, 0);
	b.y1 = min(ymax + 3, H3 - 1);
	b.bx0 = max(b.x0 - 8, 0);
	b.by0 = max(b.y0 - 8, 0);
	b.bc = min(b.x1 + 8, W3 - 1) - b.bx0 + 1;
	b.br = min(b.y1 + 8, H3 - 1) - b.by0 + 1;
	return b;
}
// (after x0 .. y1, bc, br are final: k_solve_edge takes them from its record)
__device__ __forceinline__ void edge_box_rows(EdgeBox& b, int H3)
{
	// I's stored rows: the rows that can hold a tap, y0 .. y1, and one row of zeros on either side (none beyond the canvas)
	b.iy0 = max(b.y0 - 1, 0);
	b.iRows = min(b.y1 + 1, H3 - 1) - b.iy0 + 1;
	// E / A / cnt: the rows the eigenvalue region (y0 - 4 .. y1 + 3 inside the gradient domain) or a tap can touch, plus
	// one row either side inside the canvas
	b.qy0 = max(min(max(b.y0 - 4, 0), b.y0) - 1, 0);
	b.qRows = min(max(min(b.y1 + 3, H3 - 2), b.y1) + 1, H3 - 1) - b.qy0 + 1;
}
// The LDS layouts with aliased E / A place E right behind I's stored rows and the claim counters behind E: a box
// fits when the three arrays fit the bytes of capPx untrimmed pixels and the box has no more pixels than the
// direction table and the argmax list (a window per four pixels) are laid out for (maxPx = ec.cs_stride).
__device__ __forceinline__ bool edge_box_fits_alias(const EdgeBox& b, int capPx, int maxPx, bool cnt4)
{
	const int nI = b.bc * b.iRows, nE = b.bc * b.qRows;
	const int cntInts = cnt4 ? ((nE + 7) >> 3) : nE, capCntInts = cnt4 ? (capPx >> 3) : capPx;
	return 2 * (nI + nE) + cntInts <= 4 * capPx + capCntInts && b.bc * b.br <= maxPx;
}

// The edge objective of one unit at one flow: bounding box of the event taps, then edge_unit on
// LDS arrays when the box fits, else on the unit's global slice.  Every thread gets r, j0, j1.
// ALIAS_LDS selects the LDS layout (a template parameter, not a runtime branch: with three
// inlined copies of edge_unit in one kernel the register allocator spills ~400 VGPRs).
template <bool ALIAS_LDS, bool JAC, int REVU = 1, bool SOLVE = false, int PRE = 0>
__device__ __forceinline__ void edge_eval_point(const uint64_t* __restrict__ ev, const Unit& u, double m0, double m1,
												 bool wantJac, int capPx, char* slice, double* lds,
												 const EvalConsts& c, const EdgeConsts& ec, double2* csUnit, double& r,
												 double& j0, double& j1, int listCap = kEdgeListCap, EdgeReuse* ruArg = nullptr,
												 int hdrDoubles = kEdgeHeader, bool cnt4 = false, int* deferList = nullptr,
												 int* deferCount = nullptr, int deferItem = 0, bool* deferred = nullptr,
												 const int4* bboxPreArg = nullptr)
{
	// PRE: 1 = the box comes from k_edge_classify (no pass over the events compiled in), -1 = never, 0 = decided at run time
	const int4* const bboxPre = PRE < 0 ? nullptr : bboxPreArg;
	EdgeReuse* const ru = SOLVE ? ruArg : nullptr;
	EDGE_TICK_DECL;
	double* red = lds;
	int* ired = reinterpret_cast<int*>(lds + kRedDoubles);
	const int W3 = 3 * u.rw, H3 = 3 * u.rh;

	// (uniform: every thread reads the same record, written before the barrier that separates two evaluations)
	const bool reuse = ru && wantJac && ru->valid == 1.0 && __double_as_longlong(ru->m0) == __double_as_longlong(m0) &&
					   __double_as_longlong(ru->m1) == __double_as_longlong(m1);
	// bounding box of the centre taps that touch the canvas
	int xmin = 0x7fffffff, xmax = -0x7fffffff, ymin = 0x7fffffff, ymax = -0x7fffffff;
	const uint64_t rec0 = threadIdx.x < u.n_ev ? ev[threadIdx.x] : 0ull;
	// (bboxPre: k_edge_classify has made this pass for the whole launch -- the two-launch path of the compact layout)
	for (uint32_t e = threadIdx.x; e < ((reuse || bboxPre || PRE > 0) ? 0u : u.n_ev); e += blockDim.x)
	{
		int pxc, pyc;
		double fx, fy, tau;
		if (warp_event(e == threadIdx.x ? rec0 : ev[e], u.rx, u.ry, u.rw, u.rh, m0, m1, c, pxc, pyc, fx, fy, tau))
		{
			xmin = min(xmin, pxc);
			xmax = max(xmax, pxc);
			ymin = min(ymin, pyc);
			ymax = max(ymax, pyc);
		}
	}
	if (bboxPre || PRE > 0)
	{
		const int4 bb = *bboxPre;
		xmin = __builtin_amdgcn_readfirstlane(bb.x);
		xmax = __builtin_amdgcn_readfirstlane(bb.y);
		ymin = __builtin_amdgcn_readfirstlane(bb.z);
		ymax = __builtin_amdgcn_readfirstlane(bb.w);
	}
	else if (!reuse)
	{
		block_minmax(xmin, xmax, ymin, ymax, ired);
		xmin = __builtin_amdgcn_readfirstlane(xmin);  // (uniform: the geometry that follows lives in scalar registers)
		xmax = __builtin_amdgcn_readfirstlane(xmax);
		ymin = __builtin_amdgcn_readfirstlane(ymin);
		ymax = __builtin_amdgcn_readfirstlane(ymax);
		if (ru && threadIdx.x == 0)
		{
			ru->valid = 0.0;  // the arrays are about to be rebuilt (every thread has read the record: block_minmax's barriers)
		}
	}
	EDGE_TICK(0);
	if (!reuse && xmin > xmax)
	{
		// nothing in the window: mean = 0 <= 1e-4 => penalty (:159-165)
		r = c.max_res * (1.0 + m0 * m0 + m1 * m1);
		j0 = c.max_res * (m0 + m0);
		j1 = c.max_res * (m1 + m1);
		return;
	}
	EdgeBox box = edge_box_of(xmin, xmax, ymin, ymax, W3, H3);
	if (reuse)
	{
		box.x0 = __builtin_amdgcn_readfirstlane(ru->x0);
		box.x1 = __builtin_amdgcn_readfirstlane(ru->x1);
		box.y0 = __builtin_amdgcn_readfirstlane(ru->y0);
		box.y1 = __builtin_amdgcn_readfirstlane(ru->y1);
		box.bx0 = __builtin_amdgcn_readfirstlane(ru->bx0);
		box.by0 = __builtin_amdgcn_readfirstlane(ru->by0);
		box.bc = __builtin_amdgcn_readfirstlane(ru->bc);
		box.br = __builtin_amdgcn_readfirstlane(ru->br);
		r = ru->r;
	}
	edge_box_rows(box, H3);
	const int x0 = box.x0, x1 = box.x1, y0 = box.y0, y1 = box.y1, bx0 = box.bx0, by0 = box.by0, bc = box.bc, br = box.br;
	const int iy0 = box.iy0, iRows = box.iRows, qy0 = box.qy0, qRows = box.qRows;
	const int npx = bc * br;
	const int nIal = bc * iRows;  // <= npx: a box of at most capPx pixels always fits
	const int nE = bc * qRows;
	const bool fits = ALIAS_LDS ? edge_box_fits_alias(box, capPx, ec.cs_stride, cnt4) : npx <= capPx;
	bool fwdDone = false;
	const bool keepFwd = ru != nullptr;
	if (deferList && !fits)
	{
		// the box does not fit this launch's (small) LDS arrays: the unit goes on the list of the launch that follows
		// with the large ones, instead of onto its global slice (k_edge_classify has put it there if it ran)
		if (threadIdx.x == 0 && !bboxPre)
		{
			deferList[atomicAdd(deferCount, 1)] = deferItem;
		}
		*deferred = true;
		EDGE_TICK_FLUSH;
		return;
	}
	if (fits && ALIAS_LDS)
	{
		double* I = lds + hdrDoubles;
		double* E = I + nIal;
		int* cnt = reinterpret_cast<int*>(E + nE);
		edge_unit<true, JAC, REVU, SOLVE>(ev, u, m0, m1, wantJac, bx0, by0, bc, br, iy0, iRows, qy0, qRows, x0, x1, y0, y1, I, E, E, cnt,
						ired + kEdgeCellOff, listCap, red, ired, c, ec, csUnit, rec0, reuse, keepFwd, fwdDone, r, j0, j1, cnt4 EDGE_TICK_PASS);
	}
	else if (fits && !ALIAS_LDS)
	{
		double* I = lds + kEdgeHeader;
		double* E = I + capPx;
		double* A = E + capPx;
		int* cnt = reinterpret_cast<int*>(A + capPx);
		edge_unit<false, JAC, REVU, SOLVE>(ev, u, m0, m1, wantJac, bx0, by0, bc, br, iy0, iRows, qy0, qRows, x0, x1, y0, y1, I, E, A, cnt,
						 ired + kEdgeCellOff, listCap, red, ired, c, ec, csUnit, rec0, reuse, keepFwd, fwdDone, r, j0, j1, false EDGE_TICK_PASS);
	}
	else
	{
		const size_t cap = static_cast<size_t>(W3) * H3;
		double* I = reinterpret_cast<double*>(slice);
		double* E = I + cap;
		double* A = E + cap;
		int* cnt = reinterpret_cast<int*>(A + cap);
		// the list of a box that large goes behind cnt in the slice (a window per 2x2 pixels at most)
		// (REVU 1: the rolled reverse sweep -- this rare path must not set the kernel's register budget)
		edge_unit<false, JAC, 1>(ev, u, m0, m1, wantJac, bx0, by0, bc, br, iy0, iRows, qy0, qRows, x0, x1, y0, y1, I, E, A, cnt,
						 cnt + cap, static_cast<int>(cap / 4) + 64, red, ired, c, ec, nullptr, rec0, false, false, fwdDone, r, j0, j1, false EDGE_TICK_PASS);
		fwdDone = false;  // the global slice is not what the record describes
	}
	if (ru && reuse && threadIdx.x == 0)
	{
		ru->valid = 0.0;  // the reverse pass has taken E's storage and the claims are in cnt: nothing to start from again
	}
	// (only a VALUE-ONLY evaluation leaves E and zero claim counters behind)
	if (ru && !reuse && fwdDone && !wantJac && threadIdx.x == 0)
	{
		// (the next evaluation's threads read this behind the barrier that separates two evaluations)
		ru->m0 = m0;
		ru->m1 = m1;
		ru->r = r;
		ru->bx0 = bx0;
		ru->by0 = by0;
		ru->bc = bc;
		ru->br = br;
		ru->x0 = x0;
		ru->x1 = x1;
		ru->y0 = y0;
		ru->y1 = y1;
		ru->valid = 1.0;
	}
	EDGE_TICK_FLUSH;
}

// Workgroup = unit.  scratch: per-unit global slice for boxes that do not fit LDS.
// JAC = false is the value-only kernel (launches in which no slot wants a Jacobian: 14 of the
// 19 rounds of a reference-default solve): the reverse pass it never runs otherwise costs the
// forward pass registers (measured: a heavier reverse pass slowed VALUE-only launches by 9 %).
// MAXT: the largest workgroup the instantiation is launched with, which sets its register budget --
//    256: 256 VGPRs, two 256-lane workgroups per CU (2 waves per SIMD): the layouts whose canvas fits a
//         CU's LDS twice (the reference's 20x20 patches, C3);
//    512: 256 VGPRs, ONE 512-lane workgroup per CU: the device-resident solve of the other layouts;
//    768: 168 VGPRs, ONE 768-lane workgroup per CU (12 waves = 3 per SIMD): their batched evaluation
//         (+4..6 % over 1024 lanes at 128 VGPRs, C2 and C4).
// None of them spills a vector register.  Round 2 ran 512 / 1024 lanes at 128 VGPRs with 13-31 spilled
// VGPRs in the evaluation and 176-185 in the solve.  (Two 384-lane workgroups per CU at 168 VGPRs do
// not co-reside: six waves land 2+2+1+1 on the four SIMDs and a second workgroup would need a fourth
// wave slot on two of them -- measured 2.55 ms against 1.58 for the reference-default configuration.)
constexpr int edge_min_waves(int maxt) { return maxt == 768 ? 3 : 2; }

// One work item of k_eval_edge: unit bx of the launch's list, flow set `set`.  wgSlot: the index of the WORKGROUP
// that runs it -- the per-evaluation temporaries (the global fallback slice, the eigenvector-direction table) are
// keyed by it, not by the unit: a workgroup uses its slot for one unit at a time.
template <bool ALIAS_LDS, bool JAC, int MAXT>
__device__ __forceinline__ void edge_item(const uint64_t* __restrict__ events, const Unit* __restrict__ units,
										   const double* __restrict__ flows, int wantJac, int capPx, double fdStep,
										   char* __restrict__ scratch, size_t scratchStride, double* __restrict__ sets,
										   double* __restrict__ out, const EvalConsts& c, const EdgeConsts& ec,
										   const unsigned char* __restrict__ modes, const LiveWindows& live, int bx, int set,
										   int nItemsX, int nSets, int wgSlot, double* lds, const int4* __restrict__ bbox)
{
	// live.n > 0: the items cover the units of the listed windows only (ebo_internal.h, LiveWindows)
	int unitIdx = bx, liveMode = -1;
	if (live.n > 0)
	{
		const int k = bx / live.upw;
		const int ent = live.ent[k];
		unitIdx = (ent >> 2) * live.upw + (bx - k * live.upw);
		liveMode = ent & 3;
	}
	const Unit u = units[unitIdx];
	if (u.flags & kUnitStray)
	{
		return;
	}
	// per-flow-slot mode of a lock-step solve: 0 = nothing wanted (output untouched),
	// 1 = value only, 2 = value and Jacobian
	if (modes || liveMode >= 0)
	{
		const int mode = liveMode >= 0 ? liveMode : modes[u.flow_idx];
		if (mode == 0)
		{
			return;
		}
		wantJac = wantJac && mode == 2;
	}
	// one flow set: results go straight to out[flow slot]; five sets (central
	// differences): to the staging array [set][unit][3] that k_edge_central reduces
	double* dst = (nSets == 1) ? out + 3 * static_cast<size_t>(u.flow_idx)
							   : sets + (static_cast<size_t>(set) * nItemsX + bx) * 3;
	if (!(u.flags & kUnitActive))
	{
		if (threadIdx.x < 3)
		{
			dst[threadIdx.x] = 0.0;
		}
		return;
	}
	double m0 = flows[2 * u.flow_idx];
	double m1 = flows[2 * u.flow_idx + 1];
	fd_offset(set, fdStep, m0, m1);
	double r, j0, j1;
	edge_eval_point<ALIAS_LDS, JAC, (MAXT == 256 ? 8 : 1)>(events + u.ev_off, u, m0, m1, wantJac != 0, capPx,
									scratch + static_cast<size_t>(wgSlot) * scratchStride,
									lds, c, ec,
									// (the eigenvector directions are for the reverse pass: a unit of a mixed round that only wants its value writes none)
									(ec.cs && nSets == 1 && wantJac) ? reinterpret_cast<double2*>(ec.cs) + static_cast<size_t>(wgSlot) * ec.cs_stride : nullptr,
									r, j0, j1, kEdgeListCap, nullptr, kEdgeHeader, false, nullptr, nullptr, 0, nullptr,
									bbox ? bbox + bx : nullptr);
	if (threadIdx.x == 0)
	{
		dst[0] = r;
		dst[1] = j0;
		dst[2] = j1;
	}
}

// PERSISTENT workgroups (round 5) for the 20 B layout: the grid is what the chip holds at once (two 256-lane workgroups
// per CU) and every workgroup walks the launch's items bx = blockIdx.x, + gridDim.x, ...; the per-evaluation temporaries
// (direction table, global slice) shrink from one slot per UNIT (1.6 GB for 256 reference-default windows) to one per
// resident WORKGROUP (29 MB).  Measured: the same time as one workgroup per item (1.537 against 1.540 ms) -- workgroup
// launch, argument loads and the table's HBM misses were hidden already; kept for the memory and because the launch of
// the deferred units (below) needs a grid that does not depend on a count only the device knows.  Same bits.
struct EdgeKArgs
{
	const uint64_t* events;
	const Unit* units;
	const double* flows;
	int wantJac;
	int capPx;
	double fdStep;
	char* scratch;
	size_t scratchStride;
	double* sets;
	double* out;
	EvalConsts c;
	EdgeConsts ec;
	const unsigned char* modes;
	LiveWindows live;
	int nItemsX;  // units (or units of the listed windows) per flow set
	int nSets;    // 1, or 5 (central differences)
	const int* itemList;   // null, or DEVICE list of the items (bx) this launch evaluates: what the launch of the compact layout deferred
	const int* itemCount;  // its DEVICE length
	const int4* bbox;      // null, or DEVICE [items]: the tap bounding boxes k_edge_classify computed for this launch's flows
};

// The one argument IS the kernel-argument segment, and the persistent loop (the 256-lane instantiations: two
// workgroups per CU) reads it through a pointer that is laundered in every iteration: what an item's prologue needs (unit table, flows, modes, window list, destinations) is then a few scalar
// loads at the top of the item instead of scalar registers held -- and, under this kernel's pressure, spilled to
// vector-register lanes -- across the whole evaluation of the item before it.
template <bool ALIAS_LDS, bool JAC, int MAXT>
__global__ void __launch_bounds__(MAXT, edge_min_waves(MAXT)) k_eval_edge(EdgeKArgs unusedByName)
{
	extern __shared__ double lds[];
	static_assert(MAXT == 256, "the persistent loop is built for the 256-lane instantiations (k_eval_edge_wg: the others)");
	typedef const __attribute__((address_space(4))) EdgeKArgs* KArgPtr;
	const KArgPtr ka = (KArgPtr)__builtin_amdgcn_kernarg_segment_ptr();
	for (int item = blockIdx.x;; item += gridDim.x)  // uniform: every wave leaves after the same item
	{
		KArgPtr kl = ka;
		asm volatile("" : "+s"(kl));
		const EdgeKArgs& k = *(const EdgeKArgs*)kl;
		const int nItemsX = k.nItemsX, nSets = k.nSets;
		const int* const itemList = k.itemList;
		if (item >= (itemList ? *k.itemCount : nItemsX * nSets))
		{
			break;
		}
		int bx = itemList ? itemList[item] : item, set = 0;  // central differences: 5 value-only sets
		if (nSets != 1)
		{
			set = item / nItemsX;
			bx = item - set * nItemsX;
		}
		edge_item<ALIAS_LDS, JAC, MAXT>(k.events, k.units, k.flows, k.wantJac, k.capPx, k.fdStep, k.scratch, k.scratchStride, k.sets,
										k.out, k.c, k.ec, k.modes, k.live, bx, set, nItemsX, nSets, static_cast<int>(blockIdx.x), lds, k.bbox);
		__syncthreads();  // the next item's arrays and scalars are written only after every read of this one
	}
}

// One workgroup per item (rounds 1-4), kept for the 768-lane instantiations: at 168 VGPRs the persistent loop of
// k_eval_edge costs them 25-89 spilled vector registers whichever way its arguments travel.  Launched with 256 lanes
// and the compact layout (EdgeCompact: 52 KB of LDS) the same instantiation runs THREE workgroups per CU -- round 5's
// gain on the reference default: 1.63 -> 1.38 ms for 256 windows on one box, same bits.
template <bool ALIAS_LDS, bool JAC, int MAXT, bool PRE = false>
__global__ void __launch_bounds__(MAXT, edge_min_waves(MAXT)) k_eval_edge_wg(const uint64_t* __restrict__ events,
													const Unit* __restrict__ units,
													const double* __restrict__ flows, int wantJac,
													int capPx, double fdStep, char* __restrict__ scratch,
													size_t scratchStride, double* __restrict__ sets,
													double* __restrict__ out, EvalConsts c, EdgeConsts ec,
													const unsigned char* __restrict__ modes, LiveWindows live, EdgeCompact cp,
													const int4* __restrict__ bbox)
{
	extern __shared__ double lds[];
	// live.n > 0: the grid covers the units of the listed windows only (ebo_internal.h, LiveWindows)
	int unitIdx = blockIdx.x, liveMode = -1;
	if (live.n > 0)
	{
		const int k = blockIdx.x / live.upw;
		const int ent = live.ent[k];
		unitIdx = (ent >> 2) * live.upw + (blockIdx.x - k * live.upw);
		liveMode = ent & 3;
	}
	const Unit u = units[unitIdx];
	const int set = blockIdx.y;  // central differences: 5 value-only sets
	if (u.flags & kUnitStray)
	{
		return;
	}
	// per-flow-slot mode of a lock-step solve: 0 = nothing wanted (output untouched),
	// 1 = value only, 2 = value and Jacobian
	if (modes || liveMode >= 0)
	{
		const int mode = liveMode >= 0 ? liveMode : modes[u.flow_idx];
		if (mode == 0)
		{
			return;
		}
		wantJac = wantJac && mode == 2;
	}
	// one flow set: results go straight to out[flow slot]; five sets (central
	// differences): to the staging array [set][unit][3] that k_edge_central reduces
	double* dst = (gridDim.y == 1) ? out + 3 * static_cast<size_t>(u.flow_idx)
								   : sets + (static_cast<size_t>(set) * gridDim.x + blockIdx.x) * 3;
	if (!(u.flags & kUnitActive))
	{
		if (threadIdx.x < 3)
		{
			dst[threadIdx.x] = 0.0;
		}
		return;
	}
	double m0 = flows[2 * u.flow_idx];
	double m1 = flows[2 * u.flow_idx + 1];
	fd_offset(set, fdStep, m0, m1);
	double r, j0, j1;
	bool deferred = false;
	edge_eval_point<ALIAS_LDS, JAC, (MAXT == 256 ? 8 : 1), false, (PRE ? 1 : -1)>(events + u.ev_off, u, m0, m1, wantJac != 0, capPx,
									scratch + static_cast<size_t>(blockIdx.y * gridDim.x + blockIdx.x) * scratchStride,
									lds, c, ec,
									// (the eigenvector directions are for the reverse pass: a unit of a mixed round that only wants its value writes none)
									(ec.cs && gridDim.y == 1 && wantJac) ? reinterpret_cast<double2*>(ec.cs) + static_cast<size_t>(blockIdx.x) * ec.cs_stride : nullptr,
									r, j0, j1, cp.list_cap > 0 ? cp.list_cap : kEdgeListCap, nullptr, cp.list_cap > 0 ? cp.hdr_doubles : kEdgeHeader,
									cp.list_cap > 0, cp.defer_list, cp.defer_count, static_cast<int>(blockIdx.x), &deferred,
									bbox ? bbox + blockIdx.x : nullptr);
	if (deferred)
	{
		return;  // (uniform) the launch of the large boxes evaluates this unit
	}
	if (threadIdx.x == 0)
	{
		dst[0] = r;
		dst[1] = j0;
		dst[2] = j1;
	}
}

// The bounding-box pass of a whole launch in ONE small kernel (a wave per unit, no LDS, sixteen waves per CU) in front of
// the two launches of the compact path: the evaluating workgroups read their box instead of making the pass at three /
// two workgroups per CU, and the units whose arrays do not fit the compact layout are on the second launch's list before
// either launch starts.  Same integers as the pass inside edge_eval_point (min / max of the same warped taps), the same
// fit test (edge_box_fits_alias): same results.
__global__ void __launch_bounds__(1024) k_edge_classify(const uint64_t* __restrict__ events, const Unit* __restrict__ units,
														const double* __restrict__ flows, const unsigned char* __restrict__ modes,
														LiveWindows live, int nItems, int capPx, int maxPx, EvalConsts c,
														int4* __restrict__ bbox, int* __restrict__ deferList, int* __restrict__ deferCount)
{
	// sixteen units per workgroup, one list reservation per workgroup (one atomic per unit on the one counter took
	// 94 us at the ground-truth flows, where a third of 27 648 units goes on the list)
	__shared__ int nDefer, base;
	__shared__ int mine[16];
	const int wave = static_cast<int>(threadIdx.x >> 6);
	const int item = blockIdx.x * 16 + wave;
	const uint32_t lane = threadIdx.x & 63u;
	if (threadIdx.x == 0)
	{
		nDefer = 0;
	}
	__syncthreads();
	bool evaluated = item < nItems;
	int unitIdx = evaluated ? item : 0, liveMode = -1;
	if (evaluated && live.n > 0)
	{
		const int k = item / live.upw;
		const int ent = live.ent[k];
		unitIdx = (ent >> 2) * live.upw + (item - k * live.upw);
		liveMode = ent & 3;
	}
	const Unit u = units[unitIdx];
	// (a unit that is never evaluated -- stray, inactive, mode 0 -- has no box: nobody reads it)
	evaluated = evaluated && !(u.flags & kUnitStray) && (u.flags & kUnitActive);
	if (evaluated && (modes || liveMode >= 0) && (liveMode >= 0 ? liveMode : modes[u.flow_idx]) == 0)
	{
		evaluated = false;
	}
	int slot = -1;
	if (evaluated)  // (uniform per wave)
	{
		const double m0 = flows[2 * u.flow_idx], m1 = flows[2 * u.flow_idx + 1];
		const uint64_t* ev = events + u.ev_off;
		int xmin = 0x7fffffff, xmax = -0x7fffffff, ymin = 0x7fffffff, ymax = -0x7fffffff;
		for (uint32_t e = lane; e < u.n_ev; e += 64u)
		{
			int pxc, pyc;
			double fx, fy, tau;
			if (warp_event(ev[e], u.rx, u.ry, u.rw, u.rh, m0, m1, c, pxc, pyc, fx, fy, tau))
			{
				xmin = min(xmin, pxc);
				xmax = max(xmax, pxc);
				ymin = min(ymin, pyc);
				ymax = max(ymax, pyc);
			}
		}
		xmin = wave_min(xmin);
		xmax = wave_max(xmax);
		ymin = wave_min(ymin);
		ymax = wave_max(ymax);
		if (lane == kWaveResultLane)
		{
			bbox[item] = make_int4(xmin, xmax, ymin, ymax);
			if (xmin <= xmax)  // (an empty window is the penalty branch: no arrays)
			{
				const int H3 = 3 * u.rh;
				EdgeBox box = edge_box_of(xmin, xmax, ymin, ymax, 3 * u.rw, H3);
				edge_box_rows(box, H3);
				if (!edge_box_fits_alias(box, capPx, maxPx, true))
				{
					slot = atomicAdd(&nDefer, 1);
					mine[slot] = item;
				}
			}
		}
	}
	__syncthreads();
	if (threadIdx.x == 0 && nDefer > 0)
	{
		base = atomicAdd(deferCount, nDefer);
	}
	__syncthreads();
	if (static_cast<int>(threadIdx.x) < nDefer)
	{
		deferList[base + threadIdx.x] = mine[threadIdx.x];
	}
}

// EBO_SOLVE_INDEPENDENT with the edge loss in ONE launch: workgroup = unit runs the whole
// per-patch LM (lm_unit) on top of edge_eval_point -- the reference's own objective with no host
// round trip per LM round.  The JAC instantiation serves both kinds of evaluation (the flag is a
// runtime argument of edge_unit; calling the value-only instantiation for the cost evaluations
// as well doubles the code and gains nothing: 200 ms either way for 256 reference-default windows).
template <bool ALIAS_LDS, int MAXT>
__global__ void __launch_bounds__(MAXT, edge_min_waves(MAXT)) k_solve_edge(const uint64_t* __restrict__ events,
													 const Unit* __restrict__ units, int capPx,
													 char* __restrict__ scratch, size_t scratchStride,
													 double* __restrict__ flowsOut, int32_t* __restrict__ stats,
													 EvalConsts c, EdgeConsts ec, SolveConsts o, int noReuse)
{
	extern __shared__ double lds[];
	const Unit u = units[blockIdx.x];
	const uint64_t* ev = events + u.ev_off;
	char* slice = scratch + static_cast<size_t>(blockIdx.x) * scratchStride;
	double2* csUnit = ec.cs ? reinterpret_cast<double2*>(ec.cs) + static_cast<size_t>(blockIdx.x) * ec.cs_stride : nullptr;
	int iteration = 0, evalsCost = 0, evalsJac = 0, termination = 0;
	double best0 = 0.0, best1 = 0.0;
	if (u.flags & kUnitActive)
	{
		// the solver state: LDS, behind the argmax list (kEdgeLmInts); thread 0 runs the solver
		int* const reserved = reinterpret_cast<int*>(lds + kRedDoubles) + kEdgeCellOff + kEdgeListCap - kEdgeLmInts;
		EdgeReuse* ru = noReuse ? nullptr : reinterpret_cast<EdgeReuse*>(reserved);
		LmUnit& lm = *reinterpret_cast<LmUnit*>(reserved + kEdgeReuseInts);
		if (threadIdx.x == 0)
		{
			lm.begin();
			if (ru)
			{
				ru->valid = 0.0;
			}
		}
		for (;;)
		{
			__syncthreads();  // the point to evaluate (or the end) is published; every thread is past the previous evaluation
			if (!lm.more)
			{
				break;
			}
			const double q0 = lm.q0, q1 = lm.q1;
			const bool qJac = lm.qJac;
			double r, a, b;
			// (the eigenvector directions are for the reverse pass: with the record, a cost evaluation leaves them
			// behind for the Jacobian evaluation that may follow at the same point; without it, it writes none)
			edge_eval_point<ALIAS_LDS, true, 1, true>(ev, u, q0, q1, qJac, capPx, slice, lds, c, ec, (qJac || ru) ? csUnit : nullptr, r, a, b,
											 kEdgeListCap - kEdgeLmInts, ru);
			if (threadIdx.x == 0)
			{
				lm.more = lm.advance(r, a, b, o) ? 1 : 0;
			}
		}
		if (threadIdx.x == 0)
		{
			iteration = lm.iteration;
			evalsCost = lm.evalsCost;
			evalsJac = lm.evalsJac;
			termination = lm.termination;
			best0 = lm.best0;
			best1 = lm.best1;
		}
	}
	if (threadIdx.x == 0 && !(u.flags & kUnitStray))
	{
		flowsOut[2 * u.flow_idx] = best0;
		flowsOut[2 * u.flow_idx + 1] = best1;
		if (stats)
		{
			stats[4 * u.flow_idx + 0] = iteration;
			stats[4 * u.flow_idx + 1] = evalsCost;
			stats[4 * u.flow_idx + 2] = evalsJac;
			stats[4 * u.flow_idx + 3] = termination;
		}
	}
}

// central differences of the value-only edge objective: sets [5][units][3] -> out
__global__ void k_edge_central(const Unit* __restrict__ units, int nUnits, double fdStep,
							   const double* __restrict__ sets, double* __restrict__ out)
{
	const int unit = blockIdx.x * blockDim.x + threadIdx.x;
	if (unit >= nUnits)
	{
		return;
	}
	const Unit u = units[unit];
	if (u.flags & kUnitStray)
	{
		return;
	}
	const size_t n3 = static_cast<size_t>(nUnits) * 3;
	const double r = sets[3 * unit];
	double j0 = 0.0, j1 = 0.0;
	if (u.flags & kUnitActive)
	{
		j0 = (sets[n3 + 3 * unit] - sets[2 * n3 + 3 * unit]) / (2.0 * fdStep);
		j1 = (sets[3 * n3 + 3 * unit] - sets[4 * n3 + 3 * unit]) / (2.0 * fdStep);
	}
	out[3 * u.flow_idx] = r;
	out[3 * u.flow_idx + 1] = j0;
	out[3 * u.flow_idx + 2] = j1;
}
