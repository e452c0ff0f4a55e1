// ebo_eval3.inc — the variance objective of one unit at one flow (k_eval3, and the evaluation inside
// k_solve_independent), included inside ebo_kernels.hip's anonymous namespace.
//
// Scatter the VALUE, gather the DERIVATIVES.  The Jacobian of the variance objective needs only
// D1k = sum_px dI_k  and  D2k = sum_px I dI_k  over the touched pixels (every touched pixel has I > 0:
// Gaussian taps are strictly positive).  With dI_k(px) = sum_e d_k(e, px):
//     D1k = sum_e sum_taps d_k(e,tap)                    -- no image at all
//     D2k = sum_e sum_taps I(px(e,tap)) d_k(e,tap)       -- a READ of the value image
// i.e. forward-mode Jets are re-associated into "value image, then one gather pass": 49 LDS atomics +
// 49 LDS reads per event instead of 147 atomics, and a third of the LDS.  Mathematically identical to
// the Jet result.
//
// Further: (a) the image covers only the bounding box of the warped events inside the 3W x 3H canvas
// (the canvas is mostly empty), split in `tiles` row bands (parallel workgroups) and, if a band exceeds
// the workgroup's LDS, in sequential sub-bands; (b) taps accumulate as exact 64-bit fixed point
// (ds_add_u64): tap values are < 0.5, so (v + 1.5) has ulp 2^-52 and its mantissa IS the fixed-point
// number.  Integer adds commute: the image, and with the fixed reduction order the whole result, is
// bit-reproducible from run to run; it is also faster than ds_add_f64 under same-address conflicts
// (tools/microbench/lds_atomics.hip); (c) the 7 taps of an axis come from 3 exps:
// exp(hs (k-f)^2) = exp(hs k^2) exp(hs f^2) exp(f/s^2)^k; (d) k_eval3 deals a unit's events once per evaluation so that
// the lanes of one LDS instruction fall on different bank pairs (eval_deal.h; the block in front of the sub-band loop).
//
// What binds is the instruction count per tap (a straightforward version of this algorithm took ~1000
// VALU instructions per event by its PMC profile), hence:
//   * interior fast path: an event whose 7x7 footprint lies inside the band (almost all
//     of them) runs unpredicated loops: per tap  v_mul_f64 + ds_add_u64
//     with immediate offsets (scatter) /  ds_read_b64 + 2 v_fma_f64 (gather: the row's weighted sum and its first moment,
//     tap_moments.h -- no derivative factor per tap); in k_eval3 a unit whose every event is
//     such an event, known from the box alone (eval_interior.h), runs its event loops without asking (INNER);
//   * the fixed-point value is the bit pattern of the SUBNORMAL product of the two pre-scaled
//     weights (value_tap): the exact product is rounded ONCE onto the 2^(k-52) grid.  Where the
//     weights can be tiny (sigma < 1) it is  fma(wx, wy, bias): bias = 1.5 * 2^k has a zero low
//     dword, so removing it is a 32-bit subtract on the high dword (fix_tap);
//   * exp on [-1, 1] without range reduction (Taylor on x/4, two squarings; exp(a) and exp(-a) share
//     their even and odd parts: exp_taps.h) when sigma >= 1 (the reference's sigma is 1).

// SMALL (sigma >= 1): hs f^2 lies in [-0.5, 0] and |a| <= 1 (|f| < 1), the ranges of exp_taps.h's polynomials; exp(a)
// and exp(-a) come as a pair from one cosh / sinh evaluation.
template <bool SMALL>
__device__ __forceinline__ void axis_taps3(double f, double pre, const EvalConsts& c, double hsQ, double isQ, double (&w)[7])
{
	// SMALL: the polynomials' quarter arguments straight from the quarter constants (exact: powers of two), one
	// multiply less per exponential and per pair
	const double e0 = pre * (SMALL ? exp_gauss_quarter(hsQ * (f * f)) : exp(c.hs * (f * f)));
	double p, q;
	if (SMALL)
	{
		exp_pair_quarter(f * isQ, p, q);
	}
	else
	{
		const double a = f * c.inv_sigsq;
		p = exp(a);
		q = exp(-a);
	}
	const double p2 = p * p, q2 = q * q;
	const double e1 = c.ck1 * e0, e2 = c.ck2 * e0, e3 = c.ck3 * e0;
	w[3] = e0;
	w[4] = e1 * p;
	w[5] = e2 * p2;
	w[6] = e3 * (p2 * p);
	w[2] = e1 * q;
	w[1] = e2 * q2;
	w[0] = e3 * (q2 * q);
}

// SMALL = false: a tap below half a grid step is stored as one step, not 0.  The reference counts every pixel
// with a value > 0 (contrast_functor.h:113) and the gather sums the derivatives of every tap; for sigma < ~0.6
// the outer taps fall below the grid (at sigma >= 1 the smallest tap, norm e^-16, is 1e8 steps).
template <bool SMALL>
__device__ __forceinline__ unsigned long long fix_tap(double wx, double wy, double bias, int biasHi)
{
	const double b = fma(wx, wy, bias);
	unsigned int hi = static_cast<unsigned int>(__double2hiint(b) - biasHi);
	keep32(hi);  // ONE 32-bit subtract (ebo_kernels.hip)
	const unsigned int lo = static_cast<unsigned int>(__double2loint(b));
	const unsigned long long q = (static_cast<unsigned long long>(hi) << 32) | lo;
	return (!SMALL && q == 0ull && wx * wy > 0.0) ? 1ull : q;
}

// The scatter's tap.  sub: wx and wy carry the prefactors 2^-511 norm and 2^-(511 + k) (unit_fix_grid), their product is
// subnormal and its bit pattern is the fixed-point word: ONE v_mul_f64, rounded once to nearest even onto the same grid
// as the biased form, so the same word (fix_form.h; the kernels run with f64 denormals on, float_denorm_mode_16_64 = 3).
template <bool SMALL, bool SUB>
__device__ __forceinline__ unsigned long long value_tap(double wx, double wy, double bias, int biasHi)
{
	return SUB ? static_cast<unsigned long long>(__double_as_longlong(wx * wy)) : fix_tap<SMALL>(wx, wy, bias, biasHi);
}

// What a device-resident solve keeps of an evaluation for the NEXT one (k_solve_independent; in LDS behind the
// bounding-box scratch).  The trust-region loop evaluates the cost at a candidate and, when it accepts the
// step, value AND Jacobian at the very same point: the second evaluation's bounding box, scatter and
// conversion would rebuild, bit for bit, the image that is still in LDS.  With this record it runs the gather
// pass only and takes the three value sums from here -- same operations on the same operands, so the same
// (r, J) as the full evaluation (18 of a C3 patch's 54 evaluations lose 2/3 of their work).  Valid only for an
// image that fitted ONE band (else the LDS holds its last sub-band only).
struct EvalReuse
{
	double valid;        // 1.0: the fields below describe the image in LDS
	double m0, m1;       // the flow it was built at (compared bit for bit)
	double x0, y0, bw, rows;
	double s0, s1, s2;   // sum I, sum I^2, number of non-zero pixels
};

// D1S: which pass forms the image-free Jacobian sums D1k (S[3], S[4]).  They need the weights only, so either pass
// can.  k_eval3 forms them in the scatter (D1S = true; only where wantJac is set): that takes the four sums and their
// two accumulators, 12 registers live across the gather's rows, out of the pass that needs registers for its rows
// (measured, DESIGN.md 4.1 item 16: the move alone costs 1 %, the gather's table without the move 1.5 %,
// both together nothing, and they leave the registers the cheaper exponentials need).  k_solve_independent keeps them
// in the gather (D1S = false): an EvalReuse hit runs no scatter.  Same operations on the same operands in the same order
// either way (the scatter's weights carry exact power-of-two prefactors in the subnormal form, taken off each sum
// by one exact multiply BEFORE the two products, which would underflow scaled), so S[3] and S[4] have the same bits.
template <bool SMALL, bool D1S>
__device__ __forceinline__ void eval_unit3(const uint64_t* __restrict__ ev, const Unit& u, double m0,
											double m1, bool wantJac, int tile, int tiles,
											int capDoubles, const EvalConsts& c, double* lds,
											double (&S)[7], int hdrWaves, EvalReuse* ru = nullptr,
											const int32_t* __restrict__ ext = nullptr,
											[[maybe_unused]] unsigned int* boxStats = nullptr,
											[[maybe_unused]] bool dealOff = false, [[maybe_unused]] uint32_t* dealDump = nullptr,
											[[maybe_unused]] bool interiorOff = false)
{
	EDGE_TICK_DECL;
	// the header is sized for hdrWaves waves (eval_plan.h; uniform): the sums, block_minmax's scratch, then the image
	double* red = lds;
	int* ired = reinterpret_cast<int*>(lds + ebo::eval_sum_doubles(hdrWaves));
	double* img = lds + ebo::eval_header_doubles(hdrWaves);
	unsigned long long* imgq = reinterpret_cast<unsigned long long*>(img);
	const int rx = u.rx, ry = u.ry, rw = u.rw, rh = u.rh;
	const int W3 = 3 * rw, H3 = 3 * rh;
	const uint32_t nEv = u.n_ev;
#pragma unroll
	for (int k = 0; k < 7; ++k)
	{
		S[k] = 0.0;
	}
	// Optional register cache of a thread's events across the three passes.  Measured:
	// the kCache-times unrolled pass bodies push the kernel to > 3 KB/lane of scratch, so
	// it is compiled out; every pass re-reads its events (L1/L2 hits after pass A).
	constexpr int kCache = 4;
	constexpr bool kUseCache = false;
	const bool cached = kUseCache && nEv <= kCache * blockDim.x;
	uint64_t recs[kCache];
	if (cached)
	{
#pragma unroll
		for (int k = 0; k < kCache; ++k)
		{
			const uint32_t e = threadIdx.x + k * blockDim.x;
			recs[k] = (e < nEv) ? ev[e] : 0ull;
		}
	}
	// D1S: the unit's dealt list (eval_deal.h), null until it is built and where the unit is not dealt; position q holds the
	// canonical index of the event that lane q mod blockDim takes in round q div blockDim
	[[maybe_unused]] const uint16_t* dlist = nullptr;
	auto for_each_event = [&](auto&& body) {
		if (cached)
		{
#pragma unroll
			for (int k = 0; k < kCache; ++k)
			{
				if (threadIdx.x + k * blockDim.x < nEv)
				{
					body(recs[k]);
				}
			}
		}
		else
		{
			for (uint32_t e = threadIdx.x; e < nEv; e += blockDim.x)
			{
				if constexpr (D1S)
				{
					body(ev[dlist ? dlist[e] : e]);  // (uniform: the dealt list, once the unit has one)
				}
				else
				{
					body(ev[e]);
				}
			}
		}
	};

	// (uniform: every thread reads the same record, written before the barriers that separate two evaluations)
	// !D1S: a hit runs no scatter, so only an evaluation whose gather forms D1 may take it
	const bool reuse = !D1S && ru && wantJac && ru->valid == 1.0 && __double_as_longlong(ru->m0) == __double_as_longlong(m0) &&
					   __double_as_longlong(ru->m1) == __double_as_longlong(m1);
	int xmin = 0x7fffffff, xmax = -0x7fffffff, ymin = 0x7fffffff, ymax = -0x7fffffff;
	bool tabled = false;  // the box came from the extents table (uniform)
	if (!reuse)
	{
	// The box from the unit's time extents where they give it exactly (box_extents.h, ebo_extents.inc; ext: the unit's
	// slot, or null), else by a pass over the events.  Uniform over the workgroup: slot and flow alone decide.
	// With the table, the scatter would be the first to ask for the events, behind two barriers and the zeroing of
	// the image: the workgroup's first records are asked for HERE, beside the slot, and only waited for (their
	// cache lines are what is wanted, not their values: the scatter loads them again, from the cache).
	// (k_eval3 only: of a solve's evaluations only the first finds the events cold)
	uint64_t warm = 0;
	if (D1S && ext && threadIdx.x < nEv)
	{
		warm = ev[threadIdx.x];
	}
	tabled = ext && box_from_extents(ext, rx, ry, rw, rh, m0, m1, c, xmin, xmax, ymin, ymax);
	if (tabled)
	{
		asm volatile("" ::"v"(warm));
		__syncthreads();  // what block_minmax's last barrier is relied on for below: red and ru are read no more
	}
	else
	{
	for_each_event([&](uint64_t rec) {
		int pxc, pyc;
		double fx, fy, tau;
		if (warp_event(rec, rx, ry, rw, rh, m0, m1, c, pxc, pyc, fx, fy, tau))
		{
			xmin = min(xmin, pxc);
			xmax = max(xmax, pxc);
			ymin = min(ymin, pyc);
			ymax = max(ymax, pyc);
		}
	});
	block_minmax(xmin, xmax, ymin, ymax, ired);
	}
#ifdef EBO_AB
	if (boxStats && threadIdx.x == 0 && tile == 0)
	{
		atomicAdd(&boxStats[tabled ? 1 : 0], 1u);  // ebo_box_path_counts
	}
#endif
	if (ru && threadIdx.x == 0)
	{
		ru->valid = 0.0;  // the image is about to be rebuilt (every thread has read the record: the barriers above)
	}
	}
	EDGE_TICK(16);
	// the box is the same in every lane: scalar registers for it and for everything derived from it (pitch,
	// band rows, offsets), which the compiler cannot know of values read back from LDS
	xmin = __builtin_amdgcn_readfirstlane(xmin);
	xmax = __builtin_amdgcn_readfirstlane(xmax);
	ymin = __builtin_amdgcn_readfirstlane(ymin);
	ymax = __builtin_amdgcn_readfirstlane(ymax);
	if (!reuse && xmin > xmax)
	{
		return;
	}
	// The seven sums are kept per WAVE in red[wave * 8 + k], not in registers across the passes: a pass
	// accumulates its own in locals, reduces them over the wave (DPP) and the wave's result lane adds them to
	// the wave's slots.  No sum is live during another pass's tap loops -- 14 registers, which is what lets the
	// kernel run at 128 = four waves per SIMD without a spilled register.  Order: lanes by the DPP tree, then
	// sub-bands, then waves 0..nw-1: fixed, so the result is reproducible.
	const int lane = threadIdx.x & 63;
	double* slot = red + (threadIdx.x >> 6) * 8;
	if (lane == kWaveResultLane)
	{
#pragma unroll
		for (int k = 0; k < 7; ++k)
		{
			slot[k] = 0.0;  // the box ended with a barrier on either path: nobody reads red any more
		}
	}
	int x0 = max(xmin - 3, 0), x1 = min(xmax + 3, W3 - 1);
	int y0 = max(ymin - 3, 0), y1 = min(ymax + 3, H3 - 1);
	if (reuse)
	{
		x0 = __builtin_amdgcn_readfirstlane(static_cast<int>(ru->x0));
		y0 = __builtin_amdgcn_readfirstlane(static_cast<int>(ru->y0));
		x1 = x0 + __builtin_amdgcn_readfirstlane(static_cast<int>(ru->bw)) - 1;
		y1 = y0 + __builtin_amdgcn_readfirstlane(static_cast<int>(ru->rows)) - 1;
	}
	const int bw = x1 - x0 + 1;
	// the pitch of the LDS image is ODD: with an even pitch the rows of one column share a few bank pairs
	// (one, if the pitch is a multiple of 16) and the gather's reads of events stacked on a vertical structure
	// serialise; an odd pitch costs at most one column (measured on 4 sizes x 3 flow scales: with Jacobian
	// -5 % time at zero flow, where the box is the patch's own even width, -0.5 ... -1.5 % mid-solve, 0 at
	// the ground truth; value only unchanged -- the atomics are not bound by bank conflicts)
	const int cols = ((bw | 1) <= capDoubles) ? (bw | 1) : bw;  // (a canvas row that fills the capacity exactly keeps its even pitch)
	const int rowsAll = y1 - y0 + 1;
	const int R = (rowsAll + tiles - 1) / tiles;
	const int ty0 = y0 + tile * R;
	const int ty1 = min(ty0 + R, y1 + 1);
	const int maxRows = max(capDoubles / cols, 1);
	double fixBias, fixScale, preX, preY;
	unit_fix_grid(c, nEv, fixBias, fixScale, preX, preY);
	const int biasHi = __double2hiint(fixBias);
	// sigma >= 1: the scatter's taps are subnormal products (value_tap); the A/B build keeps the biased form behind a switch
#ifdef EBO_AB
	const bool subTaps = SMALL && c.fix_form == kFixSubnormal;
#else
	constexpr bool subTaps = SMALL;
#endif
	// D1S: what takes the scatter's prefactors off a sum of weights again, norm 2^-511 -> norm and 2^-(511 + k) -> 1
	// (powers of two: the quotient is exact)
	const double unX = subTaps ? 0x1p511 : 1.0;
	const double unY = subTaps ? 1.0 / preY : 1.0;
	// SMALL: the quarter arguments' constants (exact: powers of two), formed once per unit into two uniform register pairs.
	// As two more kernel-argument doubles they cost scalar spills instead (k_eval3<true> 12 -> 17, k_solve_independent<true>
	// 92 -> 103) and the c4 solve 1.5 % (measured, DESIGN.md 4.1 item 21).
	const double hsQ = c.hs * 0.25, isQ = c.inv_sigsq * 0.25;

	// ---- all-interior units (k_eval3 only; eval_interior.h, DESIGN.md 4.1 item 20) ----
	// Where the rule holds, warp_event rejects no event of the unit, the one sub-band's row test skips none and every
	// footprint lies inside the image: the three event passes below run the statements of an accepted interior event
	// without asking (INNER).  Uniform over the workgroup: scalars of the box alone.
	bool allInterior = false;
	if constexpr (D1S)
	{
		allInterior = ebo::unit_all_interior(tabled, tiles, xmin, xmax, ymin, ymax, rw, rh, rowsAll, maxRows);
#ifdef EBO_AB
		allInterior = allInterior && !interiorOff;
		if (boxStats && allInterior && threadIdx.x == 0)
		{
			// ebo_interior_path_counts (tiles == 1: one workgroup per unit; its own line of kInteriorStatSlots)
			atomicAdd(&boxStats[kInteriorStatStride * (1 + (blockIdx.x & (kInteriorStatSlots - 1)))], 1u);
		}
#endif
	}
	// a pass body takes INNER as a compile-time constant (as taps(form) takes the form): k_eval3 holds both variants of
	// the three event loops behind this one uniform condition, every other caller the general one only
	auto by_interior = [&](auto&& pass) {
		if constexpr (D1S)
		{
			if (allInterior)
			{
				pass(std::true_type{});
				return;
			}
		}
		pass(std::false_type{});
	};

	// ---- the bank deal (k_eval3 only; eval_deal.h, DESIGN.md 4.1 item 19) ----
	// Both tap passes below are bound by the LDS, and two thirds of its cycles are conflicts between the lanes of one
	// instruction: in the canonical order the bank pairs of the lanes' first taps are random.  Once per evaluation the
	// workgroup sorts its events by that bank pair (mod 16, relative to y0: a sub-band shifts every residue alike) and deals
	// them so that the lanes of a 16-lane group hold different ones.  A counting sort with PRIVATE counters hist[key][lane]
	// (plain read-modify-write by their owner) and an exclusive prefix in memory order: no atomic's return order decides
	// anything, the order is unique.  The counters and the sorted indices live in the image, which is not zeroed yet; what
	// survives is the list of 16-bit canonical indices at the END of the image area, behind the largest sub-band.  Image
	// place, pitch and sub-bands are untouched, so the three value sums keep their bits; J changes by summation order only.
	if constexpr (D1S)
	{
		const int B = blockDim.x;
		bool deal = ebo::deal_admits(nEv, B, tiles) && ebo::deal_fits(nEv, B, capDoubles, min(maxRows, ty1 - ty0) * cols);
#ifdef EBO_AB
		deal = deal && !dealOff;
		if (dealDump && threadIdx.x == 0)
		{
			dealDump[0] = deal ? nEv : 0u;  // ebo_unit_deal
		}
#endif
		if (deal)
		{
			const int tid = threadIdx.x;
			uint16_t* list = reinterpret_cast<uint16_t*>(img + (capDoubles - ebo::deal_list_doubles(nEv)));
			uint32_t* hist = reinterpret_cast<uint32_t*>(img);
			uint16_t* sorted = reinterpret_cast<uint16_t*>(img + ebo::deal_counter_doubles(B));
			// (the box ended with a barrier on either path: block_minmax's scratch is free, and nothing has used the image yet)
#pragma unroll
			for (int k = 0; k < ebo::kDealKeys; ++k)
			{
				hist[k * B + tid] = 0u;
			}
			// the keys of the lane's events, 5 bits a round, and their counts
			unsigned long long keys = 0ull;
			by_interior([&](auto inner) {
				constexpr bool INNER = decltype(inner)::value;
				int sh = 0;
				for (uint32_t e = tid; e < nEv; e += B, sh += ebo::kDealKeyBits)
				{
					int pxc, pyc;
					double fx, fy, tau;
					uint32_t key = ebo::kDealGroup;
					if (warp_event<INNER>(ev[e], rx, ry, rw, rh, m0, m1, c, pxc, pyc, fx, fy, tau))
					{
						key = static_cast<uint32_t>(__mul24(pyc - 3 - y0, cols) + (pxc - 3 - x0)) & (ebo::kDealGroup - 1);
					}
					keys |= static_cast<unsigned long long>(key) << sh;
					hist[key * B + tid] += 1u;
				}
			});
			__syncthreads();
			// exclusive prefix over the counters in memory order = (key, lane): thread t owns entries [17 t, 17 t + 17)
			{
				uint32_t v[ebo::kDealKeys];
				uint32_t sum = 0u;
#pragma unroll
				for (int k = 0; k < ebo::kDealKeys; ++k)
				{
					v[k] = hist[tid * ebo::kDealKeys + k];
					sum += v[k];
				}
				uint32_t incl = sum;
#pragma unroll
				for (int d = 1; d < 64; d <<= 1)
				{
					const uint32_t t = __shfl_up(incl, d, 64);
					incl += ((tid & 63) >= d) ? t : 0u;
				}
				if ((tid & 63) == 63)
				{
					ired[tid >> 6] = static_cast<int>(incl);
				}
				__syncthreads();
				uint32_t run = incl - sum;
				for (int w = 0; w < (tid >> 6); ++w)
				{
					run += static_cast<uint32_t>(ired[w]);
				}
#pragma unroll
				for (int k = 0; k < ebo::kDealKeys; ++k)
				{
					hist[tid * ebo::kDealKeys + k] = run;
					run += v[k];
				}
			}
			__syncthreads();
			// place: the lane's events in round order, each at its (key, lane) counter
			{
				int sh = 0;
				for (uint32_t e = tid; e < nEv; e += B, sh += ebo::kDealKeyBits)
				{
					const uint32_t key = static_cast<uint32_t>(keys >> sh) & 31u;
					const uint32_t pos = hist[key * B + tid];
					hist[key * B + tid] = pos + 1u;
					sorted[pos] = static_cast<uint16_t>(e);
				}
			}
			__syncthreads();
			// the layout: position q = round * B + lane takes the round-th element of the lane's slot
			{
				uint32_t s = ebo::deal_start(tid, nEv, B);
				for (uint32_t q = tid; q < nEv; q += B, ++s)
				{
					list[q] = sorted[s];
				}
			}
			dlist = list;  // (visible behind the sub-band loop's first barrier, which also precedes the zeroing)
#ifdef EBO_AB
			if (dealDump)
			{
				for (uint32_t q = tid; q < nEv; q += B)  // (the positions the lane wrote itself)
				{
					dealDump[1 + q] = list[q];
				}
			}
#endif
		}
	}

	for (int sy0 = ty0; sy0 < ty1; sy0 += maxRows)
	{
		const int srows = min(maxRows, ty1 - sy0);
		const int npx = srows * cols;
		if (!reuse)
		{
		__syncthreads();
		for (int i = threadIdx.x; i < npx; i += blockDim.x)
		{
			img[i] = 0.0;
		}
		__syncthreads();
		}
		EDGE_TICK(17);

		// ---- scatter the value taps ----
		if (!reuse)
		{
		double h3 = 0.0, h4 = 0.0;  // D1S: this sub-band's D1 sums
		by_interior([&](auto inner) {
		constexpr bool INNER = decltype(inner)::value;  // (all-interior unit: no event is rejected, skipped or clipped)
		for_each_event([&](uint64_t rec) {
			int pxc, pyc;
			double fx, fy, tau;
			if (!warp_event<INNER>(rec, rx, ry, rw, rh, m0, m1, c, pxc, pyc, fx, fy, tau))
			{
				return;
			}
			const int rowLo = pyc - 3 - sy0;
			if (!INNER && (rowLo + 6 < 0 || rowLo >= srows))
			{
				return;
			}
			const int colLo = pxc - 3 - x0;
			double wx[7], wy[7];
			axis_taps3<SMALL>(fx, subTaps ? preX : c.norm, c, hsQ, isQ, wx);
			axis_taps3<SMALL>(fy, subTaps ? preY : 1.0, c, hsQ, isQ, wy);
			const bool interior = INNER || (rowLo >= 0 && rowLo + 6 < srows && colLo >= 0 && colLo + 6 < bw);
			if (D1S && wantJac)
			{
				// the sums of the weights and of the derivative weights over the taps this sub-band holds: the statements
				// of the gather's two paths (below, !D1S), on weights that may carry the prefactors
				const double g = tau * c.inv_sigsq;
				double sumWy = 0.0, sumAy = 0.0, sumW = 0.0, sumA = 0.0;
				if (interior)
				{
					// whole footprint: the derivative sums from the weights' first moments (tap_moments.h)
					ebo::axis_d1(wx, g, fx, sumW, sumA);
					ebo::axis_d1(wy, g, fy, sumWy, sumAy);
				}
				else
				{
					const double gfx = g * fx, gfy = g * fy;
#pragma unroll
					for (int i = 0; i < 7; ++i)
					{
						const int col = colLo + i;
						const double w = (col >= 0 && col < bw) ? wx[i] : 0.0;
						const double a = w * fma(g, static_cast<double>(i - 3), -gfx);
						sumW += w;
						sumA += a;
					}
#pragma unroll
					for (int j = 0; j < 7; ++j)
					{
						const int row = rowLo + j;
						if (row < 0 || row >= srows)
						{
							continue;
						}
						const double ay = wy[j] * fma(g, static_cast<double>(j - 3), -gfy);
						sumWy += wy[j];
						sumAy += ay;
					}
				}
				h3 = fma(sumA * unX, sumWy * unY, h3);
				h4 = fma(sumW * unX, sumAy * unY, h4);
			}
			// (the form is a compile-time constant of the tap loops; only the A/B build holds both)
			auto taps = [&](auto form) {
				constexpr bool SUB = decltype(form)::value;
				if (interior)
				{
					unsigned long long* p = imgq + __mul24(rowLo, cols) + colLo;  // (both far below 2^24: not the quarter-rate v_mul_lo_u32)
#pragma unroll
					for (int j = 0; j < 7; ++j)
					{
#pragma unroll
						for (int i = 0; i < 7; ++i)
						{
							atomicAdd(p + i, value_tap<SMALL, SUB>(wx[i], wy[j], fixBias, biasHi));
						}
						p += cols;
					}
				}
				else
				{
#pragma unroll
					for (int j = 0; j < 7; ++j)
					{
						const int row = rowLo + j;
						if (row < 0 || row >= srows)
						{
							continue;
						}
#pragma unroll
						for (int i = 0; i < 7; ++i)
						{
							const int col = colLo + i;
							if (col >= 0 && col < bw)
							{
								atomicAdd(&imgq[row * cols + col], value_tap<SMALL, SUB>(wx[i], wy[j], fixBias, biasHi));
							}
						}
					}
				}
			};
#ifdef EBO_AB
			if (subTaps)
			{
				taps(std::true_type{});
			}
			else
			{
				taps(std::false_type{});
			}
#else
			taps(std::integral_constant<bool, subTaps>{});
#endif
		});
		});
		if (D1S && wantJac)
		{
			h3 = wave_sum(h3);
			h4 = wave_sum(h4);
			if (lane == kWaveResultLane)
			{
				slot[3] += h3;
				slot[4] += h4;
			}
		}
		__syncthreads();
		EDGE_TICK(18);

		// ---- pixel sums; fixed point -> f64 in place ----
		{
			double s0 = 0.0, s1 = 0.0, s2 = 0.0;
			for (int p = threadIdx.x; p < npx; p += blockDim.x)
			{
				const unsigned long long q = imgq[p];
				const double I = static_cast<double>(q) * fixScale;
				img[p] = I;
				if (q != 0ull)
				{
					s0 += I;
					s1 = fma(I, I, s1);
					s2 += 1.0;
				}
			}
			s0 = wave_sum(s0);
			s1 = wave_sum(s1);
			s2 = wave_sum(s2);
			if (lane == kWaveResultLane)
			{
				slot[0] += s0;
				slot[1] += s1;
				slot[2] += s2;
			}
		}
		}
		if (!wantJac)
		{
			continue;
		}
		__syncthreads();
		EDGE_TICK(19);

		// ---- gather the derivative sums ----
		[[maybe_unused]] double g3 = 0.0, g4 = 0.0;
		double g5 = 0.0, g6 = 0.0;
		by_interior([&](auto inner) {
		constexpr bool INNER = decltype(inner)::value;
		for_each_event([&](uint64_t rec) {
			int pxc, pyc;
			double fx, fy, tau;
			if (!warp_event<INNER>(rec, rx, ry, rw, rh, m0, m1, c, pxc, pyc, fx, fy, tau))
			{
				return;
			}
			const int rowLo = pyc - 3 - sy0;
			if (!INNER && (rowLo + 6 < 0 || rowLo >= srows))
			{
				return;
			}
			const int colLo = pxc - 3 - x0;
			double wx[7], wy[7];
			axis_taps3<SMALL>(fx, c.norm, c, hsQ, isQ, wx);
			axis_taps3<SMALL>(fy, 1.0, c, hsQ, isQ, wy);
			const double g = tau * c.inv_sigsq;
			double d2a = 0.0, d2b = 0.0;
			[[maybe_unused]] double sumWy = 0.0, sumAy = 0.0, sumW = 0.0, sumA = 0.0;  // !D1S: the D1 sums are formed here
			if (INNER || (rowLo >= 0 && rowLo + 6 < srows && colLo >= 0 && colLo + 6 < bw))
			{
				// moment form (tap_moments.h): no derivative factor per tap; four moment weights for the x axis, none for y.
				// Per row 13 operations for rb and rc, then A, B and C; g, fx and fy come in once, behind the rows.
				if constexpr (!D1S)
				{
					ebo::axis_d1(wx, g, fx, sumW, sumA);
					ebo::axis_d1(wy, g, fy, sumWy, sumAy);
				}
				double kx[4];
				ebo::moment_table(wx, kx);
				double mA = 0.0, mB = 0.0, mC = 0.0;
				const double* rowp = img + __mul24(rowLo, cols) + colLo;
				// (the row index as a compile-time constant, seven calls: as an unrolled loop over j with a run-time argument
				// the same statements put k_eval3<true> at 26 spilled vector registers and 200 B of scratch, and the gate refuses it)
				auto row = [&](auto jc) {
					constexpr int J = decltype(jc)::value;
					double v[7];
#pragma unroll
					for (int i = 0; i < 7; ++i)
					{
						v[i] = lds_ld(rowp + i);  // the row's seven reads back to back, then the arithmetic (measured: within
												  // 0.5 % of reads interleaved with the arithmetic -- the pass is throughput-bound)
					}
					double rb, rc;
					ebo::moment_row(wx, kx, v, rb, rc);
					ebo::moment_acc<J>(wy[J], rb, rc, mA, mB, mC);
					rowp += cols;
				};
				row(std::integral_constant<int, 0>{});
				row(std::integral_constant<int, 1>{});
				row(std::integral_constant<int, 2>{});
				row(std::integral_constant<int, 3>{});
				row(std::integral_constant<int, 4>{});
				row(std::integral_constant<int, 5>{});
				row(std::integral_constant<int, 6>{});
				ebo::moment_d2(g, fx, fy, mA, mB, mC, d2a, d2b);
			}
			else
			{
				const double gfx = g * fx, gfy = g * fy;
				double ax[7];
				int ci[7];
#pragma unroll
				for (int i = 0; i < 7; ++i)
				{
					const int col = colLo + i;
					const bool ok = col >= 0 && col < bw;
					wx[i] = ok ? wx[i] : 0.0;
					ax[i] = wx[i] * fma(g, static_cast<double>(i - 3), -gfx);
					ci[i] = min(max(col, 0), bw - 1);
					if constexpr (!D1S)
					{
						sumW += wx[i];
						sumA += ax[i];
					}
				}
#pragma unroll
				for (int j = 0; j < 7; ++j)
				{
					const int row = rowLo + j;
					if (row < 0 || row >= srows)
					{
						continue;
					}
					const double ay = wy[j] * fma(g, static_cast<double>(j - 3), -gfy);
					if constexpr (!D1S)
					{
						sumWy += wy[j];
						sumAy += ay;
					}
					const double* rowp = img + row * cols;
					double ra = 0.0, rb = 0.0;
#pragma unroll
					for (int i = 0; i < 7; ++i)
					{
						const double I = rowp[ci[i]];
						ra = fma(ax[i], I, ra);
						rb = fma(wx[i], I, rb);
					}
					d2a = fma(wy[j], ra, d2a);
					d2b = fma(ay, rb, d2b);
				}
			}
			if constexpr (!D1S)
			{
				g3 = fma(sumA, sumWy, g3);
				g4 = fma(sumW, sumAy, g4);
			}
			g5 += d2a;
			g6 += d2b;
		});
		});
		if constexpr (!D1S)
		{
			g3 = wave_sum(g3);
			g4 = wave_sum(g4);
		}
		g5 = wave_sum(g5);
		g6 = wave_sum(g6);
		if (lane == kWaveResultLane)
		{
			if constexpr (!D1S)
			{
				slot[3] += g3;
				slot[4] += g4;
			}
			slot[5] += g5;
			slot[6] += g6;
		}
		EDGE_TICK(20);
	}
	__syncthreads();
	{
		const int nw = (blockDim.x + 63) >> 6;
#pragma unroll
		for (int k = 0; k < 7; ++k)
		{
			double t = red[k];
			for (int w = 1; w < nw; ++w)
			{
				t += red[w * 8 + k];
			}
			S[k] = t;
		}
	}
	if (reuse)
	{
		S[0] = ru->s0;
		S[1] = ru->s1;
		S[2] = ru->s2;
	}
	else if (ru && threadIdx.x == 0 && tiles == 1 && rowsAll <= maxRows)
	{
		// (the next evaluation's threads read this behind the barrier that separates two evaluations)
		ru->m0 = m0;
		ru->m1 = m1;
		ru->x0 = static_cast<double>(x0);
		ru->y0 = static_cast<double>(y0);
		ru->bw = static_cast<double>(bw);
		ru->rows = static_cast<double>(rowsAll);
		ru->s0 = S[0];
		ru->s1 = S[1];
		ru->s2 = S[2];
		ru->valid = 1.0;
	}
	EDGE_TICK(21);
	EDGE_TICK_FLUSH;
}

template <bool SMALL>
// Four waves per SIMD = 128 VGPRs (round 3; 137 VGPRs and three waves before).  The kernel is bound by the
// LDS, which idles while a workgroup is between its tap passes, so a fifth 192-lane workgroup per CU is worth
// 4-5 % -- but only without spills: the first attempt (round 1) spilled inside the tap loops and was 8x slower.
// What fits the kernel into 128 registers: the seven sums live in per-wave LDS slots instead of registers
// across the passes, the box and everything derived from it are scalars (readfirstlane), and the D1 sums are
// formed in the scatter pass (D1S), and the gather holds four moment weights instead of seven derivative weights (tap_moments.h).
// The sigma < 1 instantiation (library exp, the one-step floor of fix_tap) is
// given three waves per SIMD: at four it spills a register.  It is not the reference's sigma.
__global__ void __launch_bounds__(512, SMALL ? 4 : 3) k_eval3(const uint64_t* __restrict__ events,
												const Unit* __restrict__ units,
												const double* __restrict__ flows, int tiles, int wantJac,
												int capDoubles, int hdrWaves, double fdStep, double* __restrict__ partials,
												double* __restrict__ out, EvalConsts c,
												const unsigned char* __restrict__ modes, LiveWindows live,
												const uint32_t* __restrict__ order, BoxTable box)
{
	extern __shared__ double lds[];
	int unit = blockIdx.x / tiles;
	const int tile = blockIdx.x - unit * tiles;
	const int set = blockIdx.y;
	// live.n > 0 (tiles == 1): the grid covers the units of the listed windows only (ebo_internal.h, LiveWindows)
	int liveMode = -1;
	if (live.n > 0)
	{
		const int k = unit / live.upw;
		const int ent = live.ent[k];
		unit = (ent >> 2) * live.upw + (unit - k * live.upw);
		liveMode = ent & 3;
	}
	else
	{
		// a launch over every unit hands them out heaviest first (launch_order.h): workgroups start in blockIdx
		// order, and the last to start should be the shortest-lived.  One scalar load; which workgroup evaluates a
		// unit changes nothing in what it computes.
		unit = static_cast<int>(order[unit]);
	}
	const Unit u = units[unit];
	// (by unit, not by blockIdx: k_combine_variance reads a unit's tiles at [set][unit][tile])
	double* part = partials + ((static_cast<size_t>(set) * gridDim.x) + static_cast<size_t>(unit) * tiles + tile) * kPartialStride;
	const bool fused = (tiles == 1 && gridDim.y == 1);
	if (!(u.flags & kUnitActive))
	{
		if (!fused && threadIdx.x < 7)
		{
			part[threadIdx.x] = 0.0;
		}
		if (fused && !(u.flags & kUnitStray) && threadIdx.x < 3)
		{
			out[3 * u.flow_idx + threadIdx.x] = 0.0;
		}
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
	double m0 = flows[2 * u.flow_idx];
	double m1 = flows[2 * u.flow_idx + 1];
	fd_offset(set, fdStep, m0, m1);
	double S[7];
	// (the slot is the unit's, not the workgroup's: scalar address, scalar status)
	const int32_t* ext = box.ext ? box.ext + static_cast<size_t>(unit) * kExtStride : nullptr;
#ifdef EBO_AB
	eval_unit3<SMALL, true>(events + u.ev_off, u, m0, m1, wantJac != 0, tile, tiles, capDoubles, c, lds, S, hdrWaves, nullptr,
							ext, set == 0 ? box.stats : nullptr, box.deal_off != 0,
							(set == 0 && unit == box.deal_unit) ? box.deal_dump : nullptr, box.interior_off != 0);
#else
	eval_unit3<SMALL, true>(events + u.ev_off, u, m0, m1, wantJac != 0, tile, tiles, capDoubles, c, lds, S, hdrWaves, nullptr,
							ext);
#endif
	if (threadIdx.x == 0)
	{
		if (fused)
		{
			double r, j0 = 0.0, j1 = 0.0;
			variance_from_sums(S, wantJac != 0, m0, m1, c.max_res, r, j0, j1);
			out[3 * u.flow_idx + 0] = r;
			out[3 * u.flow_idx + 1] = j0;
			out[3 * u.flow_idx + 2] = j1;
		}
		else
		{
#pragma unroll
			for (int k = 0; k < 7; ++k)
			{
				part[k] = S[k];
			}
		}
	}
}
