// ebo_count.inc — integer event-count images (ebo_count_image*), included inside ebo_kernels.hip's anonymous
// namespace after the helpers it shares with the row-shard kernels (count_target, stray_flow).
//   EBO_COUNT_INTEGRATED feature_detector.cpp:466-482
//   EBO_COUNT_WARPED     feature_detector.cpp:433-463  round() = half away from zero
//   EBO_COUNT_FIELD      feature_detector.cpp:270-295  float32 field (at<Vec2f>)
//
// Bit-exact by construction: every event adds 1 to one integer counter, and integer adds commute, so any
// order, any split of the image and any privatisation gives the reference's image.  What the kernels differ
// in is where the counters live and how often an event is read:
//   k_count_tiles      warped: 2-D tiles of 16-bit LDS counters; a wave takes one unit at a time (flow and
//                      reference time wave-uniform), a tile only the units whose events can reach it
//   k_count_units      warped: the same with full-width row bands, 16- or 32-bit counters
//   k_count_window_lds warped / field: row bands; every band streams all events of its window
//   k_csort_*          warped / field, many events: events sorted by destination band first, then counted
//   k_count_bands      un-warped: bands of whole patch rows; an event never leaves its band, so it is read once
//   k_count_scatter    anything: global int32 atomics, then k_counts_to_f64
// Which one runs for a shape is plan_count_image's choice (count_plan.h).  All but the last store finished
// f64 rows straight from LDS: HBM traffic = events once (plus re-reads that hit L2) + image once.

// Global int atomics.  Workgroup = unit (its events are one contiguous range and share one flow).
__global__ void k_count_scatter(const uint64_t* __restrict__ events, const Unit* __restrict__ units,
								int unitsPerWindow, int mode, const void* __restrict__ aux,
								int32_t* __restrict__ counts, EvalConsts c)
{
	const Unit u = units[blockIdx.x];
	const int w = blockIdx.x / unitsPerWindow;
	const int P = c.npx * c.npy;
	const size_t imgSize = static_cast<size_t>(c.image_w) * c.image_h;
	int32_t* img = counts + static_cast<size_t>(w) * imgSize;
	const uint64_t* ev = events + u.ev_off;
	const bool stray = (u.flags & kUnitStray) != 0;
	double m0 = 0.0, m1 = 0.0;
	if (mode == 1 && !stray)
	{
		const double* flows = static_cast<const double*>(aux);
		m0 = flows[2 * u.flow_idx];
		m1 = flows[2 * u.flow_idx + 1];
	}
	for (uint32_t e = threadIdx.x; e < u.n_ev; e += blockDim.x)
	{
		int x, y, pos, dt;
		unpack(ev[e], x, y, pos, dt);
		int nx = x, ny = y;
		if (mode != 0)
		{
			if (mode == 1 && stray)
			{
				// :436-441 with the index clamped at 0 (negative indices are undefined there)
				const int px = max(min(x / c.patch_w, c.npx - 1), 0);
				const int py = max(min(y / c.patch_h, c.npy - 1), 0);
				const double* flows = static_cast<const double*>(aux);
				m0 = flows[2 * (static_cast<size_t>(w) * P + py * c.npx + px)];
				m1 = flows[2 * (static_cast<size_t>(w) * P + py * c.npx + px) + 1];
			}
			if (mode == 2)
			{
				if (x < 0 || x >= c.image_w || y < 0 || y >= c.image_h)
				{
					continue;
				}
				const float* field = static_cast<const float*>(aux) +
									 2 * (static_cast<size_t>(w) * imgSize +
										  static_cast<size_t>(y) * c.image_w + x);
				m0 = static_cast<double>(field[0]);
				m1 = static_cast<double>(field[1]);
			}
			const double dtw = static_cast<double>(dt + u.dt_win);
			const double fx = static_cast<double>(x) + dtw * c.scale * m0;
			const double fy = static_cast<double>(y) + dtw * c.scale * m1;
			if (!convertible(fx) || !convertible(fy))
			{
				continue;
			}
			nx = static_cast<int>(round(fx));
			ny = static_cast<int>(round(fy));
		}
		if (nx >= 0 && nx < c.image_w && ny >= 0 && ny < c.image_h)
		{
			atomicAdd(&img[static_cast<size_t>(ny) * c.image_w + nx], 1);
		}
	}
}

// The unit of an event from its own coordinates, without walking the unit table: the grid patch
// that contains it (feature_detector.cpp:332-355: index min(x / pw, npx - 1)), or the stray unit P
// for an event outside the sensor, whose flow is that of the clamped patch (:436-441).  Division
// by the (uniform) patch size is one mul_hi: exact for 0 <= x < 2^15 (coordinates are 15-bit).
__device__ __forceinline__ void event_unit(uint64_t rec, const EvalConsts& c, int& patch, int& unit)
{
	int x, y, pos, dt;
	unpack(rec, x, y, pos, dt);
	const bool inSensor = static_cast<unsigned>(x) < static_cast<unsigned>(c.image_w) &&
						  static_cast<unsigned>(y) < static_cast<unsigned>(c.image_h);
	const unsigned xc = static_cast<unsigned>(max(x, 0)), yc = static_cast<unsigned>(max(y, 0));
	const int bx = min(static_cast<int>(c.patch_w == 1 ? xc : __umulhi(xc, c.inv_pw)), c.npx - 1);
	const int by = min(static_cast<int>(c.patch_h == 1 ? yc : __umulhi(yc, c.inv_ph)), c.npy - 1);
	patch = by * c.npx + bx;
	unit = inSensor ? patch : c.npx * c.npy;
}

// LDS-privatised count image: workgroup = (row band, window).  The band's counters
// live in LDS (16-bit counters packed two per dword when the window has < 65536
// events, else 32-bit); the workgroup streams ALL events of its window once
// (8 B/lane coalesced; with more than one band the re-reads are L2 hits), counts
// those that land in its band with ds_add_u32, and writes the finished f64 rows
// with plain coalesced stores.  HBM traffic = events once + image once: no global
// atomics, no int32 intermediate image.  Bit-exact (integer adds commute).
template <bool U16, int MODE>
__global__ void __launch_bounds__(1024) k_count_window_lds(
	const uint64_t* __restrict__ events, const Unit* __restrict__ units, int unitsPerWindow,
	const void* __restrict__ aux, int rowsPerBand, int nWindows, double* __restrict__ image,
	EvalConsts c)
{
	extern __shared__ unsigned int cnt[];
	// 1-D grid; consecutive workgroup ids go round-robin over the 8 XCDs, so the bands of one
	// window take consecutive slots of ONE XCD: the second band's event reads hit that L2.
	const int nBands = (c.image_h + rowsPerBand - 1) / rowsPerBand;
	const int slot = blockIdx.x >> 3;
	const int w = (slot / nBands) * 8 + (blockIdx.x & 7);
	if (w >= nWindows)
	{
		return;
	}
	const int row0 = (slot % nBands) * rowsPerBand;
	const int rows = min(rowsPerBand, c.image_h - row0);
	const int W = c.image_w;
	const int npx = rows * W;
	const int nWords = U16 ? (npx + 1) >> 1 : npx;
	for (int i = threadIdx.x; i < nWords; i += blockDim.x)
	{
		cnt[i] = 0u;
	}
	const Unit* wu = units + static_cast<size_t>(w) * unitsPerWindow;
	const int P = c.npx * c.npy;
	const size_t imgSize = static_cast<size_t>(W) * c.image_h;
	const double* windowFlows = static_cast<const double*>(aux) + (MODE == 1 ? 2 * static_cast<size_t>(w) * P : 0);
	const float* windowField = static_cast<const float*>(aux) + (MODE == 2 ? 2 * static_cast<size_t>(w) * imgSize : 0);
	// The window's unit table -- reference-time offset per unit, flow per patch -- behind the
	// counters in LDS: every event looks its unit up (event_unit), and three gathers per event
	// through the vector memory path cost more than the warp arithmetic (an LDS read of an
	// address shared by most of a wave is a broadcast).
	const int tblBase = (rowsPerBand * W * (U16 ? 2 : 4) + 15) & ~15;  // bytes; the band size of the launch
	double* tblFlow = reinterpret_cast<double*>(reinterpret_cast<char*>(cnt) + tblBase);
	int* tblDt = reinterpret_cast<int*>(tblFlow + (MODE == 1 ? 2 * P : 0));
	if (MODE != 0)
	{
		for (int i = threadIdx.x; i <= P; i += blockDim.x)
		{
			tblDt[i] = wu[i].dt_win;
		}
		if (MODE == 1)
		{
			for (int i = threadIdx.x; i < 2 * P; i += blockDim.x)
			{
				tblFlow[i] = windowFlows[i];
			}
		}
	}
	__syncthreads();
	// kInFlight independent 8-byte loads per lane are issued before the first is
	// consumed: ~64 KiB in flight per CU, enough to cover HBM latency (Little's law).
	constexpr int kInFlight = 8;
	// Every event finds its unit (reference time, flow) from its own coordinates: no walk along
	// the unit table, no branch per event, and the 8 in-flight events of a lane are independent
	// (the first version tracked the current unit per lane: two dependent loads and a divergent
	// loop per event).  The window's units, the stray one included, are contiguous in `events`.
	{
		const uint32_t evBegin = wu[0].ev_off;
		const uint32_t evEnd = wu[P].ev_off + wu[P].n_ev;
		for (uint32_t eb = evBegin + threadIdx.x; eb < evEnd; eb += kInFlight * blockDim.x)
		{
			uint64_t recs[kInFlight];
#pragma unroll
			for (int k = 0; k < kInFlight; ++k)
			{
				const uint32_t ek = eb + k * blockDim.x;
				recs[k] = (ek < evEnd) ? events[ek] : 0ull;
			}
			int dtWin[kInFlight];
			double m0[kInFlight], m1[kInFlight];
#pragma unroll
			for (int k = 0; k < kInFlight; ++k)
			{
				dtWin[k] = 0;
				m0[k] = 0.0;
				m1[k] = 0.0;
				if (MODE != 0)
				{
					int patch, unit;
					event_unit(recs[k], c, patch, unit);
					dtWin[k] = tblDt[unit];
					if (MODE == 1)
					{
						m0[k] = tblFlow[2 * patch];
						m1[k] = tblFlow[2 * patch + 1];
					}
				}
			}
#pragma unroll
			for (int k = 0; k < kInFlight; ++k)
			{
				const bool live = eb + k * blockDim.x < evEnd;
				int nx = 0, ny = -1;
				const bool hit = count_target<MODE>(recs[k], live, dtWin[k], m0[k], m1[k], windowField, c, nx, ny);
				const int ry = ny - row0;
				if (hit && ry >= 0 && ry < rows)
				{
					const int p = ry * W + nx;
					if (U16)
					{
						atomicAdd(&cnt[p >> 1], 1u << ((p & 1) * 16));
					}
					else
					{
						atomicAdd(&cnt[p], 1u);
					}
				}
			}
		}
	}
	__syncthreads();
	double* out = image + static_cast<size_t>(w) * imgSize + static_cast<size_t>(row0) * W;
	if (U16 && (reinterpret_cast<uintptr_t>(out) & 15) == 0)
	{
		// one packed dword = two pixels = one 16-byte store
		const int pairs = npx >> 1;
		double2* out2 = reinterpret_cast<double2*>(out);
		for (int i = threadIdx.x; i < pairs; i += blockDim.x)
		{
			const unsigned int v = cnt[i];
			out2[i] = make_double2(static_cast<double>(v & 0xFFFFu), static_cast<double>(v >> 16));
		}
		if ((npx & 1) && threadIdx.x == 0)
		{
			out[npx - 1] = static_cast<double>(cnt[pairs] & 0xFFFFu);
		}
	}
	else
	{
		for (int p = threadIdx.x; p < npx; p += blockDim.x)
		{
			const unsigned int v = U16 ? ((cnt[p >> 1] >> ((p & 1) * 16)) & 0xFFFFu) : cnt[p];
			out[p] = static_cast<double>(v);
		}
	}
}

// Unit waves (impl 4): the warped image (mode 1); workgroup = (row band, window) with the band's counters in LDS, as impl 1;
// but the events are taken UNIT BY UNIT, one wave per unit at a time (a work counter in LDS hands
// the units out).  A unit's reference-time offset and flow are then wave-uniform scalars -- no
// per-event patch lookup, no table reads -- and a band only takes the units whose events can
// reach it: a unit's rows grown by its largest possible displacement,
// max|t_ref - t| (kept per unit by the bucketing) x scale x |flow_y|, rounded up.  With several
// bands a window's events are then warped ~1.2-2 times instead of once per band.
template <bool U16>
__global__ void __launch_bounds__(1024) k_count_units(
	const uint64_t* __restrict__ events, const Unit* __restrict__ units, const int32_t* __restrict__ unitMaxDt,
	int unitsPerWindow, const void* __restrict__ aux, int rowsPerBand, int nWindows, double* __restrict__ image,
	EvalConsts c)
{
	extern __shared__ unsigned int cnt[];
	const int nBands = (c.image_h + rowsPerBand - 1) / rowsPerBand;
	const int slot = blockIdx.x >> 3;
	const int w = (slot / nBands) * 8 + (blockIdx.x & 7);
	if (w >= nWindows)
	{
		return;
	}
	const int row0 = (slot % nBands) * rowsPerBand;
	const int rows = min(rowsPerBand, c.image_h - row0);
	const int W = c.image_w;
	const int npx = rows * W;
	const int nWords = U16 ? (npx + 1) >> 1 : npx;
	const int P = c.npx * c.npy;
	const int hdr = (rowsPerBand * W * (U16 ? 2 : 4) + 15) & ~15;  // bytes; the band size of the launch
	int* ctl = reinterpret_cast<int*>(reinterpret_cast<char*>(cnt) + hdr);  // [0] next, [1] nSel, [2..] list
	int* list = ctl + 2;
	for (int i = threadIdx.x; i < nWords; i += blockDim.x)
	{
		cnt[i] = 0u;
	}
	if (threadIdx.x < 2)
	{
		ctl[threadIdx.x] = 0;
	}
	__syncthreads();
	const Unit* wu = units + static_cast<size_t>(w) * unitsPerWindow;
	const int32_t* wmax = unitMaxDt + static_cast<size_t>(w) * unitsPerWindow;
	const size_t imgSize = static_cast<size_t>(W) * c.image_h;
	const double* windowFlows = static_cast<const double*>(aux) + 2 * static_cast<size_t>(w) * P;
	// which units can reach this band
	for (int u = threadIdx.x; u <= P; u += blockDim.x)
	{
		const Unit un = wu[u];
		bool take = un.n_ev > 0;
		if (take && u < P && nBands > 1)
		{
			// |fl(fl(dtw * scale) * m1)| <= fl(fl(maxdt * |scale|) * |m1|): rounding is monotonic
			const double reach = static_cast<double>(wmax[u]) * fabs(c.scale) * fabs(windowFlows[2 * u + 1]) + 1.0;
			const double lo = static_cast<double>(un.ry) - reach, hi = static_cast<double>(un.ry + un.rh - 1) + reach;
			// NaN / inf reach: comparisons false -> taken
			take = !(hi < static_cast<double>(row0) - 0.5 || lo > static_cast<double>(row0 + rows) - 0.5);
		}
		if (take)
		{
			list[atomicAdd(&ctl[1], 1)] = u;
		}
	}
	__syncthreads();
	const int nSel = ctl[1];
	const int lane = threadIdx.x & 63;
	constexpr int kInFlight = 4;
	for (;;)
	{
		int pick = 0;
		if (lane == 0)
		{
			pick = atomicAdd(&ctl[0], 1);
		}
		pick = __shfl(pick, 0, 64);
		if (pick >= nSel)
		{
			break;
		}
		const int u = list[pick];
		const Unit un = wu[u];
		const bool stray = u == P;
		double m0 = 0.0, m1 = 0.0;
		if (!stray)
		{
			m0 = windowFlows[2 * u];
			m1 = windowFlows[2 * u + 1];
		}
		const int dtWin = un.dt_win;
		const uint32_t evEnd = un.ev_off + un.n_ev;
		for (uint32_t eb = un.ev_off + lane; eb < evEnd; eb += kInFlight * 64)
		{
			uint64_t recs[kInFlight];
#pragma unroll
			for (int k = 0; k < kInFlight; ++k)
			{
				const uint32_t ek = eb + k * 64;
				recs[k] = (ek < evEnd) ? events[ek] : 0ull;
			}
#pragma unroll
			for (int k = 0; k < kInFlight; ++k)
			{
				const bool live = eb + k * 64 < evEnd;
				if (stray)
				{
					stray_flow(recs[k], windowFlows, c, m0, m1);
				}
				int nx, ny;
				const bool hit = count_target<1>(recs[k], live, dtWin, m0, m1, nullptr, c, nx, ny);
				const int ry = ny - row0;
				if (hit && ry >= 0 && ry < rows)
				{
					const int p = ry * W + nx;
					if (U16)
					{
						atomicAdd(&cnt[p >> 1], 1u << ((p & 1) * 16));
					}
					else
					{
						atomicAdd(&cnt[p], 1u);
					}
				}
			}
		}
	}
	__syncthreads();
	double* out = image + static_cast<size_t>(w) * imgSize + static_cast<size_t>(row0) * W;
	if (U16 && (reinterpret_cast<uintptr_t>(out) & 15) == 0)
	{
		const int pairs = npx >> 1;
		double2* out2 = reinterpret_cast<double2*>(out);
		for (int i = threadIdx.x; i < pairs; i += blockDim.x)
		{
			const unsigned int v = cnt[i];
			out2[i] = make_double2(static_cast<double>(v & 0xFFFFu), static_cast<double>(v >> 16));
		}
		if ((npx & 1) && threadIdx.x == 0)
		{
			out[npx - 1] = static_cast<double>(cnt[pairs] & 0xFFFFu);
		}
	}
	else
	{
		for (int p = threadIdx.x; p < npx; p += blockDim.x)
		{
			const unsigned int v = U16 ? ((cnt[p >> 1] >> ((p & 1) * 16)) & 0xFFFFu) : cnt[p];
			out[p] = static_cast<double>(v);
		}
	}
}

// One event of a unit whose flow is wave-uniform, added to the tile [x0, x0 + tw) x [row0, row0 + th)
// of the warped count image (feature_detector.cpp:443-455): straight-line code, ONE divergent
// branch (the exact path) and one predicated LDS add.  The first versions of the count kernels
// spent more scalar instructions on exec-mask bookkeeping (nested && tests, per-event patch
// lookups) than vector instructions on the events: ~85 SALU per 64 events against the one scalar
// unit a CU has.  Float first: the float position differs from the reference's f64 one,
// fl64(x + fl64(fl64(dtw * scale) * m)), by at most 4e-7 |displacement| + 6e-8 |x|; farther than
// that from every half-integer both round to the same pixel; the rest (~0.4 % of the events, and
// anything huge or NaN: comparisons false) takes the f64 expression in the reference's order.
template <bool U16>
__device__ __forceinline__ void count_hit_uniform(uint64_t rec, bool live, int dtWin, double m0, double m1, float m0f,
												   float m1f, float thrX, float thrY, float scalef, double scale, int x0,
												   int row0, int tw, int th, unsigned int* cnt)
{
	int x, y, pos, dt;
	unpack(rec, x, y, pos, dt);
	const int dtw = dt + dtWin;
	const float prod = static_cast<float>(dtw) * scalef;
	const float vx = static_cast<float>(x) + prod * m0f, vy = static_cast<float>(y) + prod * m1f;
	const float rx = rintf(vx), ry = rintf(vy);
	// thrX / thrY: the unit's tolerance (count_unit_tolerance), wave-uniform -- the per-event form
	// kSureBase - 4e-7 |px| - 6e-8 |vx| cost eight vector instructions of the ~30 an event takes
	// (bitwise, not &&: no short-circuit branches)
	const bool sure = (static_cast<int>(fabsf(vx - rx) < thrX) & static_cast<int>(fabsf(vy - ry) < thrY)) != 0;
	int nx = static_cast<int>(rx), ny = static_cast<int>(ry);
	if (!sure)
	{
		const double d = static_cast<double>(dtw);
		const double fx = static_cast<double>(x) + d * scale * m0;
		const double fy = static_cast<double>(y) + d * scale * m1;
		live = (static_cast<int>(live) & static_cast<int>(convertible(fx)) & static_cast<int>(convertible(fy))) != 0;
		nx = static_cast<int>(round(live ? fx : 0.0));
		ny = static_cast<int>(round(live ? fy : 0.0));
	}
	const int cx = nx - x0, cy = ny - row0;
	if (static_cast<int>(live) & static_cast<int>(static_cast<unsigned>(cx) < static_cast<unsigned>(tw)) &
		static_cast<int>(static_cast<unsigned>(cy) < static_cast<unsigned>(th)))
	{
		// cy < th, tw < 2^15: the 24-bit multiply-add (full rate; v_mul_lo_u32 is a quarter-rate instruction)
		const unsigned int p = __umul24(static_cast<unsigned int>(cy), static_cast<unsigned int>(tw)) + static_cast<unsigned int>(cx);
		if (U16)
		{
			atomicAdd(&cnt[p >> 1], 1u << ((p & 1u) * 16u));
		}
		else
		{
			atomicAdd(&cnt[p], 1u);
		}
	}
}

// The float pre-test's tolerance for every event of a unit, one number per axis: the float
// position differs from the reference's f64 one by at most 4e-7 |displacement| + 6e-8 |position|
// (count_hit_uniform), |displacement| <= max|t_ref - t| |scale| |flow| (rounding is monotonic; 1e-6
// relative covers the float conversions of scale and flow and the float products), |position| <= the
// sensor's extent + the displacement.  NaN / inf flow: the tolerance is NaN or -inf, no event is
// "sure", all take the exact path.
__device__ __forceinline__ float count_unit_tolerance(int maxDt, double scale, double m, int extent)
{
	const float reach = static_cast<float>(static_cast<double>(maxDt) * fabs(scale) * fabs(m)) * 1.000001f;
	return kSureBase - 4e-7f * reach - 6e-8f * (static_cast<float>(extent) + reach + 1.0f);
}

// Unit waves over 2-D tiles (impl 5; the warped image of R2's final loop): workgroup = (tile,
// window) with the tile's counters in LDS; the events are taken unit by unit, one wave per unit at
// a time (an LDS work counter hands the units out), so a unit's reference-time offset and flow
// are wave-uniform scalars; a tile only takes the units whose events can reach it: the unit's rect
// grown by max|t_ref - t| x |scale| x |flow| (+1) on each axis.  Full-width row bands (impl 4) make
// a large sensor's units visit 5-6 bands each (C4: 15-row bands against a reach of +-25 rows);
// tiles a few hundred pixels on a side cut that to ~1.7 visits.  Tiles of a window take
// consecutive slots of one XCD (blockIdx % 8) so that re-reads of a unit's events hit that L2.
// One pass of a tile workgroup: rows [row0, row0 + th) x columns [x0, x0 + tw) counted in LDS from the
// selected units (headers in hdr[0, nSel)), then stored.  U16: two 16-bit counters per dword.
template <bool U16>
__device__ __forceinline__ void tile_pass(const uint64_t* __restrict__ events, const double* __restrict__ windowFlows,
										   const int32_t* __restrict__ wmax, const int4* hdr, int nSel, int* ctl, unsigned int* cnt, int x0, int row0, int tw, int th,
										   double* __restrict__ out /* image(row0, x0) */, int W, bool alignedImage,
										   const EvalConsts& c, bool preZeroed EDGE_TICK_ARG)
{
	const int npx = tw * th;
	const int nWords = U16 ? (npx + 1) >> 1 : npx;
	if (!preZeroed)  // (the caller zeroed the counters and ctl[0] under the latency of its unit-table loads)
	{
		for (int i = threadIdx.x; i < nWords; i += blockDim.x)
		{
			cnt[i] = 0u;
		}
		if (threadIdx.x == 0)
		{
			ctl[0] = 0;
		}
		__syncthreads();
	}
	EDGE_TICK(17);
	const int lane = threadIdx.x & 63;
	const float scalef = static_cast<float>(c.scale);
	// six 8-byte loads per lane and batch (round 4, end: 4 -> 6 is +1 point of HBM fraction at every size, 7 is mixed, 8 takes
	// the kernel over 64 VGPRs = one workgroup per CU; 16-byte loads are 3-5 points SLOWER: profiles/r04_count_*_ab.txt)
	constexpr int kInFlight = 6;
	// Software pipeline: the loads of the NEXT batch of 384 events (the same unit's, or the first
	// of the next unit the wave picks) are in flight while the current batch is counted.
	// what a wave needs of a unit, fetched when the unit is PICKED (one batch ahead of its use):
	// header, flow (f64 and float) and the float pre-test's tolerances -- all wave-uniform
	struct Picked
	{
		int4 h;
		double m0, m1;
		float m0f, m1f, thrX, thrY;
	};
	auto pick_unit = [&](Picked& q) -> bool {
		int pick = 0;
		if (lane == 0)
		{
			pick = atomicAdd(&ctl[0], 1);
		}
		pick = __builtin_amdgcn_readfirstlane(pick);
		if (pick >= nSel)
		{
			return false;
		}
		q.h = hdr[pick];
		const int u = q.h.w;
		q.m0 = windowFlows[2 * u];  // 16 KB per window: L1 / L2
		q.m1 = windowFlows[2 * u + 1];
		q.m0f = static_cast<float>(q.m0);
		q.m1f = static_cast<float>(q.m1);
		const int maxDt = wmax[u];
		q.thrX = count_unit_tolerance(maxDt, c.scale, q.m0, c.image_w);
		q.thrY = count_unit_tolerance(maxDt, c.scale, q.m1, c.image_h);
		return true;
	};
	Picked A;
	A.h = make_int4(0, 0, 0, 0);
	uint32_t posA = 0;
	bool haveA = pick_unit(A);
	if (haveA)
	{
		posA = static_cast<uint32_t>(A.h.x);
	}
	uint64_t recsA[kInFlight];
	if (haveA)
	{
#pragma unroll
		for (int k = 0; k < kInFlight; ++k)
		{
			const uint32_t ek = posA + lane + k * 64;
			recsA[k] = (ek < static_cast<uint32_t>(A.h.y)) ? events[ek] : 0ull;
		}
	}
	while (haveA)
	{
		// the batch after this one
		Picked B = A;
		uint32_t posB = posA + kInFlight * 64;
		bool haveB = true;
		if (posB >= static_cast<uint32_t>(A.h.y))
		{
			haveB = pick_unit(B);
			if (haveB)
			{
				posB = static_cast<uint32_t>(B.h.x);
			}
		}
		uint64_t recsB[kInFlight];
		if (haveB)
		{
#pragma unroll
			for (int k = 0; k < kInFlight; ++k)
			{
				const uint32_t ek = posB + lane + k * 64;
				recsB[k] = (ek < static_cast<uint32_t>(B.h.y)) ? events[ek] : 0ull;
			}
		}
		// count batch A
#pragma unroll
		for (int k = 0; k < kInFlight; ++k)
		{
			count_hit_uniform<U16>(recsA[k], posA + lane + k * 64 < static_cast<uint32_t>(A.h.y), A.h.z, A.m0, A.m1, A.m0f,
								   A.m1f, A.thrX, A.thrY, scalef, c.scale, x0, row0, tw, th, cnt);
		}
		haveA = haveB;
		A = B;
		posA = posB;
#pragma unroll
		for (int k = 0; k < kInFlight; ++k)
		{
			recsA[k] = recsB[k];
		}
	}
	EDGE_TICK(18);
	__syncthreads();
	EDGE_TICK(19);
	if (U16 && !(tw & 1) && !(W & 1) && !(x0 & 1) && alignedImage)
	{
		// one packed dword = two pixels of one row = one 16-byte store
		const int pairsPerRow = tw >> 1;
		for (int i = threadIdx.x; i < (npx >> 1); i += blockDim.x)
		{
			const int r = i / pairsPerRow, q = i - r * pairsPerRow;
			const unsigned int v = cnt[i];
			*reinterpret_cast<double2*>(out + static_cast<size_t>(r) * W + 2 * q) =
				make_double2(static_cast<double>(v & 0xFFFFu), static_cast<double>(v >> 16));
		}
	}
	else
	{
		for (int p = threadIdx.x; p < npx; p += blockDim.x)
		{
			const int r = p / tw, q = p - r * tw;
			const unsigned int v = U16 ? ((cnt[p >> 1] >> ((p & 1) * 16)) & 0xFFFFu) : cnt[p];
			out[static_cast<size_t>(r) * W + q] = static_cast<double>(v);
		}
	}
	EDGE_TICK(20);
	__syncthreads();
	EDGE_TICK(21);
}

__global__ void __launch_bounds__(1024) k_count_tiles(
	const uint64_t* __restrict__ events, const Unit* __restrict__ units, const int32_t* __restrict__ unitMaxDt,
	int unitsPerWindow, const double* __restrict__ flows, int tileW, int tileH, int tilesX, int tilesY, int cntBytes,
	int nWindows, double* __restrict__ image, EvalConsts c)
{
	// tileW x tileH: the pitch of the tile grid (the last tile of a row / column takes what is left
	// of the image); cntBytes: 2 bytes per pixel of a full tile
	extern __shared__ unsigned int cnt[];
	const int nTiles = tilesX * tilesY;
	const int slot = blockIdx.x >> 3;
	const int w = (slot / nTiles) * 8 + (blockIdx.x & 7);
	if (w >= nWindows)
	{
		return;
	}
	const int tile = slot % nTiles;
	const int tix = tile % tilesX, tiy = tile / tilesX;
	const int x0 = tix * tileW, row0 = tiy * tileH;
	const int tw = (tix == tilesX - 1) ? c.image_w - x0 : tileW, th = (tiy == tilesY - 1) ? c.image_h - row0 : tileH;
	const int W = c.image_w;
	const int P = c.npx * c.npy;
	// behind the counters: [0] next, [1] nSel, [2] most events of a selected unit, [3] largest reach
	// (ceil, both axes), then one 4-int header per selected unit {first event, end, dt_win, unit}: the
	// waves walk the units from LDS, not through dependent global loads
	EDGE_TICK_DECL;
	int* ctl = reinterpret_cast<int*>(reinterpret_cast<char*>(cnt) + cntBytes);
	int4* hdr = reinterpret_cast<int4*>(ctl + 4);
	const Unit* wu = units + static_cast<size_t>(w) * unitsPerWindow;
	const int32_t* wmax = unitMaxDt + static_cast<size_t>(w) * unitsPerWindow;
	const size_t imgSize = static_cast<size_t>(W) * c.image_h;
	const double* windowFlows = flows + 2 * static_cast<size_t>(w) * P;
	// which units can reach this tile (the stray unit is left to k_count_stray).  The first round of
	// unit-table loads is issued, the tile's counters are zeroed while they are in flight (a loaded
	// memory system answers in microseconds), then the units are sorted out.
	auto consider = [&](int u, const Unit& un, int maxDt, double f0, double f1) {
		bool take = un.n_ev > 0;
		// |fl(fl(dtw * scale) * m)| <= fl(fl(maxdt * |scale|) * |m|): rounding is monotonic
		const double t = static_cast<double>(maxDt) * fabs(c.scale);
		const double reachX = t * fabs(f0) + 1.0, reachY = t * fabs(f1) + 1.0;
		if (take && nTiles > 1)
		{
			const double lox = static_cast<double>(un.rx) - reachX, hix = static_cast<double>(un.rx + un.rw - 1) + reachX;
			const double loy = static_cast<double>(un.ry) - reachY, hiy = static_cast<double>(un.ry + un.rh - 1) + reachY;
			// NaN / inf reach: comparisons false -> taken
			take = !(hix < static_cast<double>(x0) - 0.5 || lox > static_cast<double>(x0 + tw) - 0.5 ||
					 hiy < static_cast<double>(row0) - 0.5 || loy > static_cast<double>(row0 + th) - 0.5);
		}
		if (take)
		{
			hdr[atomicAdd(&ctl[1], 1)] = make_int4(static_cast<int>(un.ev_off), static_cast<int>(un.ev_off + un.n_ev), un.dt_win, u);
			atomicMax(&ctl[2], static_cast<int>(min(un.n_ev, 0x7fffffffu)));
			const double rr = fmax(reachX, reachY);
			atomicMax(&ctl[3], (rr < 1e6) ? static_cast<int>(ceil(rr)) : 1000000);  // NaN -> 1000000
		}
	};
	{
		const int u0 = threadIdx.x;
		const bool have0 = u0 < P;
		Unit un0 = {};
		int maxDt0 = 0;
		double f00 = 0.0, f01 = 0.0;
		if (have0)
		{
			un0 = wu[u0];
			maxDt0 = wmax[u0];
			f00 = windowFlows[2 * u0];
			f01 = windowFlows[2 * u0 + 1];
		}
		const int nWords16 = (tw * th + 1) >> 1;
		for (int i = threadIdx.x; i < nWords16; i += blockDim.x)
		{
			cnt[i] = 0u;
		}
		if (threadIdx.x < 4)
		{
			ctl[threadIdx.x] = 0;
		}
		__syncthreads();
		if (have0)
		{
			consider(u0, un0, maxDt0, f00, f01);
		}
		for (int u = threadIdx.x + blockDim.x; u < P; u += blockDim.x)
		{
			consider(u, wu[u], wmax[u], windowFlows[2 * u], windowFlows[2 * u + 1]);
		}
	}
	__syncthreads();
	EDGE_TICK(16);
	const int nSel = ctl[1];
	EDGE_COUNT(22, nSel);
	EDGE_COUNT(23, 1);
	// 16-bit counters are safe when no pixel can collect 65536 events: a pixel is within reach of at
	// most (1 + 2 ceil(R / pw)) (1 + 2 ceil(R / ph)) patches (the grid's last patches are larger: fewer),
	// each with at most ctl[2] events.  Otherwise (wild flows, one patch holding most of a window)
	// the tile is counted in slices of half its rows with 32-bit counters: any input is handled, that one slowly.
	const long nx = 1 + 2 * ((ctl[3] + c.patch_w - 1) / c.patch_w), ny = 1 + 2 * ((ctl[3] + c.patch_h - 1) / c.patch_h);
	const bool safe16 = nx * ny * static_cast<long>(ctl[2]) < 65536;
	double* out = image + static_cast<size_t>(w) * imgSize + static_cast<size_t>(row0) * W + x0;
	const bool alignedImage = (reinterpret_cast<uintptr_t>(image) & 15) == 0;
	if (safe16)
	{
		tile_pass<true>(events, windowFlows, wmax, hdr, nSel, ctl, cnt, x0, row0, tw, th, out, W, alignedImage, c, true EDGE_TICK_PASS);
	}
	else
	{
		// the LDS holds 2 bytes per pixel of a full tile: 32-bit counters for tileH / 2 rows at a time
		const int hMax = max(tileH / 2, 1);
		for (int r = 0; r < th; r += hMax)
		{
			tile_pass<false>(events, windowFlows, wmax, hdr, nSel, ctl, cnt, x0, row0 + r, tw, min(hMax, th - r),
							 out + static_cast<size_t>(r) * W, W, alignedImage, c, false EDGE_TICK_PASS);
		}
	}
	EDGE_TICK_FLUSH;
}

// The stray unit of every window (events outside the sensor; none in a real recording) for the
// kernels that leave it out: warped by the flow of the clamped patch (:436-441), added with f64
// atomics after the image has been stored.
__global__ void k_count_stray(const uint64_t* __restrict__ events, const Unit* __restrict__ units, int unitsPerWindow,
							  const double* __restrict__ flows, double* __restrict__ image, EvalConsts c)
{
	const int w = blockIdx.x;
	const int P = c.npx * c.npy;
	const Unit un = units[static_cast<size_t>(w) * unitsPerWindow + P];
	const double* windowFlows = flows + 2 * static_cast<size_t>(w) * P;
	double* img = image + static_cast<size_t>(w) * c.image_w * c.image_h;
	for (uint32_t e = threadIdx.x; e < un.n_ev; e += blockDim.x)
	{
		const uint64_t rec = events[un.ev_off + e];
		double m0, m1;
		stray_flow(rec, windowFlows, c, m0, m1);
		int nx, ny;
		if (count_target<1>(rec, true, un.dt_win, m0, m1, nullptr, c, nx, ny))
		{
			unsafeAtomicAdd(&img[static_cast<size_t>(ny) * c.image_w + nx], 1.0);  // exact on integer counts
		}
	}
}

// Patch-row bands (impl 2): the un-warped image (mode 0); workgroup = (band of whole patch rows,
// window).  Events are stored unit by unit in patch order, so the events of a band are one
// contiguous range and stay in it: the workgroup streams only those (no re-reads by other bands,
// any image size), counts them in LDS and stores its rows.  The stray unit of the window (events
// outside the sensor) is streamed by band 0.  HBM traffic = events once + image once; integer
// adds commute => bit-exact.
template <bool U16>
__global__ void __launch_bounds__(512) k_count_bands(
	const uint64_t* __restrict__ events, const Unit* __restrict__ units, int unitsPerWindow,
	int patchRowsPerBand, int nRegular, int colTiles, double* __restrict__ image, EvalConsts c)
{
	extern __shared__ unsigned int cnt[];
	const int w = blockIdx.y;
	// colTiles > 1 (large sensors, one patch row per band): the band is cut into column tiles of
	// whole patches -- the units of a tile are still one contiguous event range -- so that the
	// counters of a workgroup stay small enough for several workgroups per CU
	const int band = blockIdx.x / colTiles;
	const int tile = blockIdx.x - band * colTiles;
	const int unitsPerTile = (c.npx + colTiles - 1) / colTiles;
	const int uLo = min(tile * unitsPerTile, c.npx), uHi = min(uLo + unitsPerTile, c.npx);
	const int x0 = uLo * c.patch_w;
	const int x1 = (uHi == c.npx) ? c.image_w : uHi * c.patch_w;
	if (uLo >= uHi)
	{
		return;
	}
	// bands 0..nRegular-1: patchRowsPerBand whole patch rows each, over patch rows [0, npy-1);
	// then the last patch row (which absorbs the remainder of the image height and can be
	// almost twice as tall) in sub-bands of at most patchRowsPerBand * patch_h rows.
	int pr0, pr1, row0, row1;
	if (band < nRegular)
	{
		pr0 = band * patchRowsPerBand;
		pr1 = min(pr0 + patchRowsPerBand, c.npy - 1);
		row0 = pr0 * c.patch_h;
		row1 = pr1 * c.patch_h;
	}
	else
	{
		pr0 = c.npy - 1;
		pr1 = c.npy;
		const int sub = band - nRegular;
		row0 = pr0 * c.patch_h + sub * patchRowsPerBand * c.patch_h;
		row1 = min(row0 + patchRowsPerBand * c.patch_h, c.image_h);
	}
	const int rows = row1 - row0;
	const int W = c.image_w;
	const int tw = x1 - x0;  // == W without column tiles
	const int npx = rows * tw;
	const int nWords = U16 ? (npx + 1) >> 1 : npx;
	for (int i = threadIdx.x; i < nWords; i += blockDim.x)
	{
		cnt[i] = 0u;
	}
	__syncthreads();
	const Unit* wu = units + static_cast<size_t>(w) * unitsPerWindow;
	const int P = c.npx * c.npy;
	const size_t imgSize = static_cast<size_t>(W) * c.image_h;
	constexpr int kInFlight = 8;
	// pass 0: the band's own patch units; pass 1 (band 0, tile 0 only): the stray unit
	for (int pass = 0; pass < ((band == 0 && tile == 0) ? 2 : 1); ++pass)
	{
		const int ui = pass == 0 ? pr0 * c.npx + uLo : P;
		const int uLast = pass == 0 ? (pr1 - 1) * c.npx + uHi - 1 : P;
		const uint32_t evBegin = wu[ui].ev_off;
		const uint32_t evEnd = wu[uLast].ev_off + wu[uLast].n_ev;
		for (uint32_t eb = evBegin + threadIdx.x; eb < evEnd; eb += kInFlight * blockDim.x)
		{
			uint64_t recs[kInFlight];
#pragma unroll
			for (int k = 0; k < kInFlight; ++k)
			{
				const uint32_t ek = eb + k * blockDim.x;
				recs[k] = (ek < evEnd) ? events[ek] : 0ull;
			}
#pragma unroll
			for (int k = 0; k < kInFlight; ++k)
			{
				const uint32_t e = eb + k * blockDim.x;
				int nx, ny;
				const bool live = count_target<0>(recs[k], e < evEnd, 0, 0.0, 0.0, nullptr, c, nx, ny);
				const int ry = ny - row0;
				const bool inBand = live && ry >= 0 && ry < rows && nx >= x0 && nx < x1;
				if (inBand)
				{
					const int p = ry * tw + (nx - x0);
					if (U16)
					{
						atomicAdd(&cnt[p >> 1], 1u << ((p & 1) * 16));
					}
					else
					{
						atomicAdd(&cnt[p], 1u);
					}
				}
			}
		}
	}
	__syncthreads();
	double* out = image + static_cast<size_t>(w) * imgSize + static_cast<size_t>(row0) * W;
	if (tw != W)
	{
		// column tile: row segments of tw pixels
		for (int p = threadIdx.x; p < npx; p += blockDim.x)
		{
			const int r = p / tw, lx = p - r * tw;
			const unsigned int v = U16 ? ((cnt[p >> 1] >> ((p & 1) * 16)) & 0xFFFFu) : cnt[p];
			out[static_cast<size_t>(r) * W + x0 + lx] = static_cast<double>(v);
		}
	}
	else if (U16 && (reinterpret_cast<uintptr_t>(out) & 15) == 0)
	{
		const int pairs = npx >> 1;
		double2* out2 = reinterpret_cast<double2*>(out);
		for (int i = threadIdx.x; i < pairs; i += blockDim.x)
		{
			const unsigned int v = cnt[i];
			out2[i] = make_double2(static_cast<double>(v & 0xFFFFu), static_cast<double>(v >> 16));
		}
		if ((npx & 1) && threadIdx.x == 0)
		{
			out[npx - 1] = static_cast<double>(cnt[pairs] & 0xFFFFu);
		}
	}
	else
	{
		for (int p = threadIdx.x; p < npx; p += blockDim.x)
		{
			const unsigned int v = U16 ? ((cnt[p >> 1] >> ((p & 1) * 16)) & 0xFFFFu) : cnt[p];
			out[p] = static_cast<double>(v);
		}
	}
}

// ---------------------------------------------------------------------------------------
// Sorted bands (impl 3): warped count images of sensors too large for a whole-window LDS image.
// Every event's DESTINATION decides which row band counts it, so the events are first sorted
// by destination band -- histogram, scan, scatter of 4-byte destination pixels -- and then each
// (band, window) workgroup counts its own list in LDS and writes finished f64 rows.  No global
// atomics on the image, no per-event random HBM access, the same cost for any flow magnitude.
// Traffic per event: 8 B (histogram) + 8 B (scatter) + 4 B written + 4 B read, + the image
// once: ~2x the algorithmic bytes, all of it streaming.
//   sortBins: [0, nBins) counts, [nBins, 2 nBins] exclusive starts, [2 nBins + 1, 3 nBins + 1)
//   cursors; bin = window * bandsPerWindow + band.
// ---------------------------------------------------------------------------------------

// The chunk [e0, e1) of window w: destination pixel (ny * W + nx) of each of the lane's 16
// events, or 0xFFFFFFFF when the event contributes nothing.
template <int MODE>
__device__ __forceinline__ void sort_targets(const uint64_t* __restrict__ events, const Unit* __restrict__ wu,
											 int unitsPerWindow, const void* __restrict__ aux, int w, uint32_t e0,
											 uint32_t e1, const EvalConsts& c, unsigned int (&dst)[16])
{
	const int P = c.npx * c.npy;
	const size_t imgSize = static_cast<size_t>(c.image_w) * c.image_h;
	const double* windowFlows = static_cast<const double*>(aux) + (MODE == 1 ? 2 * static_cast<size_t>(w) * P : 0);
	const float* windowField = static_cast<const float*>(aux) + (MODE == 2 ? 2 * static_cast<size_t>(w) * imgSize : 0);
	uint64_t recs[16];
#pragma unroll
	for (int k = 0; k < 16; ++k)
	{
		const uint32_t e = e0 + threadIdx.x + k * 256;
		recs[k] = e < e1 ? events[e] : 0ull;
	}
#pragma unroll
	for (int k = 0; k < 16; ++k)
	{
		const uint32_t e = e0 + threadIdx.x + k * 256;
		int patch, unit;
		event_unit(recs[k], c, patch, unit);
		double m0 = 0.0, m1 = 0.0;
		if (MODE == 1)
		{
			m0 = windowFlows[2 * patch];
			m1 = windowFlows[2 * patch + 1];
		}
		int nx, ny;
		const bool hit = count_target<MODE>(recs[k], e < e1, wu[unit].dt_win, m0, m1, windowField, c, nx, ny);
		dst[k] = hit ? static_cast<unsigned int>(ny * c.image_w + nx) : 0xFFFFFFFFu;
	}
}

template <int MODE>
__global__ void __launch_bounds__(256) k_csort_hist(const uint64_t* __restrict__ events, const Unit* __restrict__ units,
													 int unitsPerWindow, const void* __restrict__ aux, int rowsPerBand,
													 int bandsPerWindow, unsigned int* __restrict__ sortBins,
													 unsigned int* __restrict__ dstList, EvalConsts c)
{
	extern __shared__ unsigned int hist[];
	const int w = blockIdx.y;
	const Unit* wu = units + static_cast<size_t>(w) * unitsPerWindow;
	const uint32_t evBegin = wu[0].ev_off;
	const uint32_t evEnd = wu[unitsPerWindow - 1].ev_off + wu[unitsPerWindow - 1].n_ev;
	const uint32_t e0 = evBegin + blockIdx.x * kSortChunk;
	if (e0 >= evEnd)
	{
		return;
	}
	const uint32_t e1 = min(e0 + kSortChunk, evEnd);
	for (int b = threadIdx.x; b < bandsPerWindow; b += blockDim.x)
	{
		hist[b] = 0u;
	}
	__syncthreads();
	unsigned int dst[16];
	sort_targets<MODE>(events, wu, unitsPerWindow, aux, w, e0, e1, c, dst);
	const unsigned int bandPx = static_cast<unsigned int>(rowsPerBand) * c.image_w;
#pragma unroll
	for (int k = 0; k < 16; ++k)
	{
		// the destinations are kept (4 B/event, in event order) so that the scatter pass does
		// not warp again: the f64 warp arithmetic, not the traffic, is what these passes cost
		const uint32_t e = e0 + threadIdx.x + k * 256;
		if (e < e1)
		{
			dstList[e] = dst[k];
		}
		if (dst[k] != 0xFFFFFFFFu)
		{
			atomicAdd(&hist[dst[k] / bandPx], 1u);
		}
	}
	__syncthreads();
	for (int b = threadIdx.x; b < bandsPerWindow; b += blockDim.x)
	{
		if (hist[b])
		{
			atomicAdd(&sortBins[static_cast<size_t>(w) * bandsPerWindow + b], hist[b]);
		}
	}
}

// Exclusive scan of the bin counts (a few thousand bins: one workgroup), cursors = starts.
__global__ void __launch_bounds__(1024) k_csort_scan(unsigned int* __restrict__ sortBins, int nBins)
{
	__shared__ unsigned int part[1024];
	unsigned int* counts = sortBins;
	unsigned int* starts = sortBins + nBins;
	unsigned int* cursors = sortBins + 2 * nBins + 1;
	const int per = (nBins + 1023) / 1024;
	const int b0 = threadIdx.x * per, b1 = min(b0 + per, nBins);
	unsigned int s = 0;
	for (int b = b0; b < b1; ++b)
	{
		s += counts[b];
	}
	unsigned int total;
	unsigned int run = block_exclusive_scan(s, part, total);
	if (threadIdx.x == 0)
	{
		starts[nBins] = total;
	}
	for (int b = b0; b < b1; ++b)
	{
		starts[b] = run;
		cursors[b] = run;
		run += counts[b];
	}
}

__global__ void __launch_bounds__(256) k_csort_scatter(const Unit* __restrict__ units, int unitsPerWindow,
														const unsigned int* __restrict__ dstList, int rowsPerBand,
														int bandsPerWindow, unsigned int* __restrict__ sortBins, int nBins,
														unsigned int* __restrict__ sorted, EvalConsts c)
{
	extern __shared__ unsigned int sortLds[];
	unsigned int* hist = sortLds;                       // counts of this chunk per band
	unsigned int* base = sortLds + bandsPerWindow;      // start of the chunk's range in the band's list
	unsigned int* lstart = base + bandsPerWindow;       // start of the band inside the staged chunk
	unsigned int* lcur = lstart + bandsPerWindow;       // cursor inside the staged chunk
	unsigned int* staged = lcur + bandsPerWindow;       // [kSortChunk] destinations grouped by band
	unsigned short* bandOf = reinterpret_cast<unsigned short*>(staged + kSortChunk);  // [kSortChunk]
	__shared__ unsigned int part[256];
	const int w = blockIdx.y;
	const Unit* wu = units + static_cast<size_t>(w) * unitsPerWindow;
	const uint32_t evBegin = wu[0].ev_off;
	const uint32_t evEnd = wu[unitsPerWindow - 1].ev_off + wu[unitsPerWindow - 1].n_ev;
	const uint32_t e0 = evBegin + blockIdx.x * kSortChunk;
	if (e0 >= evEnd)
	{
		return;
	}
	const uint32_t e1 = min(e0 + kSortChunk, evEnd);
	for (int b = threadIdx.x; b < bandsPerWindow; b += blockDim.x)
	{
		hist[b] = 0u;
	}
	__syncthreads();
	unsigned int dst[16];
#pragma unroll
	for (int k = 0; k < 16; ++k)
	{
		const uint32_t e = e0 + threadIdx.x + k * 256;
		dst[k] = e < e1 ? dstList[e] : 0xFFFFFFFFu;
	}
	const unsigned int bandPx = static_cast<unsigned int>(rowsPerBand) * c.image_w;
#pragma unroll
	for (int k = 0; k < 16; ++k)
	{
		if (dst[k] != 0xFFFFFFFFu)
		{
			atomicAdd(&hist[dst[k] / bandPx], 1u);
		}
	}
	__syncthreads();
	// exclusive scan of hist over the bands (segments per thread, then 256 partials), and one
	// global atomic per (chunk, band) reserves the chunk's range in the band's list
	unsigned int* cursors = sortBins + 2 * nBins + 1;
	const int per = (bandsPerWindow + 255) / 256;
	const int s0 = min(static_cast<int>(threadIdx.x) * per, bandsPerWindow), s1 = min(s0 + per, bandsPerWindow);
	unsigned int sum = 0;
	for (int bnd = s0; bnd < s1; ++bnd)
	{
		sum += hist[bnd];
	}
	unsigned int chunkTotal;
	unsigned int run = block_exclusive_scan(sum, part, chunkTotal);  // (a serial scan of the 256 partials by one thread was 45 % of this kernel)
	for (int bnd = s0; bnd < s1; ++bnd)
	{
		const unsigned int h = hist[bnd];
		lstart[bnd] = run;
		lcur[bnd] = run;
		base[bnd] = h ? atomicAdd(&cursors[static_cast<size_t>(w) * bandsPerWindow + bnd], h) : 0u;
		run += h;
	}
	__syncthreads();
	// group the chunk's destinations by band in LDS, then stream them out: consecutive lanes
	// write consecutive entries of a band's list (4-byte stores scattered per lane were the
	// bottleneck of the first version)
#pragma unroll
	for (int k = 0; k < 16; ++k)
	{
		if (dst[k] != 0xFFFFFFFFu)
		{
			// (one LDS atomic per distinct band of the wave -- ballot, leader add, prefix count -- was
			// tried for these ranks and for the histograms: C3 0.34 -> 0.23 ms, but C4 0.32 -> 0.49 ms,
			// where a wave's events spread over ~12 of the 180 four-row bands; C3 runs impl 1 anyway)
			const unsigned int bnd = dst[k] / bandPx;
			const unsigned int at = atomicAdd(&lcur[bnd], 1u);
			staged[at] = dst[k];
			bandOf[at] = static_cast<unsigned short>(bnd);
		}
	}
	__syncthreads();
	const unsigned int nValid = lstart[bandsPerWindow - 1] + hist[bandsPerWindow - 1];
	for (unsigned int j = threadIdx.x; j < nValid; j += blockDim.x)
	{
		const unsigned int bnd = bandOf[j];
		sorted[base[bnd] + (j - lstart[bnd])] = staged[j];
	}
}

template <bool U16>
__global__ void __launch_bounds__(512) k_csort_count(const unsigned int* __restrict__ sortBins, int nBins,
													  const unsigned int* __restrict__ sorted, int rowsPerBand,
													  int bandsPerWindow, double* __restrict__ image, EvalConsts c)
{
	extern __shared__ unsigned int cnt[];
	const int w = blockIdx.y, band = blockIdx.x;
	const int row0 = band * rowsPerBand;
	const int rows = min(rowsPerBand, c.image_h - row0);
	const int W = c.image_w;
	const int npx = rows * W;
	const int nWords = U16 ? (npx + 1) >> 1 : npx;
	for (int i = threadIdx.x; i < nWords; i += blockDim.x)
	{
		cnt[i] = 0u;
	}
	__syncthreads();
	const unsigned int* starts = sortBins + nBins;
	const size_t bin = static_cast<size_t>(w) * bandsPerWindow + band;
	const unsigned int b0 = starts[bin], b1 = starts[bin + 1];
	const unsigned int origin = static_cast<unsigned int>(row0) * W;
	for (unsigned int i = b0 + threadIdx.x; i < b1; i += blockDim.x)
	{
		const int p = static_cast<int>(sorted[i] - origin);
		if (U16)
		{
			atomicAdd(&cnt[p >> 1], 1u << ((p & 1) * 16));
		}
		else
		{
			atomicAdd(&cnt[p], 1u);
		}
	}
	__syncthreads();
	double* out = image + static_cast<size_t>(w) * W * c.image_h + static_cast<size_t>(row0) * W;
	if (U16 && (reinterpret_cast<uintptr_t>(out) & 15) == 0)
	{
		const int pairs = npx >> 1;
		double2* out2 = reinterpret_cast<double2*>(out);
		for (int i = threadIdx.x; i < pairs; i += blockDim.x)
		{
			const unsigned int v = cnt[i];
			out2[i] = make_double2(static_cast<double>(v & 0xFFFFu), static_cast<double>(v >> 16));
		}
		if ((npx & 1) && threadIdx.x == 0)
		{
			out[npx - 1] = static_cast<double>(cnt[pairs] & 0xFFFFu);
		}
	}
	else
	{
		for (int p = threadIdx.x; p < npx; p += blockDim.x)
		{
			const unsigned int v = U16 ? ((cnt[p >> 1] >> ((p & 1) * 16)) & 0xFFFFu) : cnt[p];
			out[p] = static_cast<double>(v);
		}
	}
}

// int32 counts -> f64 image (the reference's CV_64F); re-zeroes the scratch.
__global__ void k_counts_to_f64(int32_t* __restrict__ counts, double* __restrict__ image, size_t n)
{
	const size_t stride = static_cast<size_t>(gridDim.x) * blockDim.x;
	for (size_t i = static_cast<size_t>(blockIdx.x) * blockDim.x + threadIdx.x; i < n; i += stride)
	{
		image[i] = static_cast<double>(counts[i]);
		counts[i] = 0;
	}
}
