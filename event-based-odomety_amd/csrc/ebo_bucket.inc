// ebo_bucket.inc — device-side bucketing of raw events (SURVEY §8(f) #2): replaces the
// O(P*N) per-patch scan of FeatureDetector::compensateEventsContrast
// (feature_detector.cpp:348-355) and the host counting sort of ebo_set_windows.
// Included inside ebo_kernels.hip's anonymous namespace.
//
// Input: raw 24-byte ebo_event records (the layout of common::EventSample) of n windows,
// window w = raw[offsets[w] .. offsets[w+1]), time ordered.  Output: the packed 8-byte
// records grouped by unit + the unit table, exactly what the host path produces, the order
// INSIDE a unit included: the canonical order of order_deal.h (k_bucket_canon below), units
// above kSortMax events in list order.  A unit's reference time is the int32-truncated mean
// of its EARLIEST and LATEST event time: the functor's front / back (contrast_functor.h:18-20)
// for a time-ordered window, and the same number for any permutation of a window that is
// not -- the host path (set_windows_host) takes it the same way.  The window's reference
// time is the mean of its first and last LISTED event time (feature_detector.cpp:305-306).
//
// Five launches: count (+ per-bucket min/max time and per-chunk histograms), scan (unit table),
// chunk scan (first ranks), scatter (pack, stable), canon (canonical order).
// Error bits in *flag: 1 coordinate range, 2 mid-time beyond int32, 4 dt beyond int32.

struct RawEvent
{
	int32_t x, y, sign, reserved;
	long long t_us;
};

// Input formats of the bucketing kernels: the 24-byte common::EventSample layout (ebo_event) or
// the 8-byte compact record (ebo_event8: x:15 | polarity:1 | y:15 | 0:1, then int32 microseconds
// relative to the window's base time) -- a third of the bytes over PCIe.
struct Rec24
{
	const RawEvent* p;
	__device__ __forceinline__ void load(unsigned long long e, int /*w*/, int& x, int& y, int& pos, long long& t) const
	{
		const RawEvent r = p[e];
		x = r.x;
		y = r.y;
		pos = r.sign > 0 ? 1 : 0;
		t = r.t_us;
	}
	static constexpr bool kCheckRange = true;
};
struct Rec8
{
	const uint2* p;
	const long long* tbase;  // [n_windows]
	__device__ __forceinline__ void load(unsigned long long e, int w, int& x, int& y, int& pos, long long& t) const
	{
		const uint2 r = p[e];
		x = static_cast<int>(r.x << 17) >> 17;
		y = static_cast<int>(r.x << 1) >> 17;
		pos = (r.x >> 15) & 1u;
		t = tbase[w] + static_cast<long long>(static_cast<int>(r.y));
	}
	static constexpr bool kCheckRange = false;  // 15-bit fields cannot leave the packed range
};

__device__ __forceinline__ int bucket_of(int x, int y, const EvalConsts& c, int P)
{
	if (x < 0 || x >= c.image_w || y < 0 || y >= c.image_h)
	{
		return P;  // stray bucket
	}
	const int bx = min(x / c.patch_w, c.npx - 1);
	const int by = min(y / c.patch_h, c.npy - 1);
	return by * c.npx + bx;
}

__device__ __forceinline__ bool mid_time_dev(long long a, long long b, long long& out)
{
	const double half = static_cast<double>(a + b) * 0.5;
	if (!(half > -2147483648.0 && half < 2147483648.0))
	{
		return false;
	}
	out = static_cast<long long>(static_cast<int>(half));
	return true;
}

constexpr int kBucketChunk = 2048;       // events per chunk (one workgroup of the count pass, one wave of the scatter)
constexpr int kBucketChunkSmall = 256;   // ... for small inputs: a single 15 k-event window is 59 chunks instead of 8

__global__ void k_bucket_init(int* __restrict__ cnt, long long* __restrict__ tmin,
							  long long* __restrict__ tmax, int n, int* __restrict__ flag)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i < n)
	{
		cnt[i] = 0;
		tmin[i] = 0x7fffffffffffffffll;
		tmax[i] = -0x7fffffffffffffffll - 1;
	}
	if (i == 0)
	{
		*flag = 0;
	}
}

// grid (chunks, windows); LDS: (P+1) x {int count, i64 min, i64 max}
template <class Rec>
__global__ void k_bucket_count(Rec raw, const unsigned long long* __restrict__ offsets, int wBase,
							   int P, int* __restrict__ cnt, long long* __restrict__ tmin,
							   long long* __restrict__ tmax, int* __restrict__ flag,
							   unsigned int* __restrict__ chunkHist /* [windows][maxChunks][P + 1] */, int chunk, EvalConsts c)
{
	extern __shared__ long long bsm[];
	const int w = wBase + blockIdx.y;
	const unsigned long long e0 = offsets[w], e1 = offsets[w + 1];
	const unsigned long long begin = e0 + static_cast<unsigned long long>(blockIdx.x) * chunk;
	if (begin >= e1)
	{
		return;
	}
	const unsigned long long end = begin + chunk < e1 ? begin + chunk : e1;
	long long* lmin = bsm;
	long long* lmax = bsm + (P + 1);
	int* lcnt = reinterpret_cast<int*>(bsm + 2 * (P + 1));
	for (int b = threadIdx.x; b <= P; b += blockDim.x)
	{
		lmin[b] = 0x7fffffffffffffffll;
		lmax[b] = -0x7fffffffffffffffll - 1;
		lcnt[b] = 0;
	}
	__syncthreads();
	bool bad = false;
	for (unsigned long long e = begin + threadIdx.x; e < end; e += blockDim.x)
	{
		int x, y, pos;
		long long t;
		raw.load(e, w, x, y, pos, t);
		if (Rec::kCheckRange && (x < kCoordMin || x > kCoordMax || y < kCoordMin || y > kCoordMax))
		{
			bad = true;
			continue;
		}
		const int b = bucket_of(x, y, c, P);
		atomicAdd(&lcnt[b], 1);
		atomicMin(&lmin[b], t);
		atomicMax(&lmax[b], t);
	}
	if (bad)
	{
		atomicOr(flag, 1);
	}
	__syncthreads();
	const size_t base = static_cast<size_t>(w) * (P + 1);
	// the chunk's own histogram: k_bucket_chunk_scan turns the column of a bucket into the chunk's
	// first rank inside that bucket, which makes the scatter STABLE (time order inside a unit)
	unsigned int* hrow = chunkHist + (static_cast<size_t>(w) * gridDim.x + blockIdx.x) * (P + 1);
	for (int b = threadIdx.x; b <= P; b += blockDim.x)
	{
		hrow[b] = static_cast<unsigned int>(lcnt[b]);
		if (lcnt[b])
		{
			atomicAdd(&cnt[base + b], lcnt[b]);
			atomicMin(&tmin[base + b], lmin[b]);
			atomicMax(&tmax[base + b], lmax[b]);
		}
	}
}

// column-wise exclusive scan of the chunk histograms: table[w][chunk][b] = events of bucket b in the
// chunks before `chunk`.  One thread per (window, bucket), coalesced over the buckets.
__global__ void k_bucket_chunk_scan(const unsigned long long* __restrict__ offsets, int wBase, int P, int maxChunks,
									int chunk, unsigned int* __restrict__ table)
{
	const int w = wBase + blockIdx.y;
	const int b = blockIdx.x * blockDim.x + threadIdx.x;
	if (b > P)
	{
		return;
	}
	const unsigned long long n = offsets[w + 1] - offsets[w];
	const int nChunks = static_cast<int>((n + chunk - 1) / chunk);
	unsigned int* col = table + static_cast<size_t>(w) * maxChunks * (P + 1) + b;
	unsigned int running = 0;
	for (int k = 0; k < nChunks; ++k)
	{
		const unsigned int v = col[static_cast<size_t>(k) * (P + 1)];
		col[static_cast<size_t>(k) * (P + 1)] = running;
		running += v;
	}
}

// one workgroup per window: prefix sums (shuffle scan over the buckets, 256 at a time), unit
// table, reference times; cnt becomes the scatter cursor (reset to 0).  (One THREAD per window
// walked the buckets serially at first: 0.85 ms for 32 windows of 1025 units.)
template <class Rec>
__global__ void __launch_bounds__(256) k_bucket_scan(Rec raw, const unsigned long long* __restrict__ offsets, int wBase,
							  int nWindows, int P, int* __restrict__ cnt, const long long* __restrict__ tmin,
							  const long long* __restrict__ tmax, unsigned int minEvents,
							  Unit* __restrict__ units, long long* __restrict__ unitTref, int32_t* __restrict__ unitMaxDt,
							  long long* __restrict__ winTref, int* __restrict__ flag, EvalConsts c)
{
	__shared__ unsigned int scanTmp[8];
	const int w = wBase + blockIdx.x;
	if (w >= nWindows)
	{
		return;
	}
	const unsigned long long e0 = offsets[w], e1 = offsets[w + 1];
	long long tw = 0;
	long long tFirst = 0, tLast = 0;
	if (e1 > e0)
	{
		int x, y, pos;
		raw.load(e0, w, x, y, pos, tFirst);
		raw.load(e1 - 1, w, x, y, pos, tLast);
	}
	if (e1 > e0 && !mid_time_dev(tFirst, tLast, tw))  // feature_detector.cpp:305-306
	{
		if (threadIdx.x == 0)
		{
			atomicOr(flag, 2);
		}
	}
	if (threadIdx.x == 0)
	{
		winTref[w] = tw;
	}
	unsigned long long chunkOff = e0 - offsets[0];
	const size_t base = static_cast<size_t>(w) * (P + 1);
	for (int b0 = 0; b0 <= P; b0 += static_cast<int>(blockDim.x))
	{
		const int b = b0 + static_cast<int>(threadIdx.x);
		const bool have = b <= P;
		const int n = have ? cnt[base + b] : 0;
		unsigned int total;
		const unsigned int before = block_exclusive_scan(static_cast<unsigned int>(n), scanTmp, total);
		if (have)
		{
			Unit u;
			u.ev_off = static_cast<uint32_t>(chunkOff + before);
			u.n_ev = static_cast<uint32_t>(n);
			u.flags = 0;
			u.flow_idx = static_cast<uint32_t>(static_cast<size_t>(w) * P + min(b, P - 1));
			long long tu = tw;
			if (b < P)
			{
				const int px = b % c.npx, py = b / c.npx;
				u.rx = static_cast<int16_t>(px * c.patch_w);
				u.ry = static_cast<int16_t>(py * c.patch_h);
				u.rw = static_cast<int16_t>(px == c.npx - 1 ? c.image_w - px * c.patch_w : c.patch_w);
				u.rh = static_cast<int16_t>(py == c.npy - 1 ? c.image_h - py * c.patch_h : c.patch_h);
				if (n > 0 && !mid_time_dev(tmin[base + b], tmax[base + b], tu))  // contrast_functor.h:18-20
				{
					atomicOr(flag, 2);
				}
				if (static_cast<unsigned int>(n) > minEvents)  // feature_detector.cpp:357
				{
					u.flags |= kUnitActive;
				}
			}
			else
			{
				u.rx = 0;
				u.ry = 0;
				u.rw = 1;
				u.rh = 1;
				u.flags |= kUnitStray;
			}
			const long long dwin = tw - tu;
			if (dwin < -2147483648ll || dwin > 2147483647ll)
			{
				atomicOr(flag, 4);
			}
			u.dt_win = static_cast<int32_t>(dwin);
			units[base + b] = u;
			unitTref[base + b] = tu;
			long long md = 0;
			if (n > 0)
			{
				const long long a = tw - tmin[base + b], z = tw - tmax[base + b];
				md = max(a < 0 ? -a : a, z < 0 ? -z : z);
			}
			unitMaxDt[base + b] = static_cast<int32_t>(min(md, 2147483647ll));
			cnt[base + b] = 0;
		}
		chunkOff += total;
		__syncthreads();  // scanTmp is reused by the next 256 buckets
	}
}

// Canonical order inside a unit: RANK = ascending packed record (as u64), i.e. by (uint32) dt = t_ref - t,
// then by the x | polarity | y word; POSITION = the ranks dealt out with a fixed stride (ebo_internal.h:
// order_stride -- consecutive records far apart in time, hence scattered in space: fewer same-word LDS atomics in
// the evaluation kernels).  It makes every result independent of the order the events
// arrived in (any permutation of a window's events gives the same bits) and identical to the host
// path, which sorts the same way.  Round 1 sorted every unit with a bitonic network in LDS (55
// compare-exchange stages with barriers: 59 % of the bucketing time).  The scatter is now STABLE --
// a unit's records arrive in time order -- and the canonical order follows from that order by a
// closed-form permutation: the records with dt >= 0 form a prefix A in descending dt, those with
// dt < 0 a suffix B (also descending as uint32), so ascending order is reverse(A) then reverse(B),
// and only records with EQUAL timestamps (a handful per unit) have to be ranked among themselves by
// their coordinate word.  One workgroup per unit; units above kSortMax stay in time order (the
// host path leaves those in time order too).
constexpr int kSortMax = 8192;

__global__ void __launch_bounds__(256) k_bucket_canon(const Unit* __restrict__ units, uint64_t* __restrict__ packed)
{
	extern __shared__ unsigned long long skey[];
	__shared__ int nNonNeg, unsorted;
	__shared__ uint32_t dealInv;  // rank r goes to position (r * dealInv) mod n: the strided deal of ebo_internal.h
	const Unit u = units[blockIdx.x];
	const int n = static_cast<int>(u.n_ev);
	if (n < 2 || n > kSortMax)
	{
		return;
	}
	uint64_t* p = packed + u.ev_off;
	if (threadIdx.x == 0)
	{
		nNonNeg = 0;
		unsorted = 0;
		dealInv = order_inverse(order_stride(static_cast<uint32_t>(n)), static_cast<uint32_t>(n));
	}
	__syncthreads();
	int mine = 0;
	for (int i = threadIdx.x; i < n; i += blockDim.x)
	{
		const unsigned long long k = p[i];
		skey[i] = k;
		mine += static_cast<int>(k >> 63) ^ 1;  // dt >= 0
	}
	atomicAdd(&nNonNeg, mine);
	__syncthreads();
	// the closed form needs the unit in time order (signed dt non-increasing); a window that was not
	// handed over time-ordered takes the bitonic network below instead
	// ... and runs of equal timestamps short: the closed form ranks a record inside its run by walking the
	// run (O(run) per record, O(run^2) per run) -- fine for the handful of coincidences of a microsecond
	// clock, a cliff for recordings with quantised stamps (a simulator's frame times, a millisecond driver:
	// a whole unit of 8192 events at ONE timestamp would be ~260 k serial LDS reads per thread).  In time
	// order equal stamps are adjacent, so a run longer than kRunMax shows as equal stamps kRunMax apart:
	// such a unit takes the bitonic network too (same result: the canonical order is unique).
	constexpr int kRunMax = 32;
	bool inversion = false;
	for (int i = threadIdx.x; i + 1 < n; i += blockDim.x)
	{
		inversion |= static_cast<int>(skey[i] >> 32) < static_cast<int>(skey[i + 1] >> 32);
		inversion |= i + kRunMax < n && static_cast<uint32_t>(skey[i] >> 32) == static_cast<uint32_t>(skey[i + kRunMax] >> 32);
	}
	if (inversion)
	{
		unsorted = 1;
	}
	__syncthreads();
	if (!unsorted)
	{
		const int m = nNonNeg;
		for (int i = threadIdx.x; i < n; i += blockDim.x)
		{
			const unsigned long long k = skey[i];
			const uint32_t dt = static_cast<uint32_t>(k >> 32);
			// the run of equal timestamps around i, [a, b)
			int a = i, b = i + 1, rank = 0;
			while (a > 0 && static_cast<uint32_t>(skey[a - 1] >> 32) == dt)
			{
				--a;
				rank += skey[a] <= k ? 1 : 0;  // before i: smaller or equal word comes first
			}
			while (b < n && static_cast<uint32_t>(skey[b] >> 32) == dt)
			{
				rank += skey[b] < k ? 1 : 0;   // after i: strictly smaller word comes first
				++b;
			}
			// reverse(A) ++ reverse(B): the run keeps its place in the reversed half, ordered by the word
			const int pos = (i < m) ? (m - b) + rank : m + (n - b) + rank;
			p[(static_cast<uint32_t>(pos) * dealInv) % static_cast<uint32_t>(n)] = k;
		}
		return;
	}
	int m2 = 1;
	while (m2 < n)
	{
		m2 <<= 1;
	}
	for (int i = n + threadIdx.x; i < m2; i += blockDim.x)
	{
		skey[i] = ~0ull;
	}
	__syncthreads();
	for (int k = 2; k <= m2; k <<= 1)
	{
		for (int j = k >> 1; j > 0; j >>= 1)
		{
			for (int i = threadIdx.x; i < m2; i += blockDim.x)
			{
				const int l = i ^ j;
				if (l > i)
				{
					const unsigned long long a = skey[i], b = skey[l];
					const bool up = (i & k) == 0;
					if ((a > b) == up)
					{
						skey[i] = b;
						skey[l] = a;
					}
				}
			}
			__syncthreads();
		}
	}
	for (int i = threadIdx.x; i < n; i += blockDim.x)
	{
		p[(static_cast<uint32_t>(i) * dealInv) % static_cast<uint32_t>(n)] = skey[i];
	}
}

// STABLE scatter: one wave per chunk (2048 events; 256 for small inputs) walks it in time order, 64 events per step.  The
// rank of an event inside its unit = the chunk's first rank in that unit (k_bucket_chunk_scan, kept
// in LDS as a running cursor) + the number of earlier events of the chunk in the same unit; inside a
// step the lanes of equal bucket are ranked by ballot (one round per distinct bucket of the step,
// the round's leader advances the cursor).  No global atomics, a deterministic order.
template <class Rec>
__global__ void __launch_bounds__(64) k_bucket_scatter(Rec raw, const unsigned long long* __restrict__ offsets, int wBase,
								 int P, const unsigned int* __restrict__ chunkBase, const Unit* __restrict__ units,
								 const long long* __restrict__ unitTref, const long long* __restrict__ winTref,
								 uint64_t* __restrict__ packed, int* __restrict__ flag, int chunk, EvalConsts c)
{
	extern __shared__ unsigned int cursor[];  // [P + 1]
	const int w = wBase + blockIdx.y;
	const unsigned long long e0 = offsets[w], e1 = offsets[w + 1];
	const unsigned long long begin = e0 + static_cast<unsigned long long>(blockIdx.x) * chunk;
	if (begin >= e1)
	{
		return;
	}
	const unsigned long long end = begin + chunk < e1 ? begin + chunk : e1;
	const size_t base = static_cast<size_t>(w) * (P + 1);
	const unsigned int* row = chunkBase + (static_cast<size_t>(w) * gridDim.x + blockIdx.x) * (P + 1);
	const int lane = threadIdx.x;
	for (int b = lane; b <= P; b += 64)
	{
		cursor[b] = row[b];
	}
	__syncthreads();
	const long long tw = winTref[w];
	const unsigned long long below = (lane == 0) ? 0ull : (~0ull >> (64 - lane));
	bool bad = false;
	for (unsigned long long e = begin; e < end; e += 64)
	{
		const bool have = e + lane < end;
		int x = 0, y = 0, pos = 0;
		long long t = 0;
		if (have)
		{
			raw.load(e + lane, w, x, y, pos, t);
		}
		const bool valid = have && !(Rec::kCheckRange && (x < kCoordMin || x > kCoordMax || y < kCoordMin || y > kCoordMax));
		const int b = valid ? bucket_of(x, y, c, P) : -1;
		// Every lane fetches its own bucket's cursor ONCE per step (one LDS gather; lanes of a bucket
		// read the same word), then the rounds are ballots only: the leader's bucket by v_readlane,
		// the rank by a population count, the cursor's new value written by the leader without
		// anybody waiting for it.  (The first form went through the LDS twice per ROUND -- a
		// ds_bpermute for the leader's bucket, a read-modify-write of the cursor and another
		// ds_bpermute to broadcast it -- and a step of 64 events of a 108-patch window has ~45
		// rounds: 227 us for one 15 k-event window, 0.3-0.4 ms for 12.8 M events.)
		const unsigned int mine = valid ? cursor[b] : 0u;
		unsigned int rank = 0;
		unsigned long long todo = __ballot(valid);
		while (todo)
		{
			const int leader = __ffsll(static_cast<long long>(todo)) - 1;
			const int b0 = __builtin_amdgcn_readlane(b, leader);
			const unsigned long long same = __ballot(b == b0);
			if (b == b0)
			{
				rank = mine + static_cast<unsigned int>(__popcll(same & below));
				if (lane == leader)
				{
					cursor[b0] = mine + static_cast<unsigned int>(__popcll(same));
				}
			}
			todo &= ~same;
		}
		if (valid)
		{
			const long long dt = unitTref[base + b] - t;
			const long long dtw = tw - t;
			if (dt < -2147483648ll || dt > 2147483647ll || dtw < -2147483648ll || dtw > 2147483647ll)
			{
				bad = true;  // the call fails; the slot keeps whatever it held
			}
			else
			{
				const uint32_t lo = (static_cast<uint32_t>(x) & 0x7FFFu) | (static_cast<uint32_t>(pos) << 15) |
									((static_cast<uint32_t>(y) & 0x7FFFu) << 16);
				packed[units[base + b].ev_off + rank] =
					static_cast<uint64_t>(lo) | (static_cast<uint64_t>(static_cast<uint32_t>(static_cast<int32_t>(dt))) << 32);
			}
		}
	}
	if (bad)
	{
		atomicOr(flag, 4);
	}
}
