// ebo_depth.inc — semi-dense depth from events by space sweep, on the device (include/ebo.h, "depth from events", rules
// M1-M9): every event of the resident windows is back-projected as a ray through the depth planes of a reference view
// and votes bilinearly, in exact fixed point, into the uint32 volume H[k][y][x]; the extraction keeps the pixels where
// rays meet.  Included inside ebo_kernels.hip's anonymous namespace, after ebo_rotation.inc.  tests/depth_ref.py
// restates the rules in numpy.  The rule functions (dsi_ray, dsi_uv, dsi_tap, dsi_weights) round every float64
// operation of M2-M4 on its own; tools/dsi_serial.cpp compiles them for the host behind EBO_DEPTH_RULES_ONLY.

struct DsiRay
{
	double a, b;        // M2's normalised pixel
	double d0, d1, d2;  // its ray in the reference frame
};
struct DsiTap
{
	int x0, y0;  // floor(u), floor(v): in [-1, w - 1] x [-1, h - 1]
	double al, be, ial, ibe;
};

// M2, per event
__device__ __forceinline__ void dsi_ray(const DsiConsts& k, const DsiPose& p, int x, int y, DsiRay& r)
{
	r.a = __ddiv_rn(__dsub_rn(static_cast<double>(x), k.cx), k.fx);
	r.b = __ddiv_rn(__dsub_rn(static_cast<double>(y), k.cy), k.fy);
	r.d0 = __dadd_rn(__dadd_rn(__dmul_rn(p.Rr[0], r.a), __dmul_rn(p.Rr[1], r.b)), p.Rr[2]);
	r.d1 = __dadd_rn(__dadd_rn(__dmul_rn(p.Rr[3], r.a), __dmul_rn(p.Rr[4], r.b)), p.Rr[5]);
	r.d2 = __dadd_rn(__dadd_rn(__dmul_rn(p.Rr[6], r.a), __dmul_rn(p.Rr[7], r.b)), p.Rr[8]);
}

// M3 up to (u, v); false: lam is not positive, no vote on this plane
__device__ __forceinline__ bool dsi_uv(const DsiConsts& k, const DsiPose& p, const DsiRay& r, double zk, double& u, double& v)
{
	const double lam = __ddiv_rn(__dsub_rn(zk, p.tr[2]), r.d2);
	if (!(lam > 0.0))
	{
		return false;
	}
	const double X = __dadd_rn(p.tr[0], __dmul_rn(lam, r.d0));
	const double Y = __dadd_rn(p.tr[1], __dmul_rn(lam, r.d1));
	u = __dadd_rn(__dmul_rn(k.fx, __ddiv_rn(X, zk)), k.cx);
	v = __dadd_rn(__dmul_rn(k.fy, __ddiv_rn(Y, zk)), k.cy);
	return true;
}

// M3's in-image test, in double before any conversion (a NaN fails it), and the fractions of M4
__device__ __forceinline__ bool dsi_tap(const DsiConsts& k, double u, double v, DsiTap& o)
{
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
	return true;
}

// M4: the four fixed-point votes, in the order (x0, y0), (x0+1, y0), (x0, y0+1), (x0+1, y0+1)
__device__ __forceinline__ void dsi_weights(const DsiTap& e, unsigned int (&q)[4])
{
	const double s = 1024.0;  // 2^10
	q[0] = static_cast<unsigned int>(rint(__dmul_rn(__dmul_rn(e.ial, e.ibe), s)));
	q[1] = static_cast<unsigned int>(rint(__dmul_rn(__dmul_rn(e.al, e.ibe), s)));
	q[2] = static_cast<unsigned int>(rint(__dmul_rn(__dmul_rn(e.ial, e.be), s)));
	q[3] = static_cast<unsigned int>(rint(__dmul_rn(__dmul_rn(e.al, e.be), s)));
}

#ifndef EBO_DEPTH_RULES_ONLY

constexpr int kDsiMargin = 1;
constexpr int kDsiWaves = kDsiBlock / 64;
constexpr int kDsiTilePx = 1024;  // a wave's tile: 4 KB of uint32, 16 KB a workgroup

// The tile of one (patch, plane): a plane maps the patch's rect by a homography, and where lam > 0 at the four corners
// it is positive on the whole rect, so every tap of the patch's events lies in the bounding box of the mapped corners
// plus one pixel; kDsiMargin more allows for the rounding of the map.  Clipped to the image.  tw = th = 0: no tile
// (a corner with no image, a box that is not finite or larger than kDsiTilePx): the taps go to H directly.  A tap
// outside whatever tile this gives goes to H directly too, so the tile decides speed only.
__device__ __forceinline__ void dsi_tile(const DsiConsts& k, const DsiPose& p, const Unit& u, double zk, int& tx0, int& ty0, int& tw,
										 int& th)
{
	tx0 = ty0 = tw = th = 0;
	double ulo = 0.0, uhi = 0.0, vlo = 0.0, vhi = 0.0;
#pragma unroll
	for (int c = 0; c < 4; ++c)
	{
		DsiRay r;
		dsi_ray(k, p, u.rx + ((c & 1) ? u.rw - 1 : 0), u.ry + ((c >> 1) ? u.rh - 1 : 0), r);
		double cu, cv;
		if (!dsi_uv(k, p, r, zk, cu, cv))
		{
			return;
		}
		ulo = c ? fmin(ulo, cu) : cu;
		uhi = c ? fmax(uhi, cu) : cu;
		vlo = c ? fmin(vlo, cv) : cv;
		vhi = c ? fmax(vhi, cv) : cv;
		if (!(cu > -1e6 && cu < 1e6 && cv > -1e6 && cv < 1e6))  // a NaN fails it
		{
			return;
		}
	}
	const int x0 = max(static_cast<int>(floor(ulo)) - kDsiMargin, 0), x1 = min(static_cast<int>(floor(uhi)) + 1 + kDsiMargin, k.w - 1);
	const int y0 = max(static_cast<int>(floor(vlo)) - kDsiMargin, 0), y1 = min(static_cast<int>(floor(vhi)) + 1 + kDsiMargin, k.h - 1);
	if (x1 < x0 || y1 < y0 || (x1 - x0 + 1) * (y1 - y0 + 1) > kDsiTilePx)
	{
		return;
	}
	tx0 = x0;
	ty0 = y0;
	tw = x1 - x0 + 1;
	th = y1 - y0 + 1;
}

// The vote (M2-M4).  Grid (patch, chunk slot, chunk of planes): a workgroup takes one unit's events through k.planes
// planes, four planes at a time, one per wave: wave v walks the planes k0 + v, k0 + v + 4, ..., its lanes dealing the
// unit's events by 64.  Per plane the wave's tile (dsi_tile, a quarter of sTile) is accumulated in LDS and its non-zero
// pixels are added to H[plane] once; with k.tile == 0 (the A/B build's plain form) or no tile every tap is a global
// atomic.  A wave touches no other wave's quarter; the two barriers of a round order a wave's own LDS adds against its
// own reads, and every wave reaches them (a wave past its last plane does no work in between).  H is an integer sum:
// every split gives the same bits.  Every H access sits behind the tap's own in-image test; sTile is indexed behind
// the tile's own.
__global__ void __launch_bounds__(kDsiBlock) k_dsi_vote(const uint64_t* __restrict__ events, const Unit* __restrict__ units, DsiWindows L,
														 DsiConsts k, const DsiPose* __restrict__ poses, const double* __restrict__ zt,
														 unsigned int* __restrict__ H)
{
	__shared__ unsigned int sTile[kDsiWaves * kDsiTilePx];
	const int win = L.win[blockIdx.y];
	const Unit u = units[static_cast<size_t>(win) * k.upw + blockIdx.x];
	if (u.n_ev == 0)
	{
		return;
	}
	const DsiPose p = poses[win];
	const size_t np = static_cast<size_t>(k.w) * k.h;
	const int k0 = blockIdx.z * k.planes, k1 = min(k0 + k.planes, k.nz);
	const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
	unsigned int* __restrict__ tile = sTile + wave * kDsiTilePx;
	if (k.tile)
	{
		for (int i = lane; i < kDsiTilePx; i += 64)
		{
			tile[i] = 0u;
		}
	}
	const uint64_t* ev = events + u.ev_off;
	for (int kr = k0; kr < k1; kr += kDsiWaves)
	{
		const int kp = kr + wave;
		const bool live = kp < k1;
		const double zk = zt[live ? kp : k0];
		unsigned int* __restrict__ Hk = H + static_cast<size_t>(live ? kp : k0) * np;
		int tx0 = 0, ty0 = 0, tw = 0, th = 0;
		if (k.tile && live)
		{
			dsi_tile(k, p, u, zk, tx0, ty0, tw, th);
		}
		__syncthreads();  // the wave's tile is zero: by the loop above, or by its previous plane's flush
		for (uint32_t e = lane; live && e < u.n_ev; e += 64)
		{
			int x, y, pos, dt;
			unpack(ev[e], x, y, pos, dt);
			DsiRay r;
			dsi_ray(k, p, x, y, r);
			double uu, vv;
			DsiTap t;
			if (!dsi_uv(k, p, r, zk, uu, vv) || !dsi_tap(k, uu, vv, t))
			{
				continue;
			}
			unsigned int q[4];
			dsi_weights(t, q);
#pragma unroll
			for (int i = 0; i < 4; ++i)
			{
				const int px = t.x0 + (i & 1), py = t.y0 + (i >> 1);
				if (q[i] == 0u || px < 0 || px >= k.w || py < 0 || py >= k.h)
				{
					continue;
				}
				const int lx = px - tx0, ly = py - ty0;
				if (lx >= 0 && lx < tw && ly >= 0 && ly < th)
				{
					atomicAdd(&tile[ly * tw + lx], q[i]);
				}
				else
				{
					atomicAdd(&Hk[static_cast<size_t>(py) * k.w + px], q[i]);
				}
			}
		}
		__syncthreads();
		const int tn = tw * th;  // 0 for a wave that is not live
		for (int i = lane; i < tn; i += 64)
		{
			const unsigned int v = tile[i];
			if (v)
			{
				tile[i] = 0u;
				const int px = tx0 + i % tw, py = ty0 + i / tw;
				atomicAdd(&Hk[static_cast<size_t>(py) * k.w + px], v);
			}
		}
	}
}

// M5, one lane per pixel: the planes' coalesced rows of H; a later plane wins only when strictly larger
__global__ void __launch_bounds__(kDsiBlock) k_dsi_argmax(DsiConsts k, const unsigned int* __restrict__ H, unsigned int* __restrict__ conf,
														   int* __restrict__ kbest)
{
	const int p = blockIdx.x * kDsiBlock + threadIdx.x, np = k.w * k.h;
	if (p >= np)
	{
		return;
	}
	unsigned int c = 0u;
	int kb = 0;
	for (int kp = 0; kp < k.nz; ++kp)
	{
		const unsigned int v = H[static_cast<size_t>(kp) * np + p];
		if (v > c)
		{
			c = v;
			kb = kp;
		}
	}
	conf[p] = c;
	kbest[p] = kb;
}

// M6, one lane per pixel: the box sum of c and the test in int64
__global__ void __launch_bounds__(kDsiBlock) k_dsi_keep(DsiConsts k, int r, long long off, const unsigned int* __restrict__ conf,
														 unsigned char* __restrict__ keep)
{
	const int p = blockIdx.x * kDsiBlock + threadIdx.x, np = k.w * k.h;
	if (p >= np)
	{
		return;
	}
	const int x = p % k.w, y = p / k.w;
	long long S = 0, cnt = 0;
	for (int yy = max(y - r, 0); yy <= min(y + r, k.h - 1); ++yy)
	{
		for (int xx = max(x - r, 0); xx <= min(x + r, k.w - 1); ++xx)
		{
			S += static_cast<long long>(conf[yy * k.w + xx]);
			cnt += 1;
		}
	}
	const long long c = static_cast<long long>(conf[p]);
	keep[p] = (c > 0 && c * cnt > S + off * cnt) ? 1 : 0;
}

// M7 and M8's maps, one lane per pixel.  The lower median of n small integers is the smallest value v with at least
// (n - 1) / 2 + 1 of them <= v: a bisection over the plane indices, each step one pass over the box, with no list to
// keep -- no per-lane array in scratch or LDS.
__global__ void __launch_bounds__(kDsiBlock) k_dsi_median(DsiConsts k, int m, const int* __restrict__ kbest,
														   const unsigned char* __restrict__ keep, const double* __restrict__ zt,
														   int* __restrict__ index, double* __restrict__ depth)
{
	const int p = blockIdx.x * kDsiBlock + threadIdx.x, np = k.w * k.h;
	if (p >= np)
	{
		return;
	}
	if (!keep[p])
	{
		index[p] = -1;
		depth[p] = 0.0;
		return;
	}
	int best = kbest[p];
	if (m > 0)
	{
		const int x = p % k.w, y = p / k.w;
		const int xa = max(x - m, 0), xb = min(x + m, k.w - 1), ya = max(y - m, 0), yb = min(y + m, k.h - 1);
		int n = 0;
		for (int yy = ya; yy <= yb; ++yy)
		{
			for (int xx = xa; xx <= xb; ++xx)
			{
				n += keep[yy * k.w + xx];
			}
		}
		const int need = (n - 1) / 2 + 1;
		int lo = 0, hi = k.nz - 1;
		while (lo < hi)
		{
			const int mid = (lo + hi) / 2;
			int le = 0;
			for (int yy = ya; yy <= yb; ++yy)
			{
				for (int xx = xa; xx <= xb; ++xx)
				{
					const int q = yy * k.w + xx;
					le += (keep[q] && kbest[q] <= mid) ? 1 : 0;
				}
			}
			if (le >= need)
			{
				hi = mid;
			}
			else
			{
				lo = mid + 1;
			}
		}
		best = lo;
	}
	index[p] = best;
	depth[p] = zt[best];
}

// a lane's rank among the workgroup's kept pixels, in pixel order, and the workgroup's count; sWave: kDsiBlock / 64 ints
__device__ __forceinline__ int dsi_block_rank(bool kept, int* sWave, int& total)
{
	const unsigned long long b = __ballot(kept);
	const int lane = threadIdx.x & 63, wave = threadIdx.x / 64;
	const int rank = __popcll(b & ((1ull << lane) - 1ull));
	if (lane == 0)
	{
		sWave[wave] = __popcll(b);
	}
	__syncthreads();
	int before = 0;
	total = 0;
#pragma unroll
	for (int i = 0; i < kDsiBlock / 64; ++i)
	{
		before += i < wave ? sWave[i] : 0;
		total += sWave[i];
	}
	return before + rank;
}

// M8's point list, step 1: kept pixels per workgroup of kDsiBlock consecutive pixels
__global__ void __launch_bounds__(kDsiBlock) k_dsi_count(DsiConsts k, const int* __restrict__ index, int* __restrict__ blockCount)
{
	__shared__ int sWave[kDsiBlock / 64];
	const int p = blockIdx.x * kDsiBlock + threadIdx.x, np = k.w * k.h;
	int total;
	dsi_block_rank(p < np && index[p] >= 0, sWave, total);
	if (threadIdx.x == 0)
	{
		blockCount[blockIdx.x] = total;
	}
}

// step 2, one workgroup: blockCount[0 .. nb) -> its exclusive scan in place, the total in blockCount[nb].  Lane t takes
// the ceil(nb / kDsiBlock) consecutive entries from t * that; the lanes' sums are scanned in LDS.
__global__ void __launch_bounds__(kDsiBlock) k_dsi_scan(int nb, int* __restrict__ blockCount)
{
	__shared__ int sSum[kDsiBlock];
	const int per = (nb + kDsiBlock - 1) / kDsiBlock;
	const int a = min(static_cast<int>(threadIdx.x) * per, nb), b = min(a + per, nb);
	int s = 0;
	for (int i = a; i < b; ++i)
	{
		s += blockCount[i];
	}
	sSum[threadIdx.x] = s;
	__syncthreads();
	for (int d = 1; d < kDsiBlock; d *= 2)
	{
		const int v = static_cast<int>(threadIdx.x) >= d ? sSum[threadIdx.x - d] : 0;
		__syncthreads();
		sSum[threadIdx.x] += v;
		__syncthreads();
	}
	int run = sSum[threadIdx.x] - s;  // exclusive
	for (int i = a; i < b; ++i)
	{
		const int c = blockCount[i];
		blockCount[i] = run;
		run += c;
	}
	if (threadIdx.x == kDsiBlock - 1)
	{
		blockCount[nb] = sSum[kDsiBlock - 1];
	}
}

// step 3: the kept pixels' points (a * z, b * z, z), the first max_points of them in row-major pixel order
__global__ void __launch_bounds__(kDsiBlock) k_dsi_points(DsiConsts k, const int* __restrict__ index, const double* __restrict__ zt,
														   const int* __restrict__ blockOff, int max_points, double* __restrict__ points)
{
	__shared__ int sWave[kDsiBlock / 64];
	const int p = blockIdx.x * kDsiBlock + threadIdx.x, np = k.w * k.h;
	const bool kept = p < np && index[p] >= 0;
	int total;
	const int at = blockOff[blockIdx.x] + dsi_block_rank(kept, sWave, total);
	if (kept && at < max_points)
	{
		const double z = zt[index[p]];
		const double a = __ddiv_rn(__dsub_rn(static_cast<double>(p % k.w), k.cx), k.fx);
		const double b = __ddiv_rn(__dsub_rn(static_cast<double>(p / k.w), k.cy), k.fy);
		points[3 * static_cast<size_t>(at)] = __dmul_rn(a, z);
		points[3 * static_cast<size_t>(at) + 1] = __dmul_rn(b, z);
		points[3 * static_cast<size_t>(at) + 2] = z;
	}
}

#endif  // EBO_DEPTH_RULES_ONLY
