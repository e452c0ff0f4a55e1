// ebo_frontend.inc — the image front end of FeatureDetector::newImage on the device (include/ebo.h,
// "image front end"): log-image gradients, Harris corners (goodFeaturesToTrack) and pyramidal LK
// (calcOpticalFlowPyrLK).  Included inside ebo_kernels.hip's anonymous namespace; the rules every
// kernel follows are written out in ebo.h and restated on the CPU by tests/frontend_ref.py.
//   k_fe_gradients   2-D tile, uint8 image + 1-pixel halo read once into LDS as log values, separable
//                    Sobel in double (row pass, column pass) in the header's association.
//   k_fe_harris      2-D tile, image + halo in LDS, integer moments for the tile + box halo, box sums,
//                    response R (double), per-workgroup masked maximum.
//   k_fe_candidates  threshold + 3x3 non-maximum suppression + compaction (R, raster index) by atomics;
//                    the order of the list is fixed afterwards by the sort.
//   k_fe_select      one workgroup: bitonic sort of the list in LDS (or of a globally sorted list beyond
//                    kFeLdsSort entries: k_fe_bitonic_step), then the greedy minimum-distance pick in one wave.
//   k_fe_pyrdown / k_fe_scharr   one level of the pyramid / its int16 Scharr derivatives.
//   k_fe_lk          one wave per point, all levels in one launch; window pixels strided over the lanes,
//                    sums exact in integers (reduced as integer-valued doubles), then float32 as OpenCV.

__device__ __forceinline__ int fe_refl(int i, int n)
{
	// BORDER_REFLECT_101 for any i (cv::borderInterpolate)
	if (n == 1)
	{
		return 0;
	}
	const int period = 2 * n - 2;
	i = i < 0 ? -i : i;
	i %= period;
	return i < n ? i : period - i;
}

constexpr int kFeTileW = 32, kFeTileH = 8;

__global__ void __launch_bounds__(kFeTileW * kFeTileH) k_fe_gradients(const uint8_t* __restrict__ img,
																		  const double* __restrict__ lut, int w, int h,
																		  double* __restrict__ gx, double* __restrict__ gy)
{
	__shared__ double sL[kFeTileH + 2][kFeTileW + 2];
	__shared__ double sR[kFeTileH + 2][kFeTileW];  // row pass of grad_x
	__shared__ double sS[kFeTileH + 2][kFeTileW];  // row pass of grad_y
	const int x0 = blockIdx.x * kFeTileW, y0 = blockIdx.y * kFeTileH;
	const int tid = threadIdx.y * kFeTileW + threadIdx.x;
	for (int k = tid; k < (kFeTileH + 2) * (kFeTileW + 2); k += kFeTileW * kFeTileH)
	{
		const int j = k / (kFeTileW + 2), i = k % (kFeTileW + 2);
		const int ry = fe_refl(y0 - 1 + j, h), rx = fe_refl(x0 - 1 + i, w);
		sL[j][i] = lut[img[static_cast<size_t>(ry) * w + rx]];
	}
	__syncthreads();
	for (int k = tid; k < (kFeTileH + 2) * kFeTileW; k += kFeTileW * kFeTileH)
	{
		const int j = k / kFeTileW, i = k % kFeTileW;
		sR[j][i] = __dsub_rn(sL[j][i + 2], sL[j][i]);
		sS[j][i] = __dadd_rn(__dadd_rn(sL[j][i], __dmul_rn(2.0, sL[j][i + 1])), sL[j][i + 2]);
	}
	__syncthreads();
	const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
	if (x >= w || y >= h)
	{
		return;
	}
	const int i = threadIdx.x, j = threadIdx.y;
	const size_t o = static_cast<size_t>(y) * w + x;
	gx[o] = __dadd_rn(__dadd_rn(sR[j][i], __dmul_rn(2.0, sR[j + 1][i])), sR[j + 2][i]);
	gy[o] = __dsub_rn(sS[j + 2][i], sS[j][i]);
}

constexpr int kFeHarrisT = 16;                  // output tile kFeHarrisT x kFeHarrisT
constexpr int kFeMaxBlock = 7;                  // block_size limit (ebo.h)
constexpr int kFeHalo = kFeMaxBlock / 2 + 1;    // image halo: box half-width + the Sobel's 1
constexpr int kFeImgT = kFeHarrisT + 2 * kFeHalo;
constexpr int kFeMomT = kFeHarrisT + kFeMaxBlock - 1;

__global__ void __launch_bounds__(kFeHarrisT * kFeHarrisT) k_fe_harris(const uint8_t* __restrict__ img,
																	   const uint8_t* __restrict__ mask, int w, int h,
																	   int bs, double k, double* __restrict__ resp,
																	   double* __restrict__ blockMax)
{
	__shared__ int sImg[kFeImgT][kFeImgT];
	__shared__ int sM[3][kFeMomT][kFeMomT];
	__shared__ double sMax[kFeHarrisT * kFeHarrisT / 64];
	const int x0 = blockIdx.x * kFeHarrisT, y0 = blockIdx.y * kFeHarrisT;
	const int tid = threadIdx.y * kFeHarrisT + threadIdx.x;
	const int nt = kFeHarrisT * kFeHarrisT;
	// real pixels [x0 - kFeHalo, x0 + T + kFeHalo) of the image, stored at their real coordinates (clamped)
	const int ix0 = x0 - kFeHalo, iy0 = y0 - kFeHalo;
	for (int q = tid; q < kFeImgT * kFeImgT; q += nt)
	{
		const int j = q / kFeImgT, i = q % kFeImgT;
		const int ry = min(max(iy0 + j, 0), h - 1), rx = min(max(ix0 + i, 0), w - 1);
		sImg[j][i] = img[static_cast<size_t>(ry) * w + rx];
	}
	__syncthreads();
	// a real pixel read from the staged tile; the clamp keeps every index inside it
	auto at = [&](int ry, int rx) {
		const int j = min(max(ry - iy0, 0), kFeImgT - 1), i = min(max(rx - ix0, 0), kFeImgT - 1);
		return sImg[j][i];
	};
	const int lo = bs / 2;
	const int mt = kFeHarrisT + bs - 1;
	for (int q = tid; q < mt * mt; q += nt)
	{
		const int j = q / mt, i = q % mt;
		const int ry = fe_refl(y0 - lo + j, h), rx = fe_refl(x0 - lo + i, w);
		const int ym = fe_refl(ry - 1, h), yp = fe_refl(ry + 1, h), xm = fe_refl(rx - 1, w), xp = fe_refl(rx + 1, w);
		const int a = at(ym, xm), b = at(ym, rx), c = at(ym, xp);
		const int d = at(ry, xm), f = at(ry, xp);
		const int g = at(yp, xm), hh = at(yp, rx), ii = at(yp, xp);
		const int dx = (c + 2 * f + ii) - (a + 2 * d + g);
		const int dy = (g + 2 * hh + ii) - (a + 2 * b + c);
		sM[0][j][i] = dx * dx;
		sM[1][j][i] = dx * dy;
		sM[2][j][i] = dy * dy;
	}
	__syncthreads();
	const int x = x0 + threadIdx.x, y = y0 + threadIdx.y;
	double mine = -INFINITY;
	if (x < w && y < h)
	{
		int A = 0, B = 0, C = 0;
		for (int j = 0; j < bs; ++j)
		{
			for (int i = 0; i < bs; ++i)
			{
				A += sM[0][threadIdx.y + j][threadIdx.x + i];
				B += sM[1][threadIdx.y + j][threadIdx.x + i];
				C += sM[2][threadIdx.y + j][threadIdx.x + i];
			}
		}
		const long long det = static_cast<long long>(A) * C - static_cast<long long>(B) * B;
		const double tr = static_cast<double>(static_cast<long long>(A) + C);
		const double R = __dsub_rn(static_cast<double>(det), __dmul_rn(k, __dmul_rn(tr, tr)));
		const size_t o = static_cast<size_t>(y) * w + x;
		resp[o] = R;
		if (!mask || mask[o])
		{
			mine = R;
		}
	}
	for (int off = 32; off > 0; off >>= 1)
	{
		mine = fmax(mine, __shfl_xor(mine, off));
	}
	if ((tid & 63) == 0)
	{
		sMax[tid >> 6] = mine;
	}
	__syncthreads();
	if (tid == 0)
	{
		double m = sMax[0];
		for (int q = 1; q < nt / 64; ++q)
		{
			m = fmax(m, sMax[q]);
		}
		blockMax[blockIdx.y * gridDim.x + blockIdx.x] = m;
	}
}

// threshold, 3x3 NMS on the thresholded map, compaction of (R, raster index)
__global__ void __launch_bounds__(256) k_fe_candidates(const double* __restrict__ resp, const uint8_t* __restrict__ mask,
													   int w, int h, double quality, const double* __restrict__ blockMax,
													   int nBlocks, double* __restrict__ candR, int* __restrict__ candI,
													   int* __restrict__ count)
{
	__shared__ double sRed[4];
	double m = -INFINITY;
	for (int q = threadIdx.x; q < nBlocks; q += blockDim.x)
	{
		m = fmax(m, blockMax[q]);
	}
	for (int off = 32; off > 0; off >>= 1)
	{
		m = fmax(m, __shfl_xor(m, off));
	}
	if ((threadIdx.x & 63) == 0)
	{
		sRed[threadIdx.x >> 6] = m;
	}
	__syncthreads();
	m = fmax(fmax(sRed[0], sRed[1]), fmax(sRed[2], sRed[3]));
	if (m == -INFINITY)
	{
		m = 0.0;  // empty mask: minMaxLoc reports 0
	}
	const double thr = __dmul_rn(quality, m);
	const int p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= w * h)
	{
		return;
	}
	const int x = p % w, y = p / w;
	if (x < 1 || x > w - 2 || y < 1 || y > h - 2 || (mask && !mask[p]))
	{
		return;
	}
	const double r = resp[p];
	const double t = r > thr ? r : 0.0;
	if (t == 0.0)
	{
		return;
	}
	double mx = t;
	for (int j = -1; j <= 1; ++j)
	{
		for (int i = -1; i <= 1; ++i)
		{
			const double rn = resp[p + j * w + i];
			mx = fmax(mx, rn > thr ? rn : 0.0);
		}
	}
	if (t != mx)
	{
		return;
	}
	const int slot = atomicAdd(count, 1);
	candR[slot] = r;
	candI[slot] = p;
}

// the order of ebo.h: R descending, ties by the larger raster index
__device__ __forceinline__ bool fe_before(double ra, int ia, double rb, int ib)
{
	return ra > rb || (ra == rb && ia > ib);
}

// the tail [n, cap) of the candidate lists: entries that sort after every candidate
__global__ void __launch_bounds__(256) k_fe_pad(double* __restrict__ r, int* __restrict__ idx, const int* __restrict__ count,
												int cap)
{
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	if (t < cap && t >= *count)
	{
		r[t] = -INFINITY;
		idx[t] = -1;
	}
}

// one compare-exchange stage of a bitonic sort over the whole (power-of-two) list in global memory
__global__ void __launch_bounds__(256) k_fe_bitonic_step(double* __restrict__ r, int* __restrict__ idx, int n, int kk,
														 int jj)
{
	const int t = blockIdx.x * blockDim.x + threadIdx.x;
	const int u = t ^ jj;
	if (t >= n || u <= t)
	{
		return;
	}
	const bool up = (t & kk) == 0;
	const double rt = r[t], ru = r[u];
	const int it = idx[t], iu = idx[u];
	if (up ? fe_before(ru, iu, rt, it) : fe_before(rt, it, ru, iu))
	{
		r[t] = ru;
		r[u] = rt;
		idx[t] = iu;
		idx[u] = it;
	}
}

constexpr int kFeLdsSort = kFeSortLds;
constexpr int kFeMaxCorners = kFeMaxCornersLds;  // accepted corners kept in LDS by the greedy pick

// n candidates (sorted == 0: unsorted, n <= kFeLdsSort; sorted == 1: candR / candI already in order) ->
// corners [*nOut][2].  One workgroup of 1024 lanes; the greedy pick runs in wave 0.
__global__ void __launch_bounds__(1024) k_fe_select(const double* __restrict__ candR, const int* __restrict__ candI,
													 const int* __restrict__ count, int sorted, int w, int maxCorners,
													 double minDist, float* __restrict__ corners, int* __restrict__ nOut)
{
	__shared__ double sR[kFeLdsSort];
	__shared__ int sI[kFeLdsSort];
	__shared__ unsigned int sAcc[kFeMaxCorners];
	const int n = *count;
	const int tid = threadIdx.x;
	if (!sorted)
	{
		int N = 1;
		while (N < n)
		{
			N <<= 1;
		}
		for (int t = tid; t < N; t += blockDim.x)
		{
			sR[t] = t < n ? candR[t] : -INFINITY;
			sI[t] = t < n ? candI[t] : -1;
		}
		__syncthreads();
		for (int kk = 2; kk <= N; kk <<= 1)
		{
			for (int jj = kk >> 1; jj > 0; jj >>= 1)
			{
				for (int t = tid; t < N; t += blockDim.x)
				{
					const int u = t ^ jj;
					if (u > t)
					{
						const bool up = (t & kk) == 0;
						const double rt = sR[t], ru = sR[u];
						const int it = sI[t], iu = sI[u];
						if (up ? fe_before(ru, iu, rt, it) : fe_before(rt, it, ru, iu))
						{
							sR[t] = ru;
							sR[u] = rt;
							sI[t] = iu;
							sI[u] = it;
						}
					}
				}
				__syncthreads();
			}
		}
	}
	if (tid >= 64)
	{
		return;
	}
	// greedy pick, wave 0: 64 candidates at a time are checked against the corners accepted so far, then the
	// survivors are taken in order, each removing the later survivors it is too close to
	const double md2 = __dmul_rn(minDist, minDist);
	const bool check = md2 > 1.0;  // distinct pixels are >= 1 apart
	int nAcc = 0;
	for (int base = 0; base < n && nAcc < maxCorners; base += 64)
	{
		const int c = base + tid;
		const int pi = c < n ? (sorted ? candI[c] : sI[c]) : 0;
		const int cx = pi % w, cy = pi / w;
		bool ok = c < n;
		if (ok && check)
		{
			for (int a = 0; a < nAcc; ++a)
			{
				const unsigned int pa = sAcc[a];
				const int dx = cx - static_cast<int>(pa & 0xffffu), dy = cy - static_cast<int>(pa >> 16);
				if (static_cast<double>(dx * dx + dy * dy) < md2)
				{
					ok = false;
					break;
				}
			}
		}
		unsigned long long live = __ballot(ok);
		while (live && nAcc < maxCorners)
		{
			const int s = __ffsll(static_cast<long long>(live)) - 1;
			const int sx = __shfl(cx, s), sy = __shfl(cy, s);
			if (tid == 0)
			{
				sAcc[nAcc] = static_cast<unsigned int>(sx) | (static_cast<unsigned int>(sy) << 16);
				corners[2 * nAcc] = static_cast<float>(sx);
				corners[2 * nAcc + 1] = static_cast<float>(sy);
			}
			++nAcc;
			if (ok && tid > s && check)
			{
				const int dx = cx - sx, dy = cy - sy;
				if (static_cast<double>(dx * dx + dy * dy) < md2)
				{
					ok = false;
				}
			}
			live = __ballot(ok && tid > s);
		}
		__builtin_amdgcn_wave_barrier();  // sAcc written by lane 0 is read by every lane next round
		__builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
	}
	if (tid == 0)
	{
		*nOut = nAcc;
	}
}

// ---- pyramidal LK -----------------------------------------------------------------------------
constexpr int kFeLkPerLane = 16;   // window pixels per lane: win_w * win_h <= 64 * 16 (kFeMaxWindow)

// dst level (dw x dh) = pyrDown(src level): [1 4 6 4 1]^2, refl(), (sum + 128) >> 8
__global__ void __launch_bounds__(256) k_fe_pyrdown(const uint8_t* __restrict__ src, int sw, int sh,
													uint8_t* __restrict__ dst, int dw, int dh)
{
	const int p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= dw * dh)
	{
		return;
	}
	const int x = p % dw, y = p / dw;
	const int kw[5] = {1, 4, 6, 4, 1};
	int sum = 0;
#pragma unroll
	for (int j = 0; j < 5; ++j)
	{
		const uint8_t* row = src + static_cast<size_t>(fe_refl(2 * y + j - 2, sh)) * sw;
		int rs = 0;
#pragma unroll
		for (int i = 0; i < 5; ++i)
		{
			rs += kw[i] * row[fe_refl(2 * x + i - 2, sw)];
		}
		sum += kw[j] * rs;
	}
	dst[p] = static_cast<uint8_t>((sum + 128) >> 8);
}

// calcSharrDeriv of one level: (Ix, Iy) int16 per pixel, refl()
__global__ void __launch_bounds__(256) k_fe_scharr(const uint8_t* __restrict__ img, int w, int h,
												   short2* __restrict__ der)
{
	const int p = blockIdx.x * blockDim.x + threadIdx.x;
	if (p >= w * h)
	{
		return;
	}
	const int x = p % w, y = p / w;
	const uint8_t* r0 = img + static_cast<size_t>(fe_refl(y - 1, h)) * w;
	const uint8_t* r1 = img + static_cast<size_t>(y) * w;
	const uint8_t* r2 = img + static_cast<size_t>(fe_refl(y + 1, h)) * w;
	int v0[3], v1[3];
#pragma unroll
	for (int i = 0; i < 3; ++i)
	{
		const int xx = fe_refl(x + i - 1, w);
		v0[i] = 3 * (r0[xx] + r2[xx]) + 10 * r1[xx];
		v1[i] = r2[xx] - r0[xx];
	}
	der[p] = make_short2(static_cast<short>(v0[2] - v0[0]), static_cast<short>(3 * (v1[0] + v1[2]) + 10 * v1[1]));
}

__device__ __forceinline__ double fe_wave_sum(double v)
{
	for (int off = 32; off > 0; off >>= 1)
	{
		v += __shfl_xor(v, off);
	}
	return v;
}

__device__ __forceinline__ void fe_weights(float a, float b, int& w00, int& w01, int& w10, int& w11)
{
	w00 = static_cast<int>(rintf(__fmul_rn(__fmul_rn(__fsub_rn(1.f, a), __fsub_rn(1.f, b)), 16384.f)));
	w01 = static_cast<int>(rintf(__fmul_rn(__fmul_rn(a, __fsub_rn(1.f, b)), 16384.f)));
	w10 = static_cast<int>(rintf(__fmul_rn(__fmul_rn(__fsub_rn(1.f, a), b), 16384.f)));
	w11 = 16384 - w00 - w01 - w10;
}

// image sample at (x, y) .. (x+1, y+1), -win <= x, x+1 < w + win: refl() reads, 5 fractional bits kept
__device__ __forceinline__ int fe_sample(const uint8_t* __restrict__ im, int w, int h, int x, int y, int w00, int w01,
										 int w10, int w11)
{
	const int x0 = fe_refl(x, w), x1 = fe_refl(x + 1, w);
	const uint8_t* r0 = im + static_cast<size_t>(fe_refl(y, h)) * w;
	const uint8_t* r1 = im + static_cast<size_t>(fe_refl(y + 1, h)) * w;
	return (r0[x0] * w00 + r0[x1] * w01 + r1[x0] * w10 + r1[x1] * w11 + 256) >> 9;
}

// one wave per point; levels from the top (nLevels - 1) down to 0
__global__ void __launch_bounds__(256) k_fe_lk(const char* __restrict__ prevPyr, const char* __restrict__ nextPyr,
											   const FeLevel* __restrict__ lv, int nLevels, int n,
											   const float* __restrict__ prevXY, float* __restrict__ nextXY,
											   uint8_t* __restrict__ status, float* __restrict__ err, int winW, int winH,
											   int maxCount, double eps2, float minEigThr)
{
	const int lane = threadIdx.x & 63;
	const int pt = blockIdx.x * (blockDim.x >> 6) + (threadIdx.x >> 6);
	if (pt >= n)
	{
		return;
	}
	const int area = winW * winH;
	int wxy[kFeLkPerLane];  // window offsets of this lane's pixels, x | y << 16
#pragma unroll
	for (int q = 0; q < kFeLkPerLane; ++q)
	{
		const int idx = lane + 64 * q;
		wxy[q] = idx < area ? (idx % winW) | ((idx / winW) << 16) : -1;
	}
	const float hx = __fmul_rn(static_cast<float>(winW - 1), 0.5f), hy = __fmul_rn(static_cast<float>(winH - 1), 0.5f);
	const float px0 = prevXY[2 * pt], py0 = prevXY[2 * pt + 1];
	bool ok = true;
	float resX = 0.f, resY = 0.f;
	const float FLT_SCALE = 1.f / (1 << 20);
	for (int level = nLevels - 1; level >= 0; --level)
	{
		const int w = lv[level].w, h = lv[level].h;
		const uint8_t* I = reinterpret_cast<const uint8_t*>(prevPyr + lv[level].img);
		const uint8_t* J = reinterpret_cast<const uint8_t*>(nextPyr + lv[level].img);
		const short2* dI = reinterpret_cast<const short2*>(prevPyr + lv[level].der);
		const float sc = 1.f / static_cast<float>(1 << level);
		float prevX = __fmul_rn(px0, sc), prevY = __fmul_rn(py0, sc);
		if (level == nLevels - 1)
		{
			resX = prevX;
			resY = prevY;
		}
		else
		{
			resX = __fmul_rn(resX, 2.f);
			resY = __fmul_rn(resY, 2.f);
		}
		prevX = __fsub_rn(prevX, hx);
		prevY = __fsub_rn(prevY, hy);
		const int ipx = static_cast<int>(floorf(prevX)), ipy = static_cast<int>(floorf(prevY));
		if (ipx < -winW || ipx >= w || ipy < -winH || ipy >= h)
		{
			if (level == 0)
			{
				ok = false;
			}
			continue;
		}
		int w00, w01, w10, w11;
		fe_weights(__fsub_rn(prevX, static_cast<float>(ipx)), __fsub_rn(prevY, static_cast<float>(ipy)), w00, w01, w10,
				   w11);
		int ival[kFeLkPerLane], ixv[kFeLkPerLane], iyv[kFeLkPerLane];
		int a11 = 0, a12 = 0, a22 = 0;
#pragma unroll
		for (int q = 0; q < kFeLkPerLane; ++q)
		{
			ival[q] = 0;
			ixv[q] = 0;
			iyv[q] = 0;
			if (wxy[q] >= 0)
			{
				const int x = ipx + (wxy[q] & 0xffff), y = ipy + (wxy[q] >> 16);
				ival[q] = fe_sample(I, w, h, x, y, w00, w01, w10, w11);
				// derivatives read 0 outside the level
				short2 d00 = make_short2(0, 0), d01 = d00, d10 = d00, d11 = d00;
				const bool c0 = x >= 0 && x < w, c1 = x + 1 >= 0 && x + 1 < w;
				const bool r0 = y >= 0 && y < h, r1 = y + 1 >= 0 && y + 1 < h;
				if (r0 && c0) d00 = dI[static_cast<size_t>(y) * w + x];
				if (r0 && c1) d01 = dI[static_cast<size_t>(y) * w + x + 1];
				if (r1 && c0) d10 = dI[static_cast<size_t>(y + 1) * w + x];
				if (r1 && c1) d11 = dI[static_cast<size_t>(y + 1) * w + x + 1];
				ixv[q] = (d00.x * w00 + d01.x * w01 + d10.x * w10 + d11.x * w11 + 8192) >> 14;
				iyv[q] = (d00.y * w00 + d01.y * w01 + d10.y * w10 + d11.y * w11 + 8192) >> 14;
				a11 += ixv[q] * ixv[q];
				a12 += ixv[q] * iyv[q];
				a22 += iyv[q] * iyv[q];
			}
		}
		const float A11 = __fmul_rn(static_cast<float>(fe_wave_sum(static_cast<double>(a11))), FLT_SCALE);
		const float A12 = __fmul_rn(static_cast<float>(fe_wave_sum(static_cast<double>(a12))), FLT_SCALE);
		const float A22 = __fmul_rn(static_cast<float>(fe_wave_sum(static_cast<double>(a22))), FLT_SCALE);
		float D = __fsub_rn(__fmul_rn(A11, A22), __fmul_rn(A12, A12));
		const float dd = __fsub_rn(A11, A22);
		const float disc = __fadd_rn(__fmul_rn(dd, dd), __fmul_rn(__fmul_rn(4.f, A12), A12));
		const float minEig = __fdiv_rn(__fsub_rn(__fadd_rn(A22, A11), __fsqrt_rn(disc)), static_cast<float>(2 * area));
		if (minEig < minEigThr || D < 1.19209290e-7f)  // FLT_EPSILON
		{
			if (level == 0)
			{
				ok = false;
			}
			continue;
		}
		D = __fdiv_rn(1.f, D);
		float qx = __fsub_rn(resX, hx), qy = __fsub_rn(resY, hy);
		float pdx = 0.f, pdy = 0.f;
		for (int it = 0; it < maxCount; ++it)
		{
			const int iqx = static_cast<int>(floorf(qx)), iqy = static_cast<int>(floorf(qy));
			if (iqx < -winW || iqx >= w || iqy < -winH || iqy >= h)
			{
				if (level == 0)
				{
					ok = false;
				}
				break;
			}
			fe_weights(__fsub_rn(qx, static_cast<float>(iqx)), __fsub_rn(qy, static_cast<float>(iqy)), w00, w01, w10,
					   w11);
			int b1 = 0, b2 = 0;
#pragma unroll
			for (int q = 0; q < kFeLkPerLane; ++q)
			{
				if (wxy[q] >= 0)
				{
					const int diff =
						fe_sample(J, w, h, iqx + (wxy[q] & 0xffff), iqy + (wxy[q] >> 16), w00, w01, w10, w11) - ival[q];
					b1 += diff * ixv[q];
					b2 += diff * iyv[q];
				}
			}
			const float B1 = __fmul_rn(static_cast<float>(fe_wave_sum(static_cast<double>(b1))), FLT_SCALE);
			const float B2 = __fmul_rn(static_cast<float>(fe_wave_sum(static_cast<double>(b2))), FLT_SCALE);
			const float dx = __fmul_rn(__fsub_rn(__fmul_rn(A12, B2), __fmul_rn(A22, B1)), D);
			const float dy = __fmul_rn(__fsub_rn(__fmul_rn(A12, B1), __fmul_rn(A11, B2)), D);
			qx = __fadd_rn(qx, dx);
			qy = __fadd_rn(qy, dy);
			resX = __fadd_rn(qx, hx);
			resY = __fadd_rn(qy, hy);
			if (__dadd_rn(__dmul_rn(static_cast<double>(dx), static_cast<double>(dx)),
						  __dmul_rn(static_cast<double>(dy), static_cast<double>(dy))) <= eps2)
			{
				break;
			}
			if (it > 0 && static_cast<double>(fabsf(__fadd_rn(dx, pdx))) < 0.01 &&
				static_cast<double>(fabsf(__fadd_rn(dy, pdy))) < 0.01)
			{
				resX = __fsub_rn(resX, __fmul_rn(dx, 0.5f));
				resY = __fsub_rn(resY, __fmul_rn(dy, 0.5f));
				break;
			}
			pdx = dx;
			pdy = dy;
		}
	}
	float e = 0.f;
	if (ok)
	{
		// level 0: position check and the mean absolute difference at the result
		const int w = lv[0].w, h = lv[0].h;
		const uint8_t* J = reinterpret_cast<const uint8_t*>(nextPyr + lv[0].img);
		const uint8_t* I = reinterpret_cast<const uint8_t*>(prevPyr + lv[0].img);
		const float qx = __fsub_rn(resX, hx), qy = __fsub_rn(resY, hy);
		const int iqx = static_cast<int>(floorf(qx)), iqy = static_cast<int>(floorf(qy));
		if (iqx < -winW || iqx >= w || iqy < -winH || iqy >= h)
		{
			ok = false;
		}
		else
		{
			// the I window of level 0 again (the loop above kept only the last level's, which is level 0 unless
			// level 0 was skipped -- and a skipped level 0 has status 0)
			const float prevX = __fsub_rn(px0, hx), prevY = __fsub_rn(py0, hy);
			const int ipx = static_cast<int>(floorf(prevX)), ipy = static_cast<int>(floorf(prevY));
			int p00, p01, p10, p11, q00, q01, q10, q11;
			fe_weights(__fsub_rn(prevX, static_cast<float>(ipx)), __fsub_rn(prevY, static_cast<float>(ipy)), p00, p01,
					   p10, p11);
			fe_weights(__fsub_rn(qx, static_cast<float>(iqx)), __fsub_rn(qy, static_cast<float>(iqy)), q00, q01, q10,
					   q11);
			int s = 0;
#pragma unroll
			for (int q = 0; q < kFeLkPerLane; ++q)
			{
				if (wxy[q] >= 0)
				{
					const int ox = wxy[q] & 0xffff, oy = wxy[q] >> 16;
					const int diff = fe_sample(J, w, h, iqx + ox, iqy + oy, q00, q01, q10, q11) -
									 fe_sample(I, w, h, ipx + ox, ipy + oy, p00, p01, p10, p11);
					s += diff < 0 ? -diff : diff;
				}
			}
			e = __fdiv_rn(static_cast<float>(fe_wave_sum(static_cast<double>(s))), static_cast<float>(32 * area));
		}
	}
	if (lane == 0)
	{
		nextXY[2 * pt] = resX;
		nextXY[2 * pt + 1] = resY;
		status[pt] = ok ? 1 : 0;
		if (err)
		{
			err[pt] = ok ? e : 0.f;
		}
	}
}
