// ebo_camera.inc — common::CameraModel on the device (camera_model.h:27-126): batched unproject and project, the
// rectification map of a sensor, the fit of a rectified camera that keeps the sensor's border in view, the remap
// of a frame into that camera, and the record wrapper through which the bucketing kernels of
// ebo_bucket.inc read rectified events.  Included inside ebo_kernels.hip's anonymous namespace, after
// ebo_bucket.inc.  The rules are written out in include/ebo.h ("camera model"); tests/camera_ref.py restates
// them in numpy.  Every float64 operation is rounded on its own (__dadd_rn / __dmul_rn / __ddiv_rn / __dsqrt_rn).

// getTangentialDistortion (camera_model.h:35-40): Scalar(2) * pa * a * b + pb * (r2 + Scalar(2) * a * a)
__device__ __forceinline__ double cam_tangential(double pa, double pb, double a, double b, double r2)
{
	const double lhs = __dmul_rn(__dmul_rn(__dmul_rn(2.0, pa), a), b);
	const double rhs = __dmul_rn(pb, __dadd_rn(r2, __dmul_rn(__dmul_rn(2.0, a), a)));
	return __dadd_rn(lhs, rhs);
}

// getRadialDistortion (camera_model.h:42-47): Scalar(1) + k1 * r2 + k2 * r2 * r2 (k3 is carried, never used)
__device__ __forceinline__ double cam_radial(const CameraConsts& k, double r2)
{
	return __dadd_rn(__dadd_rn(1.0, __dmul_rn(k.k1, r2)), __dmul_rn(__dmul_rn(k.k2, r2), r2));
}

// the first half of unproject (camera_model.h:91-106): normalise, then ten fixed-point iterations
__device__ __forceinline__ void cam_undistort(const CameraConsts& k, double u, double v, double& xOpt, double& yOpt)
{
	const double xD = __ddiv_rn(__dsub_rn(u, k.cx), k.fx);
	const double yD = __ddiv_rn(__dsub_rn(v, k.cy), k.fy);
	xOpt = xD;
	yOpt = yD;
	for (int i = 0; i < 10; ++i)
	{
		const double r2 = __dadd_rn(__dmul_rn(xOpt, xOpt), __dmul_rn(yOpt, yOpt));
		const double radial = cam_radial(k, r2);
		const double dX = cam_tangential(k.p1, k.p2, xOpt, yOpt, r2);
		const double dY = cam_tangential(k.p2, k.p1, yOpt, xOpt, r2);
		xOpt = __ddiv_rn(__dsub_rn(xD, dX), radial);
		yOpt = __ddiv_rn(__dsub_rn(yD, dY), radial);
	}
}

// project (camera_model.h:49-77): divide by z, distort, apply the pinhole part
__device__ __forceinline__ void cam_project(const CameraConsts& k, double x, double y, double z, double& u, double& v)
{
	const double xP = __ddiv_rn(x, z);
	const double yP = __ddiv_rn(y, z);
	const double r2 = __dadd_rn(__dmul_rn(xP, xP), __dmul_rn(yP, yP));
	const double radial = cam_radial(k, r2);
	const double xDist = __dadd_rn(__dmul_rn(xP, radial), cam_tangential(k.p1, k.p2, xP, yP, r2));
	const double yDist = __dadd_rn(__dmul_rn(yP, radial), cam_tangential(k.p2, k.p1, yP, xP, r2));
	u = __dadd_rn(__dmul_rn(k.fx, xDist), k.cx);
	v = __dadd_rn(__dmul_rn(k.fy, yDist), k.cy);
}

// one lane per point: xyz [n][3] -> pixel [n][2]
__global__ void __launch_bounds__(256) k_camera_project(CameraConsts k, int n, const double* __restrict__ xyz,
														double* __restrict__ uv)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
	{
		return;
	}
	const double* p = xyz + 3 * static_cast<size_t>(i);
	double u, v;
	cam_project(k, p[0], p[1], p[2], u, v);
	uv[2 * static_cast<size_t>(i)] = u;
	uv[2 * static_cast<size_t>(i) + 1] = v;
}

// one lane per point: uv [n][2] -> unit bearing [n][3] (camera_model.h:108-113)
__global__ void __launch_bounds__(256) k_camera_unproject(CameraConsts k, int n, const double* __restrict__ uv,
														  double* __restrict__ bearing)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= n)
	{
		return;
	}
	double xo, yo;
	cam_undistort(k, uv[2 * static_cast<size_t>(i)], uv[2 * static_cast<size_t>(i) + 1], xo, yo);
	const double norm = __dsqrt_rn(__dadd_rn(__dadd_rn(__dmul_rn(xo, xo), __dmul_rn(yo, yo)), 1.0));
	double* o = bearing + 3 * static_cast<size_t>(i);
	o[0] = __ddiv_rn(xo, norm);
	o[1] = __ddiv_rn(yo, norm);
	o[2] = __ddiv_rn(1.0, norm);
}

// one lane per sensor pixel: the float64 map (u, v) = (r.fx * xOpt + r.cx, r.fy * yOpt + r.cy) into the rectified
// camera r, and the int16 table round(u), round(v) (half away from zero).  *bad gets bit 1 for a pixel whose map is not finite, bit 2 for a
// rounded coordinate outside the packed range of an event record.
__global__ void __launch_bounds__(256) k_rectify_map(CameraConsts k, RectifiedConsts r, int w, int h,
													 double* __restrict__ map, short2* __restrict__ lut,
													 int* __restrict__ bad)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= w * h)
	{
		return;
	}
	const int x = i % w, y = i / w;
	double xo, yo;
	cam_undistort(k, static_cast<double>(x), static_cast<double>(y), xo, yo);
	const double u = __dadd_rn(__dmul_rn(r.fx, xo), r.cx);
	const double v = __dadd_rn(__dmul_rn(r.fy, yo), r.cy);
	map[2 * static_cast<size_t>(i)] = u;
	map[2 * static_cast<size_t>(i) + 1] = v;
	int flags = 0;
	short2 q = make_short2(0, 0);
	if (!(isfinite(u) && isfinite(v)))
	{
		flags = 1;
	}
	else
	{
		const double ru = round(u), rv = round(v);
		if (ru < static_cast<double>(kCoordMin) || ru > static_cast<double>(kCoordMax) ||
			rv < static_cast<double>(kCoordMin) || rv > static_cast<double>(kCoordMax))
		{
			flags = 2;
		}
		else
		{
			q = make_short2(static_cast<short>(static_cast<int>(ru)), static_cast<short>(static_cast<int>(rv)));
		}
	}
	lut[i] = q;
	if (flags)
	{
		atomicOr(bad, flags);
	}
}

// One workgroup: lanes stride over the 2w + 2h border pixels (rows 0 and h-1, columns 0 and w-1; a corner counted
// twice changes no extreme), minimum and maximum of xOpt and yOpt by a wave-shuffle tree, then across the waves
// through LDS.  out = xmin, xmax, ymin, ymax; *bad is set when a border pixel's undistorted coordinate is not
// finite (fmin / fmax would pass over a NaN).  Minimum and maximum do not depend on the order.
constexpr int kFitThreads = 256;
__global__ void __launch_bounds__(kFitThreads) k_rectify_fit(CameraConsts k, int w, int h, double* __restrict__ out,
															 int* __restrict__ bad)
{
	__shared__ double sRed[kFitThreads / 64][4];
	__shared__ int sBad;
	if (threadIdx.x == 0)
	{
		sBad = 0;
	}
	__syncthreads();
	const double inf = __longlong_as_double(0x7ff0000000000000ll);
	double e[4] = {inf, -inf, inf, -inf};
	int notFinite = 0;
	const int n = 2 * w + 2 * h;
	for (int i = threadIdx.x; i < n; i += kFitThreads)
	{
		int x, y;
		if (i < 2 * w)
		{
			x = i < w ? i : i - w;
			y = i < w ? 0 : h - 1;
		}
		else
		{
			const int j = i - 2 * w;
			x = j < h ? 0 : w - 1;
			y = j < h ? j : j - h;
		}
		double xo, yo;
		cam_undistort(k, static_cast<double>(x), static_cast<double>(y), xo, yo);
		notFinite |= !(isfinite(xo) && isfinite(yo));
		e[0] = fmin(e[0], xo);
		e[1] = fmax(e[1], xo);
		e[2] = fmin(e[2], yo);
		e[3] = fmax(e[3], yo);
	}
#pragma unroll
	for (int s = 32; s > 0; s /= 2)
	{
		e[0] = fmin(e[0], __shfl_down(e[0], s, 64));
		e[1] = fmax(e[1], __shfl_down(e[1], s, 64));
		e[2] = fmin(e[2], __shfl_down(e[2], s, 64));
		e[3] = fmax(e[3], __shfl_down(e[3], s, 64));
	}
	if ((threadIdx.x & 63) == 0)
	{
#pragma unroll
		for (int q = 0; q < 4; ++q)
		{
			sRed[threadIdx.x / 64][q] = e[q];
		}
	}
	if (notFinite)
	{
		atomicOr(&sBad, 1);
	}
	__syncthreads();
	if (threadIdx.x == 0)
	{
		for (int wv = 1; wv < kFitThreads / 64; ++wv)
		{
			e[0] = fmin(e[0], sRed[wv][0]);
			e[1] = fmax(e[1], sRed[wv][1]);
			e[2] = fmin(e[2], sRed[wv][2]);
			e[3] = fmax(e[3], sRed[wv][3]);
		}
#pragma unroll
		for (int q = 0; q < 4; ++q)
		{
			out[q] = e[q];
		}
		*bad = sBad;
	}
}

// One tap of the remap: the byte at (x, y) as a double, 0 outside the image.  The load is predicated on the tap's own
// in-image test and its address is formed from clamped indices, so no lane reads outside the frame.
__device__ __forceinline__ double cam_tap(const uint8_t* __restrict__ img, int w, int h, int x, int y)
{
	const bool inside = x >= 0 && x < w && y >= 0 && y < h;
	const size_t cx = static_cast<size_t>(min(max(x, 0), w - 1)), cy = static_cast<size_t>(min(max(y, 0), h - 1));
	unsigned int p = 0;
	if (inside)
	{
		p = img[cy * static_cast<size_t>(w) + cx];
	}
	return static_cast<double>(p);
}

// One lane per output pixel (x', y') of the rectified camera r, in 32 x 8 tiles: the source position
// (us, vs) = project((x' - r.cx) / r.fx, (y' - r.cy) / r.fy, 1) of the lens camera k, recomputed per pixel, and the
// bilinear sample of the frame there, constant border 0, rounded half away from zero.  src (optional) receives
// (us, vs); img / out may be null together (the source map alone).
constexpr int kRectTileW = 32, kRectTileH = 8;
__global__ void __launch_bounds__(kRectTileW * kRectTileH) k_rectify_image(CameraConsts k, RectifiedConsts r, int w, int h,
																		   const uint8_t* __restrict__ img,
																		   uint8_t* __restrict__ out,
																		   double* __restrict__ src)
{
	const int x = blockIdx.x * kRectTileW + threadIdx.x, y = blockIdx.y * kRectTileH + threadIdx.y;
	if (x >= w || y >= h)
	{
		return;
	}
	const size_t o = static_cast<size_t>(y) * w + x;
	const double xn = __ddiv_rn(__dsub_rn(static_cast<double>(x), r.cx), r.fx);
	const double yn = __ddiv_rn(__dsub_rn(static_cast<double>(y), r.cy), r.fy);
	double us, vs;
	cam_project(k, xn, yn, 1.0, us, vs);
	if (src)
	{
		src[2 * o] = us;
		src[2 * o + 1] = vs;
	}
	if (!out)
	{
		return;
	}
	uint8_t res = 0;
	// in double, before any conversion to an integer; a NaN fails the test
	if (us > -1.0 && us < static_cast<double>(w) && vs > -1.0 && vs < static_cast<double>(h))
	{
		const double fx0 = floor(us), fy0 = floor(vs);
		const double a = __dsub_rn(us, fx0), b = __dsub_rn(vs, fy0);
		const double ia = __dsub_rn(1.0, a), ib = __dsub_rn(1.0, b);
		const int x0 = static_cast<int>(fx0), y0 = static_cast<int>(fy0);  // in [-1, w - 1] x [-1, h - 1]
		const double p00 = cam_tap(img, w, h, x0, y0), p10 = cam_tap(img, w, h, x0 + 1, y0);
		const double p01 = cam_tap(img, w, h, x0, y0 + 1), p11 = cam_tap(img, w, h, x0 + 1, y0 + 1);
		const double top = __dadd_rn(__dmul_rn(ia, p00), __dmul_rn(a, p10));
		const double bot = __dadd_rn(__dmul_rn(ia, p01), __dmul_rn(a, p11));
		const double val = __dadd_rn(__dmul_rn(ib, top), __dmul_rn(b, bot));
		res = static_cast<uint8_t>(static_cast<int>(round(val)));
	}
	out[o] = res;
}

// An event record read through the rectification table: a raw coordinate inside the sensor is replaced by its
// table entry (which may lie outside the sensor: bucket_of sends it to the stray unit); one outside the sensor
// stays as it is.  Table entries were range-checked when the table was built, so the inner record's range check
// still covers every coordinate the kernels see.
template <class Rec>
struct Rectified
{
	Rec inner;
	const short2* lut;  // [h][w]
	int w, h;
	__device__ __forceinline__ void load(unsigned long long e, int win, int& x, int& y, int& pos, long long& t) const
	{
		inner.load(e, win, x, y, pos, t);
		if (x >= 0 && x < w && y >= 0 && y < h)
		{
			const short2 q = lut[y * w + x];
			x = q.x;
			y = q.y;
		}
	}
	static constexpr bool kCheckRange = Rec::kCheckRange;
};
