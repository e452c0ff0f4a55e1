// ebo_camera.inc — common::CameraModel on the device (camera_model.h:27-126): batched unproject, the
// rectification map of a sensor, and the record wrapper through which the bucketing kernels of
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

// one lane per sensor pixel: the float64 map (u, v) = (fx * xOpt + cx, fy * yOpt + cy) and the int16 table
// round(u), round(v) (half away from zero).  *bad gets bit 1 for a pixel whose map is not finite, bit 2 for a
// rounded coordinate outside the packed range of an event record.
__global__ void __launch_bounds__(256) k_rectify_map(CameraConsts k, int w, int h, double* __restrict__ map,
													 short2* __restrict__ lut, int* __restrict__ bad)
{
	const int i = blockIdx.x * blockDim.x + threadIdx.x;
	if (i >= w * h)
	{
		return;
	}
	const int x = i % w, y = i / w;
	double xo, yo;
	cam_undistort(k, static_cast<double>(x), static_cast<double>(y), xo, yo);
	const double u = __dadd_rn(__dmul_rn(k.fx, xo), k.cx);
	const double v = __dadd_rn(__dmul_rn(k.fy, yo), k.cy);
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
