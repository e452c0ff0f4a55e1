// ebo_frontend.cpp — the image front end entry points of include/ebo.h (FeatureDetector::newImage's
// goodFeaturesToTrack, log image + Sobel and calcOpticalFlowPyrLK); the kernels are in ebo_frontend.inc.
#include "ebo_ctx.h"

using namespace ebo;

namespace
{
int entry_checks(ebo_ctx* c)
{
	if (c->capturing)
	{
		return c->fail(EBO_ERR_STATE, kNotWhileRecording);
	}
	(void)hipSetDevice(c->prm.device);
	return EBO_OK;
}

int finish(ebo_ctx* c, hipError_t e, const char* what)
{
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	return c->hip(e, what);
}
}  // namespace

extern "C" {

// FeatureDetector::getLogImage + getGradients (feature_detector.cpp:713-731)
int ebo_image_gradients(ebo_ctx* c, const uint8_t* image, double* grad_x, double* grad_y)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	int rc = entry_checks(c);
	if (rc)
	{
		return rc;
	}
	if (!image || !grad_x || !grad_y)
	{
		return c->fail(EBO_ERR_ARG, "ebo_image_gradients: null image or output");
	}
	const int w = c->prm.image_w, h = c->prm.image_h;
	const size_t npx = static_cast<size_t>(w) * h;
	if (!c->d_fe_lut)
	{
		// convertTo(CV_64F, 1/255), + 10e-2, log, / 8: per grey value, in double on the host
		double lut[256];
		for (int v = 0; v < 256; ++v)
		{
			lut[v] = std::log(v * (1.0 / 255.0) + 10e-2) / 8;
		}
		rc = c->grow(c->d_fe_lut, 256, "hipMalloc log table");
		if (rc)
		{
			return rc;
		}
		rc = c->hip(hipMemcpy(c->d_fe_lut, lut, sizeof(lut), hipMemcpyHostToDevice), "H2D log table");
		if (rc)
		{
			c->d_fe_lut.reset();  // (its presence says that it is filled)
			return rc;
		}
	}
	const size_t bImg = align256(npx), bG = align256(npx * 8);
	rc = c->grow(c->d_fe, bImg + 2 * bG, "hipMalloc front-end workspace");
	if (rc)
	{
		return rc;
	}
	char* base = static_cast<char*>(c->d_fe.get());
	uint8_t* d_img = reinterpret_cast<uint8_t*>(base);
	double* d_gx = reinterpret_cast<double*>(base + bImg);
	double* d_gy = reinterpret_cast<double*>(base + bImg + bG);
	hipError_t e = hipMemcpyAsync(d_img, image, npx, hipMemcpyHostToDevice, c->stream);
	if (e != hipSuccess)
	{
		return c->hip(e, "H2D image");
	}
	if (launch_fe_gradients(d_img, c->d_fe_lut, w, h, d_gx, d_gy, c->stream))
	{
		return c->hip(hipGetLastError(), "gradients launch");
	}
	e = hipMemcpyAsync(grad_x, d_gx, npx * 8, hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess)
	{
		e = hipMemcpyAsync(grad_y, d_gy, npx * 8, hipMemcpyDeviceToHost, c->stream);
	}
	return finish(c, e, "D2H gradients");
}

// cv::goodFeaturesToTrack(..., useHarrisDetector = true, k) (feature_detector.cpp:568-583)
int ebo_good_features(ebo_ctx* c, const uint8_t* image, const uint8_t* mask, int max_corners, double quality_level,
					  double min_distance, int block_size, double harris_k, float* corners_xy, int* n_out)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	int rc = entry_checks(c);
	if (rc)
	{
		return rc;
	}
	if (!image || !corners_xy || !n_out)
	{
		return c->fail(EBO_ERR_ARG, "ebo_good_features: null image or output");
	}
	if (max_corners < 1 || max_corners > kFeMaxCornersLds || block_size < 1 || block_size > 7 ||
		!(quality_level >= 0) || !(min_distance >= 0) || !std::isfinite(harris_k))
	{
		return c->fail(EBO_ERR_ARG, "ebo_good_features: max_corners 1..8192, block_size 1..7, quality_level and "
									"min_distance >= 0");
	}
	const int w = c->prm.image_w, h = c->prm.image_h;
	const size_t npx = static_cast<size_t>(w) * h;
	size_t capPow2 = 1;
	while (capPow2 < npx)
	{
		capPow2 <<= 1;
	}
	const size_t nb = static_cast<size_t>(fe_harris_blocks(w, h));
	const size_t bImg = align256(npx), bResp = align256(npx * 8), bMax = align256(nb * 8);
	const size_t bCR = align256(capPow2 * 8), bCI = align256(capPow2 * 4);
	const size_t bCorners = align256(static_cast<size_t>(max_corners) * 8);
	rc = c->grow(c->d_fe, 2 * bImg + bResp + bMax + bCR + bCI + bCorners + 256,
				"hipMalloc front-end workspace");
	if (rc)
	{
		return rc;
	}
	char* p = static_cast<char*>(c->d_fe.get());
	uint8_t* d_img = reinterpret_cast<uint8_t*>(p);
	uint8_t* d_mask = reinterpret_cast<uint8_t*>(p + bImg);
	p += 2 * bImg;
	double* d_resp = reinterpret_cast<double*>(p);
	p += bResp;
	double* d_bmax = reinterpret_cast<double*>(p);
	p += bMax;
	double* d_candR = reinterpret_cast<double*>(p);
	p += bCR;
	int* d_candI = reinterpret_cast<int*>(p);
	p += bCI;
	float* d_corners = reinterpret_cast<float*>(p);
	p += bCorners;
	int* d_count = reinterpret_cast<int*>(p);
	int* d_nout = d_count + 1;
	hipError_t e = hipMemcpyAsync(d_img, image, npx, hipMemcpyHostToDevice, c->stream);
	if (e == hipSuccess && mask)
	{
		e = hipMemcpyAsync(d_mask, mask, npx, hipMemcpyHostToDevice, c->stream);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "H2D image / mask");
	}
	if (launch_fe_harris(d_img, mask ? d_mask : nullptr, w, h, block_size, harris_k, quality_level, d_resp, d_bmax,
						 d_candR, d_candI, d_count, c->stream))
	{
		return c->hip(hipGetLastError(), "Harris launch");
	}
	int n = 0;
	e = hipMemcpyAsync(&n, d_count, sizeof(int), hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "D2H candidate count");
	}
	if (launch_fe_select(d_candR, d_candI, d_count, n, static_cast<int>(capPow2), w, max_corners, min_distance,
						 d_corners, d_nout, c->stream))
	{
		return c->hip(hipGetLastError(), "corner selection launch");
	}
	int nOut = 0;
	e = hipMemcpyAsync(&nOut, d_nout, sizeof(int), hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	if (e == hipSuccess && nOut > 0)
	{
		e = hipMemcpy(corners_xy, d_corners, static_cast<size_t>(nOut) * 8, hipMemcpyDeviceToHost);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "D2H corners");
	}
	*n_out = nOut;
	return EBO_OK;
}

// FlowEstimator::addImage (flow_estimator.cpp:16-25): the pyramid and its derivatives, built once per image
int ebo_lk_add_image(ebo_ctx* c, const uint8_t* image)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	int rc = entry_checks(c);
	if (rc)
	{
		return rc;
	}
	if (!image)
	{
		return c->fail(EBO_ERR_ARG, "ebo_lk_add_image: null image");
	}
	if (c->fe_lv.empty())
	{
		// levels while the next one is at least 2 x 2 (ebo.h), images then derivatives, 256-byte aligned
		std::vector<FeLevel> lv;
		int w = c->prm.image_w, h = c->prm.image_h;
		size_t off = 0;
		while (true)
		{
			FeLevel L;
			L.w = w;
			L.h = h;
			L.img = off;
			off += align256(static_cast<size_t>(w) * h);
			L.der = off;
			off += align256(static_cast<size_t>(w) * h * 4);
			lv.push_back(L);
			const int nw = (w + 1) / 2, nh = (h + 1) / 2;
			if (static_cast<int>(lv.size()) == kFeLevels || nw < 2 || nh < 2 || (nw == w && nh == h))
			{
				break;
			}
			w = nw;
			h = nh;
		}
		// (fe_lv says that all of this succeeded: a failed attempt leaves nothing behind)
		rc = c->grow(c->d_fe_pyr[0], off, "hipMalloc pyramid");
		if (rc == EBO_OK) rc = c->grow(c->d_fe_pyr[1], off, "hipMalloc pyramid");
		if (rc == EBO_OK) rc = c->grow(c->d_fe_lv, lv.size(), "hipMalloc levels");
		if (rc == EBO_OK) rc = c->hip(hipMemcpy(c->d_fe_lv, lv.data(), lv.size() * sizeof(FeLevel), hipMemcpyHostToDevice), "H2D levels");
		if (rc)
		{
			c->d_fe_pyr[0].reset();
			c->d_fe_pyr[1].reset();
			c->d_fe_lv.reset();
			return rc;
		}
		c->fe_lv = lv;
	}
	// the older image's slot takes the new one; the newer becomes the older without recomputation
	const int slot = c->fe_images == 0 ? c->fe_newer : c->fe_newer ^ 1;
	char* pyr = c->d_fe_pyr[slot];
	hipError_t e = hipMemcpyAsync(pyr, image, static_cast<size_t>(c->prm.image_w) * c->prm.image_h,
								  hipMemcpyHostToDevice, c->stream);
	if (e != hipSuccess)
	{
		return c->hip(e, "H2D image");
	}
	if (launch_fe_pyramid(pyr, c->fe_lv.data(), static_cast<int>(c->fe_lv.size()), c->stream))
	{
		return c->hip(hipGetLastError(), "pyramid launch");
	}
	rc = finish(c, hipSuccess, "pyramid");
	if (rc)
	{
		return rc;
	}
	c->fe_newer = slot;
	c->fe_images = std::min(c->fe_images + 1, 2);
	return EBO_OK;
}

// cv::calcOpticalFlowPyrLK from the older image to the newer one (flow_estimator.cpp:86-108), n points at once
int ebo_lk_track(ebo_ctx* c, int n, const float* prev_xy, float* next_xy, uint8_t* status, float* err, int win_w,
				 int win_h, int max_level, int max_count, double epsilon, double min_eig_threshold)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	int rc = entry_checks(c);
	if (rc)
	{
		return rc;
	}
	if (n < 0 || (n > 0 && (!prev_xy || !next_xy || !status)) || win_w < 3 || win_h < 3 ||
		win_w * win_h > kFeMaxWindow || max_level < 0 || max_level > kFeLevels - 1 || max_count < 1 ||
		!(epsilon >= 0) || !std::isfinite(min_eig_threshold))
	{
		return c->fail(EBO_ERR_ARG, "ebo_lk_track: bad points or parameters (3 <= win, win_w * win_h <= 1024, "
									"0 <= max_level <= 7, max_count >= 1)");
	}
	if (c->fe_images < 2)
	{
		return c->fail(EBO_ERR_STATE, "ebo_lk_track needs two images (ebo_lk_add_image)");
	}
	if (n == 0)
	{
		return EBO_OK;
	}
	// buildOpticalFlowPyramid: level l + 1 only while it is larger than the window in both dimensions
	int levels = 1;
	while (levels - 1 < max_level && levels < static_cast<int>(c->fe_lv.size()) && c->fe_lv[levels].w > win_w &&
		   c->fe_lv[levels].h > win_h)
	{
		++levels;
	}
	const size_t bXY = align256(static_cast<size_t>(n) * 8), bSt = align256(static_cast<size_t>(n)),
				 bErr = align256(static_cast<size_t>(n) * 4);
	rc = c->grow(c->d_fe_pts, 2 * bXY + bSt + bErr, "hipMalloc LK points");
	if (rc)
	{
		return rc;
	}
	char* p = static_cast<char*>(c->d_fe_pts.get());
	float* d_prev = reinterpret_cast<float*>(p);
	float* d_next = reinterpret_cast<float*>(p + bXY);
	uint8_t* d_status = reinterpret_cast<uint8_t*>(p + 2 * bXY);
	float* d_err = reinterpret_cast<float*>(p + 2 * bXY + bSt);
	hipError_t e = hipMemcpyAsync(d_prev, prev_xy, static_cast<size_t>(n) * 8, hipMemcpyHostToDevice, c->stream);
	if (e != hipSuccess)
	{
		return c->hip(e, "H2D points");
	}
	// as calcOpticalFlowPyrLK: max_count clamped to 100, epsilon to 10 and squared, the threshold taken as float
	const double eps = std::min(epsilon, 10.0);
	if (launch_fe_lk(c->d_fe_pyr[c->fe_newer ^ 1], c->d_fe_pyr[c->fe_newer], c->d_fe_lv, levels, n, d_prev, d_next,
					 d_status, d_err, win_w, win_h, std::min(max_count, 100), eps * eps,
					 static_cast<float>(min_eig_threshold),
					 c->stream))
	{
		return c->hip(hipGetLastError(), "LK launch");
	}
	e = hipMemcpyAsync(next_xy, d_next, static_cast<size_t>(n) * 8, hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess)
	{
		e = hipMemcpyAsync(status, d_status, static_cast<size_t>(n), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess && err)
	{
		e = hipMemcpyAsync(err, d_err, static_cast<size_t>(n) * 4, hipMemcpyDeviceToHost, c->stream);
	}
	return finish(c, e, "D2H LK results");
}

}  // extern "C"
