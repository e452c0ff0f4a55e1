// ebo_camera.cpp — the camera-model entry points of include/ebo.h: common::CameraModel::unproject and project for many
// points (camera_model.h:49-114), the rectification of a context's loaders and of its frames, and the fit of a rectified
// camera; the kernels are in ebo_camera.inc.  Compiled without contraction: the fit's scalar steps (rule C3) are here.
#include "ebo_ctx.h"

using namespace ebo;

namespace
{
CameraConsts consts_of(const ebo_camera* cam)
{
	CameraConsts k;
	k.fx = cam->fx;
	k.fy = cam->fy;
	k.cx = cam->cx;
	k.cy = cam->cy;
	k.k1 = cam->k1;
	k.k2 = cam->k2;
	k.k3 = cam->k3;
	k.p1 = cam->p1;
	k.p2 = cam->p2;
	return k;
}

RectifiedConsts rectified_of(const ebo_camera& r)
{
	RectifiedConsts o;
	o.fx = r.fx;
	o.fy = r.fy;
	o.cx = r.cx;
	o.cy = r.cy;
	return o;
}

// rules C1 + C2: the map and table of `cam` into the rectified camera `r`; a refused call leaves no rectification set
int set_rectification(ebo_ctx* c, const ebo_camera* cam, const ebo_camera* r)
{
	c->rect_set = false;
	c->rect_lut.clear();
	if (r->k1 != 0.0 || r->k2 != 0.0 || r->p1 != 0.0 || r->p2 != 0.0)
	{
		return c->fail(EBO_ERR_ARG, "ebo_set_rectification_camera: a rectified camera has k1 = k2 = p1 = p2 = 0");
	}
	if (!std::isfinite(cam->fx) || !std::isfinite(cam->fy) || cam->fx == 0.0 || cam->fy == 0.0 || !std::isfinite(r->fx) ||
		!std::isfinite(r->fy) || r->fx == 0.0 || r->fy == 0.0)
	{
		return c->fail(EBO_ERR_RANGE, "ebo_set_rectification: fx and fy must be finite and non-zero");
	}
	(void)hipSetDevice(c->prm.device);
	const size_t npx = static_cast<size_t>(c->prm.image_w) * c->prm.image_h;
	int rc = c->grow(c->d_rect_lut, npx * 2 * sizeof(int16_t), "hipMalloc rectification table");
	if (rc == EBO_OK) rc = c->grow(c->d_rect_map, npx * 2, "hipMalloc rectification map");
	if (rc == EBO_OK) rc = c->grow(c->d_rect_bad, 256 / sizeof(int), "hipMalloc rectification flag");
	if (rc)
	{
		return rc;
	}
	if (launch_rectify_map(consts_of(cam), rectified_of(*r), c->prm.image_w, c->prm.image_h, c->d_rect_map, c->d_rect_lut,
						   c->d_rect_bad, c->stream))
	{
		return c->hip(hipGetLastError(), "rectification map launch");
	}
	int bad = 0;
	hipError_t e = hipMemcpyAsync(&bad, c->d_rect_bad, sizeof(int), hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "rectification flag");
	}
	if (bad)
	{
		return c->fail(EBO_ERR_RANGE, (bad & 1) ? "ebo_set_rectification: the map of a sensor pixel is not finite"
												: "ebo_set_rectification: a rectified coordinate lies outside [-16384,16383]");
	}
	c->rect_cam = *cam;
	c->rect_out = ebo_camera{r->fx, r->fy, r->cx, r->cy, 0.0, 0.0, 0.0, 0.0, 0.0};
	c->rect_set = true;
	return EBO_OK;
}

// the entry checks every rectified-frame call shares; 0 or the code to return
int need_rectification(ebo_ctx* c, const char* what)
{
	if (c->capturing)
	{
		return c->fail(EBO_ERR_STATE, kNotWhileRecording);
	}
	if (!c->rect_set)
	{
		return c->fail(EBO_ERR_STATE, what);
	}
	return EBO_OK;
}
}  // namespace

extern "C" {

int ebo_camera_unproject_device(ebo_ctx* c, const ebo_camera* cam, int n, const double* d_uv, double* d_bearing)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	if (c->capturing)
	{
		return c->fail(EBO_ERR_STATE, kNotWhileRecording);
	}
	if (!cam || n < 0 || (n > 0 && (!d_uv || !d_bearing)))
	{
		return c->fail(EBO_ERR_ARG, "ebo_camera_unproject: null camera, points or output, or a negative count");
	}
	(void)hipSetDevice(c->prm.device);
	if (launch_camera_unproject(consts_of(cam), n, d_uv, d_bearing, c->stream))
	{
		return c->hip(hipGetLastError(), "unproject launch");
	}
	return EBO_OK;
}

int ebo_camera_unproject(ebo_ctx* c, const ebo_camera* cam, int n, const double* uv, double* bearing)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	if (c->capturing)
	{
		return c->fail(EBO_ERR_STATE, kNotWhileRecording);
	}
	if (!cam || n < 0 || (n > 0 && (!uv || !bearing)))
	{
		return c->fail(EBO_ERR_ARG, "ebo_camera_unproject: null camera, points or output, or a negative count");
	}
	if (n == 0)
	{
		return EBO_OK;
	}
	(void)hipSetDevice(c->prm.device);
	const size_t bIn = align256(static_cast<size_t>(n) * 2 * sizeof(double)), bOut = static_cast<size_t>(n) * 3 * sizeof(double);
	int rc = c->grow(c->d_scratch, bIn + bOut, "hipMalloc scratch");
	if (rc)
	{
		return rc;
	}
	double* d_uv = reinterpret_cast<double*>(static_cast<char*>(c->d_scratch.get()));
	double* d_out = reinterpret_cast<double*>(static_cast<char*>(c->d_scratch.get()) + bIn);
	rc = c->hip(hipMemcpyAsync(d_uv, uv, static_cast<size_t>(n) * 2 * sizeof(double), hipMemcpyHostToDevice, c->stream),
				"H2D points");
	if (rc)
	{
		return rc;
	}
	if (launch_camera_unproject(consts_of(cam), n, d_uv, d_out, c->stream))
	{
		return c->hip(hipGetLastError(), "unproject launch");
	}
	hipError_t e = hipMemcpyAsync(bearing, d_out, bOut, hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	return c->hip(e, "D2H bearing vectors");
}

int ebo_set_rectification(ebo_ctx* c, const ebo_camera* cam)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	if (c->capturing)
	{
		return c->fail(EBO_ERR_STATE, kNotWhileRecording);
	}
	if (!cam)
	{
		return c->fail(EBO_ERR_ARG, "ebo_set_rectification: null camera");
	}
	// the rectified camera keeps fx fy cx cy
	const ebo_camera same{cam->fx, cam->fy, cam->cx, cam->cy, 0.0, 0.0, 0.0, 0.0, 0.0};
	return set_rectification(c, cam, &same);
}

int ebo_set_rectification_camera(ebo_ctx* c, const ebo_camera* cam, const ebo_camera* rectified)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	if (c->capturing)
	{
		return c->fail(EBO_ERR_STATE, kNotWhileRecording);
	}
	if (!cam || !rectified)
	{
		c->rect_set = false;
		c->rect_lut.clear();
		return c->fail(EBO_ERR_ARG, "ebo_set_rectification_camera: null camera");
	}
	return set_rectification(c, cam, rectified);
}

int ebo_rectified_camera(ebo_ctx* c, ebo_camera* out)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	const int rc = need_rectification(c, "ebo_rectified_camera: no rectification is set");
	if (rc)
	{
		return rc;
	}
	if (!out)
	{
		return c->fail(EBO_ERR_ARG, "ebo_rectified_camera: null output");
	}
	*out = c->rect_out;
	return EBO_OK;
}

int ebo_fit_rectified_camera(ebo_ctx* c, const ebo_camera* cam, ebo_camera* rectified_out)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	if (c->capturing)
	{
		return c->fail(EBO_ERR_STATE, kNotWhileRecording);
	}
	if (!cam || !rectified_out)
	{
		return c->fail(EBO_ERR_ARG, "ebo_fit_rectified_camera: null camera or output");
	}
	const int w = c->prm.image_w, h = c->prm.image_h;
	if (w < 2 || h < 2 || !(cam->fx > 0.0) || !(cam->fy > 0.0))
	{
		return c->fail(EBO_ERR_RANGE, "ebo_fit_rectified_camera: needs an image of at least 2 x 2 and fx, fy > 0");
	}
	(void)hipSetDevice(c->prm.device);
	int rc = c->grow(c->d_scratch, 256 + sizeof(int), "hipMalloc scratch");
	if (rc)
	{
		return rc;
	}
	double* d_ext = reinterpret_cast<double*>(static_cast<char*>(c->d_scratch.get()));
	int* d_bad = reinterpret_cast<int*>(static_cast<char*>(c->d_scratch.get()) + 256);
	if (launch_rectify_fit(consts_of(cam), w, h, d_ext, d_bad, c->stream))
	{
		return c->hip(hipGetLastError(), "rectified-camera fit launch");
	}
	double ext[4] = {0.0, 0.0, 0.0, 0.0};
	int bad = 0;
	hipError_t e = hipMemcpyAsync(ext, d_ext, sizeof(ext), hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess)
	{
		e = hipMemcpyAsync(&bad, d_bad, sizeof(int), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "D2H border extremes");
	}
	const double xmin = ext[0], xmax = ext[1], ymin = ext[2], ymax = ext[3];
	// rule C3, one operation per statement
	const double ex = xmax - xmin;
	const double ey = ymax - ymin;
	if (bad || !std::isfinite(xmin) || !std::isfinite(xmax) || !std::isfinite(ymin) || !std::isfinite(ymax) || !(ex > 0.0) ||
		!(ey > 0.0))
	{
		return c->fail(EBO_ERR_RANGE, "ebo_fit_rectified_camera: the undistorted border is not finite or has no extent");
	}
	const double wm = static_cast<double>(w - 1), hm = static_cast<double>(h - 1);
	const double dx = cam->fx * ex;
	const double dy = cam->fy * ey;
	const double sx = wm / dx;
	const double sy = hm / dy;
	const double s = sx < sy ? sx : sy;
	ebo_camera r{0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
	r.fx = s * cam->fx;
	r.fy = s * cam->fy;
	const double tx = xmax + xmin;
	const double ty = ymax + ymin;
	const double mx = r.fx * tx;
	const double my = r.fy * ty;
	const double nx = wm - mx;
	const double ny = hm - my;
	r.cx = nx / 2.0;
	r.cy = ny / 2.0;
	*rectified_out = r;
	return EBO_OK;
}

int ebo_rectify_image_device(ebo_ctx* c, const uint8_t* d_image, uint8_t* d_out)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	const int rc = need_rectification(c, "ebo_rectify_image: no rectification is set");
	if (rc)
	{
		return rc;
	}
	if (!d_image || !d_out || d_image == d_out)
	{
		return c->fail(EBO_ERR_ARG, "ebo_rectify_image: null image or output, or the output is the image");
	}
	(void)hipSetDevice(c->prm.device);
	if (launch_rectify_image(consts_of(&c->rect_cam), rectified_of(c->rect_out), c->prm.image_w, c->prm.image_h, d_image, d_out,
							 nullptr, c->stream))
	{
		return c->hip(hipGetLastError(), "rectify image launch");
	}
	return EBO_OK;
}

int ebo_rectify_image(ebo_ctx* c, const uint8_t* image, uint8_t* out)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	int rc = need_rectification(c, "ebo_rectify_image: no rectification is set");
	if (rc)
	{
		return rc;
	}
	if (!image || !out)
	{
		return c->fail(EBO_ERR_ARG, "ebo_rectify_image: null image or output");
	}
	(void)hipSetDevice(c->prm.device);
	const size_t npx = static_cast<size_t>(c->prm.image_w) * c->prm.image_h;
	const size_t bIn = align256(npx);
	rc = c->grow(c->d_scratch, bIn + npx, "hipMalloc scratch");
	if (rc)
	{
		return rc;
	}
	uint8_t* d_in = reinterpret_cast<uint8_t*>(static_cast<char*>(c->d_scratch.get()));
	uint8_t* d_out = d_in + bIn;
	rc = c->hip(hipMemcpyAsync(d_in, image, npx, hipMemcpyHostToDevice, c->stream), "H2D image");
	if (rc)
	{
		return rc;
	}
	if (launch_rectify_image(consts_of(&c->rect_cam), rectified_of(c->rect_out), c->prm.image_w, c->prm.image_h, d_in, d_out,
							 nullptr, c->stream))
	{
		return c->hip(hipGetLastError(), "rectify image launch");
	}
	hipError_t e = hipMemcpyAsync(out, d_out, npx, hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	return c->hip(e, "D2H rectified image");
}

int ebo_rectification_source_map(ebo_ctx* c, double* map_xy)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	int rc = need_rectification(c, "ebo_rectification_source_map: no rectification is set");
	if (rc)
	{
		return rc;
	}
	if (!map_xy)
	{
		return c->fail(EBO_ERR_ARG, "ebo_rectification_source_map: null output");
	}
	(void)hipSetDevice(c->prm.device);
	const size_t bytes = static_cast<size_t>(c->prm.image_w) * c->prm.image_h * 2 * sizeof(double);
	rc = c->grow(c->d_scratch, bytes, "hipMalloc scratch");
	if (rc)
	{
		return rc;
	}
	double* d_src = reinterpret_cast<double*>(static_cast<char*>(c->d_scratch.get()));
	if (launch_rectify_image(consts_of(&c->rect_cam), rectified_of(c->rect_out), c->prm.image_w, c->prm.image_h, nullptr, nullptr,
							 d_src, c->stream))
	{
		return c->hip(hipGetLastError(), "source map launch");
	}
	hipError_t e = hipMemcpyAsync(map_xy, d_src, bytes, hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	return c->hip(e, "D2H source map");
}

int ebo_camera_project_device(ebo_ctx* c, const ebo_camera* cam, int n, const double* d_xyz, double* d_uv)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	if (c->capturing)
	{
		return c->fail(EBO_ERR_STATE, kNotWhileRecording);
	}
	if (!cam || n < 0 || (n > 0 && (!d_xyz || !d_uv)))
	{
		return c->fail(EBO_ERR_ARG, "ebo_camera_project: null camera, points or output, or a negative count");
	}
	(void)hipSetDevice(c->prm.device);
	if (launch_camera_project(consts_of(cam), n, d_xyz, d_uv, c->stream))
	{
		return c->hip(hipGetLastError(), "project launch");
	}
	return EBO_OK;
}

int ebo_camera_project(ebo_ctx* c, const ebo_camera* cam, int n, const double* xyz, double* uv)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	if (c->capturing)
	{
		return c->fail(EBO_ERR_STATE, kNotWhileRecording);
	}
	if (!cam || n < 0 || (n > 0 && (!xyz || !uv)))
	{
		return c->fail(EBO_ERR_ARG, "ebo_camera_project: null camera, points or output, or a negative count");
	}
	if (n == 0)
	{
		return EBO_OK;
	}
	(void)hipSetDevice(c->prm.device);
	const size_t bIn = align256(static_cast<size_t>(n) * 3 * sizeof(double)), bOut = static_cast<size_t>(n) * 2 * sizeof(double);
	int rc = c->grow(c->d_scratch, bIn + bOut, "hipMalloc scratch");
	if (rc)
	{
		return rc;
	}
	double* d_xyz = reinterpret_cast<double*>(static_cast<char*>(c->d_scratch.get()));
	double* d_out = reinterpret_cast<double*>(static_cast<char*>(c->d_scratch.get()) + bIn);
	rc = c->hip(hipMemcpyAsync(d_xyz, xyz, static_cast<size_t>(n) * 3 * sizeof(double), hipMemcpyHostToDevice, c->stream),
				"H2D points");
	if (rc)
	{
		return rc;
	}
	if (launch_camera_project(consts_of(cam), n, d_xyz, d_out, c->stream))
	{
		return c->hip(hipGetLastError(), "project launch");
	}
	hipError_t e = hipMemcpyAsync(uv, d_out, bOut, hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	return c->hip(e, "D2H pixels");
}

int ebo_clear_rectification(ebo_ctx* c)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	if (c->capturing)
	{
		return c->fail(EBO_ERR_STATE, kNotWhileRecording);
	}
	c->rect_set = false;
	c->rect_lut.clear();
	return EBO_OK;
}

int ebo_rectification_map(ebo_ctx* c, double* map_xy, int16_t* lut)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	if (c->capturing)
	{
		return c->fail(EBO_ERR_STATE, kNotWhileRecording);
	}
	if (!c->rect_set)
	{
		return c->fail(EBO_ERR_STATE, "ebo_rectification_map: no rectification is set");
	}
	(void)hipSetDevice(c->prm.device);
	const size_t npx = static_cast<size_t>(c->prm.image_w) * c->prm.image_h;
	hipError_t e = hipSuccess;
	if (map_xy)
	{
		e = hipMemcpyAsync(map_xy, c->d_rect_map, npx * 2 * sizeof(double), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess && lut)
	{
		e = hipMemcpyAsync(lut, c->d_rect_lut, npx * 2 * sizeof(int16_t), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	return c->hip(e, "D2H rectification map");
}

}  // extern "C"
