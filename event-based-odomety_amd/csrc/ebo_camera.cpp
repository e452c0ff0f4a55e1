// ebo_camera.cpp — the camera-model entry points of include/ebo.h: common::CameraModel::unproject for many points
// (camera_model.h:79-114) and the rectification of a context's loaders; the kernels are in ebo_camera.inc.
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
	// a refused call leaves no rectification set
	c->rect_set = false;
	c->rect_lut.clear();
	if (!std::isfinite(cam->fx) || !std::isfinite(cam->fy) || cam->fx == 0.0 || cam->fy == 0.0)
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
	if (launch_rectify_map(consts_of(cam), c->prm.image_w, c->prm.image_h, c->d_rect_map, c->d_rect_lut, c->d_rect_bad, c->stream))
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
	c->rect_set = true;
	return EBO_OK;
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
