// ebo_maptrack.cpp — the map-tracking entry points of include/ebo.h ("pose from events against a map", E1-E9): many
// (image, start pose) units aligned to one list of world points in one launch, one workgroup per unit; the kernel is in
// ebo_maptrack.inc.  The host form uploads what it is given into the context's own buffer; the _device form only launches.
#include "ebo_ctx.h"

using namespace ebo;

// B4 on the host for ebo_map_track_starts: the rule functions of the kernel's own text, compiled here without contraction
namespace mt_host
{
#define EBO_MAPTRACK_RULES_ONLY
#include "ebo_maptrack.inc"
#undef EBO_MAPTRACK_RULES_ONLY
}  // namespace mt_host

namespace ebo_host
{
// ebo_rotation.cpp: B of every resident window into d_out ([Wn][h][w], device); omegas on the host (or null: zeros)
int event_images_resident(ebo_ctx* c, const char* entry, const ebo_camera* cam, const ebo_rotation_params* prm, const double* omegas,
						  double* d_out);
}

namespace
{
int track(ebo_ctx* c, const char* entry, const ebo_camera* cam, int w, int h, int nImages, const double* images, int nPoints,
		  const double* points, int nUnits, const int* unitImage, double* poses, double zMin, const ebo_solver_opts* opts,
		  ebo_map_track_result* results, double* trace, bool hostArrays, const double* dImages = nullptr)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	auto bad = [&](int code, const char* what) { return c->fail(code, std::string(entry) + ": " + what); };
	if (c->capturing)
	{
		return c->fail(EBO_ERR_STATE, kNotWhileRecording);
	}
	if (!cam || !opts)
	{
		return bad(EBO_ERR_ARG, "null camera or options");
	}
	if (nImages < 0 || nPoints < 0 || nUnits < 0 || nUnits > kMtMaxUnits || nPoints > kMtMaxPoints || opts->max_num_iterations < 0 ||
		opts->max_num_iterations > kMtMaxIterations)
	{
		return bad(EBO_ERR_ARG, "a negative count or iteration limit, more than 65535 units, 2^20 points or 10000 iterations");
	}
	if (w < 2 || h < 2 || !std::isfinite(zMin))
	{
		return bad(EBO_ERR_ARG, "an image narrower or lower than 2 pixels, or a z_min that is not finite");
	}
	if (cam->k1 != 0.0 || cam->k2 != 0.0 || cam->p1 != 0.0 || cam->p2 != 0.0)
	{
		return bad(EBO_ERR_ARG, "the camera has distortion (rule C1): pass the rectified camera");
	}
	if (!std::isfinite(cam->fx) || !std::isfinite(cam->fy) || cam->fx == 0.0 || cam->fy == 0.0)
	{
		return bad(EBO_ERR_RANGE, "fx or fy is zero or not finite");
	}
	if (nUnits == 0)
	{
		return EBO_OK;
	}
	if (!unitImage || !poses || !results || (nImages && !images && !dImages) || (nPoints && !points))
	{
		return bad(EBO_ERR_ARG, "a needed pointer is null");
	}
	if (hostArrays)
	{
		for (int u = 0; u < nUnits; ++u)
		{
			if (unitImage[u] < 0 || unitImage[u] >= nImages)
			{
				return bad(EBO_ERR_ARG, "a unit's image index is out of range");
			}
		}
	}
	(void)hipSetDevice(c->prm.device);
	MtCall k{};
	k.fx = cam->fx;
	k.fy = cam->fy;
	k.cx = cam->cx;
	k.cy = cam->cy;
	k.z_min = zMin;
	k.w = w;
	k.h = h;
	k.n_images = nImages;
	k.n_points = nPoints;
	k.images = images;
	k.points = points;
	const size_t traceDoubles = static_cast<size_t>(nUnits) * (static_cast<size_t>(opts->max_num_iterations) + 1) * 4;
	if (!hostArrays)
	{
		if (launch_map_track(k, nUnits, unitImage, poses, *opts, results, trace, c->stream))
		{
			return c->hip(hipGetLastError(), "map-tracking kernel launch");
		}
		return EBO_OK;
	}
	const size_t imgBytes = dImages ? 0 : static_cast<size_t>(nImages) * w * h * sizeof(double);  // dImages: already on the device
	ScratchCarve cv;
	const size_t oImg = cv.take(imgBytes), oPts = cv.take(3 * static_cast<size_t>(nPoints) * sizeof(double));
	const size_t oUi = cv.take(nUnits * sizeof(int)), oPose = cv.take(12 * static_cast<size_t>(nUnits) * sizeof(double));
	const size_t oRes = cv.take(nUnits * sizeof(ebo_map_track_result));
	const size_t oTrace = trace ? cv.take(traceDoubles * sizeof(double)) : 0;
	int rc = c->grow(c->d_maptrack, cv.at, "hipMalloc map-tracking arrays");
	if (rc)
	{
		return rc;
	}
	char* base = static_cast<char*>(c->d_maptrack.get());
	hipError_t e = hipSuccess;
	auto up = [&](size_t off, const void* src, size_t bytes) {
		if (e == hipSuccess && bytes)
		{
			e = hipMemcpyAsync(base + off, src, bytes, hipMemcpyHostToDevice, c->stream);
		}
	};
	up(oImg, images, imgBytes);
	up(oPts, points, 3 * static_cast<size_t>(nPoints) * sizeof(double));
	up(oUi, unitImage, nUnits * sizeof(int));
	up(oPose, poses, 12 * static_cast<size_t>(nUnits) * sizeof(double));
	if (e != hipSuccess)
	{
		return c->hip(e, "map-tracking uploads");
	}
	k.images = dImages ? dImages : reinterpret_cast<const double*>(base + oImg);
	k.points = reinterpret_cast<const double*>(base + oPts);
	double* dTrace = trace ? reinterpret_cast<double*>(base + oTrace) : nullptr;
	if (launch_map_track(k, nUnits, reinterpret_cast<const int*>(base + oUi), reinterpret_cast<double*>(base + oPose), *opts,
						 reinterpret_cast<ebo_map_track_result*>(base + oRes), dTrace, c->stream))
	{
		return c->hip(hipGetLastError(), "map-tracking kernel launch");
	}
	auto down = [&](void* dst, size_t off, size_t bytes) {
		if (e == hipSuccess && bytes)
		{
			e = hipMemcpyAsync(dst, base + off, bytes, hipMemcpyDeviceToHost, c->stream);
		}
	};
	down(poses, oPose, 12 * static_cast<size_t>(nUnits) * sizeof(double));
	down(results, oRes, nUnits * sizeof(ebo_map_track_result));
	if (trace)
	{
		down(trace, oTrace, traceDoubles * sizeof(double));
	}
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	return c->hip(e, "map-tracking results");
}
}  // namespace

extern "C" {

void ebo_default_map_track_opts(ebo_solver_opts* o)
{
	if (o)
	{
		mt_default_opts(*o);
	}
}

int ebo_map_track(ebo_ctx* c, const ebo_camera* cam, int w, int h, int n_images, const double* images, int n_points, const double* points,
				  int n_units, const int* unit_image, double* poses, double z_min, const ebo_solver_opts* opts,
				  ebo_map_track_result* results, double* trace)
{
	return track(c, "ebo_map_track", cam, w, h, n_images, images, n_points, points, n_units, unit_image, poses, z_min, opts, results, trace,
				 true);
}

int ebo_map_track_device(ebo_ctx* c, const ebo_camera* cam, int w, int h, int n_images, const double* d_images, int n_points,
						 const double* d_points, int n_units, const int* d_unit_image, double* d_poses, double z_min,
						 const ebo_solver_opts* opts, ebo_map_track_result* d_results, double* d_trace)
{
	return track(c, "ebo_map_track_device", cam, w, h, n_images, d_images, n_points, d_points, n_units, d_unit_image, d_poses, z_min, opts,
				 d_results, d_trace, false);
}

void ebo_map_track_starts(const double* pose, double translation_step, double rotation_step, double* starts)
{
	if (!pose || !starts)
	{
		return;
	}
	std::copy(pose, pose + 12, starts);
	for (int a = 0; a < 6; ++a)
	{
		for (int sgn = 0; sgn < 2; ++sgn)
		{
			double ups[3] = {0.0, 0.0, 0.0}, om[3] = {0.0, 0.0, 0.0};
			const double v = (sgn ? -1.0 : 1.0) * (a < 3 ? translation_step : rotation_step);
			(a < 3 ? ups[a] : om[a - 3]) = v;
			mt_host::mt_retract(pose, ups, om, starts + 12 * (1 + 2 * a + sgn));
		}
	}
}

int ebo_map_track_resident(ebo_ctx* c, const ebo_camera* cam, const ebo_rotation_params* params, const double* omegas, int make_images,
						   int n_points, const double* points, int n_units, const int* unit_window, double* poses, double z_min,
						   const ebo_solver_opts* opts, ebo_map_track_result* results, double* trace)
{
	static const char* const entry = "ebo_map_track_resident";
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	if (c->capturing)
	{
		return c->fail(EBO_ERR_STATE, kNotWhileRecording);
	}
	const int w = c->prm.image_w, h = c->prm.image_h;
	if (make_images)
	{
		c->evimg_gen = 0;
		int rc = c->grow(c->d_evimg, static_cast<size_t>(std::max(c->n_windows, 1)) * w * h, "hipMalloc event images");
		rc = rc ? rc : event_images_resident(c, entry, cam, params, omegas, c->d_evimg.get());
		if (rc)
		{
			return rc;
		}
		c->evimg_gen = c->units_gen;
		c->evimg_windows = c->n_windows;
	}
	else if (c->evimg_gen == 0 || c->evimg_gen != c->units_gen)
	{
		return c->fail(EBO_ERR_STATE, std::string(entry) + ": no event images of the resident windows: call once with make_images set after every load");
	}
	return track(c, entry, cam, w, h, c->evimg_windows, nullptr, n_points, points, n_units, unit_window, poses, z_min, opts, results, trace,
				 true, c->d_evimg.get());
}

}  // extern "C"
