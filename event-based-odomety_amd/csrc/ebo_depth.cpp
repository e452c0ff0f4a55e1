// ebo_depth.cpp — the space-sweep depth map's entry points of include/ebo.h ("depth from events", rules M1-M9): the
// volume's life (ebo_dsi_begin / _end), the votes of the resident windows (ebo_dsi_add_windows), the volume and the
// extraction (ebo_dsi_volume, ebo_dsi_depth).  The kernels are in ebo_depth.inc.  Compiled without contraction: M1's
// table and M2's relative poses are made here.
#include "ebo_ctx.h"

using namespace ebo;

namespace
{
// what the extraction needs, carved from ebo_ctx::d_dsi_x
struct DsiCarve
{
	size_t oConf, oKbest, oIndex, oDepth, oCount, oKeep, oPoints, bytes;
	DsiCarve(int w, int h, int max_points)
	{
		ScratchCarve cv;
		const size_t np = static_cast<size_t>(w) * h;
		oDepth = cv.take(np * sizeof(double));
		oPoints = cv.take(static_cast<size_t>(max_points) * 3 * sizeof(double));
		oConf = cv.take(np * sizeof(uint32_t));
		oKbest = cv.take(np * sizeof(int));
		oIndex = cv.take(np * sizeof(int));
		oCount = cv.take((static_cast<size_t>(dsi_blocks(w, h)) + 1) * sizeof(int));
		oKeep = cv.take(np);
		bytes = cv.at;
	}
	DsiScratch at(void* base, bool wantPoints) const
	{
		char* b = static_cast<char*>(base);
		DsiScratch s;
		s.conf = reinterpret_cast<uint32_t*>(b + oConf);
		s.kbest = reinterpret_cast<int*>(b + oKbest);
		s.index = reinterpret_cast<int*>(b + oIndex);
		s.depth = reinterpret_cast<double*>(b + oDepth);
		s.blockCount = reinterpret_cast<int*>(b + oCount);
		s.keep = reinterpret_cast<unsigned char*>(b + oKeep);
		s.points = wantPoints ? reinterpret_cast<double*>(b + oPoints) : nullptr;
		return s;
	}
};

// how every entry but begin starts: a context, no recording, its pointers, an open volume
int enter_open(ebo_ctx* c, const char* entry, bool ptrsOk)
{
	const int rc = enter(c, (std::string(entry) + ": a needed pointer is null or max_points is negative").c_str(), ptrsOk);
	if (rc)
	{
		return rc;
	}
	if (!c->dsi_live)
	{
		return c->fail(EBO_ERR_STATE, std::string(entry) + ": no volume is open (ebo_dsi_begin)");
	}
	return EBO_OK;
}

// M2's relative pose of a window against the reference pose
DsiPose relative_pose(const double* ref, const double* win)
{
	DsiPose p;
	for (int i = 0; i < 3; ++i)
	{
		for (int j = 0; j < 3; ++j)
		{
			p.Rr[3 * i + j] = (ref[i] * win[j] + ref[3 + i] * win[3 + j]) + ref[6 + i] * win[6 + j];
		}
	}
	const double e0 = win[9] - ref[9], e1 = win[10] - ref[10], e2 = win[11] - ref[11];
	for (int i = 0; i < 3; ++i)
	{
		p.tr[i] = (ref[i] * e0 + ref[3 + i] * e1) + ref[6 + i] * e2;
	}
	return p;
}

// planes per workgroup of the vote: one workgroup walks all planes when (patch, window) pairs alone fill the device
// four times over, otherwise the planes are dealt into chunks until they do.  The A/B build's EBO_DSI_PLANES forces it.
int planes_per_group(const ebo_ctx* c, int pairs, int nz)
{
	const int forced = static_cast<int>(ab_size("EBO_DSI_PLANES", 0));
	if (forced > 0)
	{
		return std::min(forced, nz);
	}
	const int want = 4 * (c->n_cus > 0 ? c->n_cus : 256);
	const int chunks = std::min(nz, std::max(1, (want + pairs - 1) / std::max(pairs, 1)));
	return (nz + chunks - 1) / chunks;
}
}  // namespace

extern "C" {

void ebo_default_depth_params(ebo_depth_params* p)
{
	if (p)
	{
		p->nz = 64;
		p->box_radius = 2;
		p->median_radius = 2;
		p->reserved = 0;
		p->z_near = 0.5;
		p->z_far = 8.0;
		p->min_excess = 3.0;
	}
}

int ebo_dsi_begin(ebo_ctx* c, const ebo_camera* cam, const double* ref_pose, const ebo_depth_params* params)
{
	int rc = enter(c, "ebo_dsi_begin: a needed pointer is null", cam && ref_pose);
	if (rc)
	{
		return rc;
	}
	auto bad = [&](int code, const char* what) { return c->fail(code, std::string("ebo_dsi_begin: ") + what); };
	ebo_depth_params prm;
	ebo_default_depth_params(&prm);
	if (params)
	{
		prm = *params;
	}
	if (prm.nz < 2 || prm.nz > kDsiMaxPlanes)
	{
		return bad(EBO_ERR_ARG, "nz outside 2 .. 256");
	}
	if (!std::isfinite(prm.z_near) || !std::isfinite(prm.z_far) || !(prm.z_near > 0.0) || !(prm.z_near < prm.z_far))
	{
		return bad(EBO_ERR_ARG, "z_near and z_far must be finite with 0 < z_near < z_far");
	}
	if (prm.box_radius < 0 || prm.box_radius > kDsiMaxRadius || prm.median_radius < 0 || prm.median_radius > kDsiMaxRadius)
	{
		return bad(EBO_ERR_ARG, "box_radius or median_radius outside 0 .. 7");
	}
	if (!std::isfinite(prm.min_excess) || !(prm.min_excess >= 0.0))
	{
		return bad(EBO_ERR_ARG, "min_excess is negative or not finite");
	}
	if (cam->k1 != 0.0 || cam->k2 != 0.0 || cam->p1 != 0.0 || cam->p2 != 0.0)
	{
		return bad(EBO_ERR_ARG, "the camera has distortion (rule C1): rectify the events at load and pass the rectified camera");
	}
	if (!std::isfinite(cam->fx) || !std::isfinite(cam->fy) || cam->fx == 0.0 || cam->fy == 0.0)
	{
		return bad(EBO_ERR_RANGE, "fx or fy is zero or not finite");
	}
	c->dsi_live = false;
	DsiConsts& k = c->dsi_k;
	k.fx = cam->fx;
	k.fy = cam->fy;
	k.cx = cam->cx;
	k.cy = cam->cy;
	k.w = c->prm.image_w;
	k.h = c->prm.image_h;
	k.upw = c->P + 1;
	k.nz = prm.nz;
	k.planes = prm.nz;
	k.tile = ab_size("EBO_DSI_TILE", 1) != 0 ? 1 : 0;  // read by the A/B build only (ab_env.h)
	// M1
	c->dsi_z.resize(static_cast<size_t>(prm.nz));
	const double rho0 = 1.0 / prm.z_near;
	const double drho = (1.0 / prm.z_far - rho0) / static_cast<double>(prm.nz - 1);
	for (int i = 0; i < prm.nz; ++i)
	{
		const double rho = rho0 + static_cast<double>(i) * drho;
		c->dsi_z[static_cast<size_t>(i)] = 1.0 / rho;
	}
	const size_t vox = static_cast<size_t>(prm.nz) * k.w * k.h;
	rc = c->grow(c->d_dsi, vox, "hipMalloc depth volume");
	if (rc == EBO_OK)
	{
		rc = c->grow(c->d_dsi_z, static_cast<size_t>(kDsiMaxPlanes), "hipMalloc depth planes");
	}
	if (rc)
	{
		return rc;
	}
	hipError_t e = hipMemsetAsync(c->d_dsi.get(), 0, vox * sizeof(uint32_t), c->stream);
	if (e == hipSuccess)
	{
		e = hipMemcpyAsync(c->d_dsi_z.get(), c->dsi_z.data(), c->dsi_z.size() * sizeof(double), hipMemcpyHostToDevice, c->stream);
	}
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);  // dsi_z is pageable: the copy has left it
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "depth volume clear");
	}
	c->dsi_prm = prm;
	std::memcpy(c->dsi_ref, ref_pose, sizeof(c->dsi_ref));
	c->dsi_events = 0;
	c->dsi_live = true;
	return EBO_OK;
}

int ebo_dsi_add_windows(ebo_ctx* c, const double* poses, const uint8_t* use)
{
	int rc = enter_open(c, "ebo_dsi_add_windows", poses != nullptr);
	if (rc)
	{
		return rc;
	}
	if (c->n_windows == 0)
	{
		return c->fail(EBO_ERR_STATE, "ebo_dsi_add_windows: no window loaded");
	}
	if (c->custom_n)
	{
		return c->fail(EBO_ERR_STATE,
					   "ebo_dsi_add_windows: the units were loaded by ebo_set_patches: load windows with an ebo_set_window* loader");
	}
	const int Wn = c->n_windows, P = c->P;
	std::vector<int> wins;
	uint64_t events = 0;
	for (int w = 0; w < Wn; ++w)
	{
		if (use && !use[w])
		{
			continue;
		}
		wins.push_back(w);
		for (int p = 0; p < P; ++p)
		{
			events += c->units[static_cast<size_t>(w) * (P + 1) + p].n_ev;
		}
	}
	if (c->dsi_events + events > kDsiMaxEvents)
	{
		return c->fail(EBO_ERR_RANGE, "ebo_dsi_add_windows: the volume would hold more than 2^21 events (rule M4); nothing was voted");
	}
	if (wins.empty())
	{
		return EBO_OK;
	}
	std::vector<DsiPose> rel(static_cast<size_t>(Wn));
	for (const int w : wins)
	{
		rel[static_cast<size_t>(w)] = relative_pose(c->dsi_ref, poses + 12 * static_cast<size_t>(w));
	}
	rc = c->grow(c->d_dsi_pose, static_cast<size_t>(Wn), "hipMalloc depth poses");
	if (rc)
	{
		return rc;
	}
	hipError_t e = hipMemcpyAsync(c->d_dsi_pose.get(), rel.data(), rel.size() * sizeof(DsiPose), hipMemcpyHostToDevice, c->stream);
	if (e != hipSuccess)
	{
		return c->hip(e, "H2D depth poses");
	}
	const int n = static_cast<int>(wins.size());
	for (int at = 0; at < n; at += kDsiChunkMax)
	{
		DsiWindows L;
		L.n = std::min(kDsiChunkMax, n - at);
		for (int i = 0; i < L.n; ++i)
		{
			L.win[i] = wins[static_cast<size_t>(at + i)];
		}
		DsiConsts k = c->dsi_k;
		k.planes = planes_per_group(c, P * L.n, k.nz);
		if (launch_dsi_vote(c->d_events, c->d_units, P, L, k, c->d_dsi_pose.get(), c->d_dsi_z.get(), c->d_dsi.get(), c->stream))
		{
			return c->hip(hipGetLastError(), "depth vote kernel launch");
		}
	}
	rc = c->hip(hipStreamSynchronize(c->stream), "depth votes");  // rel is pageable; and the next load may replace the events
	if (rc)
	{
		return rc;
	}
	c->dsi_events += events;
	return EBO_OK;
}

int ebo_dsi_volume(ebo_ctx* c, uint32_t* out)
{
	const int rc = enter_open(c, "ebo_dsi_volume", out != nullptr);
	if (rc)
	{
		return rc;
	}
	const size_t vox = static_cast<size_t>(c->dsi_k.nz) * c->dsi_k.w * c->dsi_k.h;
	hipError_t e = hipMemcpyAsync(out, c->d_dsi.get(), vox * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	return c->hip(e, "depth volume");
}

int ebo_dsi_depth(ebo_ctx* c, int32_t* index, uint32_t* conf, double* depth, double* points, int max_points, int* n_points_out)
{
	int rc = enter_open(c, "ebo_dsi_depth", max_points >= 0 && (points || max_points == 0));
	if (rc)
	{
		return rc;
	}
	const DsiConsts& k = c->dsi_k;
	const size_t np = static_cast<size_t>(k.w) * k.h;
	const int cap = static_cast<int>(std::min<size_t>(static_cast<size_t>(max_points), np));  // no more pixels than that can be kept
	const DsiCarve cv(k.w, k.h, cap);
	rc = c->grow(c->d_dsi_x, cv.bytes, "hipMalloc depth extraction");
	if (rc)
	{
		return rc;
	}
	const DsiScratch s = cv.at(c->d_dsi_x.get(), cap > 0);
	// M6's offset; beyond 2^22 votes nothing is kept either way
	const long long off = static_cast<long long>(std::rint(std::min(c->dsi_prm.min_excess, 4194304.0) * 1024.0));
	if (launch_dsi_extract(k, c->dsi_prm.box_radius, off, c->dsi_prm.median_radius, c->d_dsi_z.get(), c->d_dsi.get(), s, cap, c->stream))
	{
		return c->hip(hipGetLastError(), "depth extraction kernel launch");
	}
	int kept = 0;
	hipError_t e = hipMemcpyAsync(&kept, s.blockCount + dsi_blocks(k.w, k.h), sizeof(int), hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess && index)
	{
		e = hipMemcpyAsync(index, s.index, np * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess && conf)
	{
		e = hipMemcpyAsync(conf, s.conf, np * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess && depth)
	{
		e = hipMemcpyAsync(depth, s.depth, np * sizeof(double), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	if (e == hipSuccess && cap > 0 && kept > 0)
	{
		e = hipMemcpy(points, s.points, static_cast<size_t>(std::min(kept, cap)) * 3 * sizeof(double), hipMemcpyDeviceToHost);
	}
	if (e != hipSuccess)
	{
		return c->hip(e, "depth extraction results");
	}
	if (n_points_out)
	{
		*n_points_out = kept;
	}
	return EBO_OK;
}

int ebo_dsi_end(ebo_ctx* c)
{
	const int rc = enter_open(c, "ebo_dsi_end", true);
	if (rc)
	{
		return rc;
	}
	c->dsi_live = false;
	return EBO_OK;
}

}  // extern "C"
