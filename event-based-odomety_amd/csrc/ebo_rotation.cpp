// ebo_rotation.cpp — the rotational contrast maximisation entry points of include/ebo.h ("angular velocity from events"):
// the objective and gradient of every resident window at one angular velocity each (ebo_eval_rotation), the vote image
// (ebo_rotation_image), the host solver object (ebo_rot_solver_*, rot_solver.h) and the lock-step solve that drives it
// (ebo_solve_rotation).  The kernels are in ebo_rotation.inc.  Compiled without contraction: V5's weights are made here.
#include "ebo_ctx.h"
#include "rot_solver.h"

using namespace ebo;

struct ebo_rot_solver
{
	RotSolver s;
	int live;
};

namespace
{
// what one chunk of `slots` windows needs, carved from ebo_ctx::d_rot
struct RotCarve
{
	size_t oX, oY, oZ, oB, oV, oMu, oG, bytes;
	RotCarve(int slots, int w, int h, int P)
	{
		ScratchCarve cv;
		const size_t img = static_cast<size_t>(slots) * w * h * sizeof(double);
		const size_t part = static_cast<size_t>(slots) * rot_blocks(w, h) * sizeof(double);
		oX = cv.take(img);
		oY = cv.take(img);
		oZ = cv.take(img);
		oB = cv.take(part);
		oV = cv.take(part);
		oMu = cv.take(static_cast<size_t>(slots) * sizeof(double));
		oG = cv.take(static_cast<size_t>(slots) * P * 3 * sizeof(double));
		bytes = cv.at;
	}
	RotScratch at(void* base) const
	{
		char* b = static_cast<char*>(base);
		RotScratch s;
		s.imgX = b + oX;
		s.imgY = reinterpret_cast<double*>(b + oY);
		s.imgZ = reinterpret_cast<double*>(b + oZ);
		s.partB = reinterpret_cast<double*>(b + oB);
		s.partV = reinterpret_cast<double*>(b + oV);
		s.mu = reinterpret_cast<double*>(b + oMu);
		s.partG = reinterpret_cast<double*>(b + oG);
		return s;
	}
};

// windows per chunk under the byte budget: at least 1, at most kRotChunkMax
int chunk_slots(const ebo_ctx* c, int n)
{
	const size_t budget = env_size("EBO_ROTATION_SCRATCH_MB", 256) << 20;
	const size_t one = RotCarve(1, c->prm.image_w, c->prm.image_h, c->P).bytes;
	const size_t fit = std::max<size_t>(1, budget / one);
	return static_cast<int>(std::min<size_t>(std::min<size_t>(fit, kRotChunkMax), static_cast<size_t>(std::max(n, 1))));
}

// state, camera (C1) and parameters of every entry; fills the kernels' constants
int prepare(ebo_ctx* c, const char* entry, const ebo_camera* cam, const ebo_rotation_params* prm, bool ptrsOk, RotConsts& k)
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
	if (!cam || !ptrsOk)
	{
		return bad(EBO_ERR_ARG, "a needed pointer is null");
	}
	const double sigma = prm ? prm->sigma_blur : 1.0;
	if (!(sigma >= 0.0) || !std::isfinite(sigma))
	{
		return bad(EBO_ERR_ARG, "sigma_blur is negative or not finite");
	}
	if (cam->k1 != 0.0 || cam->k2 != 0.0 || cam->p1 != 0.0 || cam->p2 != 0.0)
	{
		return bad(EBO_ERR_ARG, "the camera has distortion (rule C1): rectify the events at load and pass the rectified camera");
	}
	if (!std::isfinite(cam->fx) || !std::isfinite(cam->fy) || cam->fx == 0.0 || cam->fy == 0.0)
	{
		return bad(EBO_ERR_RANGE, "fx or fy is zero or not finite");
	}
	if (c->n_windows == 0)
	{
		return bad(EBO_ERR_STATE, "no window loaded");
	}
	if (c->custom_n)
	{
		return bad(EBO_ERR_STATE, "the units were loaded by ebo_set_patches: load windows with an ebo_set_window* loader");
	}
	(void)hipSetDevice(c->prm.device);
	k.fx = cam->fx;
	k.fy = cam->fy;
	k.cx = cam->cx;
	k.cy = cam->cy;
	k.w = c->prm.image_w;
	k.h = c->prm.image_h;
	k.upw = c->P + 1;
	k.P = c->P;
	k.tile = ab_size("EBO_ROTATION_TILE", 1) != 0 ? 1 : 0;  // read by the A/B build only (ab_env.h)
	k.reserved = 0;
	k.np = static_cast<double>(k.w) * static_cast<double>(k.h);
	k.two_over_np = 2.0 / k.np;
	// V5: exp(-d^2 / (2 sigma^2)), d = -3 .. 3, divided by their sum taken in that order
	if (sigma > 0.0)
	{
		double sum = 0.0;
		for (int d = -3; d <= 3; ++d)
		{
			k.g[d + 3] = std::exp(-static_cast<double>(d * d) / (2.0 * sigma * sigma));
			sum = sum + k.g[d + 3];
		}
		for (int i = 0; i < 7; ++i)
		{
			k.g[i] = k.g[i] / sum;
		}
	}
	else
	{
		for (int i = 0; i < 7; ++i)
		{
			k.g[i] = i == 3 ? 1.0 : 0.0;
		}
	}
	return EBO_OK;
}

// r (and g) of the listed windows (null: all resident windows), chunk by chunk, on device arrays indexed by window
int eval_windows(ebo_ctx* c, const RotConsts& k, const int* wins, int n, const double* d_omegas, double* d_r, double* d_g)
{
	const int slots = chunk_slots(c, n);
	const RotCarve cv(slots, k.w, k.h, k.P);
	int rc = c->grow(c->d_rot, cv.bytes, "hipMalloc rotation scratch");
	if (rc)
	{
		return rc;
	}
	const RotScratch s = cv.at(c->d_rot.get());
	for (int at = 0; at < n; at += slots)
	{
		RotWindows L;
		L.n = std::min(slots, n - at);
		for (int i = 0; i < L.n; ++i)
		{
			L.win[i] = wins ? wins[at + i] : at + i;
		}
		if (launch_rot_eval(c->d_events, c->d_units, L, k, d_omegas, s, d_r, d_g, c->stream))
		{
			return c->hip(hipGetLastError(), "rotation evaluation kernel launch");
		}
	}
	return EBO_OK;
}

// the host entries' device arrays: omegas [Wn][3] | r [Wn] | g [Wn][3]
int grow_io(ebo_ctx* c, double*& dOm, double*& dR, double*& dG)
{
	const size_t Wn = static_cast<size_t>(c->n_windows);
	const int rc = c->grow(c->d_rot_io, 7 * Wn, "hipMalloc rotation arrays");
	if (rc)
	{
		return rc;
	}
	dOm = c->d_rot_io.get();
	dR = dOm + 3 * Wn;
	dG = dR + Wn;
	return EBO_OK;
}
}  // namespace

extern "C" {

void ebo_default_rotation_params(ebo_rotation_params* p)
{
	if (p)
	{
		p->sigma_blur = 1.0;
		p->reserved = 0.0;
	}
}

void ebo_default_rot_solver_opts(ebo_rot_solver_opts* o)
{
	if (o)
	{
		o->first_rate = 0.5;
		o->c1 = 1e-4;
		o->step_tol = 1e-4;
		o->max_backtracks = 20;
		o->max_iterations = 100;
	}
}

int ebo_eval_rotation(ebo_ctx* c, const ebo_camera* cam, const ebo_rotation_params* prm, const double* omegas, double* r, double* g)
{
	RotConsts k;
	int rc = prepare(c, "ebo_eval_rotation", cam, prm, omegas && r, k);
	if (rc)
	{
		return rc;
	}
	double *dOm, *dR, *dG;
	rc = grow_io(c, dOm, dR, dG);
	if (rc)
	{
		return rc;
	}
	const size_t Wn = static_cast<size_t>(c->n_windows);
	rc = c->hip(hipMemcpyAsync(dOm, omegas, 3 * Wn * sizeof(double), hipMemcpyHostToDevice, c->stream), "H2D omegas");
	if (rc)
	{
		return rc;
	}
	rc = eval_windows(c, k, nullptr, c->n_windows, dOm, dR, g ? dG : nullptr);
	if (rc)
	{
		return rc;
	}
	hipError_t e = hipMemcpyAsync(r, dR, Wn * sizeof(double), hipMemcpyDeviceToHost, c->stream);
	if (e == hipSuccess && g)
	{
		e = hipMemcpyAsync(g, dG, 3 * Wn * sizeof(double), hipMemcpyDeviceToHost, c->stream);
	}
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	return c->hip(e, "rotation evaluation results");
}

int ebo_eval_rotation_device(ebo_ctx* c, const ebo_camera* cam, const ebo_rotation_params* prm, const double* d_omegas, double* d_r,
							 double* d_g)
{
	RotConsts k;
	const int rc = prepare(c, "ebo_eval_rotation_device", cam, prm, d_omegas && d_r, k);
	if (rc)
	{
		return rc;
	}
	return eval_windows(c, k, nullptr, c->n_windows, d_omegas, d_r, d_g);
}

int ebo_rotation_image(ebo_ctx* c, const ebo_camera* cam, const double* omegas, int64_t* votes, double* image)
{
	RotConsts k;
	int rc = prepare(c, "ebo_rotation_image", cam, nullptr, omegas != nullptr, k);
	if (rc)
	{
		return rc;
	}
	double *dOm, *dR, *dG;
	rc = grow_io(c, dOm, dR, dG);
	if (rc)
	{
		return rc;
	}
	const size_t Wn = static_cast<size_t>(c->n_windows), np = static_cast<size_t>(k.w) * k.h;
	const int slots = chunk_slots(c, c->n_windows);
	const RotCarve cv(slots, k.w, k.h, k.P);
	rc = c->grow(c->d_rot, cv.bytes, "hipMalloc rotation scratch");
	if (rc)
	{
		return rc;
	}
	const RotScratch s = cv.at(c->d_rot.get());
	hipError_t e = hipMemcpyAsync(dOm, omegas, 3 * Wn * sizeof(double), hipMemcpyHostToDevice, c->stream);
	for (int at = 0; at < c->n_windows && e == hipSuccess; at += slots)
	{
		RotWindows L;
		L.n = std::min(slots, c->n_windows - at);
		for (int i = 0; i < L.n; ++i)
		{
			L.win[i] = at + i;
		}
		if (launch_rot_votes(c->d_events, c->d_units, L, k, dOm, s, image ? s.imgY : nullptr, c->stream))
		{
			return c->hip(hipGetLastError(), "rotation vote kernel launch");
		}
		const size_t n = static_cast<size_t>(L.n) * np;
		if (votes)
		{
			e = hipMemcpyAsync(votes + at * np, s.imgX, n * sizeof(int64_t), hipMemcpyDeviceToHost, c->stream);
		}
		if (e == hipSuccess && image)
		{
			e = hipMemcpyAsync(image + at * np, s.imgY, n * sizeof(double), hipMemcpyDeviceToHost, c->stream);
		}
	}
	if (e == hipSuccess)
	{
		e = hipStreamSynchronize(c->stream);
	}
	return c->hip(e, "rotation image");
}

// B of every resident window, chunk by chunk: to dB ([Wn][h][w], device) or, with hostArrays through the chunk's
// third image to the host array
static int event_images(ebo_ctx* c, const char* entry, const ebo_camera* cam, const ebo_rotation_params* prm, const double* omegas,
						bool hostArrays, double* out, bool hostOmegas)
{
	RotConsts k;
	int rc = prepare(c, entry, cam, prm, out != nullptr, k);
	if (rc)
	{
		return rc;
	}
	const size_t Wn = static_cast<size_t>(c->n_windows), np = static_cast<size_t>(k.w) * k.h;
	const double* dOm = omegas;
	if (!omegas || hostOmegas)
	{
		rc = c->grow(c->d_evimg_om, 3 * Wn, "hipMalloc event-image omegas");
		if (rc)
		{
			return rc;
		}
		const hipError_t e = omegas ? hipMemcpyAsync(c->d_evimg_om.get(), omegas, 3 * Wn * sizeof(double), hipMemcpyHostToDevice, c->stream)
									: hipMemsetAsync(c->d_evimg_om.get(), 0, 3 * Wn * sizeof(double), c->stream);
		if (e != hipSuccess)
		{
			return c->hip(e, "event-image omegas");
		}
		dOm = c->d_evimg_om.get();
	}
	const int slots = chunk_slots(c, c->n_windows);
	const RotCarve cv(slots, k.w, k.h, k.P);
	rc = c->grow(c->d_rot, cv.bytes, "hipMalloc rotation scratch");
	if (rc)
	{
		return rc;
	}
	const RotScratch s = cv.at(c->d_rot.get());
	hipError_t e = hipSuccess;
	for (int at = 0; at < c->n_windows && e == hipSuccess; at += slots)
	{
		RotWindows L;
		L.n = std::min(slots, c->n_windows - at);
		for (int i = 0; i < L.n; ++i)
		{
			L.win[i] = at + i;
		}
		if (launch_rot_images(c->d_events, c->d_units, L, k, dOm, s, hostArrays ? s.imgZ : out + at * np, c->stream))
		{
			return c->hip(hipGetLastError(), "event-image kernel launch");
		}
		if (hostArrays)
		{
			e = hipMemcpyAsync(out + at * np, s.imgZ, static_cast<size_t>(L.n) * np * sizeof(double), hipMemcpyDeviceToHost, c->stream);
		}
	}
	if (e == hipSuccess && hostArrays)
	{
		e = hipStreamSynchronize(c->stream);
	}
	return c->hip(e, "event images");
}

int ebo_event_images(ebo_ctx* c, const ebo_camera* cam, const ebo_rotation_params* prm, const double* omegas, double* images)
{
	return event_images(c, "ebo_event_images", cam, prm, omegas, true, images, true);
}

int ebo_event_images_device(ebo_ctx* c, const ebo_camera* cam, const ebo_rotation_params* prm, const double* d_omegas, double* d_images)
{
	return event_images(c, "ebo_event_images_device", cam, prm, d_omegas, false, d_images, false);
}

}  // extern "C"

namespace ebo_host
{
// for ebo_map_track_resident (ebo_maptrack.cpp): the omegas on the host, the images left on the device
int event_images_resident(ebo_ctx* c, const char* entry, const ebo_camera* cam, const ebo_rotation_params* prm, const double* omegas,
						  double* d_out)
{
	return event_images(c, entry, cam, prm, omegas, false, d_out, true);
}
}  // namespace ebo_host

extern "C" {

int ebo_rot_solver_create(int n, const ebo_rot_solver_opts* opts, const double* omega0, ebo_rot_solver** out)
{
	if (n < 1 || !opts || !out || !RotSolver::optsOk(*opts))
	{
		return EBO_ERR_ARG;
	}
	*out = new ebo_rot_solver{RotSolver(n, *opts, omega0), n};
	return EBO_OK;
}

int ebo_rot_solver_request(ebo_rot_solver* s, double* omegas, uint8_t* live)
{
	if (!s || !omegas)
	{
		return EBO_ERR_ARG;
	}
	s->live = s->s.request(omegas, live);
	return s->live;
}

int ebo_rot_solver_supply(ebo_rot_solver* s, const double* r, const double* g)
{
	if (!s || !r || !g)
	{
		return EBO_ERR_ARG;
	}
	if (s->live == 0)
	{
		return EBO_ERR_STATE;
	}
	s->s.supply(r, g);
	return EBO_OK;
}

int ebo_rot_solver_result(const ebo_rot_solver* s, double* omegas, ebo_rot_summary* summary)
{
	if (!s)
	{
		return EBO_ERR_ARG;
	}
	s->s.result(omegas, summary);
	return EBO_OK;
}

void ebo_rot_solver_destroy(ebo_rot_solver* s)
{
	delete s;
}

int ebo_solve_rotation(ebo_ctx* c, const ebo_camera* cam, const ebo_rotation_params* prm, const ebo_rot_solver_opts* opts,
					   const double* omega0, double* omega_out, ebo_rot_summary* summary)
{
	RotConsts k;
	int rc = prepare(c, "ebo_solve_rotation", cam, prm, omega_out != nullptr, k);
	if (rc)
	{
		return rc;
	}
	ebo_rot_solver_opts o;
	ebo_default_rot_solver_opts(&o);
	if (opts)
	{
		o = *opts;
	}
	if (!RotSolver::optsOk(o))
	{
		return c->fail(EBO_ERR_ARG, "ebo_solve_rotation: solver options outside their ranges");
	}
	double *dOm, *dR, *dG;
	rc = grow_io(c, dOm, dR, dG);
	if (rc)
	{
		return rc;
	}
	const int Wn = c->n_windows;
	RotSolver solver(Wn, o, omega0);
	std::vector<double> om(3 * static_cast<size_t>(Wn)), res(4 * static_cast<size_t>(Wn), 0.0);
	std::vector<uint8_t> live(static_cast<size_t>(Wn));
	std::vector<int> wins;
	// lock-step rounds: the windows still waiting, and only they, are evaluated in one batched pass
	while (solver.request(om.data(), live.data()) > 0)
	{
		wins.clear();
		for (int w = 0; w < Wn; ++w)
		{
			if (live[w])
			{
				wins.push_back(w);
			}
		}
		rc = c->hip(hipMemcpyAsync(dOm, om.data(), om.size() * sizeof(double), hipMemcpyHostToDevice, c->stream), "H2D omegas");
		if (rc)
		{
			return rc;
		}
		rc = eval_windows(c, k, wins.data(), static_cast<int>(wins.size()), dOm, dR, dG);
		if (rc)
		{
			return rc;
		}
		// r [Wn] and g [Wn][3] lie side by side
		hipError_t e = hipMemcpyAsync(res.data(), dR, res.size() * sizeof(double), hipMemcpyDeviceToHost, c->stream);
		if (e == hipSuccess)
		{
			e = hipStreamSynchronize(c->stream);
		}
		if (e != hipSuccess)
		{
			return c->hip(e, "rotation solve results");
		}
		solver.supply(res.data(), res.data() + Wn);
	}
	solver.result(omega_out, summary);
	return EBO_OK;
}

}  // extern "C"
