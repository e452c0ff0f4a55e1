// ebo_ctx.h — private to the host side of libebo_hip.so: the context behind the opaque ebo_ctx
// of include/ebo.h and the few helpers its translation units share (ebo_api.cpp: context, windows,
// evaluation, solves, count images; ebo_windows.cpp: loading events; ebo_tracker.cpp: tracked patches; ebo_motion_field.cpp;
// ebo_io.cpp; ebo_comm.cpp).
#pragma once

#include <hip/hip_runtime.h>
#include <dlfcn.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include <chrono>
#include <condition_variable>
#include <functional>
#include <mutex>
#include <thread>

#include "../../include/ebo.h"
#include "box_extents.h"
#include "dev_buf.h"
#include "ebo_internal.h"
#include "field_tv.h"
#include "host_lm.h"

using namespace ebo;

namespace ebo_host
{
inline size_t env_size(const char* name, size_t dflt)
{
	const char* v = std::getenv(name);
	if (!v || !*v)
	{
		return dflt;
	}
	return static_cast<size_t>(std::strtoull(v, nullptr, 10));
}

struct WindowInfo
{
	int64_t t_ref;
	uint64_t n_events;
};

// host memory that kernels read and write directly: mapped into the device's address space and
// coherent (fine-grained), whatever HIP_HOST_COHERENT says
constexpr unsigned int kZeroCopyFlags = hipHostMallocMapped | hipHostMallocCoherent;

// The two memory policies of DevBuf (dev_buf.h): the only callers of the HIP allocation functions in the host
// sources.  A failed allocation returns nullptr and leaves its code to hipGetLastError (ebo_ctx::grow reports it).
struct DeviceMem
{
	static void* allocate(size_t bytes)
	{
		void* p = nullptr;
		return hipMalloc(&p, bytes) == hipSuccess ? p : nullptr;
	}
	static void release(void* p) { (void)hipFree(p); }
};
template <unsigned int Flags>
struct PinnedMem
{
	static void* allocate(size_t bytes)
	{
		void* p = nullptr;
		return hipHostMalloc(&p, bytes, Flags) == hipSuccess ? p : nullptr;
	}
	static void release(void* p) { (void)hipHostFree(p); }
};
template <class T>
using Dev = ebo::DevBuf<T, DeviceMem>;
template <class T, unsigned int Flags = kZeroCopyFlags>
using Pinned = ebo::DevBuf<T, PinnedMem<Flags>>;

inline size_t align256(size_t v)
{
	return (v + 255) & ~static_cast<size_t>(255);
}

// a bump allocator over the context's scratch buffer: take() gives offsets for ebo_ctx::scratch<T>(), `at` is the size to grow to
struct ScratchCarve
{
	size_t at = 0;
	size_t take(size_t bytes)
	{
		const size_t o = at;
		at = align256(at + bytes);
		return o;
	}
};
}  // namespace ebo_host
using namespace ebo_host;

struct ebo_ctx
{
	ebo_params prm;
	int npx = 0, npy = 0, P = 0;
	hipStream_t stream = nullptr;
	bool own_stream = false;
	bool capturing = false;  // between ebo_graph_begin and ebo_graph_end
	std::string err;

	size_t cap_events = 0;
	int cap_windows = 0;
	int n_windows = 0;

	Dev<uint64_t> d_events;
	Dev<Unit> d_units;
	Dev<uint32_t> d_order;  // [units] the order in which a launch hands them to workgroups, heaviest first (launch_order.h); rewritten by every load
	Dev<int32_t> d_unit_ext;  // [units][kExtStride] per-column / per-row time extents behind k_eval3's bounding box (box_extents.h); sized once by ebo_create, rewritten by every load
	Dev<unsigned int> d_box_stats;  // A/B build only: [kBoxStatInts] units whose box came from the event pass / from the table, and (64 counters) units that took the all-interior path, in the last variance evaluation
	Dev<uint32_t> d_deal_dump;  // A/B build only: [1 + events of a unit] ebo_unit_deal's read-back of one unit's dealt list
	int deal_dump_unit = -1;    // the unit the next variance evaluation dumps (inside ebo_unit_deal only)
	Dev<int32_t> d_unit_maxdt;  // [units] max |t_ref(window) - t| over the unit's events (count kernels' displacement bound)
	Dev<double> d_flows;
	Dev<double> d_out;
	Dev<double> d_partials;
	Dev<int32_t> d_counts;
	Dev<double> d_image;
	Dev<void> d_aux;
	Dev<unsigned char> d_modes;  // per-flow-slot evaluation modes of a lock-step solve
	const unsigned char* modes_active = nullptr;  // non-null only inside eval_host(modes)
	LiveWindows live_active;                      // n > 0 only inside a compact round of a pipelined lock-step solve
	Dev<double2> d_opt_grid;  // Optimizer::setGrad's interleaved gradient grid [H][W]
	bool opt_grid_valid = false;
	Dev<void> d_opt;  // scratch of ebo_optimizer_eval / _solve
	Dev<unsigned int> d_count_sorted;  // k_csort_*: destination list (two halves); sized by the plan of the largest call
	Dev<unsigned int> d_count_bins;  // k_csort_*: counts, starts, cursors per (window, band)
	Dev<int32_t> d_stats;
	Dev<void> d_scratch;  // patch-integrate staging
	Dev<double> d_edge_w;  // the 49 tensor weights of the edge loss (device table)
	double edge_w_sigma = -1.0;      // sigma_st they were built for
	unsigned long long* edge_stats_dev = nullptr;  // set only while ebo_edge_work_stats runs its one evaluation
	Dev<double> d_edge_cs;  // eigenvector directions of the edge loss's eigenvalue pass, [workgroup slot][cap_px][2]
	int n_cus = 0;                   // compute units of the device
	// the compact path's per-launch tables in one allocation: int length (+ 3 ints of padding) | int list[items] (the
	// units whose arrays do not fit the compact layout) | int4 bbox[items] (k_edge_classify's tap bounding boxes)
	Dev<int> d_edge_defer;
	Dev<void> d_edge_scratch;  // edge-loss fallback arrays
	Dev<void> d_field;  // motion field of ebo_init_motion_field (+ its staging)
	bool field_valid = false;
	const int* d_field_fixed = nullptr;  // fixed points of that field, [field_nfixed][2]
	int field_nfixed = 0;
	Dev<void> d_tvf;  // workspace of ebo_interpolate_motion_field
	Dev<double> d_fe_lut;  // image front end: the 256 log-image values of ebo_image_gradients
	Dev<void> d_fe;  // its per-call workspace (image, mask, outputs, Harris response, candidate lists)
	Dev<char> d_fe_pyr[2];  // pyramids + derivatives of the last two ebo_lk_add_image images
	Dev<FeLevel> d_fe_lv;  // their level table (both have the image's shape)
	std::vector<FeLevel> fe_lv;
	int fe_newer = 0;                // slot of the newer image
	int fe_images = 0;               // images added, up to 2
	Dev<void> d_fe_pts;  // ebo_lk_track's points, status and errors
	void* comm = nullptr;            // ncclComm_t of ebo_comm_init
	int comm_rank = 0, comm_size = 1;
	Dev<uint64_t> d_comm_cnt;  // [nranks + 2] counts / flags of the exchange (allocated by ebo_comm_init)
	Pinned<uint64_t, hipHostMallocDefault> pin_comm;  // the same, pinned host side
	Dev<void> d_comm_buf;  // track exchange buffer; grown collectively (ebo_comm.cpp: ensure_comm_buf)
	Dev<void> d_raw;  // raw 24-byte (or compact 8-byte) events staged for device bucketing
	hipStream_t copy_stream = nullptr;  // uploads of ebo_set_windows / ebo_set_windows8, overlapped with the bucketing
	hipEvent_t copy_done[8] = {};
	hipEvent_t order_done = nullptr;  // behind the device path's upload of d_order, which the load does not wait for (ebo_windows.cpp)
	Dev<void> d_bucket;  // bucketing scratch
	Dev<unsigned int> d_chunk_hist;  // per-chunk bucket histograms / first ranks of the stable scatter
	// ebo_set_rectification (ebo_camera.cpp): the sensor's rectification table and map; rect_set selects the
	// Rectified<> bucketing kernels for the NEXT load
	Dev<void> d_rect_lut;  // int16 [image_h][image_w][2]
	Dev<double> d_rect_map;  // double [image_h][image_w][2]
	Dev<int> d_rect_bad;  // k_rectify_map's error bits
	std::vector<int16_t> rect_lut;   // host copy for the host counting sort, fetched on its first use
	bool rect_set = false;
	ebo_camera rect_cam = {}, rect_out = {};  // the (camera, rectified camera) pair of the call that set it

	Dev<void> d_rot;  // ebo_rotation.cpp: a chunk's three images and folds (RotScratch)
	Dev<double> d_rot_io;  // its host entries' omegas [Wn][3], r [Wn], g [Wn][3]
	Dev<double> d_evimg_om;  // ebo_event_images: zeros [Wn][3] standing in for omegas that are NULL
	Dev<double> d_evimg;  // ebo_map_track_resident: B [Wn][h][w] of the resident windows, kept between its calls
	uint64_t evimg_gen = 0;  // units_gen they were made for (0: none)
	int evimg_windows = 0;
	Dev<void> d_maptrack;  // ebo_maptrack.cpp: the host form's images, points, unit images, poses, results and trace

	// ebo_depth.cpp: the space-sweep volume between ebo_dsi_begin and ebo_dsi_end
	Dev<uint32_t> d_dsi;  // H [nz][h][w]
	Dev<double> d_dsi_z;  // M1's table [nz]
	Dev<DsiPose> d_dsi_pose;  // M2's relative poses of the resident windows [Wn]
	Dev<void> d_dsi_x;  // the extraction's maps and point list (DsiScratch)
	bool dsi_live = false;
	DsiConsts dsi_k = {};
	ebo_depth_params dsi_prm = {};
	double dsi_ref[12] = {};
	std::vector<double> dsi_z;
	uint64_t dsi_events = 0;  // events the volume has accepted (M4's cap)

	std::vector<Unit> units;       // [Wn][P+1], stray unit last in each window
	std::vector<int64_t> unit_tref;
	std::vector<int64_t> unit_tmin, unit_tmax;  // ebo_set_patches: earliest / latest event time per unit (ebo_count_image_shard)
	std::vector<int16_t> unit_box;              // ebo_set_patches: [unit][4] = min x, max x, min y, max y of the unit's events
	uint64_t units_gen = 0;                     // bumped by every ebo_set_*: invalidates the cached shard tables below
	Dev<void> d_shard_tbl;  // BandUnit[units] (band image) / int32 dt_win[units] (dense shard image)
	uint64_t shard_tbl_gen = 0;                 // units_gen the table was built for (0 = none)
	int shard_tbl_kind = 0;                     // 1 = dt_win only, 2 = BandUnit
	std::vector<int64_t> shard_tbl_tref;        // the windows' reference times it was built for
	std::vector<WindowInfo> windows;
	std::vector<uint64_t> h_packed;
	Dev<uint32_t> d_route_xy;  // ebo_route_set_events: x:16 | y:16 per event of the chunk
	size_t route_n = 0;
	Pinned<void> pin_route;  // pinned, device-visible arguments and results of ebo_route_events
	Pinned<void, hipHostMallocDefault> pin_bucket;  // pinned mirror of the bucketing results (offsets in; units, reference times, flag out)
	// pinned, device-visible staging of one evaluation round (flows in, (r, J0, J1) out, modes):
	// small rounds let the kernels read and write it directly (no copy packets at all), large
	// ones copy from/to it at DMA speed.  Three blocks of ONE logical size (grow_eval_staging, ebo_api.cpp):
	// flows [nf][2], results [nf][3], mode tables [4][nf]
	Pinned<double> pin_flows;
	Pinned<double> pin_out;
	Pinned<unsigned char> pin_modes;

	hipEvent_t ev0 = nullptr, ev1 = nullptr;
	// ebo_two_view_timing (ebo_twoview.cpp): events around the phases of a RANSAC call (ebo_ransac.cpp), created on first use
	hipEvent_t tv_ev[5] = {};
	bool tv_timing = false;
	float tv_ms[5] = {};  // hypothesis kernel, counting kernel, host walk, winner upload + inlier-list kernel, whole call (wall clock)
	int max_rw = 0, max_rh = 0;
	int grid_max_rw = 0, grid_max_rh = 0;
	// the REGULAR patch of the loaded units (the grid's patch size; of patches loaded by ebo_set_patches the
	// smallest rect, which for a shard of a grid is the grid's regular patch): what the launch shapes follow
	int reg_rw = 0, reg_rh = 0;
	int custom_n = 0;  // > 0: units were loaded by ebo_set_patches (arbitrary rects)

	int cur_patches() const { return custom_n ? custom_n : P; }
	size_t n_flows() const
	{
		return custom_n ? static_cast<size_t>(custom_n) : static_cast<size_t>(n_windows) * P;
	}
	size_t unit_index(int window, int patch) const
	{
		return custom_n ? static_cast<size_t>(patch) : static_cast<size_t>(window) * (P + 1) + patch;
	}

	template <class T>
	T* scratch(size_t off)
	{
		return reinterpret_cast<T*>(static_cast<char*>(d_scratch.get()) + off);
	}

	int fail(int code, const std::string& msg)
	{
		err = msg;
		return code;
	}
	int hip(hipError_t e, const char* what)
	{
		if (e == hipSuccess)
		{
			return EBO_OK;
		}
		err = std::string(what) + ": " + hipGetErrorString(e);
		return EBO_ERR_HIP;
	}

	// The one way a buffer of the context comes to hold at least n elements (contents not kept): `what` names it in
	// "<what>: <hip error>".  A live buffer is released only once the stream has drained (a launch in flight may still
	// use it), and never while a graph is being recorded: a recorded call cannot allocate, free or synchronise, so a
	// buffer that does not fit then is refused with EBO_ERR_STATE and left as it is -- recording and context intact.
	template <class B>
	int grow(B& b, size_t n, const char* what)
	{
		if (n > b.cap() && b.get() && !capturing)
		{
			const int rc = hip(hipStreamSynchronize(stream), "sync");
			if (rc)
			{
				return rc;
			}
		}
		return grown(b.ensure(n, !capturing), what);
	}
	int grown(Grow g, const char* what)
	{
		if (g == Grow::kRefused)
		{
			return fail(EBO_ERR_STATE, std::string(what) +
										   ": refused while recording a graph, the call needs a larger buffer than the context holds: "
										   "run the same call once before recording");
		}
		if (g == Grow::kFailed)
		{
			const hipError_t e = hipGetLastError();
			return hip(e != hipSuccess ? e : hipErrorOutOfMemory, what);
		}
		return EBO_OK;
	}
};

// Between ebo_graph_begin and ebo_graph_end only the asynchronous *_device calls may run: anything that copies
// through pageable memory, allocates or synchronises invalidates the recording -- and on ROCm 7.2 leaves the
// process unable to use the stream again -- so every other entry point refuses up front.
static const char* const kNotWhileRecording =
	"not while recording a graph (ebo_graph_begin): only ebo_eval_device, ebo_solve_device and ebo_count_image_device can be recorded";

namespace ebo_host
{
// how a synchronous entry point begins: a context, no recording, its arguments (`what` is the message when they are
// not in order), the context's device
inline int enter(ebo_ctx* c, const char* what, bool argsOk)
{
	if (!c)
	{
		return EBO_ERR_ARG;
	}
	if (c->capturing)
	{
		return c->fail(EBO_ERR_STATE, kNotWhileRecording);
	}
	if (!argsOk)
	{
		return c->fail(EBO_ERR_ARG, what);
	}
	(void)hipSetDevice(c->prm.device);
	return EBO_OK;
}

// phase marks of ebo_two_view_timing: nothing is recorded unless the caller asked for timing
inline void mark(ebo_ctx* c, int i)
{
	if (c->tv_timing)
	{
		(void)hipEventRecord(c->tv_ev[i], c->stream);
	}
}

// One RANSAC path as ebo_ransac.cpp's driver sees it.  A group is what one RANSAC runs over (a keyframe pair, a
// frame); a and b are the path's two [n][3] arrays.  The words are those of the path's error messages.
struct RansacProblem
{
	ebo::RansacKind kind;  // the problem type of the counting, winner and score kernels
	int sample;            // points a hypothesis draws
	int (*hypotheses)(int n_groups, int H, const int* d_offsets, const double* d_a, const double* d_b, uint64_t seed,
					  double* d_models, int* d_valid, int* d_samples, void* stream);
	const char* entry;     // "ebo_relative_pose_ransac"
	const char* group;     // "pair"
	const char* points;    // "correspondences"
	const char* arrays;    // "bearing vectors"
	const char* label;     // "two-view": names the path in "<label> uploads: <hip error>"
	const char* scoresArgs;    // the *_scores entries' whole argument message
	const char* scoresUpload;  // and what their upload is called
};
// hostArrays: a / b are host arrays and are staged in scratch; otherwise device pointers used in place
int ransac(ebo_ctx* c, const RansacProblem& P, int n_groups, const int* offsets, const double* a, const double* b, bool hostArrays,
		   const ebo_two_view_params* prm, ebo_two_view_result* result, int* inlier_idx, int* hyp_counts, double* hyp_models,
		   int* hyp_samples);
// hostArrays: as above, and scores / flags are host arrays too
int ransac_scores(ebo_ctx* c, const RansacProblem& P, const double* model, int n, const double* a, const double* b, bool hostArrays,
				  double threshold, double* scores, uint8_t* flags);
}  // namespace ebo_host

// helpers defined in ebo_api.cpp and shared by the other host translation units
namespace ebo_host
{
extern thread_local std::string g_create_error;  // errors without a context (ebo_last_error(NULL))
extern const size_t kLdsBudget;
ebo::EvalConsts make_consts(const ebo_ctx* c);
void rect_of(const ebo_ctx* c, int px, int py, int& x, int& y, int& w, int& h);
bool mid_timestamp(int64_t a, int64_t b, int64_t& out);
ebo::SolveConsts make_solve_consts(const ebo_solver_opts* o);
int check_solver_opts(ebo_ctx* c, const ebo_solver_opts* o);
int shard_table(ebo_ctx* c, int n_windows, const int64_t* window_t_ref_us, const ebo::BandUnit** out, bool* uniformFlows);
bool band_ok(const ebo_ctx* c, const ebo_band* b);
}  // namespace ebo_host
