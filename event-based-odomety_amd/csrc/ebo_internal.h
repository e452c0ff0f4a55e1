// ebo_internal.h — types shared by the host side (ebo_api.cpp) and the device
// side (ebo_kernels.hip) of libebo_hip.so.  Not part of the ABI.
#pragma once

#include "ab_env.h"
#include "count_plan.h"
#include "fix_form.h"
#include "order_deal.h"

#include <stddef.h>
#include <stdint.h>

#include <hip/hip_runtime.h>
#include "../../include/ebo.h"
#include "ebo_bundle.h"
#include "ebo_relpose.h"
#include "ebo_align.h"
#include "ebo_rpe.h"
#include "ebo_trackerr.h"
#include "ebo_landmark.h"
#include "ebo_rotation.h"
#include "ebo_depth.h"
#include "ebo_maptrack.h"

namespace ebo
{
// One event in HBM: 8 bytes (the algorithmic bytes per
// event-evaluation).
//   lo bits  0..14  x   (15-bit two's complement)
//      bit   15     polarity (1 = POSITIVE)
//      bits 16..30  y   (15-bit two's complement)
//      bit   31     unused
//   hi             dt = t_ref(unit) - t_event   in microseconds (int32)
// Events are stored bucketed by unit (window, patch), time order kept inside a
// unit, so that one workgroup streams one contiguous, coalesced range.
static const int kCoordMin = -16384;
static const int kCoordMax = 16383;

inline uint32_t pack_lo(int x, int y, int positive)
{
	return (static_cast<uint32_t>(x) & 0x7FFFu) |
		   (static_cast<uint32_t>(positive ? 1 : 0) << 15) |
		   ((static_cast<uint32_t>(y) & 0x7FFFu) << 16);
}

// A unit = one patch of one window (a contrastFunctor instance), or the stray
// bucket of a window (events outside the sensor; flag bit 1).
struct Unit
{
	uint32_t ev_off;   // first packed event
	uint32_t n_ev;     // number of events
	int16_t rx, ry;    // patch rect (cv::Rect2i)
	int16_t rw, rh;
	int32_t dt_win;    // t_ref(window) - t_ref(unit): dt_window = dt + dt_win
	uint32_t flags;    // bit0: active (n_ev > min_events); bit1: stray bucket
	uint32_t flow_idx; // index of this unit's flow in the [Wn][P] arrays
};
static_assert(sizeof(Unit) == 28, "Unit layout");

// The canonical order inside a unit and its strided deal (order_stride, order_inverse): order_deal.h.

// sigma_compensate range ebo_create admits (include/ebo.h): what tests/test_gpu_eval_sweep.py covers
static const double kSigmaMin = 0.25;
static const double kSigmaMax = 1e3;  // (at 1e4 the fixed-point grid step is 1.4e-7 of a tap: the variance fails 1e-9)
// sigma_st range admitted: what the sweep covers (at 0.3 the edge Jacobian turns NaN where the reference's is finite)
static const double kSigmaStMin = 1.0;
static const double kSigmaStMax = 10.0;
// (below 0.25 the variance objective disagrees with the reference: taps underflow, and the three-exp
// factorisation of a tap gives inf * 0 = NaN below sigma 0.065)

static const uint32_t kUnitActive = 1u;
static const uint32_t kUnitStray = 2u;

// Constants of one evaluation, passed by value to kernels.
struct EvalConsts
{
	double scale;         // compensateScale
	double max_res;       // maxPossibleResidual_
	double norm;          // 1 / (2 pi sigma^2)
	double hs;            // -0.5 / sigma^2
	double inv_sigsq;     // 1 / sigma^2
	double ck1, ck2, ck3; // exp(hs * k^2), k = 1..3 (factored 1-D Gaussian taps)
	double fix_bias;      // 1.5 * 2^k: adding it aligns a tap value to the fixed-point grid (k of norm alone;
	double fix_scale;     // 2^(k-52): value of one fixed-point unit              a unit raises it: unit_fix_grid)
	double fix_pre_x;     // norm * 2^-511 and 2^-(511 + k): the prefactors of the two axes' weights whose product is the
	double fix_pre_y;     // SUBNORMAL double with the tap's fixed-point word as its bit pattern (fix_form.h; 0 if not used)
	int32_t image_w, image_h;
	int32_t patch_w, patch_h;
	int32_t npx, npy;
	int32_t fix_form;     // kFixSubnormal, kFixBiasedGuard or (A/B build) kFixBiasedAb: fix_form.h
	uint32_t inv_pw, inv_ph; // floor(2^32 / patch_w) + 1 (resp. patch_h): x / patch_w == umulhi(x, inv_pw) for 0 <= x < 2^15, patch_w >= 2
};

// ceres-style solver options for the device solver (mirror of ebo_solver_opts).
struct SolveConsts
{
	int32_t max_num_iterations;
	int32_t max_nonmono;  // 0 when use_nonmonotonic is off
	int32_t max_invalid;
	int32_t jacobi_scaling;
	double function_tolerance, gradient_tolerance, parameter_tolerance;
	double initial_radius, max_radius, min_radius;
	double min_relative_decrease, min_lm_diagonal, max_lm_diagonal;
};

// The windows of a batch that a launch covers, for lock-step solves whose batch has thinned out (late rounds
// of EBO_SOLVE_GLOBAL: a few stragglers of 256 windows): workgroups are created for these windows' units
// only, and the mode of a window (1 value, 2 value + Jacobian) rides in its entry.  Passed BY VALUE as a
// kernel argument -- no copy, no extra command on the stream; n = 0: the launch covers every unit.
constexpr int kLiveMax = 64;
struct LiveWindows
{
	int n = 0;
	int upw = 1;          // units per window (P + 1: the stray unit)
	int ent[kLiveMax];    // window << 2 | mode
};

// Per-block partial sums of the variance objective: S1, S2, n, D1[2], D2[2], pad.
static const int kPartialStride = 8;

// A/B build only, the device counters of a variance evaluation: [0], [1] ebo_box_path_counts; ebo_interior_path_counts is
// the sum of kInteriorStatSlots counters, one 64-byte line each, which the workgroups take by blockIdx -- one more atomic
// per unit on ONE address costs the launch 10-20 ns a unit, more than the path it counts saves
constexpr int kInteriorStatSlots = 64;
constexpr int kInteriorStatStride = 16;
constexpr int kBoxStatInts = kInteriorStatStride * (kInteriorStatSlots + 1);

// The per-unit time-extent table of a load (box_extents.h), as an evaluation's launch sees it.
struct BoxTable
{
	const int32_t* ext = nullptr;   // [units][kExtStride], or null: every unit's box by the event pass (A/B: EBO_EVAL_BOX=events)
	unsigned int* stats = nullptr;  // A/B build only: DEVICE counters [kBoxStatInts], else null
	// A/B build only, the bank deal of k_eval3 (eval_deal.h): EBO_EVAL_DEAL=0 evaluates every unit in the canonical order;
	// ebo_unit_deal reads one unit's dealt list back ([0] its length, 0 where the unit is not dealt, then the list)
	int deal_off = 0;
	int deal_unit = -1;
	uint32_t* deal_dump = nullptr;
	// A/B build only, k_eval3's all-interior path (eval_interior.h): EBO_EVAL_INTERIOR=0 evaluates every unit by the general path
	int interior_off = 0;
};

// ---- launch wrappers implemented in ebo_kernels.hip (hipStream_t as void*) ----
struct EvalLaunch
{
	const uint64_t* d_events;
	const Unit* d_units;
	const uint32_t* d_order = nullptr;  // [n_units] launch order of the units (launch_order.h); a launch without it is refused
	int n_units;           // patch units only (strays excluded)
	const double* d_flows; // [flow sets][n_flow][2]
	int n_flow;            // flows per flow set (= Wn * P)
	int flow_sets;         // 1, or 5 for central differences
	int channels;          // 1 or 3
	int tiles;             // row tiles per unit
	int block;             // threads per workgroup
	int cap_doubles;       // k_eval3: image capacity of one workgroup's LDS, in pixels
	size_t lds_bytes;
	int header_waves;      // k_eval3: waves the LDS header in front of the image is sized for (eval_plan.h)
	int groups_per_cu;     // k_eval3: resident workgroups per CU the plan intends
	double* d_partials;    // [flow sets][n_units][tiles][kPartialStride]
	double* d_out;         // [n_flow][3]
	double fd_step;        // > 0: combine as central differences
	const unsigned char* d_modes = nullptr;  // per flow slot: 0 skip, 1 value, 2 value + Jacobian (tiles == 1, one flow set)
	LiveWindows live;      // n > 0: only these windows (tiles == 1, one flow set)
	BoxTable box;
	EvalConsts c;
};
int launch_eval_variance(const EvalLaunch& L, void* stream);
// waves per CU the k_eval3 instantiation of these constants is compiled for, and the workgroups of L's block and LDS the
// runtime keeps resident on one CU (c, block and lds_bytes are read)
int eval_variance_waves_per_cu(const EvalConsts& c);
int eval_variance_resident(const EvalLaunch& L, int* groups);
// k_unit_extents over units [0, n_units): rewrites their slots of d_unit_ext from the resident events and units
int launch_unit_extents(const uint64_t* d_events, const Unit* d_units, int n_units, int32_t* d_unit_ext, void* stream);
int launch_dump_image(const EvalLaunch& L, int unit, double* d_image, void* stream);

// Edge (structure-tensor) loss, contrast_functor.h:152-277.
struct EdgeConsts
{
	const double* w;       // DEVICE table [49]: tensor weights [i+3][j+3] = gaussian(0,0,j,i,sigmaST) (:193-202); read by scalar loads where used (49 kernel-argument doubles pinned 98 SGPRs and the reverse pass spilled hundreds)
	double w_max;          // the largest of them, w[24]
	double g[7];           // 1-D factors exp(hs_st k^2), k = -3..3:  w(i,j) = norm_st g[i] g[j]
	double norm_st;        // 1 / (2 pi sigmaST^2)
	double mean_threshold; // 1e-4 (:159)
	int ablate;            // timing-only ablation mask (EBO_EDGE_ABLATE): 1 eigen, 2 NMS, 4 reverse, 8 gather, 16 scatter, 32 no register runs, 64 reference-order image, 128 bank-spread fake entries in the reverse sweep
	double* cs;            // DEVICE table [workgroup slot][cap_px][2] or null: (s00 - s11)/d and 2 s01/d of every pixel with a positive eigenvalue, written by the eigenvalue pass of a Jacobian evaluation, read by its reverse pass for the argmax pixels (null: the reverse pass re-derives the tensor sums)
	int cs_stride;         // pixels per slot of cs = the most pixels an LDS-resident box may have (aliased layouts)
	int reserved;          // tensor filter forms (EBO_EDGE_SEPARABLE): 1 band buffers on the 28 B layout, 2 register runs on the 20 B layout, 4 register runs on the 28 B layout
	unsigned long long* stats;  // null, or DEVICE counters [6] of ebo_edge_work_stats: units past the penalty test, their events, box pixels, eigenvalue-region pixels, NMS windows, argmax entries
};

// The compact LDS layout of k_eval_edge_wg (round 5): 16.5 B per pixel (I, E / A, 4-bit claim counters) and a header
// sized by the launch, so that THREE 256-lane workgroups share a CU; a unit whose box does not fit is not evaluated
// on its global slice but appended to defer_list for the launch that follows with the 20 B layout (two per CU).
// list_cap == 0: the layouts of rounds 1-4.
struct EdgeCompact
{
	int hdr_doubles = 0;       // doubles in front of the arrays: red[128] | 80 ints | list_cap ints
	int list_cap = 0;          // ints of the list / cell region
	int* defer_list = nullptr; // DEVICE [items]
	int* defer_count = nullptr;// DEVICE, zeroed before the launch
	void* bbox = nullptr;      // DEVICE int4[items]: the tap bounding boxes of this launch's units (k_edge_classify), or null
};

struct EdgeLaunch
{
	const uint64_t* d_events;
	const Unit* d_units;
	int n_units;
	const double* d_flows;
	int want_jac;
	int flow_sets;        // 1, or 5 (central differences, value only)
	double fd_step;
	int block;
	int cap_px;           // pixels per array that fit LDS
	int alias_lds;        // 1: 20 B/pixel LDS layout (A in E's storage, direct tensor form), 2 workgroups per CU
	size_t lds_bytes;
	EdgeCompact compact;  // list_cap > 0: this launch uses the compact layout (edge_launch_setup)
	size_t compact_lds_bytes = 0;
	int compact_cap_px = 0;
	int compact_table_px = 0;  // pixels per unit of the direction table whenever SOME launch of the context takes the compact layout
	bool wide_kernel = false;  // A/B (EBO_EDGE_WIDE): the 168-VGPR instantiation whatever the workgroup size (three 256-lane workgroups per CU)
	int wg_slots = 1;     // workgroups of a k_eval_edge launch (persistent: what the chip holds at once); k_solve_edge: one per unit
	char* d_scratch;      // global fallback, [workgroup slot][stride]
	size_t scratch_stride;
	double* d_sets;       // staging [5][n_units][3] for central differences
	double* d_out;        // [n_flow][3]
	const unsigned char* d_modes = nullptr;  // per flow slot: 0 skip, 1 value, 2 value + Jacobian
	bool for_solve = false;  // the launch is k_solve_edge (picks the workgroup size of its instantiations)
	LiveWindows live;        // n > 0: only these windows (one flow set)
	EvalConsts c;
	EdgeConsts ec;
};
int launch_lds_rate(int atomic, int blocks, int iters, double* d_sink, void* stream);
int launch_stream_yardstick(const uint64_t* d_events, size_t n_events, double* d_image, size_t n_pixels, void* stream);
// what k_count_band needs of a unit of a row shard besides its Unit: times against the WINDOW's reference time,
// the bounding box of its events (they may lie outside the rect: strays take the clamped patch) and its grid patch
struct BandUnit
{
	int32_t dt_win;  // t_ref(window) - t_ref(unit)
	int32_t max_dt;  // max |t_ref(window) - t| over the unit's events
	int16_t x0, x1, y0, y1;  // inclusive bounding box of the unit's events
	int32_t flow;    // grid patch whose flow the unit's events take (feature_detector.cpp:436-441)
	int32_t reserved;
};
static_assert(sizeof(BandUnit) == 24, "BandUnit layout");

struct BandLaunch
{
	const uint64_t* d_events;
	const Unit* d_units;
	const BandUnit* d_band_units;
	int per;        // units per window
	int n_windows;
	const double* d_flows;  // [n_windows][P][2], all grid patches
	int band0, own0, own1, band1;
	unsigned int* d_top;
	unsigned int* d_own;
	unsigned int* d_bottom;
	int* d_escaped;
	EvalConsts c;
};
int launch_count_band(const BandLaunch& L, void* stream);
int launch_count_shard(const uint64_t* d_events, const Unit* d_units, int n_units, int units_per_window,
					   const BandUnit* d_table, const double* d_flows, double* d_image, const EvalConsts& c, void* stream);
int launch_band_finish(const unsigned int* d_own, const unsigned int* d_from_above, const unsigned int* d_from_below,
					   int own_rows, int recv_above, int recv_below, int W, int n_windows, double* d_image, void* stream);
int launch_eval_edge(const EdgeLaunch& L, void* stream);
int launch_solve_edge(const EdgeLaunch& L, const SolveConsts& o, double* d_flows_out, int32_t* d_stats, void* stream);

struct SolveLaunch
{
	const uint64_t* d_events;
	const Unit* d_units;
	const uint32_t* d_order = nullptr;  // [n_units] launch order of the units (launch_order.h)
	const int32_t* d_unit_ext = nullptr;  // BoxTable::ext
	int n_units;
	int cap_doubles;
	int block;
	size_t lds_bytes;
	double* d_flows_out; // [n_flow][2]
	int32_t* d_stats;    // [n_flow][4] or null
	EvalConsts c;
	SolveConsts s;
};
int launch_solve_independent(const SolveLaunch& L, void* stream);

struct CountLaunch
{
	CountPlan plan;                  // plan_count_image (count_plan.h): the kernels, their grids and geometry
	const uint64_t* d_events;
	const Unit* d_units;
	int n_windows;
	int units_per_window;            // P + 1
	int mode;                        // EBO_COUNT_*
	const int32_t* d_unit_maxdt;     // [units] max |t_ref(window) - t| per unit (the unit kernels' displacement bound)
	unsigned int* d_sort_bins;       // kCountSorted: [3 * bins + 2] counts, starts, cursors
	unsigned int* d_sorted;          // kCountSorted: [list_events] destination pixels sorted by band, then [list_events] in event order
	const void* d_aux;               // flows f64 [Wn][P][2] or field f32 [Wn][H][W][2]
	int32_t* d_counts;               // [Wn][H][W] scratch, zero on entry, zero on exit
	double* d_image;                 // [Wn][H][W]
	EvalConsts c;
};
int launch_count_image(const CountLaunch& L, void* stream);

// Device-side bucketing of raw 24-byte events (ebo_bucket.inc).
struct BucketLaunch
{
	const void* d_raw;                 // ebo_event[] (24 B) or ebo_event8[] (8 B) on the device
	int compact = 0;                   // 1: d_raw holds ebo_event8 records, times relative to d_tbase[window]
	const long long* d_tbase = nullptr; // [n_windows] base times of the compact records
	int w0 = 0, w1 = -1;               // window range of this call ([0, n_windows) when w1 < 0); init runs with w0 == 0
	const unsigned long long* d_offsets; // [n_windows + 1], absolute indices into d_raw
	int n_windows;
	int P;
	int chunk_events;                  // events per chunk of the count / scatter passes: 2048, or 256 for small inputs
	int max_chunks;                    // ceil(max events per window / chunk_events)
	unsigned int min_events;
	int* d_cnt;                        // [n_windows][P+1] scratch (counts)
	unsigned int* d_chunk_hist;        // [n_windows][max_chunks][P+1]: per-chunk histograms, then the chunks' first ranks
	long long* d_tmin;                 // [n_windows][P+1]
	long long* d_tmax;
	Unit* d_units;                     // out [n_windows][P+1]
	long long* d_unit_tref;            // out [n_windows][P+1]
	int32_t* d_unit_maxdt;             // out [n_windows][P+1]: max |t_ref(window) - t| per unit
	long long* d_win_tref;             // out [n_windows]
	uint64_t* d_packed;                // out packed events
	int* d_flag;                       // out error bits
	const void* d_rectify = nullptr;   // short2 [image_h][image_w] rectification table (ebo_camera.inc), or null: raw coordinates
	EvalConsts c;
};
int launch_bucket(const BucketLaunch& L, void* stream);

// FeatureDetector::initMotionField (ebo_field.inc).
struct FieldLaunch
{
	int w, h;
	double scale;
	int use_average;
	int n_patches;
	const unsigned long long* d_off; // [n_patches + 1]
	const double* d_xy;              // [samples][2]
	const long long* d_t;            // [samples]
	long long timestamp;
	float* d_field;                  // out [h][w][2]
	int* d_fixed;                    // out [n_patches][2]
	double* d_avg;                   // scratch [3]
	int* d_nfixed;                   // out
};
int launch_init_field(const FieldLaunch& L, void* stream);

// interpolateMotionField's per-pixel TV problem (ebo_fieldtv.inc / field_tv.cpp).
// n = w * h pixels; "2" vectors hold both flow components of a pixel side by side.
struct TvfArgs
{
	int w, h, n;
	unsigned char* mask;  // 0 free, 1 fixed point, 2 not in the problem (pixel (w-1, h-1))
	double* wh;           // weight of edge p-(p+1), 0 where the block does not exist
	double* wv;           // weight of edge p-(p+w)
	double* deg;          // sum of the incident weights = diag(J'J)
	double* s2;           // Jacobi scaling squared, from iteration 0
	double* diag;         // deg + damping (the CG preconditioner)
	double2* x;           // current point
	double2* xc;          // candidate
	double2* g;           // gradient
	double2* y;           // LM step (unscaled)
	double2* r;
	double2* z;
	double2* p0;
	double2* p1;
	double2* q;
	double* partials;     // [4 * 1024] per-workgroup sums of the last kernel
	double* partials_rz;  // [4 * 1024] same, for r'z / r'r (read while `partials` is rewritten)
	double* scal;         // [32] reduction results, see ebo_fieldtv.inc
	double huber_a;       // 0: no loss (useL1 false); 1e-5: HuberLoss(1e-5)
	double lm_lo, lm_hi;  // min/max_lm_diagonal
};
// One level of the multigrid preconditioner (ebo_fieldtv.inc): a 5-point operator
// (A x)_i = diag_i x_i - sum_e w_e x_j on a w x h grid, wh / wv = weight of the edge to the right /
// lower neighbour (0 where there is none).
struct TvfLevel
{
	int w, h;
	const double* wh;
	const double* wv;
	const double* diag;
	double2* b;   // right-hand side
	double2* x;   // after pre-smoothing
	double2* xo;  // after the coarse correction and post-smoothing
};
struct TvfMg
{
	int levels;          // 0: multigrid off (diagonal preconditioner)
	TvfLevel lv[12];
	double* wh_m[12];    // writable views of lv[l].wh / wv / diag (level 0: masked weights only)
	double* wv_m[12];
	double* diag_m[12];
	double omega, kappa;
	int coarse_sweeps;
};
size_t tvf_workspace_bytes(int w, int h);
void tvf_carve(TvfArgs& A, TvfMg& M, int w, int h, void* base, double2** xbest);
int launch_tvf_mg_build(const TvfArgs& A, const TvfMg& M, void* stream);
int launch_tvf_prepare(const TvfArgs& A, const float* d_field, const int* d_fixed, int n_fixed, void* stream);
int launch_tvf_linearize(const TvfArgs& A, const double2* X, int first, int cost_only, void* stream);
int launch_tvf_cg_init(const TvfArgs& A, const TvfMg& M, double radius, void* stream);
// CG iterations first_iter .. first_iter + iters - 1 (iteration k reads direction buffer k & 1).
int launch_tvf_cg_iters(const TvfArgs& A, const TvfMg& M, int first_iter, int iters, void* stream);
int launch_tvf_model(const TvfArgs& A, void* stream);
int launch_tvf_store(const TvfArgs& A, const double2* X, float* d_field, void* stream);

// The per-feature tracker objective (ebo_optimizer.inc): one tracked patch.
struct OptPatch
{
	double rx, ry;           // patch_.tl()
	int pw, ph;              // int(patch_.width), int(patch_.height)
	unsigned long long off;  // first residual of this patch in the concatenated arrays
};
struct OptLaunch
{
	const double2* d_grid;   // [img_h][img_w] (gradX, gradY)
	int img_w, img_h;
	const OptPatch* d_patches;
	int n_patches;
	int max_pixels;          // max pw * ph over the patches (LDS sizing)
	const double* d_nabla;   // normalizedIntegratedNabla, concatenated
	double* d_x;             // [n][5] = pose (cos, sin, tx, ty), flow direction
	double* d_res;           // eval: residuals, concatenated
	double* d_jac_pose;      // eval: [..][4] or null
	double* d_jac_flow;      // eval: [..] or null
	double* d_stats;         // solve: [n][8]
	double huber;
	SolveConsts s;
};
int launch_optimizer_eval(const OptLaunch& L, void* stream);
int launch_optimizer_solve(const OptLaunch& L, void* stream);
int launch_optimizer_cost_map(const OptLaunch& L, const double* d_xcells, int cells, double* d_out, void* stream);
int launch_optimizer_normalize(const OptPatch* d_patches, int n, const double* d_in, double* d_out, void* stream);
int launch_optimizer_interleave(const double* d_gx, const double* d_gy, size_t n, double2* d_grid, void* stream);
int launch_estimate_num_events(const double2* d_grid, int w, int h, int n, const double* d_rects, const double* d_poses,
								const double* d_flows, double* d_sums, void* stream);

int launch_patch_warp_image(const double2* d_grid, int w, int h, int n, const double* d_rects, const double* d_poses,
							const double* d_flows, const int* d_skip, const size_t* d_offsets, double* d_out, void* stream);

struct PatchIntLaunch
{
	const uint64_t* d_events;  // packed, dt = mid_time - t
	const uint32_t* d_offsets; // [n+1]
	const double* d_rects;     // [n][4]
	const double* d_traj;      // [n][4] = dirX, dirY, tDif, pass(0/1); null for R5
	const uint64_t* d_nabla_off; // [n]
	double* d_nabla;
	int n_patches;
};
int launch_patch_integrate(const PatchIntLaunch& L, void* stream);

// Event -> tracked-patch routing (FeatureDetector::updatePatches): one wave per patch.
struct RouteLaunch
{
	const uint32_t* d_xy;      // [n_events] x:16 | y:16 (two's complement halves)
	uint32_t n_events;
	int n_patches;
	const double* d_rects;     // [n][4]
	const uint32_t* d_start;   // [n]
	const uint32_t* d_take;    // [n]
	uint32_t cap;
	uint32_t* d_index;         // [n][cap]
	uint32_t* d_count;         // [n]
	uint32_t* d_next;          // [n]
};
int launch_route(const RouteLaunch& L, void* stream);

// Image front end of FeatureDetector::newImage (ebo_frontend.inc, ebo_frontend.cpp).
constexpr int kFeLevels = 8;         // pyramid levels kept per image (ebo.h: max_level <= 7)
constexpr int kFeMaxWindow = 1024;   // LK window pixels (64 lanes x 16)
constexpr int kFeMaxCornersLds = 8192;  // ebo_good_features' max_corners limit
constexpr int kFeSortLds = 4096;     // candidate lists up to this length are sorted in LDS
struct FeLevel
{
	int w, h;
	unsigned long long img;  // byte offset of the level's image in its pyramid allocation
	unsigned long long der;  // byte offset of its short2 (Ix, Iy) derivatives
};
int launch_fe_gradients(const uint8_t* d_img, const double* d_lut, int w, int h, double* d_gx, double* d_gy,
						void* stream);
// response + per-workgroup masked maximum (d_bmax: fe_harris_blocks(w, h) entries), then threshold / NMS /
// compaction into (d_candR, d_candI), *d_count candidates (zeroed here)
int fe_harris_blocks(int w, int h);
int launch_fe_harris(const uint8_t* d_img, const uint8_t* d_mask, int w, int h, int block_size, double k,
					 double quality, double* d_resp, double* d_bmax, double* d_candR, int* d_candI, int* d_count,
					 void* stream);
// sorted list + greedy pick; n = the candidate count (host copy of *d_count), cap = capacity of the lists
// (a power of two >= n when n > kFeSortLds: the lists are padded and sorted in global memory first)
int launch_fe_select(double* d_candR, int* d_candI, const int* d_count, int n, int cap, int w, int max_corners,
					 double min_distance, float* d_corners, int* d_nout, void* stream);
// levels 1 .. n_levels-1 from level 0, then the derivatives of every level (lv: host copy of the table)
int launch_fe_pyramid(char* d_pyr, const FeLevel* lv, int n_levels, void* stream);
int launch_fe_lk(const char* d_prev, const char* d_next, const FeLevel* d_lv, int n_levels, int n, const float* d_prev_xy,
				 float* d_next_xy, uint8_t* d_status, float* d_err, int win_w, int win_h, int max_count, double eps2,
				 float min_eig, void* stream);

// common::CameraModel (ebo_camera.inc, ebo_camera.cpp): the nine parameters in ebo_camera's order.
struct CameraConsts
{
	double fx, fy, cx, cy, k1, k2, k3, p1, p2;
};
// the pinhole part of a rectified camera (its distortion is zero by definition)
struct RectifiedConsts
{
	double fx, fy, cx, cy;
};
int launch_camera_unproject(const CameraConsts& k, int n, const double* d_uv, double* d_bearing, void* stream);
int launch_camera_project(const CameraConsts& k, int n, const double* d_xyz, double* d_uv, void* stream);
// d_map: double [h][w][2], d_lut: int16 [h][w][2], *d_bad: error bits (zeroed here)
int launch_rectify_map(const CameraConsts& k, const RectifiedConsts& r, int w, int h, double* d_map, void* d_lut, int* d_bad,
					   void* stream);
// d_extremes: xmin, xmax, ymin, ymax of the undistorted border pixels; *d_bad: 1 when one of them is not finite
int launch_rectify_fit(const CameraConsts& k, int w, int h, double* d_extremes, int* d_bad, void* stream);
// d_img / d_out: uint8 [h][w] (null together: the source map alone); d_src: double [h][w][2] or null
int launch_rectify_image(const CameraConsts& k, const RectifiedConsts& r, int w, int h, const uint8_t* d_img, uint8_t* d_out,
						 double* d_src, void* stream);

// two-view geometry (ebo_twoview.inc, ebo_twoview.cpp).  models: [n_pairs * H][3][4]; d_samples may be null.
int launch_tv_hypotheses(int n_pairs, int H, const int* d_offsets, const double* d_f1, const double* d_f2, uint64_t seed,
						 double* d_models, int* d_valid, int* d_samples, void* stream);
int launch_tv_triangulate(int n_poses, const double* d_poses, int n, const int* d_pose_pair, const double* d_f1,
						  const double* d_f2, double* d_points, void* stream);
int launch_tv_epipolar(const double* model12, int n, const double* d_f1, const double* d_f2, double threshold,
					   unsigned char* d_flags, void* stream);
// absolute pose (ebo_abspose.inc, ebo_abspose.cpp).  models: [n_frames * H][3][4]; d_samples may be null.
int launch_ap_hypotheses(int n_frames, int H, const int* d_offsets, const double* d_f, const double* d_points, uint64_t seed,
						 double* d_models, int* d_valid, int* d_samples, void* stream);
// What the two paths share (ebo_ransac.inc, ebo_ransac.cpp): kind selects the problem type the kernels are instantiated
// for.  A group is a keyframe pair or a frame; d_a / d_b are its two [n][3] arrays (f1, f2 or bearing vectors, landmarks).
enum class RansacKind
{
	kTwoView,
	kAbsPose
};
// d_counts [n_groups * H] must be zero on entry; max_n: points of the largest group
int launch_ransac_count(RansacKind kind, int n_groups, int H, int max_n, const int* d_offsets, const double* d_a, const double* d_b,
						const double* d_models, const int* d_valid, double threshold, int* d_counts, void* stream);
int launch_ransac_winner_flags(RansacKind kind, int n_groups, int H, int max_n, const int* d_offsets, const double* d_a,
							   const double* d_b, const double* d_models, const int* d_valid, const int* d_winner, double threshold,
							   unsigned char* d_flags, double* d_win_models, void* stream);
// model12: HOST pointer to a [3][4] model (travels as a kernel argument); either output may be null
int launch_ransac_scores(RansacKind kind, const double* model12, int n, const double* d_a, const double* d_b, double threshold,
						 double* d_scores, unsigned char* d_flags, void* stream);

// bundle adjustment (ebo_bundle.inc, ebo_bundle.cpp): where each problem's slices begin (sums of the sizes of the
// problems before it, device arrays) and the call's device arrays
struct BaTables
{
	const int* frameOff;
	const int* pointOff;
	const int* obsOff;
	const long long* tableOff;
	double* poses;
	const unsigned char* fixed;
	double* points;
	const int* of;
	const int* op;
	const double* uv;
	double* work;  // ba_work_doubles (ebo_bundle.h)
	int* iwork;    // ba_work_ints
	size_t totalF, totalP, totalN, totalTable;
};
// max_frames: frames of the problem that has most; the LDS of the reduced system is sized as if all of them were free
// (the _device form cannot read the flags): up to 83.5 KB at 24 frames.  d_trace may be null
int launch_bundle_adjust(int n_problems, int max_frames, const BaTables& t, const ebo_camera& cam, double huber, int fix_points,
						 const ebo_solver_opts& o, ebo_summary* d_summaries, double* d_trace, void* stream);

// relative-pose refinement (ebo_relpose.inc, ebo_relpose.cpp): pair p owns correspondences d_offsets[p] .. d_offsets[p + 1] - 1
// of d_f1 / d_f2; its d_n_inliers[p] listed inliers and its slice of d_work (rp_work_doubles of d_offsets[n_pairs], ebo_relpose.h)
// start at d_offsets[p] too.  d_trace may be null
int launch_relpose_refine(int n_pairs, const int* d_offsets, const int* d_n_inliers, const double* d_f1, const double* d_f2,
						  const int* d_inlier_idx, double* d_models, double* d_work, const ebo_solver_opts& o, ebo_summary* d_summaries,
						  double* d_trace, void* stream);

// trajectory alignment (ebo_align.inc, ebo_align.cpp): segment g covers points d_seg_begin[g] .. d_seg_end[g] - 1 of d_data and
// d_model (double [n_points][3]); one result per segment
int launch_align_sim3(int n_points, const double* d_data, const double* d_model, int n_segments, const int* d_seg_begin,
					  const int* d_seg_end, int fix_scale, ebo_align_result* d_results, void* stream);

// relative pose error (ebo_rpe.inc, ebo_rpe.cpp): unit g * n_deltas + k is segment g, poses d_seg_begin[g] .. d_seg_end[g] - 1 of
// d_gt and d_est (double [n_poses][12]), at step d_deltas[k] with scale d_seg_scale[g] (null: 1); one result per unit
int launch_trajectory_rpe(int n_poses, const double* d_gt, const double* d_est, int n_segments, const int* d_seg_begin,
						  const int* d_seg_end, const double* d_seg_scale, int n_deltas, const int* d_deltas, ebo_rpe_result* d_results,
						  void* stream);

// landmark maintenance (ebo_landmark.inc, ebo_landmark.cpp): solve != 0 triangulates (L1-L6), otherwise audits d_points (L7);
// `lanes` per landmark is 64, or 16 when no landmark of the call holds more than kLmGroupMaxObs observations
int launch_landmarks(int solve, int lanes, int n_poses, const double* d_poses, int n_landmarks, const int* d_offsets,
					 const int* d_obs_pose, const double* d_obs_f, const double* d_points, const ebo_landmark_params* params,
					 ebo_landmark_result* d_results, double* d_scores, uint8_t* d_flags, void* stream);

// rotational contrast maximisation (ebo_rotation.inc, ebo_rotation.cpp).  A launch covers one chunk of windows: chunk
// slot s holds window win[s], passed BY VALUE as LiveWindows is; the images and folds are indexed by slot, omegas and
// results by window (RotWindows, RotConsts: ebo_rotation.h).
// the chunk's scratch: three images [slots][h][w] of 8 bytes a pixel and the folds
struct RotScratch
{
	void* imgX;       // H, then the horizontal pass of B - mu
	double* imgY;     // the horizontal pass of F, then C
	double* imgZ;     // B
	double* partB;    // [slots][blocks]
	double* partV;    // [slots][blocks]
	double* mu;       // [slots]
	double* partG;    // [slots][P][3]
};
inline int rot_blocks(int w, int h)
{
	return (w * h + kRotBlock - 1) / kRotBlock;
}
// H of the chunk's windows into s.imgX (zeroed here); with d_F also F = H * 2^-30 into it ([slots][h][w])
int launch_rot_votes(const uint64_t* d_events, const Unit* d_units, const RotWindows& L, const RotConsts& k, const double* d_omegas,
					 const RotScratch& s, double* d_F, void* stream);
// r (and g unless d_g is null) of the chunk's windows into d_r[win] / d_g[win][3]
int launch_rot_eval(const uint64_t* d_events, const Unit* d_units, const RotWindows& L, const RotConsts& k, const double* d_omegas,
					const RotScratch& s, double* d_r, double* d_g, void* stream);

// V5's blur B of V4's image of the chunk's windows into d_B ([slots][h][w]): the vote and the two passes of
// launch_rot_eval, nothing else (s.imgX and s.imgY are overwritten)
int launch_rot_images(const uint64_t* d_events, const Unit* d_units, const RotWindows& L, const RotConsts& k, const double* d_omegas,
					  const RotScratch& s, double* d_B, void* stream);

// pose from events against a map (ebo_maptrack.inc, ebo_maptrack.cpp): unit u aligns k.points to image d_unit_image[u]
// from d_poses[u] ([12], updated in place); d_trace may be null
int launch_map_track(const MtCall& k, int n_units, const int* d_unit_image, double* d_poses, const ebo_solver_opts& o,
					 ebo_map_track_result* d_results, double* d_trace, void* stream);

// depth from events by space sweep (ebo_depth.inc, ebo_depth.cpp; DsiWindows, DsiConsts, DsiPose: ebo_depth.h).
// the votes of one chunk of windows (slot s is window win[s], BY VALUE as RotWindows is) into the volume d_H [nz][h][w];
// d_poses is indexed by window, d_z is M1's table
int launch_dsi_vote(const uint64_t* d_events, const Unit* d_units, int P, const DsiWindows& L, const DsiConsts& k, const DsiPose* d_poses,
					const double* d_z, uint32_t* d_H, void* stream);
// the extraction's scratch, all of it per pixel except blockCount [dsi_blocks + 1]
struct DsiScratch
{
	uint32_t* conf;
	int* kbest;
	int* index;
	double* depth;
	int* blockCount;
	unsigned char* keep;
	double* points;  // [max_points][3], null when no point is wanted
};
inline int dsi_blocks(int w, int h)
{
	return (w * h + kDsiBlock - 1) / kDsiBlock;
}
// M5-M8 of the volume d_H; blockCount[dsi_blocks] receives the number of kept pixels
int launch_dsi_extract(const DsiConsts& k, int r, long long off, int m, const double* d_z, const uint32_t* d_H, const DsiScratch& s,
					   int max_points, void* stream);

// track evaluation (ebo_trackerr.inc, ebo_trackerr.cpp): unit k * n_taus + j is track k, samples d_est_off[k] .. d_est_off[k + 1] - 1
// of d_est_t / d_est_xy (n_est of them) and d_gt_off[k] .. d_gt_off[k + 1] - 1 of d_gt_t / d_gt_xy (n_gt), at threshold d_taus[j];
// one result per unit; d_sample_err is double [n_est] or null
int launch_track_errors(int n_est, int n_gt, int n_tracks, const int* d_est_off, const int64_t* d_est_t, const double* d_est_xy,
						const int* d_gt_off, const int64_t* d_gt_t, const double* d_gt_xy, int n_taus, const double* d_taus,
						ebo_track_error_result* d_results, double* d_sample_err, void* stream);

}  // namespace ebo
