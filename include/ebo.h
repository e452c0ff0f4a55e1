/*
 * ebo.h — C ABI of libebo_hip.so: the MI355X (gfx950) implementation of the
 * motion-compensated event-warping path of nurlanov-zh/event-based-odomety.
 *
 * This is the drop-in boundary.  Plain pointers and sizes only; no C++ types, no
 * torch types.  Nothing allocates across the ABI: the context owns every device
 * buffer, the caller owns every host pointer it passes in or gets results in.
 * Every function returns an int status (0 = ok, negative = error) and never
 * throws; ebo_last_error() gives the message.  A context belongs to one thread and
 * one device.  There is NO CPU fallback: without a gfx950 device ebo_create fails
 * with EBO_ERR_NO_DEVICE.
 *
 * Reference interfaces replaced (paths relative to the reference checkout):
 *   R1  ceres::AutoDiffCostFunction<tracker::contrastFunctor,1,2>::Evaluate
 *       built at implementation/feature_tracker/src/feature_detector.cpp:359-363 on
 *       implementation/feature_tracker/include/feature_tracker/contrast_functor.h:10-292
 *   R2  tracker::FeatureDetector::compensateEventsContrast   feature_detector.cpp:298-464
 *   R3  tracker::FeatureDetector::integrateEvents            feature_detector.cpp:466-482
 *   R4  tracker::FeatureDetector::compensateEvents           feature_detector.cpp:243-296
 *   R5  tracker::Patch::integrateEvents                      implementation/feature_tracker/src/patch.cpp:65-85
 *   R6  tracker::Patch::integrateMotionCompensatedEvents     patch.cpp:87-130
 *   R7  tracker::DetectorParams                              include/feature_tracker/feature_detector.h:10-31
 *   R8  common::EventSample                                  common/include/common/data_types.h:12-38
 * The C++ façade with the reference's own names (tracker::FeatureDetector,
 * tracker::contrastFunctor, ...) sits on top of this header in
 * event-based-odomety_amd/include/; INTEGRATION.md shows the binding.
 */
#ifndef EBO_H
#define EBO_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define EBO_OK 0
#define EBO_ERR_ARG (-1)         /* null pointer, bad size, bad enum          */
#define EBO_ERR_HIP (-2)         /* a HIP runtime call failed                  */
#define EBO_ERR_RANGE (-3)       /* coordinate / timestamp outside packed range */
#define EBO_ERR_STATE (-4)       /* call order (no window set, ...)           */
#define EBO_ERR_UNSUPPORTED (-5) /* parameter combination not built            */
#define EBO_ERR_NO_DEVICE (-6)   /* no HIP device / not gfx950                 */
#define EBO_ERR_SOLVER (-7)      /* solver terminated with FAILURE             */
#define EBO_ERR_COMM (-8)        /* RCCL could not be loaded or a collective failed */

#define EBO_LOSS_EDGE 0     /* contrastFunctor::calculateEdgeLoss (reference default, :152-277) */
#define EBO_LOSS_VARIANCE 1 /* contrastFunctor::calculateVarianceLoss (:101-150, north-star objective) */

#define EBO_GRAD_JET 0     /* forward-mode dual numbers == ceres::Jet<double,2> (reference) */
#define EBO_GRAD_CENTRAL 1 /* central differences of the value-only objective */

#define EBO_SOLVE_GLOBAL 0      /* one problem over all patches incl. TV terms (reference, R2) */
#define EBO_SOLVE_INDEPENDENT 1 /* one 2-parameter problem per patch, solved on the device   */

#define EBO_COUNT_INTEGRATED 0 /* R3: un-warped counts                                  */
#define EBO_COUNT_WARPED 1     /* R2 final loop (:433-463): warp by per-patch flow, round() */
#define EBO_COUNT_FIELD 2      /* R4 warp loop (:270-295): warp by float32 per-pixel field  */

typedef struct ebo_ctx ebo_ctx;

/* R8: layout-compatible with common::EventSample on LP64
 * ({cv::Point2i{x,y}; enum EventPolarity sign; std::chrono::microseconds}). */
typedef struct ebo_event
{
	int32_t x;
	int32_t y;
	int32_t sign; /* -1 / +1 */
	int32_t reserved;
	int64_t t_us;
} ebo_event;

/* contrastFunctor's hard-coded members, contrast_functor.h:282-291.  ebo_create returns EBO_ERR_ARG unless
 * max_possible_residual, sigma_compensate and sigma_st are finite and > 0 (and, with EBO_GRAD_CENTRAL, fd_step;
 * scale must be finite). */
typedef struct ebo_functor_consts
{
	double max_possible_residual; /* 1e3 */
	double sigma_compensate;      /* 1; ebo_create: EBO_ERR_UNSUPPORTED outside [0.25, 1e3], the range tested */
	int32_t kernel_compensate;    /* 3 (only 3 is built)  */
	int32_t kernel_st;            /* 3 (only 3 is built)  */
	double sigma_st;              /* 1.5; ebo_create: EBO_ERR_UNSUPPORTED outside [1, 10], the range tested */
	int32_t kernel_nms;           /* 2 (only 2 is built)  */
	int32_t reserved;
} ebo_functor_consts;

/* R7: the DetectorParams fields this path reads, same defaults. */
typedef struct ebo_params
{
	int32_t device;           /* HIP device ordinal                         */
	int32_t image_w, image_h; /* imageSize {240,180}                        */
	int32_t patch_w, patch_h; /* patchCompensateSize {20,20}                */
	double tv_weight;         /* compensateTVweight 1e3                     */
	double tv_huber;          /* compensateTVHuberLoss 10                   */
	double scale;             /* compensateScale 1e-3                       */
	uint32_t min_events;      /* compensateMinNumEvents 100                 */
	int32_t loss;             /* EBO_LOSS_*  (default EDGE, as the reference) */
	int32_t grad;             /* EBO_GRAD_*  (default JET, as the reference)  */
	int32_t reserved;
	double fd_step;           /* step for EBO_GRAD_CENTRAL (default 1e-6)   */
	ebo_functor_consts k;
	uint64_t max_events;      /* device capacity, events over all windows of a batch (default 1<<20) */
	int32_t max_windows;      /* device capacity, windows per batch (default 1) */
	int32_t reserved2;
} ebo_params;

/* ceres::Solver::Options as set at feature_detector.cpp:401-410; unset fields
 * carry Ceres 2.0 defaults. */
typedef struct ebo_solver_opts
{
	int32_t max_num_iterations; /* 50    */
	int32_t use_nonmonotonic;   /* 1     */
	double function_tolerance;  /* 1e-12 */
	double gradient_tolerance;  /* 1e-12 */
	double parameter_tolerance; /* 1e-12 */
	double initial_radius;      /* 1e4   */
	double max_radius;          /* 1e16  */
	double min_radius;          /* 1e-32 */
	double min_relative_decrease; /* 1e-3 */
	double min_lm_diagonal;     /* 1e-6  */
	double max_lm_diagonal;     /* 1e32  */
	int32_t max_consecutive_nonmonotonic; /* 5 */
	int32_t max_consecutive_invalid;      /* 5 */
	int32_t jacobi_scaling;     /* 1 */
	int32_t mode;               /* EBO_SOLVE_* */
} ebo_solver_opts;

typedef struct ebo_summary
{
	int32_t iterations;     /* LM iterations (global) / max over patches (independent) */
	int32_t num_evals_cost; /* value-only evaluations of data terms     */
	int32_t num_evals_jac;  /* value+Jacobian evaluations of data terms */
	int32_t termination;    /* 0 convergence, 1 no convergence, 2 failure */
	double initial_cost;
	double final_cost;
} ebo_summary;

const char* ebo_version(void);
/* Number of HIP devices; 0 (and EBO_OK) when there is none. */
int ebo_device_count(int* n);
void ebo_default_params(ebo_params* p);
void ebo_default_solver(ebo_solver_opts* o);
/* Last error text of ctx (or of the calling thread's last failed ebo_create when ctx is NULL). */
const char* ebo_last_error(const ebo_ctx* ctx);

int ebo_create(const ebo_params* p, ebo_ctx** out);
void ebo_destroy(ebo_ctx* ctx);
/* Launch on this HIP stream (hipStream_t) instead of the context's own. */
int ebo_set_stream(ebo_ctx* ctx, void* hip_stream);
/* ---- HIP graphs over the asynchronous *_device calls ------------------------------------------
 * ebo_graph_begin starts recording the context's stream (hipStreamBeginCapture, thread-local mode);
 * the *_device calls made until ebo_graph_end (ebo_eval_device, ebo_solve_device,
 * ebo_count_image_device, ...) are recorded instead of run; ebo_graph_end instantiates the graph.
 * ebo_graph_launch replays it `times` times back to back on the context's stream, asynchronously,
 * with no host work between the steps.  Recorded calls must not allocate or synchronise: run the
 * same sequence once before recording (work tables are allocated on first use).  A recorded call
 * whose tables would have to grow, or whose edge-loss weights are not built yet, is refused with
 * EBO_ERR_STATE: nothing was recorded for it, and the recording and the context stay usable.  The graph reads
 * and writes the device pointers it was recorded with; ebo_set_windows / ebo_set_patches with the
 * same sizes reuse the same buffers, other changes need a new recording.  ebo_graph_end always
 * ends the recording, also after a failed call (EBO_ERR_HIP then, no graph).  Not in the reference:
 * the CPU path has no launch cost to hide. */
typedef struct ebo_graph ebo_graph;
int ebo_graph_begin(ebo_ctx* ctx);
int ebo_graph_end(ebo_ctx* ctx, ebo_graph** out);
int ebo_graph_launch(ebo_ctx* ctx, ebo_graph* graph, int times);
void ebo_graph_destroy(ebo_graph* graph);

int ebo_synchronize(ebo_ctx* ctx);

/* Patch grid of R2 (:301-346): npx*npy patches, last row/column absorb the remainder. */
int ebo_grid(const ebo_ctx* ctx, int* npx, int* npy);
int ebo_patch_rect(const ebo_ctx* ctx, int px, int py, int* x, int* y, int* w, int* h);

/* Load one window (the `events` list R2/R3/R4 receive), time-ordered as given.
 * The host buckets events by patch keeping their order (R2 :348-355), computes
 * the window's and each patch's reference time (:305-306, contrast_functor.h:18-20),
 * packs 8 B/event and uploads.  Replaces any previous window(s).
 * For a window that is not time-ordered, a patch's reference time is the mid of its earliest and latest
 * stamp, which is the reference's front / back whenever the window is ordered; the window's own reference time
 * stays the mid of the first and last LISTED stamp.  Inside a patch the records are kept in one canonical order
 * (csrc/order_deal.h), so every result is independent of the order of the list -- except for a patch of more
 * than 8192 events, whose records keep the order of the list. */
int ebo_set_window(ebo_ctx* ctx, const ebo_event* ev, size_t n);
/* Batch of independent windows: window w = ev[offsets[w] .. offsets[w+1]). */
int ebo_set_windows(ebo_ctx* ctx, const ebo_event* ev, const size_t* offsets, int n_windows);
/* Same with the raw events already on the device (d_ev: ebo_event[] in device memory,
 * offsets: host, indices into d_ev): bucketing, reference times and packing all run on
 * the device; nothing but the 28-byte-per-patch table comes back.  ebo_set_window(s)
 * uses this path after one H2D copy of the raw events (EBO_BUCKET=host selects the host
 * counting sort instead). */
int ebo_set_windows_device(ebo_ctx* ctx, const ebo_event* d_ev, const size_t* offsets, int n_windows);
/* Compact raw event, 8 bytes -- a third of what common::EventSample moves over PCIe, which is most
 * of a window's set-up time: xy = x:15 | polarity:1 | y:15 | 0:1 (coordinates two's complement in
 * [-16384, 16383]; polarity 1 = +1), t_rel_us = t - t_base[window] in microseconds.  The packed
 * sidecar of a recording or a sensor driver can produce it directly; ebo_pack_events8 converts a
 * window of EventSamples (EBO_ERR_RANGE for a coordinate or a time that does not fit). */
typedef struct ebo_event8
{
	uint32_t xy;
	int32_t t_rel_us;
} ebo_event8;
int ebo_pack_events8(const ebo_event* ev, size_t n, int64_t t_base, ebo_event8* out);
/* ebo_set_windows on compact records: window w = ev[offsets[w] .. offsets[w+1]) with base time
 * t_base[w] (host arrays).  ev is host memory (page-locked memory -- hipHostMalloc /
 * hipHostRegister -- reaches the PCIe rate; the upload runs in groups of windows overlapped with
 * the bucketing of the groups before), or device memory for the _device form.  Results are
 * identical to ebo_set_windows on the same events. */
int ebo_set_windows8(ebo_ctx* ctx, const ebo_event8* ev, const int64_t* t_base, const size_t* offsets, int n_windows);
int ebo_set_windows8_device(ebo_ctx* ctx, const ebo_event8* d_ev, const int64_t* t_base, const size_t* offsets,
							int n_windows);
/* Arbitrary patches instead of a window: patch i = cv::Rect2i rects[i][4] = (x,y,w,h)
 * with its own event list ev[offsets[i]..offsets[i+1]) in list order, exactly what
 * tracker::contrastFunctor's constructor takes (contrast_functor.h:12-21; events
 * are NOT filtered by the rect, as there).  Afterwards ebo_eval / ebo_solve
 * (EBO_SOLVE_INDEPENDENT) / ebo_contrast_image address n_patches flows [n][2] with
 * window = 0.  n_patches <= max_windows * grid patches. */
int ebo_set_patches(ebo_ctx* ctx, const ebo_event* ev, const size_t* offsets, const int32_t* rects,
					int n_patches);
int ebo_num_windows(const ebo_ctx* ctx, int* n_windows);
int ebo_window_info(const ebo_ctx* ctx, int window, int64_t* t_ref_us, uint64_t* n_events);
/* n_events in the patch, active = (n_events > min_events), functor reference time. */
int ebo_patch_info(const ebo_ctx* ctx, int window, int patch, int32_t* n_events,
				   int32_t* active, int64_t* t_ref_us);

/* R1, batched over every patch of every loaded window: residual r and (if jac
 * != NULL) the 1x2 Jacobian at flows[w][p][0..1].  Inactive patches give 0.
 * Host pointers: flows [Wn][P][2], r [Wn][P], jac [Wn][P][2]. Synchronous.
 * Device memory: with EBO_LOSS_EDGE a Jacobian evaluation keeps a work table of 16 bytes per
 * LDS-resident canvas pixel and patch (reference defaults: 57.6 KB per patch; allocated on first
 * use, grown on demand, given back when later batches need under a quarter of it, freed by ebo_destroy).
 * It is never larger than 4 GiB (environment EBO_EDGE_CS_MB) nor than a quarter of the device memory that
 * is free at the time; beyond that, or when its allocation fails, the kernel re-derives what it would have
 * held -- same results to 1e-18 relative, ~7 % slower. */
int ebo_eval(ebo_ctx* ctx, const double* flows, double* r, double* jac);
/* Same on device pointers, asynchronous on the context's stream:
 * d_flows [Wn][P][2], d_out [Wn][P][3] = (r, J0, J1). */
int ebo_eval_device(ebo_ctx* ctx, const double* d_flows, int want_jac, double* d_out);
/* The image of warped events the functor builds for one patch at one flow
 * (contrast_functor.h:38-88): planar [channels][3h][3w], channels = 1 or 3. Diagnostic. */
int ebo_contrast_image(ebo_ctx* ctx, int window, int patch, const double* flow,
					   int channels, double* image);

/* Solve for the flows of every loaded window starting from 0 (R2 :316-414).
 * flows_out host [Wn][P][2]; summary [Wn] (may be NULL).  EBO_SOLVE_INDEPENDENT folds a window's per-patch solves
 * into its summary: max of iterations and termination, sums of the evaluation counts.  initial_cost and final_cost
 * are reported (summed over the patches) only by its lock-step host path (EBO_GRAD_CENTRAL); the device-resident
 * path, which ebo_solve_device's d_stats describes per patch, leaves both 0. */
int ebo_solve(ebo_ctx* ctx, const ebo_solver_opts* o, double* flows_out, ebo_summary* summary);
/* EBO_SOLVE_INDEPENDENT only: the whole solve in one launch, result left on the
 * device in d_flows_out [Wn][P][2]; asynchronous. d_stats (may be NULL) [Wn][P][4]
 * int32 = (iterations, value evals, jacobian evals, termination). */
int ebo_solve_device(ebo_ctx* ctx, const ebo_solver_opts* o, double* d_flows_out,
					 int32_t* d_stats);

/* The host solver of EBO_SOLVE_GLOBAL -- the trust-region LM over ONE problem per window (a contrast data
 * term per active patch + Huber-wrapped total-variation terms between grid neighbours, R2 :357-414) -- as the
 * resumable state machine ebo_solve drives internally, for a caller that must put something BETWEEN "evaluate"
 * and "step".  SURVEY 8(e), reference-faithful TV mode across GPUs: every rank evaluates the data terms of its
 * patch rows (ebo_set_patches + ebo_eval), ONE all-gather of (r, J0, J1) = 24 B per patch per evaluation, and
 * the same solver replicated on every rank takes the same step (tests/test_gpu_multiprocess.py: equal to the
 * one-process ebo_solve bit for bit).
 *   ebo_lm_create: npx x npy grid, active[p] != 0 iff patch p has a data term (n_events > min_events),
 *     tv_weight / tv_huber = DetectorParams::compensateTVweight / compensateTVHuberLoss, o as ebo_solve.
 *   ebo_lm_request(flows [P][2]): the point the data terms are wanted at; returns 1 = residuals AND Jacobians
 *     wanted, 2 = residuals only, 0 = the solve has finished (flows untouched), < 0 = EBO_ERR_*.
 *   ebo_lm_supply(r [P], jac [P][2]): the data terms at that point (inactive patches ignored; jac may be NULL
 *     when only residuals were wanted).  EBO_ERR_STATE after the solve has finished.
 *   ebo_lm_result: the solution (the lowest-cost point visited, as Ceres returns it) and the summary
 *     (num_evals_* count evaluation ROUNDS of the whole problem here).
 * Host only: no device is touched, no context is needed. */
typedef struct ebo_lm ebo_lm;
int ebo_lm_create(int npx, int npy, const uint8_t* active, double tv_weight, double tv_huber, const ebo_solver_opts* o,
				  ebo_lm** out);
int ebo_lm_request(ebo_lm* lm, double* flows);
int ebo_lm_supply(ebo_lm* lm, const double* r, const double* jac);
int ebo_lm_result(const ebo_lm* lm, double* flows, ebo_summary* summary);
void ebo_lm_destroy(ebo_lm* lm);

/* Integer-valued event-count images (CV_64F in the reference), host out
 * [Wn][image_h][image_w].  aux: EBO_COUNT_WARPED -> host flows [Wn][P][2];
 * EBO_COUNT_FIELD -> host float32 field [Wn][image_h][image_w][2]; else NULL. */
int ebo_count_image(ebo_ctx* ctx, int mode, const void* aux, double* image);
/* Same with aux and image on the device; asynchronous. */
int ebo_count_image_device(ebo_ctx* ctx, int mode, const void* d_aux, double* d_image);

/* tracker::FeatureDetector::initMotionField (feature_detector.cpp:53-142): per-pixel motion
 * field from the trajectories of the tracked feature patches.  Patch k has trajectory samples
 * traj_xy[traj_offsets[k]..traj_offsets[k+1])[2], traj_t[...] (us, ascending).  The velocity of
 * the segment at `timestamp` (std::lower_bound) is stored at the rounded trajectory point; the
 * other pixels get the average (use_average, DetectorParams::useAverageFlow) or the nearest
 * fixed point's value.  field_out: host float32 [image_h][image_w][2] (may be NULL);
 * fixed_xy: host [n_patches][2] (may be NULL).  The field also stays on the device:
 * ebo_count_image(ctx, EBO_COUNT_FIELD, NULL, image) then is R4 (compensateEvents) end to end.
 * ebo_interpolate_motion_field applies interpolateMotionField's TV smoothing to it. */
int ebo_init_motion_field(ebo_ctx* ctx, int64_t timestamp, int use_average, int n_patches,
						  const size_t* traj_offsets, const double* traj_xy, const int64_t* traj_t,
						  float* field_out, int32_t* n_fixed, int32_t* fixed_xy);

/* tracker::FeatureDetector::interpolateMotionField (feature_detector.cpp:144-241) after its
 * initMotionField call, i.e. on the field ebo_init_motion_field left on the device: if
 * cv::norm(field) > 0 (:152), the per-pixel problem of :154-214 (totalVarianceFunctor, weight 1,
 * between every pixel and its right / lower neighbour for x < w-1, y < h-1; HuberLoss(1e-5) when
 * use_l1 = DetectorParams::useL1; fixed points constant) is solved by the same trust-region LM
 * as ceres::Solve with the options of :216-222 (opts == NULL) and the field is overwritten with
 * the result rounded to float32 (:230-239).  All per-pixel work runs on the device; the linear
 * solve of each LM iteration is a multigrid-preconditioned conjugate-gradient run to 1e-13
 * relative residual.
 * field_out: host float32 [image_h][image_w][2] (may be NULL; the field stays resident for
 * ebo_count_image(EBO_COUNT_FIELD)).  cg_iterations (may be NULL): total CG iterations.
 * EBO_ERR_STATE without a prior ebo_init_motion_field; EBO_ERR_RANGE for a fixed point at pixel
 * (w-1, h-1), which is no parameter block of that problem (the reference aborts inside Ceres). */
int ebo_interpolate_motion_field(ebo_ctx* ctx, int use_l1, const ebo_solver_opts* opts, float* field_out,
								 ebo_summary* summary, int32_t* cg_iterations);

/* Packed binary sidecar of an events.txt: 32-byte header + 16 bytes per event
 * {int64 t_us (the reader's truncated microseconds), int16 x, int16 y, int8 sign, 3 x 0}; reading
 * it back yields exactly the events ebo_read_events_txt parsed, at memory speed instead of ~100 ns
 * of strtod per event.  Host only.  EBO_ERR_RANGE: coordinates beyond int16 / a sign other than
 * -1, +1 (write); bad magic, truncated file or bad sign (read; events before it are kept). */
int ebo_write_events_bin(const char* path, const ebo_event* ev, size_t n);
int ebo_read_events_bin(const char* path, ebo_event* out, size_t cap, size_t* n);

/* DAVIS frames without OpenCV (cv::imread(path, CV_8U) in Davis240cReader::getImageSample,
 * davis240c_reader.cpp:93-107): a PNG of 8-bit greyscale, not interlaced -> *w, *h and the [h][w] pixels
 * (row-major, one byte each).  Host only, HIP-free (csrc/png8.h): own inflate (stored, fixed and dynamic
 * blocks), Adler-32 of the zlib stream and CRC-32 of the critical chunks checked, ancillary chunks skipped,
 * the five row filters.  pixels == NULL: only the size (IHDR read and checked).  Errors, with the message
 * in ebo_last_error(NULL): EBO_ERR_UNSUPPORTED for any other bit depth or colour type, Adam7 interlacing
 * or a preset dictionary; EBO_ERR_ARG for malformed input (truncation, a bad checksum, a stream short of
 * h * (w + 1) bytes, a side outside 1..16384, ...) or a file that cannot be read; EBO_ERR_RANGE when
 * capacity < w * h (*w, *h set).  Never reads outside [bytes, bytes + n). */
int ebo_decode_png8(const void* bytes, size_t n, int32_t* w, int32_t* h, uint8_t* pixels, size_t capacity);
int ebo_read_png8(const char* path, int32_t* w, int32_t* h, uint8_t* pixels, size_t capacity);

/* ---- per-feature tracker objective --------------------------------------
 * tracker::Optimizer::setGrad (optimizer.cpp:15-31): the image-gradient grid the tracker samples
 * with ceres::BiCubicInterpolator.  grad_x, grad_y: host [image_h][image_w] (CV_64F). */
int ebo_optimizer_set_grad(ebo_ctx* ctx, const double* grad_x, const double* grad_y);
/* ceres::Solver::Options as Optimizer::optimize sets them (optimizer.cpp:103-112;
 * OptimizerParams::maxNumIterations = 10). */
void ebo_optimizer_default_solver(ebo_solver_opts* o);
/* tracker::OptimizerCostFunctor (optimizer_cost.h:15-96) behind
 * ceres::AutoDiffCostFunction<OptimizerCostFunctor, ceres::DYNAMIC, 4, 1>::Evaluate
 * (optimizer.cpp:89-97), for n tracked patches in one launch.  rects [n][4] = cv::Rect2d
 * (x, y, width, height); patch i has m_i = int(width) * int(height) residuals, stored
 * consecutively; nabla: Patch::getNormalizedIntegratedNabla per patch ([m_i], row-major);
 * poses [n][4] = Sophus::SE2d::data() (cos, sin, tx, ty); flow_dirs [n].
 * residuals [sum m_i]; jac_pose [sum m_i][4] and jac_flow [sum m_i] are the Jacobians Ceres asks
 * for (row-major, w.r.t. the 4 stored SE2 parameters and the flow angle), both NULL = value only
 * (the double path of the functor, whose quotient rounds differently from the Jet path, as in
 * the reference).  Needs ebo_optimizer_set_grad (EBO_ERR_STATE). */
int ebo_optimizer_eval(ebo_ctx* ctx, int n, const double* rects, const double* nabla, const double* poses,
					   const double* flow_dirs, double* residuals, double* jac_pose, double* jac_flow);
/* The ceres::Solve of tracker::Optimizer::optimize (optimizer.cpp:83-119) for n tracked patches
 * in one launch: SE2 block with Sophus' LocalParameterizationSE2 + the flow angle, one residual
 * block with ceres::HuberLoss(huber) (OptimizerParams::huberLoss = 0.3), trust-region LM with the
 * options of :103-112 (opts == NULL; DENSE_QR there, a 4x4 Cholesky of the same normal equations
 * here).  normalize != 0: nabla is Patch::getIntegratedNabla and is normalised on the device as
 * Patch::getNormalizedIntegratedNabla does (patch.cpp:156-159; an all-zero patch gives NaN and
 * termination 2, parameters unchanged).  poses, flow_dirs: in = Patch::getWarp / getFlow, out =
 * the lowest-cost point visited.  summaries [n] may be NULL.
 * What a caller may rely on: a patch's result (parameters and summary, bit for bit) does not depend on the
 * other patches of the call, on their sizes, on its position in the call or on the run -- with ONE
 * exception: a call of 512 patches or more runs 128 lanes per patch, a smaller one 256, and the two sum a
 * patch's pixels in different orders.  The same patch in a call of 511 and of 512 has the same iteration,
 * evaluation and termination counts but parameters that differ at the rounding level (measured: up to
 * 8e-13 after 10 iterations, 1e-14 in the final cost); each agrees with the CPU restatement within the
 * 1e-5 asked of a solved parameter.  ebo_optimizer_eval and ebo_optimizer_cost_map always run 256 lanes:
 * no exception there.  A patch of more than 3000 pixels is EBO_ERR_UNSUPPORTED (all three entries). */
int ebo_optimizer_solve(ebo_ctx* ctx, int n, const double* rects, const double* nabla, int normalize, double huber,
						const ebo_solver_opts* opts, double* poses, double* flow_dirs, ebo_summary* summaries);

/* tracker::Optimizer::drawCostMap (optimizer.cpp:33-60; OptimizerParams::drawCostMap, costMapWidth / costMapHeight) for n
 * tracked patches in one launch: cost_maps [n][map_h][map_w], cell (y + (map_h-1)/2, x + (map_w-1)/2) = cv::norm(image, NORM_L2)
 * of the functor's residual image (its double path, as `(*c)(poseNew.data(), &flowDir, image.data)` evaluates it) at
 * poseNew = SE2(pose.log().z(), (float(x) + tx, float(y) + ty)), x = -(map_w-1)/2 .. (map_w-1)/2, y likewise (cells an even
 * size leaves unvisited stay 0, as in cv::Mat::zeros).  rects / nabla / normalize / poses / flow_dirs as for
 * ebo_optimizer_solve; the reference calls it after the solve with the functor built BEFORE it (the rect and the
 * normalised nabla of the optimisation) and the solved pose and flow.  EBO_ERR_STATE without ebo_optimizer_set_grad. */
int ebo_optimizer_cost_map(ebo_ctx* ctx, int n, const double* rects, const double* nabla, int normalize, const double* poses,
						   const double* flow_dirs, int map_w, int map_h, double* cost_maps);

/* The event-count estimate of FeatureDetector::updateNumOfEvents (feature_detector.cpp:689-707) for n
 * tracked patches in one launch: the L1 norm over the patch rect of
 * 0.6 gradX' cos(flow) + 0.6 gradY' sin(flow), gradX' / gradY' = the gradient images of
 * ebo_optimizer_set_grad warped by cv::warpAffine(..., patch.getWarp().matrix2x3(),
 * cv::WARP_INVERSE_MAP) -- flags without interpolation bits: INTER_NEAREST through OpenCV's 10-bit
 * fixed-point map, BORDER_CONSTANT 0 -- truncated to an integer as `size_t sumPatch = cv::norm(..)`
 * does.  rects [n][4] = cv::Rect2d, poses [n][4] = Sophus::SE2d::data(), flow_dirs [n], out [n].
 * The two border branches of updateNumOfEvents (:668-687) are the caller's (the facade has them).
 * EBO_ERR_STATE without ebo_optimizer_set_grad.  EBO_ERR_RANGE, before anything is uploaded, for a rect
 * whose corner is not finite or whose width or height is NaN or rounds (half to even) outside 0..32767; a
 * width or height that rounds to 0 is admitted and gives 0. */
int ebo_estimate_num_events(ebo_ctx* ctx, int n, const double* rects, const double* poses, const double* flow_dirs,
							uint64_t* out);

/* tracker::Patch::warpImage (patch.cpp:132-154; called at feature_detector.cpp:508,615) for n tracked
 * patches in one launch: predictedNabla_ = -gradX'(patch_) cos(flowDir_) - gradY'(patch_) sin(flowDir_) with
 * gradX' / gradY' = the gradient images of ebo_optimizer_set_grad warped by cv::warpAffine(...,
 * warp_.matrix2x3(), cv::WARP_INVERSE_MAP) (INTER_NEAREST through OpenCV's 10-bit fixed-point map,
 * BORDER_CONSTANT 0, as ebo_estimate_num_events) and flowDir_ the patch's double member.  rects [n][4] =
 * cv::Rect2d, poses [n][4] = Sophus::SE2d::data(), flow_dirs [n]; patch i's [cvRound(h)][cvRound(w)] image
 * goes to predicted + nabla_offsets[i].  updated[i] = 0 and nothing is written for a patch whose rect
 * touches the image border (the reference returns early at :145-150 and keeps the old predictedNabla_).
 * EBO_ERR_STATE without ebo_optimizer_set_grad.  EBO_ERR_RANGE for the rects ebo_estimate_num_events
 * refuses (a corner that is not finite, a size that is NaN or rounds outside 0..32767). */
int ebo_patch_warp_image(ebo_ctx* ctx, int n, const double* rects, const double* poses, const double* flow_dirs,
						 const size_t* nabla_offsets, double* predicted, int32_t* updated);

/* Event -> tracked-patch routing: what FeatureDetector::updatePatches does per event,
 * `if (patch.isInPatch(event.value.point)) patch.addEvent(event)` (feature_detector.cpp:585-596;
 * cv::Rect2d::contains on the integer point: x <= px < x + w, y <= py < y + h in double), for a
 * whole chunk of the stream and all tracked patches in one launch instead of one host test per
 * (event, patch).  ebo_route_set_events keeps the chunk's coordinates on the device (4 B/event);
 * ebo_route_events then gives, for patch i with rect rects[i][4], the indices (ascending = stream
 * order) of the first max_take[i] events at or after start[i] that fall inside it:
 * out_index[i * cap + k], k < out_count[i] <= min(max_take[i], cap), and out_next[i] = index after
 * the last event taken when the quota was reached, else n (chunk exhausted).  A patch's rect moves
 * when it is optimised, so a caller routes up to the event that makes a patch ready, optimises,
 * and routes again from out_next with the new rect (tracker::FeatureDetector::updatePatches(chunk)
 * in the facade does exactly that, all patches in lock step). */
int ebo_route_set_events(ebo_ctx* ctx, const ebo_event* ev, size_t n);
int ebo_route_events(ebo_ctx* ctx, int n_patches, const double* rects, const uint32_t* start,
					 const uint32_t* max_take, uint32_t cap, uint32_t* out_index, uint32_t* out_count,
					 uint32_t* out_next);

/* Diagnostic (bench.py's edge_roofline): ONE evaluation of the edge loss at d_flows (device, [Wn][P][2]) that
 * also counts the work it is made of, summed over the units that pass the empty-window test of
 * contrast_functor.h:159-165 -- out[0] units, [1] their events, [2] pixels of their bounding boxes, [3] pixels
 * of the eigenvalue region, [4] non-maximum-suppression windows, [5] argmax entries of the reverse pass
 * (0 without want_jac).  DESIGN.md 4.5 turns them into useful f64 operations.  Synchronous; the
 * evaluation's (r, J) go to the context's own result buffer. */
int ebo_edge_work_stats(ebo_ctx* ctx, const double* d_flows, int want_jac, uint64_t* out);

/* Diagnostic (bench.py's roofline.lds): the chip-wide rates of 64-bit LDS atomic adds (gops[0]) and single 64-bit LDS reads
 * (gops[1]) in the evaluation kernels' own access shape -- per lane a random base slot, then the 49 taps of a 7 x 7 footprint
 * at immediate offsets --, in 1e9 operations per second, measured NOW on the context's device (4 workgroups of 256 lanes
 * per CU, 42 footprints per lane, best of three; tools/microbench/lds_atomics.hip "7x7 taps, any base"): the rates the
 * scatter and the gather pass of the variance evaluation are priced against.  Synchronous. */
int ebo_lds_rates(ebo_ctx* ctx, double* gops);

/* Diagnostic (tests/test_gpu_bucket_edges.py): the packed 8-byte records of ONE unit as they lie in device memory, in
 * their order there -- lo word x:15 | polarity:1 | y:15 | 0, hi word uint32(int32(t_ref(unit) - t)).  bucket = 0 .. P-1
 * for the grid patches of `window` and P for its stray bucket; after ebo_set_patches window = 0 and bucket = the patch
 * index.  *n receives the unit's size.  EBO_ERR_ARG for a bad index, a null pointer or cap < *n (*n is still set then);
 * EBO_ERR_STATE while a graph is being recorded.  Synchronous; changes nothing. */
int ebo_unit_records(ebo_ctx* ctx, int window, int bucket, uint64_t* out, size_t cap, size_t* n);

/* Diagnostic (tests/test_gpu_launch_order.py): the launch-order table as it lies in device memory -- entry q is the index
 * (window * (P + 1) + bucket; after ebo_set_patches the patch index) of the unit that workgroup q of a variance evaluation
 * or a device-resident solve takes: descending event count of the active units, every other unit behind them, ties by
 * index.  *n receives the number of units.  EBO_ERR_ARG with nothing loaded, a null count or cap < *n (*n is still set
 * then); EBO_ERR_STATE while a graph is being recorded.  Synchronous; changes nothing. */
int ebo_launch_order(ebo_ctx* ctx, uint32_t* out, size_t cap, size_t* n);

/* Diagnostic (tests/test_gpu_box_extents.py): the time-extent table behind the variance evaluation's bounding box as it
 * lies in device memory -- per unit (index as in ebo_launch_order) a slot of 258 int32: status (1 valid, 0 no table: stray
 * bucket, rect wider or taller than 64, or an event outside the rect) | 0 | (dtMin, dtMax) of source columns 0 .. rw-1 |
 * of source rows 0 .. rh-1, dt = int32(t_ref(unit) - t); an empty column or row, and every pair behind the last row,
 * holds (INT32_MAX, INT32_MIN).  *n receives the number of int32.  Errors as ebo_launch_order.  Synchronous; changes
 * nothing. */
int ebo_unit_extents(ebo_ctx* ctx, int32_t* out, size_t cap, size_t* n);

/* Diagnostic, A/B build only (same test): of the units the last ebo_eval / ebo_eval_device variance evaluation evaluated
 * (first flow set), how many took their bounding box from a pass over their events and how many from the table.  Either
 * pointer may be null.  EBO_ERR_STATE in the shipped build and while a graph is being recorded.  Synchronous. */
int ebo_box_path_counts(ebo_ctx* ctx, unsigned int* from_events, unsigned int* from_extents);

/* Diagnostic, A/B build only (tests/test_gpu_eval_interior.py): of the units the last ebo_eval / ebo_eval_device variance
 * evaluation evaluated (first flow set), how many ran their event passes without the per-event reject, row and clip tests
 * (csrc/eval_interior.h: box from the table, not cut by the canvas, one row tile, one sub-band); 0 with
 * EBO_EVAL_INTERIOR=0.  The pointer may be null.  EBO_ERR_STATE in the shipped build and while a graph is being recorded.
 * Synchronous. */
int ebo_interior_path_counts(ebo_ctx* ctx, unsigned int* interior);

/* Diagnostic, A/B build only (tests/test_gpu_eval_deal.py): the dealt list of ONE unit (index as in ebo_launch_order) --
 * the order in which the variance evaluation's tap passes walk its events at the flows d_flows [slots][2] (device):
 * entry q is the position, in the unit's canonical order (ebo_unit_records), of the event that lane q mod block takes in
 * round q div block (csrc/eval_deal.h).  Runs one evaluation (want_jac as ebo_eval_device) into d_out [slots][3]
 * (device).  *n receives the list's length: the unit's event count, or 0 where the unit is not dealt (inactive, outside
 * the admission bounds, no room behind its image, EBO_EVAL_DEAL=0) -- it is then evaluated in the canonical order.
 * EBO_ERR_ARG for a bad index, a null pointer or cap < the unit's event count; EBO_ERR_STATE in the shipped build, with the
 * edge loss and while a graph is being recorded.  Synchronous. */
int ebo_unit_deal(ebo_ctx* ctx, int unit, const double* d_flows, int want_jac, double* d_out, uint16_t* out, size_t cap, size_t* n);

/* Diagnostic (same test): the shape ebo_eval / ebo_eval_device give the variance evaluation of the loaded units -- row
 * tiles per unit, lanes per workgroup, flow sets (5 with EBO_GRAD_CENTRAL and a Jacobian, else 1).  Any pointer may be
 * null.  Launches nothing.  EBO_ERR_STATE with nothing loaded or the edge loss. */
int ebo_eval_launch_shape(ebo_ctx* ctx, int want_jac, int* tiles, int* block, int* flow_sets);

/* Diagnostic (tests/test_gpu_eval_residency.py): the workgroups of that launch one CU keeps resident -- *planned as the
 * launch plan intends (csrc/eval_plan.h), *actual as the runtime's occupancy query answers for the kernel instantiation,
 * the block and the dynamic LDS the launch would use.  Either pointer may be null.  Launches nothing.  Errors as
 * ebo_eval_launch_shape. */
int ebo_eval_resident_workgroups(ebo_ctx* ctx, int want_jac, int* planned, int* actual);

/* Diagnostic (bench.py): the traffic of ebo_count_image_device with no work -- every packed event of the
 * loaded windows read once (16-byte loads), every pixel of d_image [Wn][image_h][image_w] written once
 * (16-byte stores, all 0.0) -- as the in-run yardstick of the HBM-bound count kernels: what a plain stream
 * of these bytes reaches on this GPU.  *bytes (may be NULL) receives the bytes moved.  Asynchronous. */
int ebo_stream_yardstick_device(ebo_ctx* ctx, double* d_image, uint64_t* bytes);

/* R2's final loop (:433-463) for windows whose PATCHES ARE SHARDED over ranks (BASELINE
 * config 4).  The context was loaded by ebo_set_patches with n_windows equal groups of units (group w =
 * this rank's patches of window w with the events inside them); flows_grid [n_windows][P][2] are the flows
 * of ALL P patches of the context's grid (every rank has them after the all-gather of the solved flows);
 * window_t_ref_us [n_windows] (host) is each WINDOW's reference time (:305-306), which a shard cannot
 * derive from its own events: ebo_window_ref_time(first, last) of the whole window's first / last event
 * time.  image [n_windows][image_h][image_w] receives the counts of THIS context's events only, each
 * warped by the flow of the grid patch its own coordinates select (:436-441); the sum of the ranks'
 * images (ebo_reduce_sum_device, or any reduce: integer-valued doubles add exactly) is the image
 * ebo_compensate_events_contrast returns for the whole window.  _device: pointers on the device,
 * asynchronous.  EBO_ERR_STATE without ebo_set_patches. */
int ebo_window_ref_time(int64_t t_first_us, int64_t t_last_us, int64_t* t_ref_us);
int ebo_count_image_shard(ebo_ctx* ctx, int n_windows, const int64_t* window_t_ref_us, const double* flows_grid,
						  double* image);
int ebo_count_image_shard_device(ebo_ctx* ctx, int n_windows, const int64_t* window_t_ref_us,
								 const double* d_flows_grid, double* d_image);

/* The same image BAND-LIMITED ("each GPU writes its own row-block; events warped across a
 * shard border need a halo"): a rank's events start in the image rows of its patch rows [own_row0,
 * own_row1) and leave them only by max|dt| * scale * |flow|, so the rank counts them into a band = its own
 * rows + `halo` rows above and below (clipped to the image), keeps the own rows and sends only the halo
 * rows to the two neighbouring ranks -- instead of reducing a full image per window from every rank onto one.
 *   ebo_band_plan            host only.  row_bounds [nranks + 1]: rank q owns image rows [row_bounds[q],
 *                            row_bounds[q + 1]) (0 ... image_h, rank order = row order).  Fills *out for `rank`.
 *                            EBO_ERR_UNSUPPORTED when some rank's halo would not fit inside its neighbour's rows
 *                            (the same verdict on every rank: all decide from the same numbers).
 *   ebo_count_image_band_device   counts this context's events (ebo_set_patches, as for ebo_count_image_shard)
 *                            into d_top [n_windows][own_row0 - band_row0][W], d_own [n_windows][own rows][W],
 *                            d_bottom [n_windows][band_row1 - own_row1][W] (uint32 counts; LDS tiles, no global
 *                            atomics).  *d_escaped (int32, device) becomes 1 when a unit's flow could carry an event
 *                            to an image row outside the band (then the caller falls back to
 *                            ebo_count_image_shard + reduce), else 0.  EBO_ERR_UNSUPPORTED when a unit's events select
 *                            more than one grid patch (arbitrary rects: use ebo_count_image_shard).  Asynchronous.
 *   ebo_band_exchange_device (ebo_comm_init) d_top -> rank - 1, d_bottom -> rank + 1, the neighbours' halos into
 *                            d_from_above [n_windows][recv_above][W] and d_from_below [n_windows][recv_below][W]
 *                            (one grouped ncclSend / ncclRecv), then *d_escaped = max over the ranks (ncclAllReduce of
 *                            one int): every rank takes the same fallback decision.  Without a communicator: no-op.
 *   ebo_band_finish_device   d_image_own [n_windows][own rows][W] (CV_64F) = own + received halos.
 *   ebo_band_gather_device   (ebo_comm_init) only when one rank wants the whole image: every rank's d_image_own into
 *                            d_full [n_windows][image_h][W] on `root` (grouped send / recv of the owned rows only).
 * Bytes a rank sends per window: (rows of top + rows of bottom) x W x 4. */
typedef struct ebo_band
{
	int band_row0, own_row0, own_row1, band_row1; /* image rows: band = [band_row0, band_row1), own inside it */
	int recv_above, recv_below;                   /* rows of the own region the neighbours' halos cover */
} ebo_band;
int ebo_band_plan(int image_h, const int* row_bounds, int nranks, int rank, int halo, ebo_band* out);
int ebo_count_image_band_device(ebo_ctx* ctx, int n_windows, const int64_t* window_t_ref_us, const double* d_flows_grid,
								const ebo_band* band, uint32_t* d_top, uint32_t* d_own, uint32_t* d_bottom, int32_t* d_escaped);
int ebo_band_exchange_device(ebo_ctx* ctx, int n_windows, const ebo_band* band, const uint32_t* d_top, const uint32_t* d_bottom,
							 uint32_t* d_from_above, uint32_t* d_from_below, int32_t* d_escaped);
int ebo_band_finish_device(ebo_ctx* ctx, int n_windows, const ebo_band* band, const uint32_t* d_own, const uint32_t* d_from_above,
						   const uint32_t* d_from_below, double* d_image_own);
int ebo_band_gather_device(ebo_ctx* ctx, int n_windows, const int* row_bounds, const double* d_image_own, int root, double* d_full);

/* R2 in one call: set window, solve, final warped count image.
 * flows_out [P][2], image_out [image_h][image_w] (may be NULL). */
int ebo_compensate_events_contrast(ebo_ctx* ctx, const ebo_event* ev, size_t n,
								   const ebo_solver_opts* o, double* flows_out,
								   double* image_out, ebo_summary* summary);

/* ---- recordings: many windows per call ------------------------------------------------------
 * tools::Evaluator::eventCallback's window rule (evaluator.cpp:32-45) together with FeatureDetector::addEvent's
 * truncation (feature_detector.cpp:621-628), applied to a time-ordered stream.  Window w is ev[begin[w] .. end[w]).
 * Host only.  Event by event: the event joins the held ones, the oldest are dropped while more than max_store
 * (maxNumEventsToStore) are held, THEN the window fires when ts - lastCompensation >= time_us
 * (compensationFrequencyTime) or when count (compensationFrequencyEvents) are held; the triggering event is the
 * window's last, and lastCompensation becomes its timestamp.  lastCompensation starts at last_compensation_us (0 in a
 * fresh detector, so the first event of a recording usually fires a one-event window); with count > max_store only
 * the time rule can fire.  *last_compensation_out: lastCompensation after the stream; *pending_begin: the first event
 * no window took (the events held at the end, which a streaming caller carries into its next call).
 * EBO_ERR_RANGE when cap is too small: *n_windows is then the number of windows needed, nothing else is valid.
 * EBO_ERR_ARG for max_store == 0 or a null pointer. */
int ebo_cut_windows(const ebo_event* ev, size_t n, int64_t last_compensation_us, uint32_t time_us, uint32_t count,
					uint64_t max_store, size_t* begin, size_t* end, size_t cap, size_t* n_windows,
					int64_t* last_compensation_out, size_t* pending_begin);

/* R2 + R3 for many windows: window w = ev[offsets[w] .. offsets[w+1]) (host memory), each solved from flow 0 like
 * ebo_compensate_events_contrast on that window alone.  The windows go through in chunks that fit the context's
 * max_windows / max_events; per chunk: ebo_set_windows, ebo_solve with o (either mode), ebo_count_image(WARPED) at the
 * chunk's flows and ebo_count_image(INTEGRATED) on the same loaded events -- each event is uploaded once.
 * Outputs per window: flows_out [Wn][P][2], warped_out [Wn][image_h][image_w] (R2's final image),
 * integrated_out [Wn][image_h][image_w] (R3), summary [Wn], status [Wn]; all but flows_out may be NULL.
 * A window the one-window path refuses (empty; a coordinate or a time outside the packed range, found by the loader;
 * more events than max_events) fails ALONE: status[w] = EBO_ERR_*, its outputs are left as they were, and the other
 * windows of its chunk are loaded again without it.  Returns EBO_OK when every window succeeded, else the code of the
 * first window that failed (ebo_last_error names it).  EBO_ERR_STATE while a graph is being recorded. */
int ebo_compensate_windows(ebo_ctx* ctx, const ebo_event* ev, const size_t* offsets, int n_windows,
						   const ebo_solver_opts* o, double* flows_out, double* warped_out, double* integrated_out,
						   ebo_summary* summary, int32_t* status);

/* R5/R6 batched over tracked feature patches.  Patch i owns events
 * ev[offsets[i]..offsets[i+1]) in deque order (front = newest), a cv::Rect2d
 * rects[i][4] = (x,y,w,h), and writes a [int(h)][int(w)] signed count image at
 * nabla + nabla_offsets[i].  For R6, traj[i][6] = (prelast x,y,t_us, last x,y,t_us)
 * and mid_time[i]; updated[i] tells whether R6's time test passed.
 * Rect sizes: w and h are whole numbers >= 1 with w * h <= 16384, as Patch builds them
 * (2 * extent + 1); x and y may be fractional (updatePatchRect).  A w or h that is not finite
 * or not whole returns EBO_ERR_ARG (the [int(h)][int(w)] image could not hold every event the
 * rect contains); a whole one below 1, or w * h > 16384, returns EBO_ERR_UNSUPPORTED.  Every
 * rect is checked before anything is written: on either error nabla, current_ts,
 * time_last_update and updated are as the caller left them.
 * Only the images are written: every word of nabla outside [nabla_offsets[i], nabla_offsets[i]
 * + w * h) stays the caller's, whatever the order of the offsets and the gaps between them, and
 * so does the image of a patch that fails R6's time test.  Images must not overlap.  Patch i
 * without events (offsets[i] == offsets[i+1]) gets a zero image from ebo_patch_integrate and
 * keeps its current_ts / time_last_update entry; R6 leaves it untouched with updated[i] = 0. */
int ebo_patch_integrate(ebo_ctx* ctx, const ebo_event* ev, const size_t* offsets,
						int n_patches, const double* rects, const size_t* nabla_offsets,
						double* nabla, int64_t* current_ts, int64_t* time_last_update);
int ebo_patch_integrate_mc(ebo_ctx* ctx, const ebo_event* ev, const size_t* offsets,
						   int n_patches, const double* rects, const double* traj,
						   const int64_t* mid_time, const size_t* nabla_offsets,
						   double* nabla, int32_t* updated);

/* DAVIS240C events.txt reader, Davis240cReader::getEventSample
 * (tools/dataset_reader/src/davis240c_reader.cpp:60-92): "<seconds> <x> <y> <0|1>" per
 * line -> out[0..*n), at most cap events.  Host only; EBO_ERR_RANGE on a malformed line or a
 * sign other than 0/1 (the reference throws there), events parsed before it are kept. */
int ebo_read_events_txt(const char* path, ebo_event* out, size_t cap, size_t* n);
/* The same in pieces, as Davis240cReader::getEvents reads a recording (davis240c_reader.cpp:186-212: EVENT_LENGTH =
 * 1 000 000 lines per call, the next call continues behind them): at most cap events from byte *offset of the file on;
 * *offset moves behind the last line taken (start with 0; *n == 0 with EBO_OK = the end of the file). */
int ebo_read_events_txt_at(const char* path, uint64_t* offset, ebo_event* out, size_t cap, size_t* n);
/* Both of them parse on the host's threads since round 5, as the reference's reader does (DatasetReader::readFile,
 * tools/dataset_reader/include/dataset_reader/dataset_reader.h:33-97: hardware_concurrency() threads over the mapped
 * file): the mapped byte range is cut at line breaks into one chunk per thread (EBO_HOST_THREADS, default: the
 * machine's hardware threads).  Events, *n, *offset and the error are those of a single-thread walk whatever the
 * thread count.  This form takes the thread count from the caller (0: the default; offset may be NULL) and reports
 * how many threads parsed (threads_used, may be NULL). */
int ebo_read_events_txt_threads(const char* path, uint64_t* offset, ebo_event* out, size_t cap, size_t* n, int threads,
								int* threads_used);
/* The same reader writing the compact 8-byte records ebo_set_windows8 takes (a third of the bytes; no 24-byte array
 * between the text and the device): *t_base = the time stamp of the first event of THIS call, every record's t_rel_us is
 * relative to it -- pass it as t_base[w] of every window cut from the call's events.  offset may be NULL (from the start);
 * threads 0 = the default.  EBO_ERR_RANGE also for an event a compact record cannot hold (a coordinate beyond +-16384, a
 * time further than 2^31 us from the base): it stays in front of that line, as for a malformed one. */
int ebo_read_events_txt8(const char* path, uint64_t* offset, ebo_event8* out, size_t cap, size_t* n, int64_t* t_base, int threads);

/* Contiguous shard [begin,end) of n_units for rank of world (multi-GPU, §8e). */
int ebo_shard_range(int n_units, int rank, int world, int* begin, int* end);

/* Multi-GPU exchange (one process per GPU, RCCL over xGMI) for callers without a framework:
 * rank 0 makes an id (ebo_comm_unique_id) and hands its 128 bytes to the other ranks by any
 * means; every rank calls ebo_comm_init on its context; ebo_allgather_device gathers
 * count_per_rank doubles from every rank into d_recv [nranks][count_per_rank] on every rank,
 * asynchronously on the context's stream -- the single all-gather of the solved flows (or of
 * the (r, J0, J1) triples) of SURVEY 8(e).  librccl.so is loaded on first use only. */
typedef struct ebo_comm_id
{
	char internal[128];
} ebo_comm_id;
int ebo_comm_unique_id(ebo_comm_id* id);
int ebo_comm_init(ebo_ctx* ctx, const ebo_comm_id* id, int rank, int nranks);
int ebo_allgather_device(ebo_ctx* ctx, const double* d_send, double* d_recv, size_t count_per_rank);
/* Rank and size of the context's communicator (0 and 1 without one). */
int ebo_comm_size(const ebo_ctx* ctx, int* rank, int* nranks);
/* Element-wise sum over the ranks of count doubles, asynchronously on the context's stream: into d_recv on
 * `root` (ncclReduce; d_recv may be NULL elsewhere) or, root < 0, on every rank (ncclAllReduce).  The one
 * reduce of SURVEY 8(e)'s "final full-frame count image": the per-rank partial images of
 * ebo_count_image_shard are integer-valued doubles, so the sum is exact in whatever order RCCL adds. */
int ebo_reduce_sum_device(ebo_ctx* ctx, const double* d_send, double* d_recv, size_t count, int root);
int ebo_comm_destroy(ebo_ctx* ctx);

/* One sample of a tracked feature's trajectory, the record tools::Evaluator::saveFeaturesTrajectory
 * writes as "feature_id timestamp x y" (tools/evaluator/src/evaluator.cpp:125-150): Patch::getTrackId()
 * and one common::Sample<Point2d> of Patch::getTrajectory(). */
typedef struct ebo_track_point
{
	int64_t id;   /* Patch::getTrackId()                 */
	int64_t t_us; /* pos.timestamp (microseconds)        */
	double x, y;  /* pos.value                           */
} ebo_track_point;

/* The exchange of BASELINE config 5 (independent sequences, one per GPU): every rank
 * contributes the n_local track points of ITS sequence (host memory, any count, 0 allowed) and
 * every rank receives all of them, rank 0's first, each rank's in the order given.  Two
 * collectives on the context's stream: an all-gather of the counts, then ONE ncclAllGather of
 * max-count-padded 32-byte records; the padding is dropped on the way back to the host.
 * all [cap] (host) receives *n_all records; counts [nranks = ebo_comm_size] (may be NULL) the per-rank
 * counts.  EBO_ERR_STATE without ebo_comm_init; EBO_ERR_ARG when cap is too small (*n_all and counts are
 * still set, nothing is written to all).  Synchronous.  Every rank of the communicator must call it, and a
 * rank whose cap is too small still takes part in BOTH collectives before it returns the error, so the
 * others never wait for it; size the buffer with ebo_allgather_track_counts (the counts collective alone,
 * also on every rank) rather than with a cap = 0 call. */
int ebo_allgather_tracks(ebo_ctx* ctx, const ebo_track_point* local, size_t n_local, ebo_track_point* all,
						 size_t cap, size_t* n_all, size_t* counts);
int ebo_allgather_track_counts(ebo_ctx* ctx, size_t n_local, size_t* n_all, size_t* counts);

/* trajectory.txt as saveFeaturesTrajectory writes it (evaluator.cpp:125-150): one line
 * "<id> <seconds> <x> <y>" per point, std::fixed with 8 decimals, seconds =
 * std::chrono::duration<double>(timestamp).  Host only.  ebo_read_tracks_txt parses that format
 * back (seconds -> microseconds rounded to nearest); EBO_ERR_RANGE on a malformed line (*n = the records
 * before it); EBO_ERR_ARG when the file holds more than cap records (*n = the number it holds, out = the
 * first cap of them): a list is never truncated silently. */
int ebo_write_tracks_txt(const char* path, const ebo_track_point* pts, size_t n);
int ebo_read_tracks_txt(const char* path, ebo_track_point* out, size_t cap, size_t* n);

/* ---- image front end (FeatureDetector::newImage without OpenCV) ------------------------------
 * Images are 8-bit grey, [image_h][image_w] row-major, at the context's ebo_params size.  Every
 * entry is synchronous and returns EBO_ERR_STATE while a graph is being recorded.  Agreement with
 * OpenCV is by construction of the rules below, not bit for bit: OpenCV is not a dependency, and the
 * rules are what the tests restate on the CPU.  refl(i, n) is BORDER_REFLECT_101 (..., 2, 1 | 0 .. n-1 | n-2, ...).
 *
 * ebo_image_gradients: FeatureDetector::getLogImage + getGradients (feature_detector.cpp:713-731).
 *   L[v] = std::log(v * (1.0 / 255.0) + 0.1) / 8 for v = 0..255, a table evaluated on the host in
 *   double (convertTo with alpha 1/255, + 10e-2, cv::log, / 8).  cv::log is OpenCV's own
 *   approximation, so the table agrees with OpenCV only to a few ulp; that cannot be checked without it.
 *   Then the separable 3x3 Sobel of cv::Sobel(L, CV_64F, dx, dy, 3), indices through refl(), in double,
 *   one rounding per operation in exactly this association (no contraction):
 *     grad_x: r(x, y) = L(x+1, y) - L(x-1, y);                gx = (r(x, y-1) + 2 * r(x, y)) + r(x, y+1)
 *     grad_y: s(x, y) = (L(x-1, y) + 2 * L(x, y)) + L(x+1, y); gy = s(x, y+1) - s(x, y-1)
 *   grad_x, grad_y: host double [image_h][image_w]; what ebo_optimizer_set_grad takes.
 *
 * ebo_good_features: cv::goodFeaturesToTrack(image, corners, max_corners, quality_level, min_distance, mask,
 *   block_size, useHarrisDetector = true, harris_k) (feature_detector.cpp:568-583):
 *   1. dx, dy: integer 3x3 Sobel of the image (refl()).  A, B, C: block_size x block_size box sums of
 *      dx*dx, dx*dy, dy*dy (window rows / columns i - block_size/2 .. i - block_size/2 + block_size - 1, the
 *      moment image read through refl()); exact in integers.
 *   2. R = (double)(A*C - B*B) - harris_k * ((double)(A+C) * (double)(A+C)): the determinant exact in int64,
 *      then the double operations rounded in this order.  OpenCV's positive scale of the derivatives changes
 *      no selection and is dropped; where two responses differ by less than OpenCV's float32 rounding the
 *      order can differ from OpenCV's float32 pipeline.
 *   3. maxVal = max of R over mask != 0 (all pixels with mask == NULL); T = R where R > quality_level * maxVal, else 0.
 *   4. Candidates: 1 <= x <= w-2, 1 <= y <= h-2, mask != 0, T != 0 and T equal to the maximum of T over its 3x3
 *      neighbourhood (pixels outside the image do not count).
 *   5. Sorted by R descending, ties by LARGER raster index y*w + x first (OpenCV >= 3.4's comparator; the
 *      reference's OpenCV 3.2 leaves ties unspecified).
 *   6. Greedy in that order: a candidate is accepted when no accepted corner lies at Euclidean distance
 *      < min_distance ((dx*dx + dy*dy) < min_distance * min_distance in double); stop at max_corners.
 *   corners_xy: host float [max_corners][2] (x, y); *n_out = corners found.  The list is deterministic.
 *   max_corners >= 1, 1 <= block_size <= 7, else EBO_ERR_ARG.
 *
 * ebo_lk_add_image: FlowEstimator::addImage (flow_estimator.cpp:16-25).  Builds the image's pyramid and the
 *   Scharr derivatives of every level on the device; the context keeps the last two images (the newer one
 *   becomes the older one on the next call, nothing is recomputed).
 *   Pyramid: level l+1 = cv::pyrDown(level l): 5x5 kernel [1 4 6 4 1]^T [1 4 6 4 1], source read through
 *   refl(), (sum + 128) >> 8; size ((w+1)/2, (h+1)/2).  Levels are built while the new level is at least 2 x 2,
 *   at most 8.
 *   Derivatives (calcSharrDeriv), int16 per level: v0 = 3*(I(x, y-1) + I(x, y+1)) + 10*I(x, y), v1 = I(x, y+1) -
 *   I(x, y-1); Ix = v0(x+1) - v0(x-1), Iy = 3*(v1(x-1) + v1(x+1)) + 10*v1(x), all indices through refl().
 *
 * ebo_lk_track: cv::calcOpticalFlowPyrLK(older, newer, prev_xy, next_xy, status, err, (win_w, win_h), max_level,
 *   TermCriteria(COUNT + EPS, max_count, epsilon), flags 0, min_eig_threshold) for n points in one launch
 *   (flow_estimator.cpp:86-108 calls it per point with (21, 21), 3, (30, 0.01), 1e-4).  EBO_ERR_STATE before two
 *   images were added.  Rules (Bouguet; float32 arithmetic, one rounding per operation, no contraction):
 *   - Levels: the pyramid is used up to the first level l < max_level whose next level is not larger than the
 *     window in both dimensions ((w_{l+1} <= win_w || h_{l+1} <= win_h) stops at l), at most max_level.
 *   - Image reads: I, J at (x, y) for -win <= x < w + win read refl(); derivatives read 0 outside the level.
 *   - Bilinear with 14-bit weights: a, b = fractional parts (float), w00 = rint((1-a)*(1-b)*16384), w01 =
 *     rint(a*(1-b)*16384), w10 = rint((1-a)*b*16384), w11 = 16384 - w00 - w01 - w10 (rint: half to even);
 *     image samples descale by 9 bits ((s + 256) >> 9, 5 fractional bits kept), derivative samples by 14 bits.
 *   - Per level l from the top: result = prev_xy / 2^l at the top level, else 2 * result; p = prev_xy / 2^l - half,
 *     half = ((win_w-1)/2, (win_h-1)/2) as float; q = result - half.  floor(p) outside [-win, w_l) x [-win, h_l):
 *     status = 0 at level 0, the level is skipped otherwise.  G = the window's sums of IxIx, IxIy, IyIy, exact in
 *     int64, times 2^-20 as float; D = G11*G22 - G12*G12; minEig = ((G22 + G11) - sqrt((G11-G22)*(G11-G22) +
 *     (4*G12)*G12)) / (2*win_w*win_h).  minEig < (float)min_eig_threshold or D < FLT_EPSILON: status = 0 at level 0,
 *     the level is skipped otherwise.
 *   - Iteration k < max_count: floor(q) outside [-win, w_l) x [-win, h_l): status = 0 at level 0, stop.  b = the sums of
 *     (J(q) - I(p)) * (Ix, Iy), exact in int64, times 2^-20 as float; delta = ((G12*b2 - G22*b1) * (1/D),
 *     (G12*b1 - G11*b2) * (1/D)); q += delta; result = q + half.  Stop when (double)dx^2 + (double)dy^2 <=
 *     epsilon^2; for k > 0 take the half-step exit when |delta + delta_prev| < 0.01 in both components:
 *     result -= 0.5 * delta, stop.
 *   - Then, with status 1: floor(result - half) outside the level-0 bounds gives status 0; err = sum |J - I| over
 *     the window at the result (integer sum) / (32 * win_w * win_h) as float (OpenCV computes it whenever an
 *     error vector is passed, as the reference does; its position check applies with err == NULL too).
 *   prev_xy, next_xy: host float [n][2]; status: host uint8 [n]; err: host float [n] (may be NULL).
 *   err is 0 where status is 0.  As OpenCV, max_count is clamped to 100 and epsilon to 10.
 *   3 <= win_w, win_h and win_w * win_h <= 1024, 0 <= max_level <= 7, max_count >= 1, else EBO_ERR_ARG.  Bit
 *   parity with OpenCV is not claimed (its sums are float, in a SIMD-dependent order). */
int ebo_image_gradients(ebo_ctx* ctx, const uint8_t* image, double* grad_x, double* grad_y);
int ebo_good_features(ebo_ctx* ctx, const uint8_t* image, const uint8_t* mask, int max_corners, double quality_level,
					  double min_distance, int block_size, double harris_k, float* corners_xy, int* n_out);
int ebo_lk_add_image(ebo_ctx* ctx, const uint8_t* image);
int ebo_lk_track(ebo_ctx* ctx, int n, const float* prev_xy, float* next_xy, uint8_t* status, float* err, int win_w,
				 int win_h, int max_level, int max_count, double epsilon, double min_eig_threshold);

/* ---- camera model (common::CameraModel, camera_model.h:27-126) --------------------------------
 * Pinhole + radial-tangential distortion.  ebo_camera is common::CameraModelParams<double> (camera_model.h:13-24)
 * in ITS field order -- fx fy cx cy k1 k2 k3 p1 p2 -- not calib.txt's (fx fy cx cy k1 k2 p1 p2 k3; the recording
 * reader untangles that).  All arithmetic is float64, one rounding per operation in exactly the association written
 * here (no contraction); tests/camera_ref.py restates it.
 *   tangential(pa, pb, a, b, r2) = ((2 * pa) * a) * b + pb * (r2 + (2 * a) * a)      (getTangentialDistortion, :35-40)
 *   radial(r2)                   = (1 + k1 * r2) + (k2 * r2) * r2                     (getRadialDistortion, :42-47;
 *                                  k3 is carried in the struct and never used, as there)
 *   undistort(u, v) (:91-106):   xD = (u - cx) / fx, yD = (v - cy) / fy; (xOpt, yOpt) = (xD, yD); TEN times:
 *                                  r2 = xOpt * xOpt + yOpt * yOpt; rad = radial(r2);
 *                                  dX = tangential(p1, p2, xOpt, yOpt, r2); dY = tangential(p2, p1, yOpt, xOpt, r2);
 *                                  xOpt = (xD - dX) / rad; yOpt = (yD - dY) / rad
 *                                ten fixed-point steps, not an inverse to convergence, as there.
 *   unproject(u, v) (:79-114):   (xOpt, yOpt) = undistort(u, v); norm = sqrt((xOpt * xOpt + yOpt * yOpt) + 1);
 *                                bearing = (xOpt / norm, yOpt / norm, 1 / norm)
 *   project(x, y, z) (:49-77):   xP = x / z, yP = y / z; r2 = xP * xP + yP * yP; rad = radial(r2);
 *                                xDist = xP * rad + tangential(p1, p2, xP, yP, r2);
 *                                yDist = yP * rad + tangential(p2, p1, yP, xP, r2); (fx * xDist + cx, fy * yDist + cy)
 *                                (ebo_camera_project and the frame remap below; common::CameraModel in the C++
 *                                facade is the same rule on the host)
 *
 * ebo_camera_unproject: n points uv [n][2] -> unit bearing vectors bearing_out [n][3], host float64 arrays
 *   (replaces the per-corner cameraModel_->unproject calls of visual_odometry.cpp:234,367,369,516,518);
 *   synchronous.  The _device form takes device pointers and runs asynchronously on the context's stream.  The
 *   parameters are not validated (fx == 0 gives the infinities the rule gives).  Both return EBO_ERR_STATE
 *   while a graph is being recorded.
 *
 * ebo_set_rectification: builds, for every sensor pixel (x, y) of the context's image size, the map
 *     (xOpt, yOpt) = undistort(x, y); u = fx * xOpt + cx; v = fy * yOpt + cy          (float64 [image_h][image_w][2])
 *   and the lookup table (round(u), round(v)), half away from zero (the rounding of the reference's count images,
 *   feature_detector.cpp:446-453), int16 [image_h][image_w][2].  The rectified camera keeps fx fy cx cy.
 *   Refused with EBO_ERR_RANGE, so that the loaders need no new error path: fx or fy not finite or zero, a pixel
 *   whose map is not finite, a rounded coordinate outside [-16384, 16383] (what an event record holds).  A refused
 *   call leaves NO rectification set.  EBO_ERR_STATE while a graph is being recorded.
 *   While a rectification is set, every loader that buckets events by the patch grid reads them through the table:
 *   ebo_set_window, ebo_set_windows, ebo_set_windows_device, ebo_set_windows8, ebo_set_windows8_device, and through
 *   them ebo_compensate_events_contrast and ebo_compensate_windows.  The caller's events are not modified.  An event
 *   whose RAW coordinate lies outside the sensor is left as it is (a stray stays a stray); an in-sensor event whose
 *   table entry lies outside the sensor goes to its window's stray unit.  The result is bit for bit that of loading
 *   the events with their coordinates replaced on the host, with no rectification set; everything after the load
 *   (objective, solves, count images) then works in rectified geometry.
 *   It affects the NEXT load, never the windows already resident.
 *   NOT rectified: ebo_route_set_events and the tracker objective (they align events with frame gradients; a caller
 *   that rectifies its frames with ebo_rectify_image hands them rectified events), ebo_patch_integrate*, the float32 motion field of EBO_COUNT_FIELD, and ebo_set_patches,
 *   which returns EBO_ERR_UNSUPPORTED while a rectification is set instead of silently ignoring it.
 * ebo_clear_rectification: later loads read raw coordinates again, exactly as a context that never had one.
 * ebo_rectification_map: copies out the map and / or the table of the rectification that is set (either pointer may
 *   be NULL); EBO_ERR_STATE when none is set.
 *
 * Rectified frames and a fitted rectified camera.  These rules are this project's own (the reference rectifies
 * nothing); tests/rectify_ref.py restates them.  w, h are the context's image size; (w-1), (h-1) are exact doubles.
 * C1. A rectified camera r is an ebo_camera whose k1 k2 p1 p2 are all zero (k3 is ignored, as everywhere).  Any other
 *     value: EBO_ERR_ARG.  r.fx or r.fy not finite or zero: EBO_ERR_RANGE.
 * C2. Forward map into r:  (xOpt, yOpt) = undistort_cam(x, y); u = r.fx * xOpt + r.cx; v = r.fy * yOpt + r.cy; the table
 *     is (round(u), round(v)), half away from zero, with the refusals of ebo_set_rectification, which is this rule
 *     with r = (cam.fx, cam.fy, cam.cx, cam.cy).
 * C3. Fit.  Needs w >= 2, h >= 2, cam.fx > 0, cam.fy > 0 (else EBO_ERR_RANGE).  xmin, xmax, ymin, ymax = the extremes
 *     of undistort_cam over the border pixels (rows 0 and h-1, columns 0 and w-1).
 *       ex = xmax - xmin; dx = fx * ex; sx = (w-1) / dx;    ey = ymax - ymin; dy = fy * ey; sy = (h-1) / dy;
 *       s = min(sx, sy); r.fx = s * fx; r.fy = s * fy;
 *       tx = xmax + xmin; mx = r.fx * tx; nx = (w-1) - mx; r.cx = nx / 2;     r.cy likewise from ymax, ymin, r.fy, h.
 *     EBO_ERR_RANGE when a border pixel's undistorted coordinate is not finite or an extent is not positive.  The
 *     border's image then spans exactly the sensor along the tighter axis and is centred along the other.  The fit
 *     does not promise that no interior pixel leaves the sensor; the tests show it for the calibrations in use.
 * C4. Source map.  For the output pixel (x', y'):  xn = (x' - r.cx) / r.fx; yn = (y' - r.cy) / r.fy;
 *     (us, vs) = project_cam(xn, yn, 1).
 * C5. Remap: bilinear, constant border 0.  If not (us > -1 and us < w and vs > -1 and vs < h) -- tested in double,
 *     before any conversion to an integer, so a NaN falls here too -- the output is 0.  Otherwise
 *       x0 = floor(us); y0 = floor(vs); a = us - x0; b = vs - y0; ia = 1 - a; ib = 1 - b;
 *       p00 p10 p01 p11 = the bytes at (x0, y0) (x0+1, y0) (x0, y0+1) (x0+1, y0+1) as doubles, 0 outside the image;
 *       top = ia * p00 + a * p10; bot = ia * p01 + a * p11; val = ib * top + b * bot   (each product and sum rounded)
 *     and the output is round(val), half away from zero, as uint8.
 * C6. project for many points: the project rule above on xyz [n][3] -> uv [n][2].  Not validated: z = 0 gives what
 *     the rule gives.
 *
 * ebo_fit_rectified_camera: C3 for `cam` on the context's image size; rectified_out gets fx fy cx cy and zeros.
 * ebo_set_rectification_camera: ebo_set_rectification with an explicit rectified camera (C1, C2): it affects the
 *   next load, a refused call leaves no rectification set, EBO_ERR_STATE while recording, the same loaders read
 *   through the table, and ebo_set_patches stays refused while it is set.  The context keeps the (cam, rectified) pair.
 * ebo_rectified_camera: the rectified camera of the rectification that is set; EBO_ERR_STATE when none is.
 * ebo_rectification_source_map: C4 for every output pixel, double [image_h][image_w][2]; EBO_ERR_STATE when none is set.
 * ebo_rectify_image: C5 on a host uint8 [image_h][image_w] frame, synchronous; the _device form takes device
 *   pointers and runs asynchronously on the context's stream (d_image == d_out: EBO_ERR_ARG).  EBO_ERR_STATE when no
 *   rectification is set.  Every tap load is predicated on its own in-image test: no map reads outside the frame.
 * ebo_camera_project: C6 on host arrays, synchronous; the _device form on device arrays, asynchronous.
 * All of them return EBO_ERR_STATE while a graph is being recorded.  ebo_route_set_events, ebo_patch_integrate* and
 * EBO_COUNT_FIELD stay un-rectified: a caller who rectifies frames rectifies the events it routes itself (the C++
 * facade's FeatureDetector::rectifyFrames does, through a host copy of the table). */
typedef struct ebo_camera
{
	double fx, fy, cx, cy, k1, k2, k3, p1, p2;
} ebo_camera;
int ebo_camera_unproject(ebo_ctx* ctx, const ebo_camera* cam, int n, const double* uv, double* bearing_out);
int ebo_camera_unproject_device(ebo_ctx* ctx, const ebo_camera* cam, int n, const double* d_uv, double* d_bearing_out);
int ebo_set_rectification(ebo_ctx* ctx, const ebo_camera* cam);
int ebo_clear_rectification(ebo_ctx* ctx);
int ebo_rectification_map(ebo_ctx* ctx, double* map_xy_f64_out, int16_t* lut_i16_out);
int ebo_fit_rectified_camera(ebo_ctx* ctx, const ebo_camera* cam, ebo_camera* rectified_out);
int ebo_set_rectification_camera(ebo_ctx* ctx, const ebo_camera* cam, const ebo_camera* rectified);
int ebo_rectified_camera(ebo_ctx* ctx, ebo_camera* out);
int ebo_rectification_source_map(ebo_ctx* ctx, double* map_xy_f64_out);
int ebo_rectify_image(ebo_ctx* ctx, const uint8_t* image, uint8_t* out);
int ebo_rectify_image_device(ebo_ctx* ctx, const uint8_t* d_image, uint8_t* d_out);
int ebo_camera_project(ebo_ctx* ctx, const ebo_camera* cam, int n, const double* xyz, double* uv_out);
int ebo_camera_project_device(ebo_ctx* ctx, const ebo_camera* cam, int n, const double* d_xyz, double* d_uv_out);

/* ---- two-view geometry: eight-point RANSAC, triangulation, the epipolar test -------------------
 * What VisualOdometryFrontEnd::initCameras / findInliersRansac (visual_odometry.cpp:176-210, 288-341) and
 * triangulation.cpp:7-63 do through OpenGV, stated here as this project's own rules (OpenGV's source is not part of
 * the reference tree, so parity with it is NOT claimed).  tests/twoview_ref.py restates every rule in numpy.
 * Float64 throughout, one rounding per operation in exactly the association written here, no contraction.
 * A *model* is (R12, t12), double [3][4] row-major = [R | t], taking camera-2 coordinates to camera-1 coordinates;
 * f1[i], f2[i] are the unit bearing vectors of correspondence i in cameras 1 and 2.
 *   dot(a, b) = (a0 * b0 + a1 * b1) + a2 * b2.   cross(a, b) = (a1*b2 - a2*b1, a2*b0 - a0*b2, a0*b1 - a1*b0).
 *
 * 1. triangulate2(R, t, f1, f2) (midpoint; what triangulateLandmarks calls, triangulation.cpp:26):
 *      g_i = dot(R[i][:], f2);  b0 = dot(t, f1);  b1 = dot(t, g);
 *      a00 = dot(f1, f1);  a01 = -dot(f1, g);  a10 = dot(f1, g);  a11 = -dot(g, g);
 *      det = a00 * a11 - a01 * a10;  l0 = (a11 * b0 - a01 * b1) / det;  l1 = (a00 * b1 - a10 * b0) / det;
 *      p_i = (l0 * f1_i + (t_i + l1 * g_i)) / 2                                 (camera-1 coordinates)
 *    Poses: inverse(R, t) = (R^T, -(R^T t)) with (R^T t)_i = dot(R[:][i], t);
 *           (Ra, ta)(Rb, tb) = (Ra Rb, Ra tb + ta) with (Ra Rb)[i][j] = dot(Ra[i][:], Rb[:][j]),
 *           (Ra tb + ta)_i = dot(Ra[i][:], tb) + ta_i;  (R, t) * p = (dot(R[i][:], p) + t_i)_i.
 *    triangulateLandmarks(pose1, pose2, ..) = pose1 * triangulate2(inverse(pose1) * pose2, f1, f2).
 * 2. score(model, i) (the bearing-vector reprojection criterion):
 *      p = triangulate2(R, t, f1, f2);  r1 = p / sqrt(dot(p, p));  d = p - t;
 *      q_j = (R[0][j] * d0 + R[1][j] * d1) + R[2][j] * d2;  r2 = q / sqrt(dot(q, q));
 *      score = (1 - dot(f1, r1)) + (1 - dot(f2, r2)).
 *    Correspondence i is an inlier when score < threshold; a NaN score is not an inlier.  The reference's default
 *    threshold is VisualOdometryParams::ransacThreshold = 5e-5.
 * 3. Sampling.  mix(z): z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9; z = (z ^ (z >> 27)) * 0x94D049BB133111EB;
 *    return z ^ (z >> 31) (splitmix64's finaliser; uint64 arithmetic, wrapping).  G = 0x9E3779B97F4A7C15.
 *      hash(seed, p, h, d) = mix((mix((mix((mix(seed + G) ^ p) + G) ^ h) + G) ^ d) + G)
 *    Hypothesis h of pair p draws 8 distinct indices of 0 .. n-1 by the first 8 steps of a Fisher-Yates shuffle of
 *    the identity permutation: for d = 0 .. 7, j = d + (hash(seed, p, h, d) >> 32) mod (n - d); sample[d] = perm[j];
 *    perm[j] = perm[d].  Integers only: device, host and restatement agree exactly, and a hypothesis does not
 *    depend on which others are evaluated.
 * 4. Eight-point solve.  Row i (i = 0 .. 7, in sample order) of the 8 x 9 matrix A is (f2x * f1, f2y * f1, f2z * f1),
 *    A[i][3a + b] = f2[i]_a * f1[i]_b.  e = the eigenvector of A^T A for its smallest eigenvalue, from a ONE-SIDED
 *    (Hestenes) Jacobi iteration on the columns of A, which never forms A^T A and so does not square A's condition
 *    number.  col(p, q) = sum over the rows i, left to right, of A[i][p] * A[i][q].  V = identity (9 x 9); TEN
 *    times, for p = 0 .. 7, for q = p+1 .. 8:
 *      app = col(p, p); aqq = col(q, q); apq = col(p, q); skipped when apq == 0 exactly;
 *      rotation(app, aqq, apq): theta = (aqq - app) / (2 * apq);  sgn = -1 if theta < 0 else +1;
 *        t = sgn / (|theta| + sqrt(theta * theta + 1));  c = 1 / sqrt(t * t + 1);  s = t * c;
 *      for every row i of A and of V, from the old pair: X[i][p] = c * X[i][p] - s * X[i][q];
 *                                                        X[i][q] = s * X[i][p] + c * X[i][q].
 *    Then d[j] = col(j, j); e = the column of V of the smallest d[j] (the FIRST of equals: j replaces the current
 *    minimum only when d[j] < it).  F[b][a] = e[3a + b], so that f1^T F f2 = 0.
 *    jacobi(M, sweeps), M symmetric 3 x 3, V = identity: `sweeps` times, for (p, q) = (0,1) (0,2) (1,2):
 *      apq = M[p][q]; skipped when apq == 0 exactly; app = M[p][p]; aqq = M[q][q]; (t, c, s) = rotation(app, aqq, apq);
 *      for the k that is neither p nor q, from the old pair: M[k][p] = M[p][k] = c * M[k][p] - s * M[k][q];
 *                                                            M[k][q] = M[q][k] = s * M[k][p] + c * M[k][q];
 *      M[p][p] = app - t * apq;  M[q][q] = aqq + t * apq;  M[p][q] = M[q][p] = 0;
 *      for every k, from the old pair: V[k][p] = c * V[k][p] - s * V[k][q];  V[k][q] = s * V[k][p] + c * V[k][q].
 *    Eigenvalues are the diagonal, eigenvectors the columns of V.
 *    3 x 3 SVD of F: G = F^T F, G[j][k] = dot(F[:][j], F[:][k]); (d, V) = jacobi(G, 8); the three (d_c, column c)
 *    are put in descending order by the compare-exchanges (0,1) (1,2) (0,1), each swapping only when
 *    d_a < d_b (stable; a NaN never swaps); s0 = sqrt(d_0), s1 = sqrt(d_1); NO MODEL unless s0 > 0 and s1 > 0.
 *      u0_i = dot(F[i][:], v0) / s0;  u0 = u0 / sqrt(dot(u0, u0));
 *      u1_i = dot(F[i][:], v1) / s1;  u1 = u1 - dot(u0, u1) * u0;  u1 = u1 / sqrt(dot(u1, u1));
 *      u2 = cross(u0, u1);  v2 = cross(v0, v1).
 *    (The essential matrix itself, U diag(1,1,0) V^T, is never formed: rule 5 needs only U and V.)
 * 5. Disambiguation.  With W = [[0,-1,0],[1,0,0],[0,0,1]]: Ra = U W V^T, Rb = U W^T V^T, entry by entry
 *      Ra[i][j] = (u1_i * v0_j - u0_i * v1_j) + u2_i * v2_j;   Rb[i][j] = (u0_i * v1_j - u1_i * v0_j) + u2_i * v2_j;
 *    each negated when det < 0, det(R) = (R00 * (R11*R22 - R12*R21) - R01 * (R10*R22 - R12*R20)) + R02 * (R10*R21 - R11*R20);
 *    t = +u2 or -u2.  Of the four (R, t) in the fixed order (Ra,+) (Ra,-) (Rb,+) (Rb,-) the model is the FIRST with
 *    the smallest sum, left to right in sample order, of the 8 sample scores; a sum that is not finite counts as
 *    +infinity; if all four are, the hypothesis has no model and zero inliers.  A hypothesis without a model is
 *    written out as an all-zero [3][4].
 * 6. Selection = the serial loop's answer.  count[h] = inliers of hypothesis h.  best = -1, k = max_iterations; for
 *    h = 0, 1, ..: when count[h] > best (strictly: the earliest of equals wins) best = count[h], winner = h,
 *    w = best / n, k = log(1 - probability) / log(clamp(1 - w^8, 1e-15, 1 - 1e-15)) with w^8 by three squarings;
 *    stop after hypothesis h when h + 1 >= k or h + 1 == max_iterations; iterations = h + 1.  Runs on the host, in
 *    double, with the C library's log.  FOUND when best >= 8.
 * 7. computeEssential(T) (triangulation.cpp:31-37) = hat(t / |t|) R:  u = t / sqrt(dot(t, t));
 *      E[0][j] = uy * R[2][j] - uz * R[1][j];  E[1][j] = uz * R[0][j] - ux * R[2][j];  E[2][j] = ux * R[1][j] - uy * R[0][j].
 *    findInliersEssential (triangulation.cpp:39-63): w_i = dot(E[i][:], f2); flag = |dot(f1, w)| < threshold.
 *
 * ebo_relative_pose_ransac (replaces opengv::sac::Ransac::computeModel over CentralRelativePoseSacProblem(EIGHTPT),
 *   visual_odometry.cpp:298-314, for MANY keyframe pairs in one call): pair p owns correspondences
 *   offsets[p] .. offsets[p+1]-1 of f1 / f2 (double [offsets[n_pairs]][3]; offsets[0] = 0).  ALL
 *   n_pairs x max_iterations hypotheses are sampled, solved (rules 3-5) and scored against every correspondence of
 *   their pair (rule 2) on the device in one pass; the counts come back once, rule 6 runs on the host, and one more
 *   launch lists the winners' inliers.  result[p]: found, winner (-1: no hypothesis), iterations, n_inliers,
 *   inlier_offset (= offsets[p]) and the winner's model; inlier_idx[inlier_offset .. + n_inliers) are the winner's
 *   inliers as indices WITHIN the pair, ascending (inlier_idx has room for offsets[n_pairs] ints).  A pair with
 *   fewer than 8 correspondences is not found (winner -1, iterations 0), not an error.  Optional outputs, NULL to
 *   skip at no cost: hyp_counts int [n_pairs][max_iterations], hyp_models double [n_pairs][max_iterations][3][4],
 *   hyp_samples int [n_pairs][max_iterations][8] (all zero for a pair with fewer than 8 correspondences).
 *   A pair's result does not depend on the other pairs of the call.
 *   EBO_ERR_ARG: max_iterations outside [1, 4096], probability outside (0, 1), threshold not positive (or NaN),
 *   a pair with more than 65535 correspondences, more than 65535 pairs, decreasing offsets, a needed pointer NULL.
 *   Synchronous.  EBO_ERR_STATE while a graph is being recorded (all entries of this section).
 * ebo_relative_pose_scores: rule 2 for a GIVEN model and n correspondences: scores double [n] and / or inlier flags
 *   uint8 [n] (either may be NULL).  The re-selection after a refinement (visual_odometry.cpp:325-328,
 *   ransac.sac_model_->selectWithinDistance).
 * ebo_triangulate (triangulateLandmarks, triangulation.cpp:7-29, with a pose pair PER POINT, which is how
 *   addNewLandmarks calls it, visual_odometry.cpp:343-377): poses double [n_poses][3][4] camera-to-world;
 *   point i is seen along f1[i] from poses[pose_pair[i][0]] and along f2[i] from poses[pose_pair[i][1]];
 *   points_out[i] = the world point of rule 1.  A pose index outside [0, n_poses) is EBO_ERR_ARG (the _device form,
 *   which cannot look, writes NaN for that point).
 * ebo_epipolar_inliers (findInliersEssential): rule 7, flags uint8 [n].
 * The _device forms take device pointers for the bearing vectors (and, for scores and triangulate, for every other
 *   array except `model`), so that the output of ebo_camera_unproject_device never visits the host; the scores and
 *   triangulate forms are asynchronous on the context's stream; the RANSAC form still returns its results to host
 *   arrays and is synchronous.
 * ebo_two_view_timing: with `enable` non-zero every later ebo_relative_pose_ransac brackets its phases with events
 *   on the context's stream; ms5_or_null receives the LAST such call's times in milliseconds: [0] hypothesis kernel,
 *   [1] counting kernel, [2] host walk of rule 6 (wall clock), [3] upload of the winners' indices + inlier-list kernel,
 *   [4] the whole call (wall clock).  [4] - ([0] + [1] + [2] + [3]) is everything else: the uploads of the bearing
 *   vectors and offsets, the copy of the counts to the host and the copies of the results.  Zeros before the first
 *   timed call.  For tools/time_two_view.py; off by default, when nothing is recorded. */
typedef struct ebo_two_view_params
{
	double threshold;    /* rule 2; default 5e-5 */
	double probability;  /* rule 6; default 0.99 */
	int max_iterations;  /* hypotheses per pair, 1 .. 4096; default 1000 */
	int reserved;        /* 0 */
	uint64_t seed;       /* rule 3; default 0 */
} ebo_two_view_params;
typedef struct ebo_two_view_result
{
	int found;
	int winner;
	int iterations;
	int n_inliers;
	int inlier_offset;
	int reserved;
	double model[3][4];
} ebo_two_view_result;
void ebo_default_two_view_params(ebo_two_view_params* params);
int ebo_two_view_timing(ebo_ctx* ctx, int enable, float* ms5_or_null);
int ebo_relative_pose_ransac(ebo_ctx* ctx, int n_pairs, const int* offsets, const double* f1, const double* f2,
							 const ebo_two_view_params* params, ebo_two_view_result* result, int* inlier_idx,
							 int* hyp_counts_or_null, double* hyp_models_or_null, int* hyp_samples_or_null);
int ebo_relative_pose_ransac_device(ebo_ctx* ctx, int n_pairs, const int* offsets, const double* d_f1, const double* d_f2,
									const ebo_two_view_params* params, ebo_two_view_result* result, int* inlier_idx,
									int* hyp_counts_or_null, double* hyp_models_or_null, int* hyp_samples_or_null);
int ebo_relative_pose_scores(ebo_ctx* ctx, const double* model, int n, const double* f1, const double* f2, double threshold,
							 double* scores_or_null, uint8_t* inlier_flags_or_null);
int ebo_relative_pose_scores_device(ebo_ctx* ctx, const double* model, int n, const double* d_f1, const double* d_f2,
									double threshold, double* d_scores_or_null, uint8_t* d_inlier_flags_or_null);
int ebo_triangulate(ebo_ctx* ctx, int n_poses, const double* poses, int n, const int* pose_pair, const double* f1,
					const double* f2, double* points_out);
int ebo_triangulate_device(ebo_ctx* ctx, int n_poses, const double* d_poses, int n, const int* d_pose_pair, const double* d_f1,
						   const double* d_f2, double* d_points_out);
int ebo_epipolar_inliers(ebo_ctx* ctx, const double* model, int n, const double* f1, const double* f2, double threshold,
						 uint8_t* flags);

/* ---- relative-pose refinement: five-variable Levenberg-Marquardt over a pair's RANSAC inliers ----------------
 * What findInliersRansac does after its RANSAC through OpenGV's relative_pose::optimize_nonlinear
 * (visual_odometry.cpp:316-330), stated as this project's own rules for MANY keyframe pairs in one call.  Parity with
 * OpenGV is NOT claimed (INTEGRATION.md 7 lists the differences).  tests/relpose_ref.py restates every rule in numpy.
 * Float64, one rounding per operation in the association written here, no contraction, only + - * / sqrt and
 * comparisons, a comparison with a NaN is false, every sum in a stated order.  model, f1, f2, dot and cross are the
 * two-view section's; B4, B6-B9 are the bundle adjustment's, further down.
 *
 * R1. Entry.  A pair with fewer than 5 listed inliers is not refined: iterations 0, termination 1, costs 0, the model
 *     untouched.  When an entry of the model or of ANY bearing vector of the pair (listed or not) is not finite, when
 *     a listed index is outside the pair, or when n = sqrt(dot(t, t)) is not > 0 or not finite: termination 2,
 *     iterations 0, costs 0, the model returned bit for bit.  Otherwise t = t / n, entry by entry, is the start, and
 *     unless its cost is not finite (B9: termination 2, the model returned bit for bit) the start is the first point
 *     visited, so what comes back has a unit t even when no step is taken.
 * R2. Tangent basis at a point (R, t):  k = the index of the smallest |t_k|, the first of equals;
 *       w = (0, t2, -t1) for k = 0, (-t2, 0, t0) for k = 1, (t1, -t0, 0) for k = 2    (= cross(t, axis k));
 *       e1 = w / sqrt(dot(w, w));  e2 = cross(t, e1).
 * R3. Residual.  For listed inlier i, in list order, p, r1, q, r2 are those of rules 1-2 of the two-view section, in
 *     their operations.  Its six residuals are the chords c = (f1 - r1, f2 - r2), rows 0 .. 5; their squared norm is
 *     2 * score up to rounding.  No loss function: the list holds inliers only.
 * R4. Variables and Jacobian.  Five variables (a, b, om_x, om_y, om_z), columns 0 .. 4.  J[k][s] = the derivative
 *     of row k along variable s, by forward mode through every operation of R3, one derivative slot per variable;
 *     .v is a quantity's value and .d its slot:
 *       x * y: x.v * y.d + y.v * x.d;   c * x and x / c with c a constant (an entry of f1 or f2, a00, the 2 of
 *       rule 1): c * x.d and x.d / c;   x / y: (x.d - (x.v / y.v) * y.d) / y.v;   sqrt(x): x.d / (2 * sqrt(x.v));
 *       sums, differences and negations termwise (dot's in its association); f - r: -(r.d).
 *     No term is left out because its slot is zero.  Seeds at the point (R, t) with R2's basis:
 *       a: t.d = e1;  b: t.d = e2;  (R.d = 0)        om_x: R.d[i][:] = (0, R[i][2], -R[i][1]);
 *       om_y: R.d[i][:] = (-R[i][2], 0, R[i][0]);  om_z: R.d[i][:] = (R[i][1], -R[i][0], 0);  (t.d = 0)
 *     i.e. R hat(e_k).  Every entry is then multiplied by the scale of its column (R7): J[k][s] = c_k.d * scale_s.
 * R5. Update by a step whose entries were first multiplied by their columns' scales, with R2's basis at (R, t):
 *       t'_i = (t_i + (a * e1_i + b * e2_i)) / sqrt(1 + (a * a + b * b));
 *       R'[i][j] = dot(R[i][:], C[:][j]) with C the matrix of B4 for om.
 *     (e1, e2, t are orthonormal, so the divisor is the sum's length; written this way, like B4's quaternion, the
 *     update is exactly the identity at a zero step.)  No sin / cos, no re-orthonormalisation.
 * R6. Sums.  tree64(v): 64 partial sums, partial l = ((0 + v[l]) + v[l + 64]) + .. ; then for s = 32, 16, .., 1:
 *     partial[i] = partial[i] + partial[i + s] for i < s; the result is partial[0].  With listed inlier i dealt to
 *     partial i mod 64 and its rows taken in the order 0 .. 5, one product added at a time:
 *       H[a][b] = tree64 of J[k][a] * J[k][b]  (b <= a; 15 sums),  g[a] = tree64 of J[k][a] * c_k,
 *       cost = 0.5 * tree64 of c_k * c_k.
 * R7. Scaling, damping, the step.  scale_s = 1 / (1 + sqrt(H[s][s])) from the sums at the start with all scales 1
 *     (B6; opts->jacobi_scaling), fixed for the solve.  S = H with damp(H[a][a]) of B7 added to every diagonal entry;
 *     S = L L^T, L y = g, L^T x = y in B8's words (5 rows); step = -x; a pivot that is not > 0 or not finite, or a
 *     step entry that is not finite, makes the step invalid.
 * R8. Trust region: B9 as it stands, with tree64 in place of tree, and
 *       model cost change = -tree64 of mr_k * (c_k + mr_k / 2), rows as in R6,
 *         mr_k = (((J[k][0] * step_0 + J[k][1] * step_1) + J[k][2] * step_2) + J[k][3] * step_3) + J[k][4] * step_4;
 *       |x| = sqrt(tree64 of the squares of the model's 12 entries in array order), the step norm the same of
 *         (x - candidate);   gradient norm = max over the 5 columns of |g_s / scale_s|.
 *     R2's basis is taken anew at every point the solve moves to.  The result is the lowest-cost point visited.
 *
 * ebo_relative_pose_refine: offsets, f1, f2 as for ebo_relative_pose_ransac; models double [n_pairs][3][4], updated
 *   in place; pair p's list is inlier_idx[offsets[p] .. offsets[p] + n_inliers[p]), indices WITHIN the pair in any
 *   order: ebo_relative_pose_ransac's layout (model, n_inliers and inlier_offset of its results), so the call chains
 *   straight off it.  One ebo_summary per pair (num_evals_jac counts Jacobian evaluations, num_evals_cost candidate
 *   evaluations); trace_or_null in ebo_bundle_adjust's format, double [n_pairs][opts->max_num_iterations + 1][4].
 *   opts as ebo_default_ba_opts fills them; opts->mode is not read.  The returned t has unit length.  A pair's result
 *   depends neither on the other pairs of the call nor on the run.  Limits: 65535 correspondences per pair, 65535
 *   pairs.  EBO_ERR_ARG beyond them and for an index outside its pair, offsets that decrease or do not start at 0,
 *   an n_inliers that is negative or beyond its pair's size, a negative max_num_iterations, a needed pointer NULL.
 *   EBO_ERR_STATE while a graph is being recorded.  Synchronous.
 * ebo_relative_pose_refine_device: device pointers for f1, f2, inlier_idx, models and the trace; offsets, n_inliers
 *   and the summaries stay host arrays.  It cannot look at the indices: a pair with one out of range is not solved
 *   (R1: termination 2, its model untouched); the kernel checks before it starts.
 * ebo_two_view_timing brackets both: slot [0] the kernel, [4] the whole call, the others 0. */
int ebo_relative_pose_refine(ebo_ctx* ctx, int n_pairs, const int* offsets, const double* f1, const double* f2, double* models,
							 const int* n_inliers, const int* inlier_idx, const ebo_solver_opts* opts, ebo_summary* summaries,
							 double* trace_or_null);
int ebo_relative_pose_refine_device(ebo_ctx* ctx, int n_pairs, const int* offsets, const double* d_f1, const double* d_f2,
									double* d_models, const int* n_inliers, const int* d_inlier_idx, const ebo_solver_opts* opts,
									ebo_summary* summaries, double* d_trace_or_null);

/* ---- trajectory alignment: Sim3 / SE3 alignment of estimated camera centres to ground truth, and the ATE ------
 * What newKeyframeCandidate does through align_cameras_sim3 / align_points_sim3 (aligner.cpp:27-114, called at
 * visual_odometry.cpp:83-97) for all keyframes so far after every new keyframe, stated as this project's own rules for
 * MANY trajectory segments in one call.  Parity with Eigen's JacobiSVD is NOT claimed (INTEGRATION.md 7 lists the
 * differences).  tests/align_ref.py restates every rule in numpy.  Float64, one rounding per operation in the
 * association written here, no contraction, only + - * / sqrt and comparisons, a comparison with a NaN is false,
 * every sum in a stated order.  dot, cross and jacobi(M, sweeps) are the two-view section's, tree64 is R6's.
 * `data` holds the ground-truth centres d_i and `model` the estimated centres m_i; the fit is
 * data ~ s * R * model + t, the reference's direction.  A segment has n points, i counted from its start.
 *
 * S1. Entry.  n < 3: status 1.  A coordinate of the segment that is not finite, in either array: status 2.  In both
 *     cases, and for status 3 below: scale 1, R the identity, t = 0, rmse = mean = min = max = 0, count = n.
 * S2. Centroids.  With point i dealt to partial i mod 64:  cd_a = tree64 of d_a / double(n);  cm_a the same of m_a.
 * S3. Centred sums.  dc = d - cd, mc = m - cm, entry by entry.  W[a][b] = tree64 of dc_a * mc_b (9 sums);
 *     nm = tree64 of (mc0 * mc0 + mc1 * mc1) + mc2 * mc2.  Centred first, as the reference does: no raw moments, so
 *     a trajectory far from the origin loses no digits.
 * S4. Singular vectors.  G[j][k] = dot(W[:][j], W[:][k]);  (d, V) = jacobi(G, 8), ordered descending with their
 *     columns by the compare-exchanges (0,1) (1,2) (0,1) of rule 4 (a swap only when strictly smaller).  Status 3
 *     unless d1 > 0, d1 finite, d1 > d0 * 2^-46 (128 ulps of d0, what the iteration's rounding leaves of an exact
 *     zero: a second singular value below 2^-23 of the first, a cloud thinner than about 1 : 2900, is a line to the
 *     digits G carries and the rotation about it is not determined), nm > 0 and nm finite.
 * S5. Rotation from the top two pairs only.  u0_i = dot(W[i][:], v0); n0 = sqrt(dot(u0, u0)); u0 = u0 / n0;
 *     u1_i = dot(W[i][:], v1); h = dot(u0, u1); u1 = u1 - h * u0; n1 = sqrt(dot(u1, u1)); u1 = u1 / n1.  Status 3
 *     unless n0 and n1 are > 0 and finite.  u2 = cross(u0, u1); v2 = cross(v0, v1);
 *       R[i][j] = (u0_i * v0_j + u1_i * v1_j) + u2_i * v2_j.
 *     The determinant is +1 by construction: this is the reference's diag(1, 1, +-1) reflection guard, and the
 *     smallest singular pair is never read, so a planar trajectory is well conditioned.
 * S6. Scale and translation.  s = (the nine products R[a][b] * W[a][b] added one at a time from 0 in row-major
 *     order) / nm, which is the sum of dot(dc, R mc) over the points by S3's sums; s = 1 with fix_scale.
 *     t_i = cd_i - s * dot(R[i][:], cm).
 * S7. Errors.  r_k = d_k - (s * dot(R[k][:], m) + t_k);  q = dot(r, r);  e = sqrt(q), per point.
 *     rmse = sqrt(tree64 of q / double(n));  mean = tree64 of e / double(n);  min and max over the same tree: a
 *     partial starts at DBL_MAX (min) or 0 (max) and takes e when e is strictly smaller / larger, partial[i] takes
 *     partial[i + s] likewise.  count = n.
 *
 * ebo_align_sim3: data and model are double [n_points][3]; segment g covers points seg_begin[g] .. seg_end[g] - 1 of
 *   BOTH arrays.  Segments may overlap and may be prefixes of one another; an empty segment is status 1.  fix_scale
 *   non-zero is the SE3 alignment of metric trajectories.  One ebo_align_result per segment; status 0 aligned, 1 fewer
 *   than 3 points, 2 a non-finite input, 3 degenerate.  A segment's result depends neither on the other segments of
 *   the call nor on the run.  Limits: 2^24 points per segment, 65535 segments.  EBO_ERR_ARG beyond them and for a
 *   needed pointer that is NULL, a negative count, seg_end < seg_begin, a segment outside [0, n_points].
 *   EBO_ERR_STATE while a graph is being recorded.  Synchronous.
 * ebo_align_sim3_device: device pointers for data and model; seg_begin, seg_end and the results stay host arrays.
 * ebo_two_view_timing brackets both: slot [0] the kernel, [4] the whole call, the others 0. */
typedef struct ebo_align_result
{
	double scale;
	double R[9]; /* row-major */
	double t[3];
	double rmse, mean, min, max; /* the reference's ErrorMetricValue */
	int32_t count;
	int32_t status;
} ebo_align_result;
int ebo_align_sim3(ebo_ctx* ctx, int n_points, const double* data, const double* model, int n_segments, const int* seg_begin,
				   const int* seg_end, int fix_scale, ebo_align_result* results);
int ebo_align_sim3_device(ebo_ctx* ctx, int n_points, const double* d_data, const double* d_model, int n_segments,
						  const int* seg_begin, const int* seg_end, int fix_scale, ebo_align_result* results);

/* ---- trajectory evaluation: relative pose error (RPE), the drift per step beside the ATE ------------------------
 * The reference judges a trajectory by the absolute trajectory error alone; this is the other half of the usual
 * pair (Sturm et al., "A Benchmark for the Evaluation of RGB-D SLAM Systems", IROS 2012): the error of the motion
 * over a fixed number of poses, for MANY (segment, delta) units over one pair of pose arrays in one call.  It needs
 * no alignment, so it has an answer where the alignment is degenerate.  tests/rpe_ref.py restates every rule in
 * numpy.  As S1-S7: float64 throughout, one rounding per operation in exactly the association written here, no
 * contraction, only + - * / sqrt and comparisons, a comparison with a NaN is false; dot is the two-view section's,
 * tree64 is R6's with pair k (counted from the unit's first) dealt to partial k mod 64.
 * A *pose* is double [3][4] row-major = [R | t], taking camera (or body) coordinates to world coordinates, as in the
 * absolute-pose section.  `gt` holds the ground-truth poses Q_i = [G_i | g_i], `est` the estimated poses
 * P_i = [R_i | p_i].  A unit is (segment [b, e), delta D >= 1, scale s); its pairs are (i, j = i + D) for
 * i = b .. e - D - 1.  X[:][k] is column k of X.
 *
 * T1. Entry.  No pair (e - b <= D): status 1, all eight statistics 0, count = 0.  Any of the 12 doubles of any pose
 *     of the segment, in either array, not finite, or s not finite: status 2, the statistics 0, count = the number
 *     of pairs.  Rotation blocks are taken as given: nothing re-orthonormalises them.
 * T2. Relative translation error, the TUM definition |trans((Q_i^-1 Q_j)^-1 (P_i^-1 P_j))| without the rotation
 *     that preserves the norm.  dp = p_j - p_i, dg = g_j - g_i, entry by entry;
 *       a_k = s * dot(R_i[:][k], dp);  b_k = dot(G_i[:][k], dg);  r = a - b;  q = dot(r, r);  e = sqrt(q).
 * T3. Relative rotation.  A[r][c] = dot(R_i[:][r], R_j[:][c]) (A = R_i^T R_j);  B the same of G_i, G_j;
 *       E[r][c] = dot(B[:][r], A[:][c]) (E = B^T A).
 * T4. Sine and cosine of its angle.  v = (0.5 * (E21 - E12), 0.5 * (E02 - E20), 0.5 * (E10 - E01));
 *       sn = sqrt(dot(v, v));  cs = (((E00 + E11) + E22) - 1) / 2.
 * T5. The angle from (sn, cs) without a library function.  h = sqrt(sn * sn + cs * cs); theta = 0 unless h > 0.
 *     Otherwise u = sn / (h + |cs|);  twice: u = u / (1 + sqrt(1 + u * u));  z = u * u;
 *       p = c12;  p = p * z + c_k for k = 11 .. 0,  c_k = (k odd ? -1 : 1) / double(2 k + 1);
 *       phi = 8 * (u * p);  theta = phi when cs >= 0, else double(pi) - phi.
 *     (u is the tangent of an eighth of the angle folded onto [0, pi / 2], at most tan(pi / 16); p is the
 *     arctangent's series to u^25.)  Exactly 0 at the identity, exactly double(pi) at a half turn; within 1e-15 of
 *     atan2(sn, cs) in between.
 * T6. Statistics, of e and of theta separately.  rmse = sqrt(tree64 of q / double(n_pairs)), the rotation's with
 *     theta * theta for q;  mean = tree64 of e / double(n_pairs);  min and max over the same tree exactly as S7's
 *     (strict comparisons, DBL_MAX and 0 as starts).  count = n_pairs, status 0.
 * T7. Independence.  A unit's result depends neither on the other units of the call nor on the run.
 *
 * ebo_trajectory_rpe: gt and est are double [n_poses][3][4]; segment g covers poses seg_begin[g] .. seg_end[g] - 1
 *   of BOTH arrays and is evaluated at every one of the n_deltas steps with the scale seg_scale[g] (NULL: 1 for
 *   all); results is [n_segments][n_deltas].  Segments may overlap and may be prefixes of one another.  Limits:
 *   2^24 poses per segment, 65535 segments, 16 deltas.  EBO_ERR_ARG beyond them and for a needed pointer that is
 *   NULL, a negative count, seg_end < seg_begin, a segment outside [0, n_poses], a delta < 1.  EBO_ERR_STATE while
 *   a graph is being recorded.  Synchronous.
 * ebo_trajectory_rpe_device: device pointers for gt and est; segments, scales, deltas and results stay host arrays.
 * ebo_two_view_timing brackets both: slot [0] the kernel, [4] the whole call, the others 0.
 * Not built: an absolute rotation error (it needs the hand-eye rotation between the ground truth's body and the
 * camera, which neither the reference nor the recording format carries); ground-truth interpolation on the device
 * (it stays syncGroundTruth's, visual_odometry/aligner.h); pairs chosen by time or by path length. */
typedef struct ebo_rpe_result
{
	double trans_rmse, trans_mean, trans_min, trans_max; /* of e (T2), in the ground truth's unit */
	double rot_rmse, rot_mean, rot_min, rot_max;         /* of theta (T5), radians */
	int32_t count;
	int32_t status;
} ebo_rpe_result;
int ebo_trajectory_rpe(ebo_ctx* ctx, int n_poses, const double* gt, const double* est, int n_segments, const int* seg_begin,
					   const int* seg_end, const double* seg_scale_or_null, int n_deltas, const int* deltas, ebo_rpe_result* results);
int ebo_trajectory_rpe_device(ebo_ctx* ctx, int n_poses, const double* d_gt, const double* d_est, int n_segments,
							  const int* seg_begin, const int* seg_end, const double* seg_scale_or_null, int n_deltas,
							  const int* deltas, ebo_rpe_result* results);

/* ---- track evaluation: KLT reference tracks on the frames, track error and feature age ------------------------
 * The two figures the reference's report judges the feature tracker by, mean track error in pixels and feature age in
 * seconds, by the protocol published for event-based trackers on real recordings (Gehrig et al., "EKLT: Asynchronous
 * Photometric Feature Tracking using Events and Frames"): a KLT track on the recording's frames, seeded at the event
 * track's position on the first frame inside its life, is the ground truth; the event track is compared against it,
 * interpolated in time, and its age ends when the error first exceeds a threshold tau.  The reference has no such
 * code.  tests/trackerr_ref.py restates every rule in numpy.  As S and T: float64 throughout, one rounding per
 * operation in exactly the association written here, no contraction, only + - * / sqrt and comparisons, a comparison
 * with a NaN is false; tree64 is R6's.
 * A *track* is its samples (t_i, x_i, y_i), i = 0 .. n - 1, t in integer microseconds (below 2^53).  The estimated
 * track's times do not decrease; the ground-truth track's, gt_t, increase strictly; first and last are its first and
 * last sample.  A unit is (track, tau).
 *
 * V1. Entry.  In this order: no estimated sample, or fewer than 2 ground-truth samples: status 1.  Any coordinate of
 *     any estimated or ground-truth sample of the track not finite, inside the span of V2 or not: status 2.  No
 *     estimated sample with gt_t[first] <= t <= gt_t[last]: status 1.  In all three every field of the result is 0
 *     (first and cut mean something under status 0 only).
 * V2. Comparable samples: the estimated samples with gt_t[first] <= t_i <= gt_t[last], a contiguous run [i0, i1)
 *     because times do not decrease.  Earlier samples are skipped, later ones are not judged.
 * V3. Interpolation of a track (t, p) at time T, t[0] <= T <= t[last]:  j = the largest index with t[j] <= T.  When
 *     t[j] == T:  g = p[j] exactly.  Otherwise  w = double(T - t[j]) / double(t[j+1] - t[j])  (the int64 differences
 *     are exact);  g = p[j] + w * (p[j+1] - p[j])  per component: subtract, multiply, add.
 * V4. Error of a comparable sample (t, x, y):  (gx, gy) = the ground-truth track at t by V3;  dx = x - gx;
 *     dy = y - gy;  q = dx * dx + dy * dy;  e = sqrt(q).
 * V5. Cut.  c = the first comparable sample in index order with e > tau (strictly); the inliers are the comparable
 *     samples before c, all of them when there is no c.  cut = c's index within the track, or -1.
 * V6. Age.  age_us = t(last inlier) - t(first inlier) as int64; the first inlier is sample i0.  With no inlier (sample
 *     i0 is beyond tau already): status 0, n_inliers = 0, cut = i0, age and statistics 0.  t_first_us = t(i0);
 *     first = i0;  n_comparable = i1 - i0.
 * V7. Statistics over the inliers, inlier k (counted from i0) dealt to partial k mod 64:
 *     err_mean = tree64 of e / double(n_inliers);  err_rmse = sqrt(tree64 of q / double(n_inliers));  err_max over
 *     the same tree exactly as S7's max (strict comparisons, 0 as start).
 * V8. Per-sample output, where asked: sample_err_out[i] = e (V4) for comparable samples and -1.0 for all others; all
 *     -1.0 for a track whose status is not 0.  It does not depend on tau.
 * V9. Independence.  A unit's result depends neither on the other units of the call nor on the run.
 *
 * ebo_track_seeds (host only, no context): where a KLT track starts for each estimated track.  Track k owns samples
 *   est_off[k] .. est_off[k+1] - 1 of est_t_us (int64) and est_xy (double [.][2]); frame_t_us [n_frames] increases
 *   strictly.  f = the first frame with frame_t_us[f] >= t_0.  seed_frame[k] = -1 and seed_xy[k] = (0, 0) when there is
 *   none, when frame_t_us[f] > t_(n-1), or when the track is empty.  Otherwise seed_frame[k] = f and seed_xy[k] = the
 *   track ITSELF at frame_t_us[f] by V3 (of samples with equal times the last one counts), rounded to float, LK's
 *   type.  EBO_ERR_ARG for a needed pointer that is NULL, a negative count, offsets that decrease or do not start at
 *   0, estimated times that decrease within a track, frame times that do not increase strictly.
 * ebo_reference_tracks: the KLT tracks of n seeds through `frames`, uint8 [n_frames][image_h][image_w] on the host at
 *   the context's size, taken at frame_t_us (not read beyond the NULL check: the frames' order is the arrays').  BY
 *   DEFINITION the hand-written loop: ebo_lk_add_image(frame 0); for f = 0 .. n_frames - 2: ebo_lk_add_image(frame
 *   f + 1), then, if any track is alive at f, ONE ebo_lk_track of all of them, in seed order, from their positions at
 *   f, with the parameters of ebo_lk_track in lk_or_null (NULL: ebo_default_lk_params' values, the reference's
 *   FlowEstimator ones: 21 x 21, 3, 30, 0.01, 1e-4).  A track becomes alive at its seed frame, at seed_xy.  After a launch it stays alive
 *   iff status == 1 and 0 <= x < image_w and 0 <= y < image_h at the new position; otherwise last[k] = f.  first[k] =
 *   seed_frame[k]; last[k] = the last frame at which the track has a position; xy is double [n][n_frames][2], the
 *   float results widened, 0 outside [first, last].  seed_frame < 0: first = last = -1.  No LK kernel of its own.  It
 *   leaves the context's "last two images" as that loop does: the last two frames (one frame: that frame as the newer
 *   image).  EBO_ERR_ARG for a needed pointer that is NULL, negative counts, a seed_frame >= n_frames, and whatever
 *   ebo_lk_track refuses.  EBO_ERR_STATE while a graph is being recorded.  Synchronous.
 * ebo_track_errors: track k owns estimated samples est_off[k] .. est_off[k+1] - 1 and ground-truth samples
 *   gt_off[k] .. gt_off[k+1] - 1; every track is evaluated at each of the n_taus thresholds (pixels); results is
 *   [n_tracks][n_taus]; sample_err_out_or_null is double [est_off[n_tracks]] (V8).  One launch, one wave per unit.
 *   Limits: 65535 tracks, 8 thresholds, 2^24 samples per track on either side.  EBO_ERR_ARG beyond them and, checked
 *   on the host before the launch, for a needed pointer that is NULL, negative counts, offsets that decrease or do not
 *   start at 0, ground-truth times not strictly increasing within a track, estimated times decreasing within a track,
 *   a tau that is NaN or negative (+infinity is allowed: it never cuts).  EBO_ERR_STATE while a graph is being
 *   recorded.  Synchronous.
 * ebo_track_errors_device: device pointers for the four sample arrays and sample_err_out; offsets, taus and results
 *   stay host arrays.  It cannot look at the times: tracks whose times are out of order get unspecified numbers, never
 *   an access outside the arrays.
 * ebo_two_view_timing brackets both: slot [0] the kernel, [4] the whole call, the others 0.
 * ebo_track_error_summary (host only): over results[k * stride] for k = 0 .. n_tracks - 1 (one tau of a results
 *   array: results + j with stride n_taus), in track order with sequential double sums.  Counted tracks have status 0
 *   and n_inliers >= 1; m = their number; discarded = n_tracks - m;  mean_error = (sum of err_mean) / double(m), the
 *   report's Table 1;  mean_age_s = ((sum of double(age_us)) / double(m)) * 1e-6, Table 2;  outlived = the counted
 *   tracks with cut == -1, whose age is censored by the end of the track or of the ground truth.  m = 0: every field 0, discarded too.
 * Not built: ground truth from a simulated recording's projected landmarks (neither the reference nor the dataset
 *   carries depth); re-seeding a reference track after it is lost. */
typedef struct ebo_track_error_result
{
	double err_mean, err_rmse, err_max; /* of e (V4) over the inliers, pixels */
	int64_t age_us, t_first_us;
	int32_t n_inliers, n_comparable, first, cut, status, pad;
} ebo_track_error_result;
typedef struct ebo_track_error_summary_result
{
	double mean_error; /* pixels */
	double mean_age_s;
	int32_t counted, discarded, outlived, pad;
} ebo_track_error_summary_result;
typedef struct ebo_lk_params
{
	int32_t win_w, win_h, max_level, max_count;
	double epsilon, min_eig_threshold;
} ebo_lk_params;
void ebo_default_lk_params(ebo_lk_params* p);
int ebo_track_seeds(int n_tracks, const int* est_off, const int64_t* est_t_us, const double* est_xy, int n_frames,
					const int64_t* frame_t_us, int* seed_frame, float* seed_xy);
int ebo_reference_tracks(ebo_ctx* ctx, int n_frames, const uint8_t* frames, const int64_t* frame_t_us, int n,
						 const int* seed_frame, const float* seed_xy, const ebo_lk_params* lk_or_null, int* first, int* last,
						 double* xy);
int ebo_track_errors(ebo_ctx* ctx, int n_tracks, const int* est_off, const int64_t* est_t_us, const double* est_xy,
					 const int* gt_off, const int64_t* gt_t_us, const double* gt_xy, int n_taus, const double* taus,
					 ebo_track_error_result* results, double* sample_err_out_or_null);
int ebo_track_errors_device(ebo_ctx* ctx, int n_tracks, const int* est_off, const int64_t* d_est_t_us, const double* d_est_xy,
							const int* gt_off, const int64_t* d_gt_t_us, const double* d_gt_xy, int n_taus, const double* taus,
							ebo_track_error_result* results, double* d_sample_err_out_or_null);
int ebo_track_error_summary(int n_tracks, const ebo_track_error_result* results, int stride,
							ebo_track_error_summary_result* out);

/* ---- absolute pose: three-point RANSAC on (bearing vector, landmark) pairs ----------------------------
 * What VisualOdometryFrontEnd::localizeCamera (visual_odometry.cpp:212-286) does through OpenGV's
 * AbsolutePoseSacProblem(KNEIP), stated as this project's own rules (OpenGV's source is not part of the reference
 * tree, so parity with it is NOT claimed).  tests/abspose_ref.py restates every rule in numpy.  As in the two-view
 * section: float64 throughout, one rounding per operation in exactly the association written here, no contraction,
 * only + - * / sqrt and comparisons, fixed iteration counts; dot, cross, mix / hash, rotation and jacobi(M, sweeps)
 * are the ones stated there.  A comparison with a NaN is false.
 * A *pose* is (R, t), double [3][4] row-major = [R | t], taking camera coordinates to world coordinates
 * (match.Tw2c as localizeCamera sets it); f[i] is the unit bearing vector of point i in the camera, p[i] its
 * landmark in world coordinates.
 *
 * A1. score(pose, i):  d = p - t;  q_j = (R[0][j] * d0 + R[1][j] * d1) + R[2][j] * d2;  r = q / sqrt(dot(q, q));
 *       score = 1 - dot(f, r).
 *     Point i is an inlier when score < threshold; a NaN score is not an inlier.
 * A2. Sampling.  Rule 3 with FOUR draws (d = 0 .. 3; `pair` = the frame's index in the call).  Points 1-3 of the
 *     sample are solved, point 4 chooses among the candidates.
 * A3. Minimal solve.  Indices 1, 2, 3 are the sample's first three points.
 *       b12 = dot(f1, f2); b13 = dot(f1, f3); b23 = dot(f2, f3);  d12 = p1 - p2; d13 = p1 - p3; d23 = p2 - p3;
 *       a12 = dot(d12, d12); a13 = dot(d13, d13); a23 = dot(d23, d23);  ww = cross(d12, d13).
 *     NO MODEL unless dot(ww, ww) > 0 (collinear or coincident landmarks) and dot(f_i, f_i) > 0 for all FOUR bearing
 *     vectors of the sample (a zero or NaN bearing).  The depths l_i (X_i = l_i f_i in the
 *     camera) satisfy l_i^2 + l_j^2 - 2 b_ij l_i l_j = a_ij; eliminating the right-hand sides gives two homogeneous
 *     conics in (l1, l2, l3), as symmetric matrices
 *       D1 = [[a23, -(b12*a23), 0], [., a23 - a12, b23*a12], [., ., -a12]]
 *       D2 = [[a23, 0, -(b13*a23)], [., -a13, b23*a13], [., ., a23 - a13]].
 *     cof(M): C[i][j] = M[i+1][j+1] * M[i+2][j+2] - M[i+1][j+2] * M[i+2][j+1] (indices mod 3);
 *             det(M) = dot(M[0][:], C[0][:]);   rows(A, B) = (dot(A[0], B[0]) + dot(A[1], B[1])) + dot(A[2], B[2]).
 *     det(D1 + g D2) = c0 + c1 g + c2 g^2 + c3 g^3 with c0 = det(D1), c3 = det(D2), c1 = rows(cof(D1), D2),
 *     c2 = rows(cof(D2), D1).  NO MODEL when c3 == 0.  b = c2 / c3, c = c1 / c3, d = c0 / c3;
 *       P(x) = ((x + b) * x + c) * x + d;   P'(x) = ((3 * x) + (2 * b)) * x + c.
 *     Start: q = b * b - 3 * c; v = sqrt(q); t1 = (-b - v) / 3; k1 = P(t1); t2 = (-b + v) / 3; k2 = P(t2);
 *       when q > 0 and k1 > 0: x = t1 - sqrt(k1 / v)     (left of the local maximum, where P is concave and negative)
 *       when q > 0 otherwise:  x = t2 + sqrt(|k2| / v)   (right of the local minimum, where P is convex and positive)
 *       otherwise:             x = -b / 3                (the inflection point)
 *     so that Newton's iteration is monotone from there.  THIRTY-TWO times: x = x - P(x) / P'(x), the iterate left
 *     as it is when P'(x) == 0.  g = x.
 *     D0 = D1 + g * D2 entry by entry; (e, V) = jacobi(D0, 8).  D0 has rank 2: the eigenvalue of smallest magnitude
 *     is dropped (m = 0; m = 1 when |e1| < |e0|; m = 2 when |e2| < the smaller of those: the first of equals), the
 *     other two, in index order, are (ea, va), (eb, vb).  NO MODEL unless (ea > 0 and eb < 0) or (ea < 0 and eb > 0).
 *     s = sqrt((-eb) / ea).  D0 then splits into the two planes n = va - sg * vb, sg = +s and then -s.  For each:
 *       dropped when n0 == 0;  w0 = (-n1) / n0;  w1 = (-n2) / n0                      (l1 = w0 l2 + w1 l3);
 *       with tau = l3 / l2 the conic D1 becomes qa tau^2 + qb tau + qc = 0,
 *         qa = a23 * (w1 * w1) - a12;
 *         qb = a23 * ((2 * w0) * w1 - (2 * b12) * w1) + (2 * a12) * b23;
 *         qc = a23 * ((w0 * w0 + 1) - (2 * b12) * w0) - a12;
 *       dropped when qa == 0;  disc = qb * qb - (4 * qa) * qc;  dropped unless disc >= 0;
 *       tau = ((-qb) + sqrt(disc)) / (2 * qa) and then ((-qb) - sqrt(disc)) / (2 * qa).  For each:
 *         dropped unless tau > 0;  den = (1 + tau * tau) - (2 * b23) * tau;  dropped unless den > 0;
 *         l2 = sqrt(a23 / den);  l3 = tau * l2;  l1 = w0 * l2 + w1 * l3;  dropped unless l1 > 0.
 *         Polish, THREE Gauss-Newton steps on the distance equations:
 *           r0 = ((l1*l1 + l2*l2) - ((2*b12) * l1) * l2) - a12;  r1 = ((l1*l1 + l3*l3) - ((2*b13) * l1) * l3) - a13;
 *           r2 = ((l2*l2 + l3*l3) - ((2*b23) * l2) * l3) - a23;
 *           J = [[2*l1 - (2*b12)*l2, 2*l2 - (2*b12)*l1, 0], [2*l1 - (2*b13)*l3, 0, 2*l3 - (2*b13)*l1],
 *                [0, 2*l2 - (2*b23)*l3, 2*l3 - (2*b23)*l2]];  C = cof(J);  dj = det(J);
 *           l_i = l_i - dot(C[:][i], r) / dj for i = 1, 2, 3 from the old values; a step with dj == 0 changes nothing.
 *         X_i = l_i * f_i;  u = X1 - X2;  v = X1 - X3;  w = cross(u, v);  Bc = [u v w] (columns);  C = cof(Bc);
 *         dc = det(Bc);  dropped when dc == 0;  inv[k][j] = C[j][k] / dc;
 *         R[i][j] = dot((d12_i, d13_i, ww_i), inv[:][j]);   t_i = p1_i - dot(R[i][:], X1).
 *     At most four candidates, in the order (+s, +sqrt) (+s, -sqrt) (-s, +sqrt) (-s, -sqrt).
 *     The counts were settled the way rule 4's sweep counts were.
 * A4. Disambiguation.  The model is the FIRST candidate with the smallest A1 score of the sample's fourth point; a
 *     score that is not finite counts as +infinity.  With no candidate, or all scores infinite, the hypothesis has
 *     no model, is written out as an all-zero [3][4] and has zero inliers.
 * A5. Selection.  Rule 6 with w^4 (two squarings) in place of w^8.  FOUND when best >= 4.
 *
 * ebo_absolute_pose_ransac (replaces opengv::sac::Ransac::computeModel over AbsolutePoseSacProblem(KNEIP),
 *   visual_odometry.cpp:236-250, for MANY keyframes in one call): the contract of ebo_relative_pose_ransac with
 *   (f, points) in place of (f1, f2).  Frame k owns points offsets[k] .. offsets[k+1]-1 of f / points (double
 *   [offsets[n_frames]][3]; offsets[0] = 0).  ALL n_frames x max_iterations hypotheses are sampled, solved (A2-A4)
 *   and scored against every point of their frame (A1) on the device in one pass; the counts come back once, A5 runs
 *   on the host, and one more launch lists the winners' inliers, ascending, as indices within the frame.  `model` of
 *   the result is the camera-to-world pose.  A frame with fewer than 4 points is not found (winner -1, iterations 0),
 *   not an error.  hyp_samples is int [n_frames][max_iterations][4].  A frame's result does not depend on the other
 *   frames of the call.  The caller sets params->threshold (localizeCamera's is
 *   (double)(float)(1 - cos(atan2(reprojectionError, 200)))); ebo_default_two_view_params' 5e-5 is the two-view one.
 *   EBO_ERR_ARG and EBO_ERR_STATE as for ebo_relative_pose_ransac.  Synchronous.
 * ebo_absolute_pose_scores: A1 for a GIVEN pose and n points: scores double [n] and / or inlier flags uint8 [n]
 *   (either may be NULL).  The re-selection after a refinement (visual_odometry.cpp:262-264).
 * The _device forms take device pointers for f and points (and, for scores, for the outputs); the scores form is
 *   asynchronous on the context's stream.
 * ebo_two_view_timing brackets ebo_absolute_pose_ransac too, with the same five slots. */
int ebo_absolute_pose_ransac(ebo_ctx* ctx, int n_frames, const int* offsets, const double* f, const double* points,
							 const ebo_two_view_params* params, ebo_two_view_result* result, int* inlier_idx,
							 int* hyp_counts_or_null, double* hyp_models_or_null, int* hyp_samples_or_null);
int ebo_absolute_pose_ransac_device(ebo_ctx* ctx, int n_frames, const int* offsets, const double* d_f, const double* d_points,
									const ebo_two_view_params* params, ebo_two_view_result* result, int* inlier_idx,
									int* hyp_counts_or_null, double* hyp_models_or_null, int* hyp_samples_or_null);
int ebo_absolute_pose_scores(ebo_ctx* ctx, const double* pose, int n, const double* f, const double* points, double threshold,
							 double* scores_or_null, uint8_t* inlier_flags_or_null);
int ebo_absolute_pose_scores_device(ebo_ctx* ctx, const double* pose, int n, const double* d_f, const double* d_points,
									double threshold, double* d_scores_or_null, uint8_t* d_inlier_flags_or_null);

/* ---- bundle adjustment: windowed Levenberg-Marquardt with a Schur complement ----------------------------
 * What VisualOdometryFrontEnd::optimize (visual_odometry.cpp:416-497) does through Ceres on reprojection_error.h and
 * local_parameterization_se3.hpp, and with the points held constant the refinement after localizeCamera's RANSAC
 * (:262), stated as this project's own rules for MANY small problems in one call.  Parity with Ceres, Sophus or Eigen
 * is NOT claimed (INTEGRATION.md 7 lists the differences).  tests/bundle_ref.py restates every rule in numpy.  The
 * conventions are those of "absolute pose": float64, one rounding per operation in the association written here, no
 * contraction, only + - * / sqrt and comparisons, a comparison with a NaN is false.  dot is the two-view section's;
 * dot6(a, b) = ((((a0*b0 + a1*b1) + a2*b2) + a3*b3) + a4*b4) + a5*b5.
 * A problem is F frames, P points and N observations (frame, point, u, v).  A pose T = [R | t] is double [3][4],
 * camera to world (Tw2c); a frame whose `fixed` flag is set is constant; the camera is constant.  Unless fix_points
 * is set, a point with fewer than two observations takes no part (the size() < 2 skip of :445): its observations
 * are dropped and it comes back unchanged.  With fix_points every point is constant and every observation takes part.
 * The variables are 6 per free frame (ups, om) and 3 per point that takes part.
 *
 * B1. Residual.  d = X - t;  q_j = (R[0][j] * d0 + R[1][j] * d1) + R[2][j] * d2;  (uh, vh) = project(q) of the camera
 *     section;  r = (u - uh, v - vh).
 * B2. Loss (ceres::HuberLoss(a) with the corrector for rho'' <= 0, as host_lm.cpp has it).  s = r0 * r0 + r1 * r1;
 *     b = a * a;  when s > b: root = sqrt(s); rho = (2 * a) * root - b; rho' = max(DBL_MIN, a / root);  otherwise
 *     rho = s, rho' = 1.  sr = sqrt(rho');  rt = (r0 * sr, r1 * sr) is the corrected residual.
 * B3. Jacobian.  With xP, yP, r2, rad of project:  dr = k1 + (2 * k2) * r2;
 *       dxx = ((rad + ((2 * xP) * xP) * dr) + (2 * p1) * yP) + (6 * p2) * xP;
 *       dxy = ((((2 * xP) * yP) * dr) + (2 * p1) * xP) + (2 * p2) * yP;
 *       dyy = ((rad + ((2 * yP) * yP) * dr) + (2 * p2) * xP) + (6 * p1) * yP;      iz = 1 / q2;
 *       A[0] = (fx * (dxx * iz), fx * (dxy * iz), fx * (-((dxx * xP + dxy * yP) * iz))) * sr    (each entry times sr)
 *       A[1] = (fy * (dxy * iz), fy * (dyy * iz), fy * (-((dxy * xP + dyy * yP) * iz))) * sr
 *     (A = sr d(project)/dq; k3 unused as in the model.)  With dq/dups = -I, dq/dom = hat(q), dq/dX = R^T, row k of
 *       Jc = (A[k][0], A[k][1], A[k][2], A[k][2]*q1 - A[k][1]*q2, A[k][0]*q2 - A[k][2]*q0, A[k][1]*q0 - A[k][0]*q1)
 *       Jp = (-dot(A[k], R[0][:]), -dot(A[k], R[1][:]), -dot(A[k], R[2][:]))
 *     and every entry is then multiplied by the scale of its column (B6).
 * B4. Update, on the right as LocalParameterizationSE3::Plus does, without sin / cos:  h = om * 0.5;
 *       n = sqrt(1 + ((hx*hx + hy*hy) + hz*hz));  (x, y, z, w) = (hx / n, hy / n, hz / n, 1 / n);  C = the matrix of
 *       that quaternion by common::Pose3d's formula (x2 = 2 * x, ..; twx = x2 * w, ..; txx = x2 * x, txy = y2 * x,
 *       txz = z2 * x, tyy = y2 * y, tyz = z2 * y, tzz = z2 * z; C = [[1 - (tyy + tzz), txy - twz, txz + twy],
 *       [txy + twz, 1 - (txx + tzz), tyz - twx], [txz - twy, tyz + twx, 1 - (txx + tyy)]]);
 *       R'[i][j] = dot(R[i][:], C[:][j]);  t'_i = t_i + dot(R[i][:], ups).   A point: X' = X + step.
 *     Every step entry is first multiplied by its column's scale.  No re-orthonormalisation.
 * B5. Sums.  Observations are in (point, frame) order, no pair twice.  With J0, J1 the two rows of an observation:
 *       U_k[a][b] = sum of (J0c[a] * J0c[b] + J1c[a] * J1c[b]),  g_k[a] = sum of (J0c[a] * rt0 + J1c[a] * rt1)
 *         over the observations of free frame k in ascending point order, from 0;
 *       V_l[a][b], g_l[a] the same with Jp over the observations of point l in ascending frame order (ALL its frames);
 *       W_o[a][b] = J0c[a] * J0p[b] + J1c[a] * J1p[b] for an observation o of a free frame.
 * B6. Column scaling (Ceres' Jacobi scaling; opts->jacobi_scaling): scale_c = 1 / (1 + sqrt(n_c)), n_c = the diagonal
 *     entry of U_k / V_l computed at the start with all scales 1; fixed for the solve.
 * B7. Damping and point blocks.  damp(d) = l * l with l = sqrt(min(max(d, min_lm_diagonal), max_lm_diagonal) / radius),
 *     added to every diagonal entry d of U_k and V_l.  inv(V_l)[i][j] = C[j][i] / det with cof / det of A3; a
 *     determinant that is not > 0 makes the step invalid.  Y_o[a][b] = dot(W_o[a][:], inv(V_l)[:][b]).
 * B8. Reduced system over the free frames in ascending order, 6 rows each:  for rows (j, a), (k, b):
 *       S = (U_k[a][b] with its damping when j = k, otherwise 0), then minus dot(Y_oj[a][:], W_ok[b][:]) for every point
 *       l seen by both, in ascending l;   rhs = g_k[a], then minus dot(Y_ok[a][:], g_l) in ascending l.
 *     Cholesky S = L L^T, lower, column by column: every entry loses its products L[i][k] * L[j][k] one at a time in
 *     ascending k, then is divided by the pivot's square root; a pivot that is not > 0 or not finite makes the step
 *     invalid.  L y = rhs: y_k = rhs_k / L[k][k], then rhs_i = rhs_i - L[i][k] * y_k for i > k, k ascending.
 *     L^T x = y: x_k = y_k / L[k][k], then y_i = y_i - L[k][i] * x_k for i < k, k DEscending.  Points:
 *       e[b] = g_l[b], then minus dot6(W_o[:][b], x_k) over the point's observations in free frames, ascending;
 *       x_l[a] = dot(inv(V_l)[a][:], e).    step = -x; an entry that is not finite makes the step invalid.
 *     With fix_points there are no point blocks: S is the damped U_k on its diagonal blocks, rhs = g_k.
 * B9. Trust region: TrustRegionMinimizer + LevenbergMarquardtStrategy as HostLm (csrc/host_lm.cpp) restates them.
 *     tree(v): 256 partial sums, partial i = v[i] + v[i + 256] + .. in that order from 0; then for s = 128, 64, .., 1:
 *     partial[i] = partial[i] + partial[i + s] for i < s; the result is partial[0].
 *       cost = 0.5 * tree(rho over the observations);
 *       model cost change = -tree(m), m = mr0 * (rt0 + mr0 / 2) + mr1 * (rt1 + mr1 / 2),
 *         mr_k = dot6(Jc row k, step of the frame) (0 for a fixed frame) + dot(Jp row k, step of the point) (0 with fix_points);
 *         a change that is not > 0 makes the step invalid;
 *       |x| = sqrt(tree(squares of the 12 pose entries of every free frame and the 3 of every point that takes part, in
 *         array order, 0 for the others)), the step norm the same of (x - candidate);
 *       gradient norm = max over the variables of |g_c / scale_c| (0 when there is none).
 *     An invalid step: radius = radius * 0.5, and termination 2 after max_consecutive_invalid in a row.  A candidate
 *     whose cost is not finite counts as DBL_MAX (a rejected step).  Then, in this order: converged when
 *     step norm <= parameter_tolerance * (|x| + parameter_tolerance); converged when
 *     |cost - candidate cost| <= function_tolerance * cost (the candidate is not taken); quality, acceptance
 *     (quality > min_relative_decrease), radius = min(max_radius, radius / max(1/3, 1 - (2q - 1)^3)) with
 *     (2q - 1)^3 = (c * c) * c, rejection radius = radius / decrease, decrease = decrease * 2, and the non-monotonic
 *     bookkeeping exactly as HostLm::supply.  Before each iteration: termination 1 at max_num_iterations, converged
 *     when the last step was taken and gradient norm <= gradient_tolerance, converged when radius < min_radius.
 *     The result is the lowest-cost point visited.  A cost that is not finite at the start is termination 2 with
 *     poses and points returned bit for bit.
 *
 * ebo_bundle_adjust: problem p owns frames frame_offsets[p] .. frame_offsets[p+1]-1 of poses ([.][3][4]) and
 *   pose_fixed, points point_offsets[p] .. of points ([.][3]) and observations obs_offsets[p] .. of obs_frame,
 *   obs_point (indices LOCAL to the problem) and obs_uv ([.][2]); all offsets start at 0.  Observations may come in
 *   any order; the entry sorts them.  poses and points are updated in place with the solver's best point; one
 *   ebo_summary per problem (num_evals_jac counts Jacobian evaluations, num_evals_cost candidate evaluations).
 *   trace_or_null: double [n_problems][opts->max_num_iterations + 1][4] = (cost, radius after the iteration, step
 *   quality, flag) per iteration, row 0 the start; flag 1 taken, 0 rejected, -1 invalid step, 2 converged at this
 *   candidate; rows never reached are 0.  fix_points non-zero holds every point constant: one 6 x 6 system per free
 *   frame, the pose refinement.  opts as ebo_default_ba_opts fills them (Ceres' Solver::Options defaults, which the
 *   reference leaves untouched at :488-491); opts->mode is not read.
 *   Limits per problem: 24 frames, 4096 points, 65535 observations; 65535 problems.  EBO_ERR_ARG beyond them and for
 *   an index out of range, a (frame, point) pair observed twice, offsets that decrease or do not start at 0, huber not
 *   positive (or NaN), a negative max_num_iterations, a needed pointer NULL.  EBO_ERR_STATE while a graph is being
 *   recorded.  A problem's result depends neither on the other problems of the call nor on the run.  Synchronous.
 * ebo_bundle_adjust_device: device pointers for every array except the offsets, cam, opts and summaries.  It cannot
 *   look at the indices: observations must already be in (point, frame) order with indices in range and no pair
 *   twice; a problem for which that does not hold is not solved (termination 2, its poses and points untouched).
 * ebo_two_view_timing brackets both: slot [0] the kernel, [4] the whole call, the others 0. */
void ebo_default_ba_opts(ebo_solver_opts* opts);
int ebo_bundle_adjust(ebo_ctx* ctx, int n_problems, const int* frame_offsets, const int* point_offsets, const int* obs_offsets,
					  double* poses, const uint8_t* pose_fixed, double* points, const int* obs_frame, const int* obs_point,
					  const double* obs_uv, const ebo_camera* cam, double huber, int fix_points, const ebo_solver_opts* opts,
					  ebo_summary* summaries, double* trace_or_null);
int ebo_bundle_adjust_device(ebo_ctx* ctx, int n_problems, const int* frame_offsets, const int* point_offsets,
							 const int* obs_offsets, double* d_poses, const uint8_t* d_pose_fixed, double* d_points,
							 const int* d_obs_frame, const int* d_obs_point, const double* d_obs_uv, const ebo_camera* cam,
							 double huber, int fix_points, const ebo_solver_opts* opts, ebo_summary* summaries,
							 double* d_trace_or_null);

/* ---- landmark maintenance: N-view triangulation and the audit of landmarks -------------------------------
 * The reference triangulates a landmark once, from the first two keyframes that observe it
 * (VisualOdometryFrontEnd::addNewLandmarks, visual_odometry.cpp:353), and never removes one (its TODOs at :169 and
 * :407).  These entries take a landmark's WHOLE observation list, for every landmark of a call at once.
 * tests/landmark_ref.py restates every rule in numpy.  The conventions are those of "absolute pose": float64, one
 * rounding per operation in exactly the association written here, no contraction, only + - * / sqrt and comparisons;
 * a comparison with a NaN is false.  dot, cross, cof, det, jacobi(M, sweeps), mix / hash and the score A1 are the ones
 * stated there.
 * A pose is camera-to-world [R | t], double [3][4].  Observation o of a landmark is (pose index k_o, bearing vector
 * f_o in that camera); landmark l owns observations obs_offsets[l] .. obs_offsets[l+1]-1 of obs_pose and obs_f, m
 * their number; o below is the index WITHIN the landmark.
 *
 * L1. World rays.  d_o[i] = dot(R[i][:], f_o);  c_o = t of the pose;  c_ref = the centre of the landmark's
 *     observation 0 (used or not);  e_o = c_o - c_ref.  Bearing vectors are taken as they come, not renormalised.
 * L2. Least-squares point over a set U of observations.  Per observation: dd = dot(d, d);  A_ii = dd - d_i * d_i;
 *     A_ij = -(d_i * d_j) for i != j;  a_i = dot(A[i][:], e).  Each of the nine sums (M00 M01 M02 M11 M12 M22 of the
 *     symmetric M = sum of A, and b = sum of a) is taken as SIXTEEN partials: partial j = +0, then plus the term of every
 *     o in U with o = j (mod 16) in ascending o; then for s = 8, 4, 2, 1: partial[i] = partial[i] + partial[i + s] for
 *     i < s; the sum is partial[0].  C = cof(M);  D = det(M).  NO POINT unless D > 0.
 *       x_i = dot((C[0][i], C[1][i], C[2][i]), b) / D;   X = c_ref + x.
 * L3. Parallax of a set U.  (lambda, V) = jacobi(M, 8);  lo = lambda_0, replaced by lambda_1 and then by lambda_2 where
 *     that is strictly smaller;  parallax = (2 * lo) / |U|.  For two unit rays at the angle theta this is
 *     1 - cos(theta); for more it is twice the mean squared sine of their angles to the principal direction.
 * L4. Hypotheses.  n_pairs = m (m - 1) / 2.  With n_pairs <= max_hypotheses there are n_pairs of them, hypothesis h
 *     the h-th pair (a, b), a < b, in lexicographic order.  Otherwise there are max_hypotheses, (a, b) = the two
 *     distinct indices of rule 3's Fisher-Yates shuffle with TWO draws, hash(seed, 0, h, d): the `pair` slot is the
 *     constant 0, so a landmark's answer depends on its own observations and the seed, not on its place in the call.
 *     Gate:  g = dot(d_a, d_b);  n2 = dot(d_a, d_a) * dot(d_b, d_b);  valid only when n2 > 0 and
 *     1 - g / sqrt(n2) >= min_parallax.  X_h = L2 over {a, b}; invalid when there is no point.
 *     count[h] = the number of the landmark's observations (all m, a and b among them) with A1(pose_o, f_o, X_h) <
 *     threshold.  The winner is the FIRST valid h with the largest count, and only when that count is >= 2.
 * L5. Final point.  U = the winner's inliers;  X = L2 over U;  parallax = L3 over U.  Then one re-selection without
 *     another solve (as selectWithinDistance after the reference's refinements, visual_odometry.cpp:270):
 *     score_o = A1(pose_o, f_o, X), inlier_o = score_o < threshold, n_inliers their number, score_max the largest
 *     finite score over all m observations (0 when none is finite).  With threshold in (0, 1) an inlier lies in front
 *     of its camera along its ray: there is no separate cheirality test.
 * L6. Status, the first that applies:
 *       2  an entry of one of the landmark's poses or bearing vectors is not finite (for the audit also an entry of
 *          its point), or a pose index is out of range in a _device call: a scan before anything else
 *       1  m < 2
 *       3  no valid hypothesis with count >= 2
 *       4  L5's solve has no point, or parallax >= min_parallax is false (parallax is computed either way)
 *       5  n_inliers < min_inliers
 *       0  otherwise.
 *     With a status other than 0 the point is zeros.  parallax, score_max and n_inliers hold what had been computed
 *     when the status was decided and zeros before that: all zero for 2, 1 and 3; parallax alone for 4; all three for 5.
 *     winner is -1 unless L4 found one; hypotheses is the number L4 formed (0 for 2 and 1).  Per-observation scores
 *     and flags are those of L5's re-selection where it ran (status 0 and 5) and zeros elsewhere.
 * L7. Audit.  X is given.  L6's scan; status 1 when m < 1; then L5's re-selection under X; then M of L2 over those
 *     inliers for L3's parallax (b and the solve are skipped; parallax = 0 with no inlier).  Status 4 when
 *     parallax >= min_parallax is false, else 5 when n_inliers < min_inliers, else 0.  winner = -1, hypotheses = 0;
 *     result.point repeats X with status 0; the points array itself is never written.  parallax, score_max, n_inliers
 *     and the per-observation scores and flags are the selection's for every status but 2 and 1, where they are zeros.
 *
 * ebo_triangulate_tracks: L1-L6 for every landmark.  ebo_landmark_scores: L7 with points double [n_landmarks][3].
 *   scores is double [obs_offsets[n_landmarks]], inlier_flags uint8 of the same length; either may be NULL.
 *   Limits: 512 observations per landmark, 2^20 landmarks per call, max_hypotheses 1 .. 4096, min_inliers >= 2.
 *   EBO_ERR_ARG beyond them, for a threshold outside (0, 1), a negative or NaN min_parallax, offsets that decrease or
 *   do not start at 0, a pose index out of range, a needed pointer NULL.  EBO_ERR_STATE while a graph is being
 *   recorded.  A landmark's result depends neither on the other landmarks of the call nor on the run.  Synchronous.
 * The _device forms take device pointers for poses, obs_pose, obs_f, points, results, scores and flags (obs_offsets
 *   and params stay on the host) and are asynchronous on the context's stream; they cannot look at the pose indices:
 *   a landmark with one out of range gets status 2.
 * ebo_two_view_timing brackets the host forms: slot [0] the kernel, [4] the whole call, the others 0. */
typedef struct ebo_landmark_params
{
	double threshold;     /* A1 score below which an observation is an inlier; in (0, 1) */
	double min_parallax;  /* L3 / L4's gate; >= 0 */
	int min_inliers;      /* >= 2 */
	int max_hypotheses;   /* 1 .. 4096 */
	uint64_t seed;        /* L4's sampling */
} ebo_landmark_params;
typedef struct ebo_landmark_result
{
	double point[3];
	double parallax;
	double score_max;
	int status;      /* L6 */
	int n_obs;       /* m */
	int n_inliers;
	int winner;      /* L4's h, or -1 */
	int hypotheses;  /* the number L4 formed */
	int reserved;    /* 0 */
} ebo_landmark_result;
/* threshold (double)(float)(1 - cos(atan2(2, 200))), localizeCamera's at its default reprojection error;
 * min_parallax 1 - cos(1 degree), a policy default in the range ORB-SLAM and COLMAP use, not a measured number;
 * min_inliers 2; max_hypotheses 300 (every landmark of up to 25 observations is exhaustive); seed 0. */
void ebo_default_landmark_params(ebo_landmark_params* params);
int ebo_triangulate_tracks(ebo_ctx* ctx, int n_poses, const double* poses, int n_landmarks, const int* obs_offsets,
						   const int* obs_pose, const double* obs_f, const ebo_landmark_params* params,
						   ebo_landmark_result* results, double* scores_or_null, uint8_t* inlier_flags_or_null);
int ebo_triangulate_tracks_device(ebo_ctx* ctx, int n_poses, const double* d_poses, int n_landmarks, const int* obs_offsets,
								  const int* d_obs_pose, const double* d_obs_f, const ebo_landmark_params* params,
								  ebo_landmark_result* d_results, double* d_scores_or_null, uint8_t* d_inlier_flags_or_null);
int ebo_landmark_scores(ebo_ctx* ctx, int n_poses, const double* poses, int n_landmarks, const int* obs_offsets,
						const int* obs_pose, const double* obs_f, const double* points, const ebo_landmark_params* params,
						ebo_landmark_result* results, double* scores_or_null, uint8_t* inlier_flags_or_null);
int ebo_landmark_scores_device(ebo_ctx* ctx, int n_poses, const double* d_poses, int n_landmarks, const int* obs_offsets,
							   const int* d_obs_pose, const double* d_obs_f, const double* d_points,
							   const ebo_landmark_params* params, ebo_landmark_result* d_results, double* d_scores_or_null,
							   uint8_t* d_inlier_flags_or_null);

/* ---- angular velocity from events: rotational contrast maximisation ------------------------------
 * A global warp of every resident window by the camera's rotation, the variance of the image of warped events as the
 * objective, its exact gradient, and a three-variable solver: one angular velocity per window.  The rules are this
 * project's own (the reference has no counterpart); tests/rotation_ref.py restates them in numpy.  All arithmetic is
 * float64; in V2 and V3 every operation is rounded on its own, in the association written, with no contraction
 * (__dadd_rn and the others, as the camera model), because they decide integer bits.
 *
 * Inputs: the windows resident in the context, loaded by any ebo_set_window* loader (rectified coordinates when a
 * rectification is set; events of a window's stray unit take no part); a pinhole camera `cam` under rule C1 (k1 k2 p1
 * p2 all zero, else EBO_ERR_ARG; fx or fy not finite or zero: EBO_ERR_RANGE); one omega = (wx, wy, wz) in rad/s per
 * window, the camera's angular velocity in the camera frame: a static point moves by dX/dt = -omega x X.
 *
 * V1. Per event: integer pixel (x, y), dt = t_ref(window) - t_event in microseconds, t_ref(window) as ebo_window_info
 *     reports it.   a = (x - cx) / fx;  b = (y - cy) / fy;  tau = dt * 1e-6;  th = (tau * wx, tau * wy, tau * wz).
 * V2. First-order rotation to the reference time, X - th x X on (a, b, 1):
 *       X = (a - thy) + thz * b;   Y = (b - thz * a) + thx;   Z = (1 - thx * b) + thy * a
 *     If not (Z > 0) the event is skipped.   u = fx * (X / Z) + cx;   v = fy * (Y / Z) + cy.
 *     If not (u > -1 and u < w and v > -1 and v < h) the event is skipped.  Both tests are made in double before any
 *     conversion to an integer: a NaN, an infinity or omega = 1e9 skips the event and reads or writes nothing.  omega is
 *     not validated; a NaN in it gives the empty image and the zeros the rules give.
 * V3. Bilinear vote in exact fixed point.  x0 = floor(u); y0 = floor(v); al = u - x0; be = v - y0; ial = 1 - al;
 *     ibe = 1 - be.  The weights ial * ibe, al * ibe, ial * be, al * be go to (x0, y0), (x0+1, y0), (x0, y0+1),
 *     (x0+1, y0+1).  Each becomes the int64 q = rint(weight * 2^30), ties to even, added to the int64 vote image H[y][x]
 *     at the taps inside the image.  Integer adds commute: H depends neither on the order of the events nor on the
 *     kernel's design, and cannot overflow below 2^31 events per window.
 * V4. F = H * 2^-30.
 * V5. Blur.  sigma_blur (default 1.0) is 0 or positive and finite, else EBO_ERR_ARG.  For sigma_blur > 0 the seven
 *     weights g_d = exp(-d^2 / (2 sigma^2)), d = -3 .. 3, are divided by their sum taken in that order, on the host (the
 *     kernels receive seven doubles and call no exp).  B = the horizontal pass followed by the vertical pass; an output
 *     is the sum, from 0, in tap order d = -3 .. 3 of g_d * value; taps outside the image are skipped, nothing is
 *     renormalised.  With sigma_blur = 0, B = F (the weights 0 0 0 1 0 0 0 give exactly that).
 * V6. Np = w * h;  mu = sum(B) / Np;  r = sum((B - mu)^2) / Np: the variance, to be maximised.
 * V7. C = the same two passes applied to B - mu.  The blur with dropped taps is a symmetric operator and
 *     sum(B - mu) = 0, so V8 is the exact gradient of V6 between pixel crossings.
 * V8. For every event that voted, c00 c10 c01 c11 = C at its four taps, 0 at a tap outside the image.
 *       Du = ibe * (c10 - c00) + be * (c11 - c01);   Dv = ial * (c01 - c00) + al * (c11 - c10)
 *       dX/dth = (0, -1, b);  dY/dth = (1, 0, -a);  dZ/dth = (-b, a, 0)
 *       du/dth_i = fx * (dX_i * Z - X * dZ_i) / Z^2;   dv/dth_i = fy * (dY_i * Z - Y * dZ_i) / Z^2
 *       g_i = (2 / Np) * sum over the events of tau * (Du * du/dth_i + Dv * dv/dth_i)
 *     At al = 0 or be = 0 this is the right-hand derivative, which is what floor gives.
 * V9. H is bit-equal to the restatement.  r and g are deterministic: the same bits for a window alone, inside any
 *     batch, at any position of it, and from run to run -- every sum follows a fixed order that does not depend on the
 *     launch: 256 consecutive pixels (resp. a patch's events, lane t taking events t, t + 256, ..) fold by the wave's
 *     shuffle tree 32, 16, .. 1 and then wave 0 + 1 + 2 + 3; of a window's folds, lane l of one wave adds folds l, l + 64, ..
 *     in ascending order and the same shuffle tree adds the lanes.  Against
 *     the restatement |dr| <= 1e-9 * sum(B^2) / Np and |dg_i| <= 1e-9 * A_i with
 *     A_i = (2 / Np) * sum |tau| * (|Du * du/dth_i| + |Dv * dv/dth_i|): a float64 sum of n <= 2e5 terms errs by at most
 *     n * 2^-53 = 2e-11 of these scales.
 *
 * The solver minimises f = -r with gf = -g; dot(a, b) = (a0 * b0 + a1 * b1) + a2 * b2.
 * N1. Evaluate at omega0.  f or gf not finite: NONFINITE.  gmax = max |gf_i|; gmax == 0: CONVERGED_GRADIENT.
 *     alpha = first_rate / gmax (the largest component of the first trial step is first_rate).
 * N2. d = -gf; slope = -dot(gf, gf); omega_t = omega + alpha * d.  Evaluate (f_t, gf_t) at omega_t.
 * N3. Accepted when f_t and gf_t are finite and f_t <= f + (c1 * alpha) * slope.  Otherwise alpha = alpha / 2,
 *     backtracks += 1; at max_backtracks: NO_PROGRESS, keeping omega; else N2.
 * N4. Accepted: s = omega_t - omega; y = gf_t - gf; (omega, f, gf) = (omega_t, f_t, gf_t); iterations += 1;
 *     backtracks = 0.  max |s_i| < step_tol: CONVERGED_STEP.  iterations == max_iterations: MAX_ITERATIONS.  Otherwise
 *     sy = dot(s, y); alpha = dot(s, s) / sy when sy > 0 (Barzilai-Borwein), else 2 * alpha; N2.
 * N5. The summary: status, iterations, evaluations, r at omega0 and r at the result.
 *
 * ebo_eval_rotation: r [Wn] and, unless g is NULL, g [Wn][3] at omegas [Wn][3] for all resident windows; with g NULL
 *   the value-only path skips V7 and V8 and returns the same r bits.  Host pointers, synchronous.  The _device form
 *   takes device pointers and is asynchronous on the context's stream.
 * ebo_rotation_image: H as int64 [Wn][h][w] and F as double [Wn][h][w] (either may be NULL): F is the image of
 *   rotationally compensated events a user looks at.
 * ebo_rot_solver_*: N1-N5 for n windows at once as a host object, no device and no context involved.
 *   _request(omegas [n][3], live [n] or NULL): the points wanted; returns the number of windows still waiting (0: all
 *   finished), < 0 = EBO_ERR_*.  _supply(r [n], g [n][3]): entries of finished windows are ignored; EBO_ERR_STATE once
 *   all have finished.  _result(omegas [n][3] or NULL, summary [n] or NULL).
 * ebo_solve_rotation: lock-step rounds over the resident windows from omega0 ([Wn][3], NULL: zeros); every round
 *   evaluates the windows still waiting, and only those, in one batched pass, then the host solver steps.  A window's
 *   result has the same bits alone and in any batch (V9).
 * Evaluation scratch is three images of 8 bytes a pixel per window; windows are evaluated in chunks of at most 64 under
 *   a budget of 256 MiB (environment EBO_ROTATION_SCRATCH_MB).
 * Errors: EBO_ERR_STATE with no windows loaded, with units loaded by ebo_set_patches, or while a graph is being
 *   recorded; EBO_ERR_ARG / EBO_ERR_RANGE as in the rules; EBO_ERR_ARG for a needed pointer that is NULL or solver
 *   options outside first_rate > 0, 0 < c1 < 1, max_backtracks >= 1, step_tol >= 0, max_iterations >= 1. */
#define EBO_ROT_RUNNING -1
#define EBO_ROT_CONVERGED_STEP 0
#define EBO_ROT_CONVERGED_GRADIENT 1
#define EBO_ROT_MAX_ITERATIONS 2
#define EBO_ROT_NO_PROGRESS 3
#define EBO_ROT_NONFINITE 4
typedef struct ebo_rotation_params
{
	double sigma_blur;  /* V5; 0 or positive and finite */
	double reserved;    /* 0 */
} ebo_rotation_params;
typedef struct ebo_rot_solver_opts
{
	double first_rate;   /* rad/s, N1 */
	double c1;           /* N3 */
	double step_tol;     /* rad/s, N4 */
	int max_backtracks;  /* N3 */
	int max_iterations;  /* N4 */
} ebo_rot_solver_opts;
typedef struct ebo_rot_summary
{
	int status;       /* EBO_ROT_* */
	int iterations;   /* accepted steps */
	int evaluations;  /* evaluations supplied */
	int reserved;     /* 0 */
	double r_initial; /* r at omega0 */
	double r_final;   /* r at the result */
} ebo_rot_summary;
/* sigma_blur 1.0 */
void ebo_default_rotation_params(ebo_rotation_params* params);
/* first_rate 0.5, c1 1e-4, step_tol 1e-4, max_backtracks 20, max_iterations 100 */
void ebo_default_rot_solver_opts(ebo_rot_solver_opts* opts);
int ebo_eval_rotation(ebo_ctx* ctx, const ebo_camera* cam, const ebo_rotation_params* params, const double* omegas, double* r,
					  double* g_or_null);
int ebo_eval_rotation_device(ebo_ctx* ctx, const ebo_camera* cam, const ebo_rotation_params* params, const double* d_omegas,
							 double* d_r, double* d_g_or_null);
int ebo_rotation_image(ebo_ctx* ctx, const ebo_camera* cam, const double* omegas, int64_t* votes_or_null, double* image_or_null);
typedef struct ebo_rot_solver ebo_rot_solver;
int ebo_rot_solver_create(int n, const ebo_rot_solver_opts* opts, const double* omega0_or_null, ebo_rot_solver** out);
int ebo_rot_solver_request(ebo_rot_solver* s, double* omegas, uint8_t* live_or_null);
int ebo_rot_solver_supply(ebo_rot_solver* s, const double* r, const double* g);
int ebo_rot_solver_result(const ebo_rot_solver* s, double* omegas_or_null, ebo_rot_summary* summary_or_null);
void ebo_rot_solver_destroy(ebo_rot_solver* s);
int ebo_solve_rotation(ebo_ctx* ctx, const ebo_camera* cam, const ebo_rotation_params* params, const ebo_rot_solver_opts* opts,
					   const double* omega0_or_null, double* omega_out, ebo_rot_summary* summary_or_null);

/* ---- depth from events: space-sweep voting --------------------------------------------------------
 * A semi-dense depth map of a reference view from the events themselves, with known poses (event-based multi-view
 * stereo by space sweep): every event is back-projected as a ray through a stack of depth planes of the reference view,
 * the votes are counted per voxel, and the pixels where rays meet are kept with their depth.  The rules are this
 * project's own; tests/depth_ref.py restates them in numpy.  All arithmetic is float64; in M2 and M3 every operation is
 * rounded on its own, in the association written, with no contraction, because they decide integer bits.
 *
 * Inputs: the windows resident in the context, loaded by any ebo_set_window* loader (rectified coordinates when a
 * rectification is set).  The event set is ebo_rotation_image's: events of a window's stray unit take no part, units
 * count whether active or not; polarity and event time are ignored.  A pinhole camera under rule C1 (k1 k2 p1 p2 all
 * zero, else EBO_ERR_ARG; fx or fy not finite or zero: EBO_ERR_RANGE).  A reference pose and one pose per window, each
 * 12 doubles (R row-major, t), camera to world, as in A1, B1 and L1.  Poses are not validated.
 *
 * M1. Planes.  2 <= Nz <= 256, 0 < z_near < z_far, both finite, else EBO_ERR_ARG.  rho_0 = 1 / z_near;
 *     drho = (1 / z_far - rho_0) / (Nz - 1);  rho_k = rho_0 + k * drho;  z_k = 1 / rho_k: uniform in inverse depth, plane
 *     0 the nearest.  The table is made on the host; the kernels receive it.
 * M2. Relative pose, on the host per window, Rref / tref the reference pose and Rw / tw the window's:
 *       Rr[i][j] = (Rref[0][i] * Rw[0][j] + Rref[1][i] * Rw[1][j]) + Rref[2][i] * Rw[2][j];   e = tw - tref;
 *       tr_i = (Rref[0][i] * e0 + Rref[1][i] * e1) + Rref[2][i] * e2
 *     Per event at integer pixel (x, y):  a = (x - cx) / fx;  b = (y - cy) / fy;
 *       d_i = (Rr[i][0] * a + Rr[i][1] * b) + Rr[i][2]
 * M3. Per event and plane k:  lam = (z_k - tr2) / d2.  If not (lam > 0) there is no vote on this plane.
 *       X = tr0 + lam * d0;   Y = tr1 + lam * d1;   u = fx * (X / z_k) + cx;   v = fy * (Y / z_k) + cy
 *     If not (u > -1 and u < w and v > -1 and v < h) there is no vote.  Both tests are made in double before any
 *     conversion: a NaN or an infinity anywhere, a pose included, reads and writes nothing.
 * M4. Vote.  The bilinear weights of V3 (x0 = floor(u), y0 = floor(v), al, be, ial, ibe and the four products) each
 *     become q = rint(weight * 2^10), ties to even, added to the uint32 volume H[k][y][x] at the taps inside the image.
 *     A volume accepts at most 2^21 events in all, counted as the events of the in-sensor units of the windows a call
 *     votes, whether or not they reach a plane; a call that would pass that returns EBO_ERR_RANGE with the volume
 *     unchanged.  With this cap no voxel can overflow.  Integer adds commute: H depends on the set of (event, pose)
 *     pairs only, not on order, batching, the number of calls or the kernel's design.
 * M5. Confidence.  c(x, y) = max_k H[k][y][x]; kbest = the smallest k attaining it.  A pixel with c = 0 is never kept.
 * M6. Adaptive threshold, in integers.  Box radius r in 0 .. 7 (default 2); min_excess in votes, finite and >= 0
 *     (default 3.0), else EBO_ERR_ARG.  off = rint(min_excess * 2^10) as int64 (a min_excess above 2^22 is taken as
 *     2^22: c never exceeds 2^31, so either keeps nothing).  S = the sum of c over the box's pixels inside the image,
 *     cnt their number.  A pixel is kept iff c * cnt > S + off * cnt, in int64.
 * M7. Median.  Radius m in 0 .. 7 (default 2), else EBO_ERR_ARG; m = 0 turns it off (the plane is kbest).  For a kept
 *     pixel: the kbest of the kept pixels of its box, itself included, sorted ascending; the pixel's plane is element
 *     (n - 1) / 2 of that list, the lower median.  The medians are taken from the kbest of M5, not from each other.
 * M8. Outputs.  The plane index int32 [h][w], -1 for a pixel that is not kept; the confidence c uint32 [h][w]; the depth
 *     double [h][w], z_k of the pixel's plane and 0.0 where not kept; the point list in row-major pixel order,
 *     (a * z, b * z, z) in the reference camera frame with a and b as in M2.
 * M9. Every output is bit-equal to the restatement.
 *
 * ebo_dsi_begin: checks camera and parameters (NULL: the defaults), grows the volume to Nz * h * w uint32 and clears
 *   it.  A begin while a volume is open starts over.
 * ebo_dsi_add_windows: votes the resident windows, poses [Wn][12]; use_or_null [Wn]: a window with use 0 is left out.
 *   May be called after every load, and accumulates.
 * ebo_dsi_volume: H as uint32 [Nz][h][w].
 * ebo_dsi_depth: M5-M8 of the volume as it stands (it may be called more than once, and voting may go on).  Every
 *   output may be NULL; points [max_points][3] receives the first max_points kept pixels' points, *n_points_out the
 *   number of kept pixels (which may exceed max_points).
 * ebo_dsi_end: closes the volume; its memory stays with the context for the next begin.
 * Host pointers, synchronous.  Errors: EBO_ERR_STATE without a begin (all but begin), with no windows loaded or units
 *   loaded by ebo_set_patches (add_windows: begin may come before the first load), and while a graph is being recorded
 *   (all); EBO_ERR_ARG /
 *   EBO_ERR_RANGE as in the rules; EBO_ERR_ARG for a needed pointer that is NULL or a negative max_points. */
typedef struct ebo_depth_params
{
	int nz;            /* M1 */
	int box_radius;    /* M6's r */
	int median_radius; /* M7's m */
	int reserved;      /* 0 */
	double z_near;     /* M1 */
	double z_far;
	double min_excess; /* M6, in votes */
} ebo_depth_params;
/* nz 64, z_near 0.5, z_far 8, box_radius 2, min_excess 3, median_radius 2 */
void ebo_default_depth_params(ebo_depth_params* params);
int ebo_dsi_begin(ebo_ctx* ctx, const ebo_camera* cam, const double* ref_pose, const ebo_depth_params* params_or_null);
int ebo_dsi_add_windows(ebo_ctx* ctx, const double* poses, const uint8_t* use_or_null);
int ebo_dsi_volume(ebo_ctx* ctx, uint32_t* out);
int ebo_dsi_depth(ebo_ctx* ctx, int32_t* index_or_null, uint32_t* conf_or_null, double* depth_or_null, double* points_or_null,
				  int max_points, int* n_points_out);
int ebo_dsi_end(ebo_ctx* ctx);

/* ---- pose from events against a map: map-to-event-image alignment ------------------------------------
 * The six-degree-of-freedom camera pose that lays a list of world points (a semi-dense map, for instance the point list
 * of ebo_dsi_depth moved to the world) onto an image, in use the blurred image of a window's events: where the map's
 * points project the image should be bright.  A Levenberg-Marquardt over a dense, image-sampling residual, for many
 * (image, start pose) units in one launch.  The rules are this project's own (the reference has no counterpart);
 * tests/maptrack_ref.py restates them in numpy.  Conventions as in "bundle adjustment": float64, one rounding per
 * operation in exactly the association written here, no contraction, only + - * / sqrt, floor and comparisons; a
 * comparison with a NaN is false.  dot(a, b) = (a0 * b0 + a1 * b1) + a2 * b2.  A pose is 12 doubles, R row-major [3][3]
 * and then t [3], camera to world, as in the depth section (NOT the [3][4] of the bundle adjustment).
 *
 * Inputs: a pinhole camera under C1; n_images images double [n][h][w]; n_points world points [n][3]; n_units units, unit u
 * naming image unit_image[u] and carrying its own start pose.  Several units may name one image (multi-start), several
 * images may be solved at once (a batch).
 *
 * E1. Image scale.  bmax = the largest pixel of the unit's image that is > 0, 0 when there is none (a NaN pixel is never
 *     taken: the result does not depend on the order).  When bmax is not finite or not > 0 the unit is not solved:
 *     termination 2, every other field of its result 0, its trace rows 0, its pose returned bit for bit.  Otherwise
 *     s = 1 / bmax.
 * E2. Projection.  d = X - t;  q_j = dot(R[:][j], d) as in B1;  iz = 1 / q2;  xP = q0 * iz;  yP = q1 * iz;
 *     u = fx * xP + cx;  v = fy * yP + cy.  A point is visible iff q2 > z_min and u >= 0 and u < w - 1 and v >= 0 and
 *     v < h - 1, every test made in double before any conversion: all four taps are inside the image, and a NaN anywhere
 *     makes the point not visible.  Nothing of the image is read for a point that is not visible.
 * E3. Sample.  x0 = floor(u); y0 = floor(v); al = u - x0; be = v - y0; ial = 1 - al; ibe = 1 - be (V3).  b00 b10 b01 b11
 *     = the image at (x0, y0), (x0 + 1, y0), (x0, y0 + 1), (x0 + 1, y0 + 1).
 *       b = ibe * (ial * b00 + al * b10) + be * (ial * b01 + al * b11)
 *       Du = ibe * (b10 - b00) + be * (b11 - b01);   Dv = ial * (b01 - b00) + al * (b11 - b10)      (V8's, on the image)
 * E4. Residual.  r = 1 - s * b for a visible point;  r = 1 with a zero Jacobian row for one that is not, so that pushing
 *     points out of view never lowers the cost.  No loss function: r lies in [0, 1] wherever the image is not negative.
 * E5. Jacobian row for B4's right-hand update.  au = Du * fx;  av = Dv * fy;
 *       A0 = -(s * (au * iz));   A1 = -(s * (av * iz));   A2 = s * ((au * xP + av * yP) * iz)          (A = dr/dq)
 *       J = (-A0, -A1, -A2, A1 * q2 - A2 * q1, A2 * q0 - A0 * q2, A0 * q1 - A1 * q0)
 *     and every entry is then multiplied by the scale of its column (B6).
 * E6. Update.  B4 as it stands: (ups, om) = the step's entries 0-2 and 3-5, each first multiplied by its column's scale.
 * E7. Sums.  The 21 entries J[a] * J[b], b <= a, of J'J, the 6 entries J[a] * r of J'r and r * r, each summed over ALL
 *     points in index order by B9's tree(v): a unit's bits do not depend on the launch.  cost = 0.5 * tree(r * r).
 * E8. Step.  B6's scale_c = 1 / (1 + sqrt(n_c)) from the diagonal of J'J at the start with all scales 1.  B7's damping on
 *     the six diagonal entries; B8's Cholesky and substitutions on that one 6 x 6 block with rhs = J'r; step = -x.  B9's
 *     trust region unchanged, with one free frame and no point variables: model cost change = -tree(m) over the points,
 *     m = mr * (r + mr / 2), mr = dot6(J, step) added as ((((J0 * s0 + J1 * s1) + J2 * s2) + J3 * s3) + J4 * s4) + J5 * s5,
 *     m = 0 for a point that is not visible; |x| and the step norm by tree over the 12 pose entries in the pose's own
 *     order (R, then t); the gradient norm max_c |(J'r)_c / scale_c|; every exit, the non-monotonic bookkeeping, and the
 *     result being the lowest-cost point visited.  A cost that is not finite at the start is termination 2 with the pose
 *     returned bit for bit.
 * E9. Outputs.  The pose, updated in place.  One ebo_map_track_result per unit: termination (0 converged, 1 iteration
 *     limit, 2 failed or not solved), iterations, Jacobian and candidate evaluation counts (as ebo_summary counts them),
 *     initial and final cost, the number of visible points at the start and at the returned pose, and s.  The optional
 *     trace has ebo_bundle_adjust's form, double [n_units][opts->max_num_iterations + 1][4].  Every double and integer is
 *     bit-equal to the restatement (a NaN cost, which E3 gives when a tap reads a NaN, equals any NaN); a unit has the
 *     same bits alone, in any batch, at any position in it and from run to run.
 *
 * ebo_default_map_track_opts: as ebo_default_ba_opts, max_num_iterations 50; opts->mode is not read.
 * ebo_map_track: host pointers, synchronous; uploads what it is given.  z_min: E2's, 0.05 is a sensible value.
 * ebo_map_track_device: device pointers for images, points, unit_image, poses, results and trace; asynchronous on the
 *   context's stream.  It cannot look at unit_image: a unit whose image index is out of range is not solved (termination 2,
 *   the other fields 0, its pose untouched).
 * Limits: 65535 units, 2^20 points, max_num_iterations 10000 (it sizes the trace).  EBO_ERR_ARG beyond them and for a
 *   needed pointer that is NULL, a unit_image out of
 *   range (host form), a camera with distortion, a negative count or max_num_iterations, w or h < 2, z_min not finite;
 *   EBO_ERR_RANGE for fx or fy zero or not finite; EBO_ERR_STATE while a graph is being recorded.  Images, points and
 *   poses are not validated: E1 and E2 say what a bad value does.
 *
 * ebo_event_images: B double [Wn][h][w], V5's blur of V4's image of every resident window at one omega per window
 *   (omegas [Wn][3]; NULL: zeros, and F is then the un-warped integer count image).  params NULL: the defaults.  The
 *   kernels and the chunks are ebo_eval_rotation's.  The _device form takes device pointers and is asynchronous on the
 *   context's stream, so that it chains into ebo_map_track_device without leaving the device.  State and argument errors
 *   as for ebo_rotation_image. */
typedef struct ebo_map_track_result
{
	int termination;    /* 0 converged, 1 iteration limit, 2 failed or not solved */
	int iterations;
	int num_evals_jac;
	int num_evals_cost;
	int visible_start;  /* visible points at the start pose */
	int visible_final;  /* and at the returned one */
	int reserved0;      /* 0 */
	int reserved1;      /* 0 */
	double initial_cost;
	double final_cost;
	double scale;       /* E1's s */
	double reserved2;   /* 0 */
} ebo_map_track_result;
void ebo_default_map_track_opts(ebo_solver_opts* opts);
/* The 13 starts of a multi-start: starts [13][12] = pose, then pose moved through B4 by +step and -step along each of the six
 * update directions in turn (translation_step for ups 0-2, rotation_step for om 0-2): start 1 + 2 a is +, 2 + 2 a is -.
 * Host only, the rule's operations. */
void ebo_map_track_starts(const double* pose, double translation_step, double rotation_step, double* starts);
/* ebo_map_track on the windows resident in ctx, for a caller without device memory of its own: with make_images non-zero
 * the images are ebo_event_images_device's (params, host omegas [Wn][3] or NULL) of every resident window, made into a
 * buffer of the context and kept; with make_images 0 the images of the last such call are used again (EBO_ERR_STATE when
 * there are none or a loader has run since).  unit_window[u] names a resident window; everything else as ebo_map_track,
 * host pointers, synchronous.  The images never leave the device. */
int ebo_map_track_resident(ebo_ctx* ctx, const ebo_camera* cam, const ebo_rotation_params* params_or_null, const double* omegas_or_null,
						   int make_images, int n_points, const double* points, int n_units, const int* unit_window, double* poses,
						   double z_min, const ebo_solver_opts* opts, ebo_map_track_result* results, double* trace_or_null);
int ebo_map_track(ebo_ctx* ctx, const ebo_camera* cam, int w, int h, int n_images, const double* images, int n_points,
				  const double* points, int n_units, const int* unit_image, double* poses, double z_min,
				  const ebo_solver_opts* opts, ebo_map_track_result* results, double* trace_or_null);
int ebo_map_track_device(ebo_ctx* ctx, const ebo_camera* cam, int w, int h, int n_images, const double* d_images, int n_points,
						 const double* d_points, int n_units, const int* d_unit_image, double* d_poses, double z_min,
						 const ebo_solver_opts* opts, ebo_map_track_result* d_results, double* d_trace_or_null);
int ebo_event_images(ebo_ctx* ctx, const ebo_camera* cam, const ebo_rotation_params* params_or_null, const double* omegas_or_null,
					 double* images);
int ebo_event_images_device(ebo_ctx* ctx, const ebo_camera* cam, const ebo_rotation_params* params_or_null,
							const double* d_omegas_or_null, double* d_images);

/* Device-side timing of everything enqueued between begin and end on the
 * context's stream (hipEvent based). */
int ebo_timer_begin(ebo_ctx* ctx);
int ebo_timer_end(ebo_ctx* ctx, float* ms);

#ifdef __cplusplus
}
#endif
#endif /* EBO_H */
