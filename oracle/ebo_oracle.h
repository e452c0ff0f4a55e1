/*
 * ebo_oracle.h — C API of the CPU ORACLE.
 *
 * THIS IS TEST INFRASTRUCTURE, NOT PRODUCT CODE.  Only tests/, __graft_entry__.smoke()
 * and bench.py's cpu_baseline leg may load this library.  The product (libebo_hip.so)
 * never links, loads or calls anything in oracle/.
 *
 * What it is: a plain single-threaded C++ restatement of the reference's
 * motion-compensation hot path (reference = nurlanov-zh/event-based-odomety,
 * paths below are relative to the reference checkout):
 *   implementation/feature_tracker/include/feature_tracker/contrast_functor.h
 *   implementation/feature_tracker/include/feature_tracker/total_variance.h
 *   implementation/feature_tracker/src/feature_detector.cpp:243-482
 *   implementation/feature_tracker/src/patch.cpp:65-130
 *   tools/dataset_reader/src/davis240c_reader.cpp:60-92
 *   implementation/feature_tracker/include/feature_tracker/optimizer_cost.h,
 *   implementation/feature_tracker/src/optimizer.cpp:62-119 (optimizer_oracle.cpp)
 * Every function cites the lines it follows in oracle.cpp / optimizer_oracle.cpp.
 *
 * PARITY PINNING STATUS
 *   - The reference cannot be built in this image: it needs Ceres, Eigen 3.3.7, OpenCV,
 *     Sophus and spdlog, none of which are installed, and thirdparty/ is empty.  No
 *     stand-in headers were written to force a build.
 *   - Pinned by the reference's own tests: Patch::integrateEvents known-answer
 *     (implementation/feature_tracker/test/patch_test.cpp:35-60), event->patch
 *     membership (feature_detector_test.cpp:43-97), DAVIS event text fixture
 *     (tools/dataset_reader/test/davis240c_reader_test.cpp:19-48 + test_data/events.txt).
 *   - contrastFunctor value/Jacobian: cross-checked against the digits recorded in
 *     SURVEY.md §8(c) (tests/golden/survey_probe_contrast.json); the reference's own
 *     tests do not exercise it.
 *   - Solver (Ceres trust-region LM).  Ceres is a third-party dependency
 *     (thirdparty/ceres-solver, >=2.0,<2.2, commit unknown) that is absent here; oracle.cpp
 *     restates its published Levenberg-Marquardt trust-region algorithm (docs "Solving
 *     Non-linear Least Squares", TrustRegionMinimizer / LevenbergMarquardtStrategy /
 *     TrustRegionStepEvaluator, v2.0 defaults).  Pinned by the iteration table Ceres' own
 *     tutorial publishes for Powell's function (orc_lm_powell, every printed digit of all 14
 *     iterations; tests/golden/ceres_tutorial_powell.json).  Unpinned: non-monotonic steps,
 *     loss corrector, local parameterisation, last bits.
 *   - Tracker objective (optimizer_oracle.cpp): PARITY UNPINNED.  Ceres' bicubic interpolator
 *     and Sophus' SE2 are restated from their published algorithms; no reference test
 *     exercises Optimizer / OptimizerCostFunctor.
 */
#ifndef EBO_ORACLE_H
#define EBO_ORACLE_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Mirror of common::EventSample (common/include/common/data_types.h:12-38):
 * {Point2i{x,y}; EventPolarity sign(-1/+1); microseconds timestamp}. 24 bytes. */
typedef struct orc_event
{
	int32_t x;
	int32_t y;
	int32_t sign;
	int32_t reserved;
	int64_t t_us;
} orc_event;

/* contrastFunctor's hard-coded members (contrast_functor.h:282-291). */
typedef struct orc_functor_consts
{
	double max_possible_residual; /* 1e3 */
	double sigma_compensate;      /* 1   */
	int32_t kernel_compensate;    /* 3   */
	int32_t kernel_st;            /* 3   */
	double sigma_st;              /* 1.5 */
	int32_t kernel_nms;           /* 2   */
	int32_t reserved;
} orc_functor_consts;

/* DetectorParams fields on the hot path (feature_detector.h:17,21-30). */
typedef struct orc_params
{
	int32_t image_w, image_h;               /* imageSize {240,180}            */
	int32_t patch_w, patch_h;               /* patchCompensateSize {20,20}    */
	double tv_weight;                       /* compensateTVweight 1e3         */
	double tv_huber;                        /* compensateTVHuberLoss 10       */
	double scale;                           /* compensateScale 1e-3           */
	uint32_t min_events;                    /* compensateMinNumEvents 100     */
	int32_t loss;                           /* 0 = edge (reference), 1 = variance */
	orc_functor_consts k;
} orc_params;

/* ceres::Solver::Options as set at feature_detector.cpp:401-410; the rest are
 * Ceres 2.0 defaults. */
typedef struct orc_solver_opts
{
	int32_t max_num_iterations;   /* 50    */
	int32_t use_nonmonotonic;     /* 1     */
	double function_tolerance;    /* 1e-12 */
	double gradient_tolerance;    /* 1e-12 */
	double parameter_tolerance;   /* 1e-12 */
	double initial_radius;        /* 1e4   */
	double max_radius;            /* 1e16  */
	double min_radius;            /* 1e-32 */
	double min_relative_decrease; /* 1e-3  */
	double min_lm_diagonal;       /* 1e-6  */
	double max_lm_diagonal;       /* 1e32  */
	int32_t max_consecutive_nonmonotonic; /* 5 */
	int32_t max_consecutive_invalid;      /* 5 */
	int32_t jacobi_scaling;       /* 1 */
	int32_t mode;                 /* 0 = one global problem (reference), 1 = one problem per patch */
} orc_solver_opts;

typedef struct orc_summary
{
	int32_t iterations;        /* LM iterations run (global) or max over patches */
	int32_t num_evals_cost;    /* residual-only evaluations of data blocks     */
	int32_t num_evals_jac;     /* residual+Jacobian evaluations of data blocks */
	int32_t termination;       /* 0 conv, 1 no-conv (max iters), 2 failure     */
	double initial_cost;
	double final_cost;
} orc_summary;

void orc_default_consts(orc_functor_consts* k);
void orc_default_params(orc_params* p);
void orc_default_solver(orc_solver_opts* o);

/* contrastFunctor::operator() on one patch (contrast_functor.h:12-36).
 * ev = the patch's events in list order (front = oldest).
 * jac may be NULL (value-only, i.e. the T=double instantiation). */
int orc_contrast_eval(const orc_event* ev, size_t n, int rx, int ry, int rw,
					  int rh, double scale, const orc_functor_consts* k,
					  int loss, const double* motion, double* residual,
					  double* jac);

/* The image built by contrastFunctor::compensateEvents (contrast_functor.h:38-88).
 * img: planar [c][3*rh][3*rw], c = 1 (value) or 3 (value, d/dm0, d/dm1). */
int orc_contrast_image(const orc_event* ev, size_t n, int rx, int ry, int rw,
					   int rh, double scale, const orc_functor_consts* k,
					   const double* motion, int channels, double* img);

/* contrastFunctor's reference time (contrast_functor.h:18-20). */
int64_t orc_mid_timestamp(int64_t front_us, int64_t back_us);

/* totalVarianceFunctor (total_variance.h:14-20): r[2], jx/jy 2x2 row-major (may be NULL). */
int orc_tv_eval(double weight, const double* x, const double* y, double* r,
				double* jx, double* jy);

/* Patch grid of compensateEventsContrast (feature_detector.cpp:301-346). */
int orc_grid(const orc_params* p, int* npx, int* npy);
int orc_patch_rect(const orc_params* p, int px, int py, int* rx, int* ry,
				   int* rw, int* rh);

/* Batched objective over the whole window at given flows [P][2]:
 * bucketing feature_detector.cpp:348-367, one contrastFunctor per patch.
 * active[p] = 1 iff patch p has > min_events events. r[P], jac[P][2] (jac may be NULL). */
int orc_window_eval(const orc_event* ev, size_t n, const orc_params* p,
					const double* flows, double* r, double* jac,
					int32_t* active, int32_t* counts);

/* cpu_baseline timing: bucket once, then `reps` batched evaluations, steady clock. */
int orc_window_eval_timed(const orc_event* ev, size_t n, const orc_params* p,
						  const double* flows, int want_jac, int reps,
						  double* seconds, uint64_t* event_evals);

/* FeatureDetector::compensateEventsContrast (feature_detector.cpp:298-464):
 * flows [P][2] out, image [image_h][image_w] out (may be NULL). */
int orc_compensate_events_contrast(const orc_event* ev, size_t n,
								   const orc_params* p,
								   const orc_solver_opts* o, double* flows,
								   double* image, orc_summary* summary);

/* Only the final warped count image of compensateEventsContrast
 * (feature_detector.cpp:433-463) for given flows. */
int orc_final_count_image(const orc_event* ev, size_t n, const orc_params* p,
						  const double* flows, double* image);

/* FeatureDetector::integrateEvents (feature_detector.cpp:466-482). */
int orc_integrate_events(const orc_event* ev, size_t n, int w, int h,
						 double* image);

/* FeatureDetector::compensateEvents' warp loop (feature_detector.cpp:246-295)
 * with a given float32 motion field [h][w][2] (the at<Vec2f> view). */
int orc_compensate_events_field(const orc_event* ev, size_t n, int w, int h,
								double scale, const float* field,
								double* image);

/* FeatureDetector::initMotionField (feature_detector.cpp:53-142): velocities at the tracked
 * patches' positions from their trajectories (lower_bound by time), the rest filled with the
 * average or the nearest fixed point.  field float32 [h][w][2]; fixed_xy [n_patches][2]. */
int orc_init_motion_field(int w, int h, double scale, int use_average, int n_patches,
						  const size_t* traj_offsets, const double* traj_xy, const int64_t* traj_t,
						  int64_t timestamp, float* field, int32_t* n_fixed, int32_t* fixed_xy);

/* FeatureDetector::interpolateMotionField after its initMotionField call
 * (feature_detector.cpp:149-240): the per-pixel TV problem (weight 1; HuberLoss(1e-5) when
 * use_l1), fixed points constant, Ceres defaults when opts == NULL.  field is read as
 * initMotionField left it and overwritten.  -2: a fixed point at pixel (w-1, h-1), which is
 * no parameter block of the reference's problem (Ceres aborts there). */
int orc_interpolate_motion_field(int w, int h, int use_l1, float* field, int n_fixed,
								 const int32_t* fixed_xy, const orc_solver_opts* opts,
								 orc_summary* sum);

/* The trust-region LM restatement (oracle.cpp::minimize) run on Powell's singular function as
 * the Ceres tutorial sets it up, with a per-accepted-step log in the columns of Ceres' progress
 * table {cost, cost_change, |gradient|, |step|, tr_ratio, tr_radius}: checked against the table
 * that tutorial publishes (tests/golden/ceres_tutorial_powell.json).  x [4] in/out. */
int orc_lm_powell(const orc_solver_opts* opts, double* x, double* trace, int cap, int* n_rows,
				  orc_summary* sum);

/* ---- per-feature tracker objective (optimizer_oracle.cpp) ----------------
 * tracker::OptimizerCostFunctor::operator() (optimizer_cost.h:30-96) as
 * ceres::AutoDiffCostFunction<.., DYNAMIC, 4, 1>::Evaluate runs it: residuals [n], and when
 * jac_pose / jac_flow are given the Jet<double,5> derivatives jac_pose [n][4] (w.r.t. the
 * Sophus::SE2d storage [cos, sin, tx, ty]) and jac_flow [n]; both NULL = the double path
 * (whose quotient rounds differently from the Jet path, as in the reference).
 * grad: Optimizer::setGrad's grid, [img_h][img_w][2] = {gradX, gradY}; (rx, ry, rw, rh): the
 * patch cv::Rect2d, n = int(rw) * int(rh); nabla: normalizedIntegratedNabla [int(rh)][int(rw)]. */
int orc_optimizer_cost(const double* grad, int img_w, int img_h, double rx, double ry, double rw, double rh,
					   const double* nabla, const double* pose, double flow_dir, double* residuals,
					   double* jac_pose, double* jac_flow);
/* Ceres defaults with optimizer.cpp:103-112 applied (10 iterations, non-monotonic). */
void orc_optimizer_default_solver(orc_solver_opts* o);
/* The ceres::Solve of Optimizer::optimize (optimizer.cpp:83-119): SE2 block with
 * LocalParameterizationSE2 + scalar flow direction, one residual block with HuberLoss(huber_a),
 * DENSE_QR.  pose [4], flow_dir in/out (lowest-cost point visited). */
int orc_optimizer_solve(const double* grad, int img_w, int img_h, double rx, double ry, double rw, double rh,
						const double* nabla, double huber_a, const orc_solver_opts* opts, double* pose,
						double* flow_dir, orc_summary* summary);
/* LocalParameterizationSE2::Plus: out = pose * exp(delta3), delta3 = (ux, uy, theta). */
int orc_se2_plus(const double* pose, const double* delta3, double* out);
/* Patch::updatePatchRect (patch.cpp:49-63): rect [4] from warp [4] and the initial centre. */
int orc_patch_update_rect(const double* warp, double init_x, double init_y, double rw, double rh, double* rect);
/* The event-count estimate of FeatureDetector::updateNumOfEvents (feature_detector.cpp:689-707):
 * cv::warpAffine of the two gradient images with flags = cv::WARP_INVERSE_MAP alone, i.e.
 * INTER_NEAREST through OpenCV's 10-bit fixed-point coordinates, then the L1 norm of
 * 0.6 gradX cos(flow) + 0.6 gradY sin(flow) over the patch rect, truncated to size_t.  OpenCV is not
 * in the image: restated from its published algorithm (imgproc/imgwarp.cpp, cv::warpAffine /
 * WarpAffineInvoker), PARITY UNPINNED; exact by construction for identity and integer-translation
 * warps.  grad [img_h][img_w][2] = (gradX, gradY); warp [4] = Sophus::SE2d::data(). */
int orc_patch_warp_image(const double* grad, int img_w, int img_h, double rx, double ry, double rw, double rh,
						 const double* warp, double flow_dir, double* out, int* updated);
int orc_estimate_num_events(const double* grad, int img_w, int img_h, double rx, double ry, double rw, double rh,
							const double* warp, double flow_dir, uint64_t* out);
/* Patch::getNormalizedIntegratedNabla (patch.cpp:156-159). */
int orc_normalize_nabla(const double* nabla, int n, double* out);

/* Patch::integrateEvents (patch.cpp:65-85). ev in deque order (front = newest).
 * nabla [int(rh)][int(rw)].  This and orc_patch_integrate_mc return -1 for an rw or rh that is
 * not finite, not whole or below 1 (the image could not hold every event the rect contains). */
int orc_patch_integrate(const orc_event* ev, size_t n, double rx, double ry,
						double rw, double rh, double* nabla,
						int64_t* current_ts, int64_t* time_last_update);

/* Patch::integrateMotionCompensatedEvents (patch.cpp:87-130).
 * traj: last two trajectory samples {x,y,t_us} (prelast, last). Returns 1 in
 * *updated if the image was rebuilt. */
/* FeatureDetector::updatePatches' event -> patch routing (feature_detector.cpp:585-596). */
int orc_route_events(const orc_event* ev, size_t n, int n_patches, const double* rects,
					 const uint32_t* start, const uint32_t* max_take, uint32_t cap, uint32_t* out_index,
					 uint32_t* out_count, uint32_t* out_next);
int orc_patch_integrate_mc(const orc_event* ev, size_t n, double rx, double ry,
						   double rw, double rh, const double* prelast_xy,
						   int64_t prelast_t, const double* last_xy,
						   int64_t last_t, int64_t mid_time, double* nabla,
						   int32_t* updated);

/* Davis240cReader::getEventSample over a whole events.txt
 * (davis240c_reader.cpp:60-92). Returns number parsed in *n (<= cap). */
int orc_parse_events_txt(const char* path, orc_event* out, size_t cap,
						 size_t* n);

#ifdef __cplusplus
}
#endif
#endif
