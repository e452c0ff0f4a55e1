"""event-based-odomety_amd — MI355X (gfx950) implementation of the motion-compensated
event-warping path of nurlanov-zh/event-based-odomety.

The product is the C-ABI library ``libebo_hip.so`` (include/ebo.h) plus the C++
façade in ``include/feature_tracker``.  This module is only the ctypes plumbing the
Python tests and bench.py use to call that ABI; it contains no compute and no CPU
fallback.  Importing it never needs a GPU; creating a Context does.

The directory name has a hyphen (the upstream repository name), so import it with
``importlib.import_module("event-based-odomety_amd")``.
"""
import ctypes as C
import os
import subprocess

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
# EBO_LIB_PATH: another build of the same library (tools/ A/B runs of two builds on one box only)
LIB_PATH = os.environ.get("EBO_LIB_PATH") or os.path.join(HERE, "libebo_hip.so")
# The A/B build (make ab: -DEBO_AB, the environment switches of csrc/ab_env.h).  A module
# instance imported under the name `..._ab` (tests' `ebo_ab` fixture, tools/ab/*) binds it; the product never does.
AB_LIB_PATH = os.path.join(HERE, "libebo_hip_ab.so")
if __name__.endswith("_ab"):
    LIB_PATH = AB_LIB_PATH
HEADER_PATH = os.path.join(ROOT, "include", "ebo.h")

OK = 0
ERR_ARG, ERR_HIP, ERR_RANGE, ERR_STATE, ERR_UNSUPPORTED, ERR_NO_DEVICE, ERR_SOLVER, ERR_COMM = (
    -1, -2, -3, -4, -5, -6, -7, -8)
LOSS_EDGE, LOSS_VARIANCE = 0, 1
GRAD_JET, GRAD_CENTRAL = 0, 1
SOLVE_GLOBAL, SOLVE_INDEPENDENT = 0, 1
COUNT_INTEGRATED, COUNT_WARPED, COUNT_FIELD = 0, 1, 2

# numpy mirror of ebo_event (== common::EventSample, 24 bytes)
EVENT_DTYPE = np.dtype(
    [("x", "<i4"), ("y", "<i4"), ("sign", "<i4"), ("reserved", "<i4"), ("t_us", "<i8")]
)

# numpy mirror of ebo_event8 (compact raw event: x:15 | polarity:1 | y:15 | 0:1, int32 us relative to a base time)
EVENT8_DTYPE = np.dtype([("xy", "<u4"), ("t_rel_us", "<i4")])

# numpy mirror of ebo_track_point (one "feature_id timestamp x y" record, 32 bytes)
TRACK_DTYPE = np.dtype([("id", "<i8"), ("t_us", "<i8"), ("x", "<f8"), ("y", "<f8")])


class FunctorConsts(C.Structure):
    _fields_ = [
        ("max_possible_residual", C.c_double),
        ("sigma_compensate", C.c_double),
        ("kernel_compensate", C.c_int32),
        ("kernel_st", C.c_int32),
        ("sigma_st", C.c_double),
        ("kernel_nms", C.c_int32),
        ("reserved", C.c_int32),
    ]


class Params(C.Structure):
    _fields_ = [
        ("device", C.c_int32),
        ("image_w", C.c_int32),
        ("image_h", C.c_int32),
        ("patch_w", C.c_int32),
        ("patch_h", C.c_int32),
        ("tv_weight", C.c_double),
        ("tv_huber", C.c_double),
        ("scale", C.c_double),
        ("min_events", C.c_uint32),
        ("loss", C.c_int32),
        ("grad", C.c_int32),
        ("reserved", C.c_int32),
        ("fd_step", C.c_double),
        ("k", FunctorConsts),
        ("max_events", C.c_uint64),
        ("max_windows", C.c_int32),
        ("reserved2", C.c_int32),
    ]


class SolverOpts(C.Structure):
    _fields_ = [
        ("max_num_iterations", C.c_int32),
        ("use_nonmonotonic", C.c_int32),
        ("function_tolerance", C.c_double),
        ("gradient_tolerance", C.c_double),
        ("parameter_tolerance", C.c_double),
        ("initial_radius", C.c_double),
        ("max_radius", C.c_double),
        ("min_radius", C.c_double),
        ("min_relative_decrease", C.c_double),
        ("min_lm_diagonal", C.c_double),
        ("max_lm_diagonal", C.c_double),
        ("max_consecutive_nonmonotonic", C.c_int32),
        ("max_consecutive_invalid", C.c_int32),
        ("jacobi_scaling", C.c_int32),
        ("mode", C.c_int32),
    ]


class Summary(C.Structure):
    _fields_ = [
        ("iterations", C.c_int32),
        ("num_evals_cost", C.c_int32),
        ("num_evals_jac", C.c_int32),
        ("termination", C.c_int32),
        ("initial_cost", C.c_double),
        ("final_cost", C.c_double),
    ]


class AlignResult(C.Structure):
    """ebo_align_result: one segment's alignment and the reference's ErrorMetricValue fields."""
    _fields_ = [("scale", C.c_double), ("R", C.c_double * 9), ("t", C.c_double * 3), ("rmse", C.c_double),
                ("mean", C.c_double), ("min", C.c_double), ("max", C.c_double), ("count", C.c_int32), ("status", C.c_int32)]


class LandmarkParams(C.Structure):
    """ebo_landmark_params."""
    _fields_ = [("threshold", C.c_double), ("min_parallax", C.c_double), ("min_inliers", C.c_int32), ("max_hypotheses", C.c_int32),
                ("seed", C.c_uint64)]


class LandmarkResult(C.Structure):
    """ebo_landmark_result: one landmark's point, parallax, largest finite score and L6 status."""
    _fields_ = [("point", C.c_double * 3), ("parallax", C.c_double), ("score_max", C.c_double), ("status", C.c_int32),
                ("n_obs", C.c_int32), ("n_inliers", C.c_int32), ("winner", C.c_int32), ("hypotheses", C.c_int32), ("reserved", C.c_int32)]


class RotationParams(C.Structure):
    """ebo_rotation_params: sigma_blur of the rotational contrast maximisation (rule V5)."""
    _fields_ = [("sigma_blur", C.c_double), ("reserved", C.c_double)]

    def __init__(self, sigma_blur=1.0):
        super().__init__(float(sigma_blur), 0.0)


class DepthParams(C.Structure):
    """ebo_depth_params: the planes (rule M1), the threshold's box radius and excess (M6), the median radius (M7)."""
    _fields_ = [("nz", C.c_int32), ("box_radius", C.c_int32), ("median_radius", C.c_int32), ("reserved", C.c_int32),
                ("z_near", C.c_double), ("z_far", C.c_double), ("min_excess", C.c_double)]


def default_depth_params(**kw):
    """ebo_default_depth_params (nz 64, z_near 0.5, z_far 8, box_radius 2, min_excess 3, median_radius 2), with overrides."""
    o = DepthParams()
    lib().ebo_default_depth_params(C.byref(o))
    for key, val in kw.items():
        if not hasattr(o, key):
            raise AttributeError(key)
        setattr(o, key, val)
    return o


class RotSolverOpts(C.Structure):
    """ebo_rot_solver_opts (rules N1-N5)."""
    _fields_ = [("first_rate", C.c_double), ("c1", C.c_double), ("step_tol", C.c_double), ("max_backtracks", C.c_int32),
                ("max_iterations", C.c_int32)]


class RotSummary(C.Structure):
    """ebo_rot_summary: status (ROT_*), accepted steps, evaluations, r at omega0 and at the result."""
    _fields_ = [("status", C.c_int32), ("iterations", C.c_int32), ("evaluations", C.c_int32), ("reserved", C.c_int32),
                ("r_initial", C.c_double), ("r_final", C.c_double)]


ROT_RUNNING, ROT_CONVERGED_STEP, ROT_CONVERGED_GRADIENT, ROT_MAX_ITERATIONS, ROT_NO_PROGRESS, ROT_NONFINITE = -1, 0, 1, 2, 3, 4


def rot_solver_opts(**kw):
    """ebo_default_rot_solver_opts (0.5 rad/s, c1 1e-4, step_tol 1e-4, 20 backtracks, 100 iterations), with overrides."""
    o = RotSolverOpts()
    lib().ebo_default_rot_solver_opts(C.byref(o))
    for key, val in kw.items():
        if not hasattr(o, key):
            raise AttributeError(key)
        setattr(o, key, val)
    return o


class RpeResult(C.Structure):
    """ebo_rpe_result: one (segment, delta) unit's relative pose error, translation then rotation."""
    _fields_ = [("trans_rmse", C.c_double), ("trans_mean", C.c_double), ("trans_min", C.c_double), ("trans_max", C.c_double),
                ("rot_rmse", C.c_double), ("rot_mean", C.c_double), ("rot_min", C.c_double), ("rot_max", C.c_double),
                ("count", C.c_int32), ("status", C.c_int32)]


class TrackErrorResult(C.Structure):
    """ebo_track_error_result: one (track, tau) unit's error statistics over its inliers, its age and where it was cut."""
    _fields_ = [("err_mean", C.c_double), ("err_rmse", C.c_double), ("err_max", C.c_double), ("age_us", C.c_int64),
                ("t_first_us", C.c_int64), ("n_inliers", C.c_int32), ("n_comparable", C.c_int32), ("first", C.c_int32),
                ("cut", C.c_int32), ("status", C.c_int32), ("pad", C.c_int32)]


class TrackErrorSummary(C.Structure):
    """ebo_track_error_summary_result."""
    _fields_ = [("mean_error", C.c_double), ("mean_age_s", C.c_double), ("counted", C.c_int32), ("discarded", C.c_int32),
                ("outlived", C.c_int32), ("pad", C.c_int32)]


class LkParams(C.Structure):
    """ebo_lk_params: ebo_lk_track's parameters as ebo_reference_tracks takes them."""
    _fields_ = [("win_w", C.c_int32), ("win_h", C.c_int32), ("max_level", C.c_int32), ("max_count", C.c_int32),
                ("epsilon", C.c_double), ("min_eig_threshold", C.c_double)]


TRACK_ERROR_FIELDS = ("err_mean", "err_rmse", "err_max")
TRACK_ERROR_INTS = ("age_us", "t_first_us", "n_inliers", "n_comparable", "first", "cut", "status")


def _pack_tracks(tracks):
    """[(t_us, xy), ..] -> (offsets int32 [n + 1], t int64, xy float64 [.][2])."""
    ts = [np.asarray(t, dtype=np.int64).reshape(-1) for t, _ in tracks]
    xs = [np.asarray(xy, dtype=np.float64).reshape(-1, 2) for _, xy in tracks]
    if any(len(t) != len(x) for t, x in zip(ts, xs)):
        raise ValueError("a track's times and positions must have the same length")
    off = np.zeros(len(tracks) + 1, dtype=np.int32)
    off[1:] = np.cumsum([len(t) for t in ts])
    t = np.ascontiguousarray(np.concatenate(ts) if ts else np.zeros(0, np.int64))
    xy = np.ascontiguousarray(np.concatenate(xs) if xs else np.zeros((0, 2)))
    return off, t, xy


def track_seeds(tracks, frame_t_us):
    """ebo_track_seeds: tracks a list of (t_us int64 [n], xy float64 [n][2]); frame_t_us strictly increasing.  ->
    (seed_frame int32 [n_tracks], -1 where no frame lies within the track's life; seed_xy float32 [n_tracks][2], the
    track's own position at that frame's time)."""
    off, t, xy = _pack_tracks(tracks)
    ft = np.ascontiguousarray(frame_t_us, dtype=np.int64).reshape(-1)
    n = len(tracks)
    sf = np.zeros(max(n, 1), dtype=np.int32)
    sx = np.zeros((max(n, 1), 2), dtype=np.float32)
    rc = lib().ebo_track_seeds(n, _vp(off), _vp(t) if len(t) else None, _vp(xy) if len(t) else None, len(ft),
                               _vp(ft) if len(ft) else None, _vp(sf), _vp(sx))
    if rc:
        raise EboError(rc, "ebo_track_seeds: offsets, track times or frame times out of order")
    return sf[:n], sx[:n]


def track_error_summary(results):
    """ebo_track_error_summary over the results of ONE tau (dicts as Context.track_errors returns them, in track
    order): -> dict(mean_error, mean_age_s, counted, discarded, outlived)."""
    n = len(results)
    res = (TrackErrorResult * max(n, 1))()
    for r, d in zip(res, results):
        for f in TRACK_ERROR_FIELDS + TRACK_ERROR_INTS:
            setattr(r, f, d[f])
    out = TrackErrorSummary()
    rc = lib().ebo_track_error_summary(n, C.addressof(res), 1, C.addressof(out))
    if rc:
        raise EboError(rc, "ebo_track_error_summary")
    return dict(mean_error=np.float64(out.mean_error), mean_age_s=np.float64(out.mean_age_s), counted=int(out.counted),
                discarded=int(out.discarded), outlived=int(out.outlived))


def default_ba_opts(**over):
    """ebo_default_ba_opts (Ceres' Solver::Options defaults) as a SolverOpts; keyword arguments override fields."""
    o = SolverOpts()
    lib().ebo_default_ba_opts(C.addressof(o))
    for k, v in over.items():
        setattr(o, k, v)
    return o


class MapTrackResult(C.Structure):
    """ebo_map_track_result: one unit's answer (rules E1-E9)."""
    _fields_ = [("termination", C.c_int32), ("iterations", C.c_int32), ("num_evals_jac", C.c_int32), ("num_evals_cost", C.c_int32),
                ("visible_start", C.c_int32), ("visible_final", C.c_int32), ("reserved0", C.c_int32), ("reserved1", C.c_int32),
                ("initial_cost", C.c_double), ("final_cost", C.c_double), ("scale", C.c_double), ("reserved2", C.c_double)]


MAP_TRACK_FIELDS = ("termination", "iterations", "num_evals_jac", "num_evals_cost", "visible_start", "visible_final", "initial_cost",
                    "final_cost", "scale")
MAP_TRACK_DTYPE = np.dtype([(f, "<i4") for f in ("termination", "iterations", "num_evals_jac", "num_evals_cost", "visible_start",
                                                  "visible_final", "reserved0", "reserved1")] +
                           [(f, "<f8") for f in ("initial_cost", "final_cost", "scale", "reserved2")])


def default_map_track_opts(**over):
    """ebo_default_map_track_opts as a SolverOpts; keyword arguments override fields."""
    o = SolverOpts()
    lib().ebo_default_map_track_opts(C.addressof(o))
    for k, v in over.items():
        if not hasattr(o, k):
            raise AttributeError(k)
        setattr(o, k, v)
    return o


def map_track_starts(pose, translation_step, rotation_step):
    """ebo_map_track_starts: pose [12] -> the 13 starts [13][12] of a multi-start (the pose, then +- a step along each of
    B4's six update directions)."""
    p = np.ascontiguousarray(pose, dtype=np.float64).reshape(12)
    out = np.zeros((13, 12))
    lib().ebo_map_track_starts(_dp(p), C.c_double(translation_step), C.c_double(rotation_step), _dp(out))
    return out


class Camera(C.Structure):
    """ebo_camera: common::CameraModelParams<double>, in its field order."""
    _fields_ = [(k, C.c_double) for k in ("fx", "fy", "cx", "cy", "k1", "k2", "k3", "p1", "p2")]


def camera(v):
    """A Camera from a Camera, a mapping of field names or nine numbers in the struct's order."""
    if isinstance(v, Camera):
        return v
    if isinstance(v, dict):
        return Camera(**{k: float(x) for k, x in v.items()})
    return Camera(*[float(x) for x in v])


class TwoViewParams(C.Structure):
    """ebo_two_view_params: threshold, probability, max_iterations, seed of ebo_relative_pose_ransac."""
    _fields_ = [("threshold", C.c_double), ("probability", C.c_double), ("max_iterations", C.c_int),
                ("reserved", C.c_int), ("seed", C.c_uint64)]


class TwoViewResult(C.Structure):
    """ebo_two_view_result: one keyframe pair's RANSAC answer."""
    _fields_ = [("found", C.c_int), ("winner", C.c_int), ("iterations", C.c_int), ("n_inliers", C.c_int),
                ("inlier_offset", C.c_int), ("reserved", C.c_int), ("model", C.c_double * 12)]


def two_view_params(**kw):
    """The defaults of ebo_default_two_view_params (5e-5, 0.99, 1000 hypotheses, seed 0), with overrides."""
    p = TwoViewParams()
    lib().ebo_default_two_view_params(C.byref(p))
    for key, val in kw.items():
        if not hasattr(p, key):
            raise AttributeError(key)
        setattr(p, key, val)
    return p


class EboError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("ebo error %d: %s" % (code, msg))
        self.code = code


_lib = None


def build(verbose=False):
    """Compile libebo_hip.so for gfx950 in-tree (hipcc cross-compiles without a GPU)."""
    cmd = ["make", "-C", os.path.join(HERE, "csrc")]
    if not verbose:
        cmd.insert(1, "-s")
    subprocess.check_call(cmd)


def lib():
    """The loaded library.  Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise ImportError(
                "%s is missing: run __graft_entry__.build() (hipcc). "
                "This package has no CPU path." % LIB_PATH)
        _lib = C.CDLL(LIB_PATH)
        _lib.ebo_version.restype = C.c_char_p
        _lib.ebo_last_error.restype = C.c_char_p
        _lib.ebo_last_error.argtypes = [C.c_void_p]
        _lib.ebo_destroy.restype = None
        _lib.ebo_destroy.argtypes = [C.c_void_p]
        _lib.ebo_graph_destroy.restype = None
        _lib.ebo_graph_destroy.argtypes = [C.c_void_p]
        _lib.ebo_graph_begin.argtypes = [C.c_void_p]
        _lib.ebo_graph_end.argtypes = [C.c_void_p, C.c_void_p]
        _lib.ebo_graph_launch.argtypes = [C.c_void_p, C.c_void_p, C.c_int]
        _lib.ebo_lm_destroy.restype = None
        _lib.ebo_lm_destroy.argtypes = [C.c_void_p]
        _lib.ebo_lm_request.argtypes = [C.c_void_p, C.c_void_p]
        _lib.ebo_lm_supply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ebo_lm_result.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ebo_default_two_view_params.restype = None
        _lib.ebo_two_view_timing.argtypes = [C.c_void_p, C.c_int, C.c_void_p]
        _tv = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p,
               C.c_void_p, C.c_void_p]
        _lib.ebo_relative_pose_ransac.argtypes = _tv
        _lib.ebo_relative_pose_ransac_device.argtypes = _tv
        _sc = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p, C.c_void_p]
        _lib.ebo_relative_pose_scores.argtypes = _sc
        _lib.ebo_relative_pose_scores_device.argtypes = _sc
        _lib.ebo_absolute_pose_ransac.argtypes = _tv
        _lib.ebo_absolute_pose_ransac_device.argtypes = _tv
        _ba = [C.c_void_p, C.c_int] + [C.c_void_p] * 10 + [C.c_double, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ebo_bundle_adjust.argtypes = _ba
        _lib.ebo_bundle_adjust_device.argtypes = _ba
        _lib.ebo_default_ba_opts.argtypes = [C.c_void_p]
        _lib.ebo_default_ba_opts.restype = None
        _rr = [C.c_void_p, C.c_int] + [C.c_void_p] * 9
        _lib.ebo_relative_pose_refine.argtypes = _rr
        _lib.ebo_relative_pose_refine_device.argtypes = _rr
        _al = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p]
        _lib.ebo_align_sim3.argtypes = _al
        _lib.ebo_align_sim3_device.argtypes = _al
        _rpe = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p]
        _lib.ebo_trajectory_rpe.argtypes = _rpe
        _lib.ebo_trajectory_rpe_device.argtypes = _rpe
        _lmt = [C.c_void_p, C.c_int, C.c_void_p, C.c_int] + [C.c_void_p] * 7
        _lib.ebo_default_landmark_params.argtypes = [C.c_void_p]
        _lib.ebo_default_landmark_params.restype = None
        _lib.ebo_triangulate_tracks.argtypes = _lmt
        _lib.ebo_triangulate_tracks_device.argtypes = _lmt
        _lib.ebo_landmark_scores.argtypes = _lmt + [C.c_void_p]
        _lib.ebo_landmark_scores_device.argtypes = _lmt + [C.c_void_p]
        _lib.ebo_default_depth_params.argtypes = [C.c_void_p]
        _lib.ebo_default_depth_params.restype = None
        _lib.ebo_dsi_begin.argtypes = [C.c_void_p] * 4
        _lib.ebo_dsi_add_windows.argtypes = [C.c_void_p] * 3
        _lib.ebo_dsi_volume.argtypes = [C.c_void_p] * 2
        _lib.ebo_dsi_depth.argtypes = [C.c_void_p] * 5 + [C.c_int, C.c_void_p]
        _lib.ebo_dsi_end.argtypes = [C.c_void_p]
        _lib.ebo_default_rotation_params.argtypes = [C.c_void_p]
        _lib.ebo_default_rotation_params.restype = None
        _lib.ebo_default_rot_solver_opts.argtypes = [C.c_void_p]
        _lib.ebo_default_rot_solver_opts.restype = None
        _lib.ebo_eval_rotation.argtypes = [C.c_void_p] * 6
        _lib.ebo_eval_rotation_device.argtypes = [C.c_void_p] * 6
        _lib.ebo_rotation_image.argtypes = [C.c_void_p] * 5
        _lib.ebo_solve_rotation.argtypes = [C.c_void_p] * 7
        _lib.ebo_event_images.argtypes = [C.c_void_p] * 5
        _lib.ebo_event_images_device.argtypes = [C.c_void_p] * 5
        _lib.ebo_default_map_track_opts.argtypes = [C.c_void_p]
        _lib.ebo_default_map_track_opts.restype = None
        _mt = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
               C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ebo_map_track.argtypes = _mt
        _lib.ebo_map_track_device.argtypes = _mt
        _lib.ebo_map_track_starts.argtypes = [C.c_void_p, C.c_double, C.c_double, C.c_void_p]
        _lib.ebo_map_track_starts.restype = None
        _lib.ebo_map_track_resident.argtypes = [C.c_void_p] * 4 + [C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p,
                                                C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ebo_rot_solver_create.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ebo_rot_solver_request.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ebo_rot_solver_supply.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ebo_rot_solver_result.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ebo_rot_solver_destroy.argtypes = [C.c_void_p]
        _lib.ebo_rot_solver_destroy.restype = None
        _te = [C.c_void_p, C.c_int] + [C.c_void_p] * 6 + [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ebo_track_errors.argtypes = _te
        _lib.ebo_track_errors_device.argtypes = _te
        _lib.ebo_track_seeds.argtypes = [C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ebo_reference_tracks.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_int] + [C.c_void_p] * 6
        _lib.ebo_track_error_summary.argtypes = [C.c_int, C.c_void_p, C.c_int, C.c_void_p]
        _lib.ebo_default_lk_params.argtypes = [C.c_void_p]
        _lib.ebo_default_lk_params.restype = None
        _lib.ebo_absolute_pose_scores.argtypes = _sc
        _lib.ebo_absolute_pose_scores_device.argtypes = _sc
        _tr = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
        _lib.ebo_triangulate.argtypes = _tr
        _lib.ebo_triangulate_device.argtypes = _tr
        _lib.ebo_epipolar_inliers.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_double, C.c_void_p]
    return _lib


def version():
    return lib().ebo_version().decode()


def device_count():
    n = C.c_int()
    lib().ebo_device_count(C.byref(n))
    return n.value


def default_params(**kw):
    p = Params()
    lib().ebo_default_params(C.byref(p))
    for key, val in kw.items():
        if not hasattr(p, key):
            raise AttributeError(key)
        setattr(p, key, val)
    return p


def default_solver(**kw):
    o = SolverOpts()
    lib().ebo_default_solver(C.byref(o))
    for key, val in kw.items():
        if not hasattr(o, key):
            raise AttributeError(key)
        setattr(o, key, val)
    return o


def optimizer_default_solver(**kw):
    """ceres::Solver::Options as Optimizer::optimize sets them (optimizer.cpp:103-112)."""
    o = SolverOpts()
    lib().ebo_optimizer_default_solver(C.byref(o))
    for key, val in kw.items():
        if not hasattr(o, key):
            raise AttributeError(key)
        setattr(o, key, val)
    return o


class HostSolver:
    """ebo_lm_*: the host LM of EBO_SOLVE_GLOBAL as a resumable state machine (request -> evaluate -> supply)."""

    DONE, NEED_JACOBIAN, NEED_VALUE = 0, 1, 2

    def __init__(self, npx, npy, active, tv_weight=1e3, tv_huber=10.0, opts=None):
        self.P = int(npx) * int(npy)
        active = np.ascontiguousarray(active, dtype=np.uint8).reshape(self.P)
        self._opts = opts if opts is not None else default_solver()
        h = C.c_void_p()
        rc = lib().ebo_lm_create(int(npx), int(npy), _vp(active), C.c_double(tv_weight), C.c_double(tv_huber),
                                 C.byref(self._opts), C.byref(h))
        if rc:
            raise EboError(rc, "ebo_lm_create")
        self._h = h

    def request(self):
        flows = np.zeros((self.P, 2))
        rc = lib().ebo_lm_request(self._h, _dp(flows))
        if rc < 0:
            raise EboError(rc, "ebo_lm_request")
        return rc, flows

    def supply(self, r, jac=None):
        r = np.ascontiguousarray(r, dtype=np.float64).reshape(self.P)
        j = None if jac is None else np.ascontiguousarray(jac, dtype=np.float64).reshape(self.P, 2)
        rc = lib().ebo_lm_supply(self._h, _dp(r), _dp(j) if j is not None else None)
        if rc:
            raise EboError(rc, "ebo_lm_supply")

    def result(self):
        flows = np.zeros((self.P, 2))
        s = Summary()
        rc = lib().ebo_lm_result(self._h, _dp(flows), C.byref(s))
        if rc:
            raise EboError(rc, "ebo_lm_result")
        return flows, s

    def close(self):
        if self._h:
            lib().ebo_lm_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class RotationSolver:
    """ebo_rot_solver_*: rules N1-N5 for n windows at once as a resumable state machine (request -> evaluate -> supply).
    Host only: no device is touched."""

    def __init__(self, n, opts=None, omega0=None):
        self.n = int(n)
        self._opts = opts if opts is not None else rot_solver_opts()
        o0 = None if omega0 is None else np.ascontiguousarray(omega0, dtype=np.float64).reshape(self.n, 3)
        h = C.c_void_p()
        rc = lib().ebo_rot_solver_create(self.n, C.byref(self._opts), _dp(o0) if o0 is not None else None, C.byref(h))
        if rc:
            raise EboError(rc, "ebo_rot_solver_create")
        self._h = h

    def request(self):
        """-> (windows still waiting, omegas [n][3], live bool [n])"""
        om = np.zeros((self.n, 3))
        live = np.zeros(self.n, dtype=np.uint8)
        rc = lib().ebo_rot_solver_request(self._h, _dp(om), _vp(live))
        if rc < 0:
            raise EboError(rc, "ebo_rot_solver_request")
        return rc, om, live.astype(bool)

    def supply(self, r, g):
        r = np.ascontiguousarray(r, dtype=np.float64).reshape(self.n)
        g = np.ascontiguousarray(g, dtype=np.float64).reshape(self.n, 3)
        rc = lib().ebo_rot_solver_supply(self._h, _dp(r), _dp(g))
        if rc:
            raise EboError(rc, "ebo_rot_solver_supply")

    def result(self):
        om = np.zeros((self.n, 3))
        s = (RotSummary * self.n)()
        rc = lib().ebo_rot_solver_result(self._h, _dp(om), s)
        if rc:
            raise EboError(rc, "ebo_rot_solver_result")
        return om, list(s)

    def close(self):
        if self._h:
            lib().ebo_rot_solver_destroy(self._h)
            self._h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def window_ref_time(t_first_us, t_last_us):
    """The reference time of a window from its first / last event time (feature_detector.cpp:305-306)."""
    out = C.c_int64()
    rc = lib().ebo_window_ref_time(C.c_int64(int(t_first_us)), C.c_int64(int(t_last_us)), C.byref(out))
    if rc:
        raise EboError(rc, "window mid-time outside int32 microseconds")
    return out.value


def shard_range(n_units, rank, world):
    b, e = C.c_int(), C.c_int()
    rc = lib().ebo_shard_range(int(n_units), int(rank), int(world), C.byref(b), C.byref(e))
    if rc:
        raise EboError(rc, "bad shard arguments")
    return b.value, e.value


class Band(C.Structure):
    """ebo_band: one rank's share of the final image of row-sharded windows."""
    _fields_ = [("band_row0", C.c_int), ("own_row0", C.c_int), ("own_row1", C.c_int), ("band_row1", C.c_int),
                ("recv_above", C.c_int), ("recv_below", C.c_int)]

    top_rows = property(lambda s: s.own_row0 - s.band_row0)
    own_rows = property(lambda s: s.own_row1 - s.own_row0)
    bottom_rows = property(lambda s: s.band_row1 - s.own_row1)


def band_plan(image_h, row_bounds, rank, halo):
    rb = np.ascontiguousarray(row_bounds, dtype=np.int32)
    out = Band()
    rc = lib().ebo_band_plan(int(image_h), rb.ctypes.data_as(C.c_void_p), len(rb) - 1, int(rank), int(halo), C.byref(out))
    if rc:
        raise EboError(rc, "no band plan: bad row bounds, or a halo that does not fit inside a neighbour's rows")
    return out


def _dp(a):
    return a.ctypes.data_as(C.POINTER(C.c_double))


def _vp(a):
    return a.ctypes.data_as(C.c_void_p)


def comm_unique_id():
    """128-byte RCCL unique id (rank 0 creates it, the other ranks receive its bytes)."""
    buf = (C.c_char * 128)()
    rc = lib().ebo_comm_unique_id(C.byref(buf))
    if rc:
        raise EboError(rc, lib().ebo_last_error(None).decode())
    return bytes(buf)


def read_events_txt(path, cap=1 << 22):
    """DAVIS240C events.txt -> structured event array (host-side parser of the library)."""
    out = np.zeros(cap, dtype=EVENT_DTYPE)
    n = C.c_size_t()
    rc = lib().ebo_read_events_txt(str(path).encode(), _vp(out), C.c_size_t(cap), C.byref(n))
    if rc:
        raise EboError(rc, "cannot parse %s (parsed %d events before the error)" % (path, n.value))
    return out[: n.value].copy()


def cut_windows(ev, time_us=300000, count=15000, max_store=15000, last_compensation_us=0):
    """ebo_cut_windows: the reference's window rule (tools::Evaluator::eventCallback after
    FeatureDetector::addEvent) on a time-ordered stream -> (begin, end, last_compensation_us, pending_begin);
    window w is ev[begin[w]:end[w]]."""
    ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
    cap = len(ev)
    begin = np.zeros(max(cap, 1), dtype=np.uint64)
    end = np.zeros(max(cap, 1), dtype=np.uint64)
    nw, last, pending = C.c_size_t(), C.c_int64(), C.c_size_t()
    rc = lib().ebo_cut_windows(_vp(ev), C.c_size_t(len(ev)), C.c_int64(int(last_compensation_us)),
                               C.c_uint32(int(time_us)), C.c_uint32(int(count)), C.c_uint64(int(max_store)),
                               _vp(begin), _vp(end), C.c_size_t(cap), C.byref(nw), C.byref(last), C.byref(pending))
    if rc:
        raise EboError(rc, "cannot cut windows (max_store must be > 0)")
    return begin[: nw.value].copy(), end[: nw.value].copy(), last.value, pending.value


def read_events_txt_threads(path, cap, threads=0, offset=None, out=None):
    """ebo_read_events_txt_threads: at most cap events with `threads` host threads (0: EBO_HOST_THREADS or the
    machine's) -> (events, next offset or None, threads that parsed).  `out`: a caller-owned array to fill (timing)."""
    out = np.zeros(cap, dtype=EVENT_DTYPE) if out is None else out
    n, used = C.c_size_t(), C.c_int()
    off = C.c_uint64(int(offset)) if offset is not None else None
    f = lib().ebo_read_events_txt_threads
    f.restype = C.c_int
    rc = f(str(path).encode(), C.byref(off) if off is not None else None, _vp(out), C.c_size_t(cap), C.byref(n),
           C.c_int(int(threads)), C.byref(used))
    if rc:
        raise EboError(rc, "cannot parse %s (parsed %d events before the error)" % (path, n.value))
    return out[: n.value], (int(off.value) if off is not None else None), int(used.value)


def read_events_txt8(path, cap, threads=0, offset=None):
    """ebo_read_events_txt8: at most cap events as compact 8-byte records -> (records, base time in us, next offset or
    None); every record's t_rel_us is relative to the base = the first event's time stamp of this call."""
    out = np.zeros(cap, dtype=EVENT8_DTYPE)
    n, base = C.c_size_t(), C.c_int64()
    off = C.c_uint64(int(offset)) if offset is not None else None
    f = lib().ebo_read_events_txt8
    f.restype = C.c_int
    rc = f(str(path).encode(), C.byref(off) if off is not None else None, _vp(out), C.c_size_t(cap), C.byref(n), C.byref(base),
           C.c_int(int(threads)))
    if rc:
        raise EboError(rc, "cannot parse %s into compact records (%d events before the error)" % (path, n.value))
    return out[: n.value], int(base.value), (int(off.value) if off is not None else None)


def read_events_txt_at(path, offset, cap=1_000_000):
    """At most cap events of an events.txt from byte `offset` on -> (events, next offset): the pieces
    Davis240cReader::getEvents reads a recording in (EVENT_LENGTH lines per call)."""
    out = np.zeros(cap, dtype=EVENT_DTYPE)
    n = C.c_size_t()
    off = C.c_uint64(int(offset))
    rc = lib().ebo_read_events_txt_at(str(path).encode(), C.byref(off), _vp(out), C.c_size_t(cap), C.byref(n))
    if rc:
        raise EboError(rc, "cannot parse %s (parsed %d events before the error)" % (path, n.value))
    return out[: n.value].copy(), int(off.value)


def write_events_bin(path, ev):
    """Packed binary sidecar (32-byte header + 16 B per event) of an event array."""
    ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
    rc = lib().ebo_write_events_bin(str(path).encode(), _vp(ev), C.c_size_t(len(ev)))
    if rc:
        raise EboError(rc, "cannot write %s" % path)


def read_events_bin(path, cap=1 << 24):
    out = np.zeros(cap, dtype=EVENT_DTYPE)
    n = C.c_size_t()
    rc = lib().ebo_read_events_bin(str(path).encode(), _vp(out), C.c_size_t(cap), C.byref(n))
    if rc:
        raise EboError(rc, "cannot read %s (read %d events before the error)" % (path, n.value))
    return out[: n.value].copy()


def _png8(call):
    w, h = C.c_int32(), C.c_int32()
    rc = call(C.byref(w), C.byref(h), None, C.c_size_t(0))
    if rc:
        raise EboError(rc, lib().ebo_last_error(None).decode(errors="replace"))
    out = np.zeros((h.value, w.value), dtype=np.uint8)
    rc = call(C.byref(w), C.byref(h), _vp(out), C.c_size_t(out.size))
    if rc:
        raise EboError(rc, lib().ebo_last_error(None).decode(errors="replace"))
    return out


def decode_png8(data):
    """ebo_decode_png8: the bytes of an 8-bit greyscale, non-interlaced PNG -> uint8 [h][w] (a DAVIS frame as
    cv::imread(path, CV_8U) returns it).  EboError with EBO_ERR_UNSUPPORTED / EBO_ERR_ARG otherwise."""
    data = bytes(data)
    buf = C.create_string_buffer(data, len(data))
    f = lib().ebo_decode_png8
    f.restype = C.c_int
    return _png8(lambda w, h, px, cap: f(buf, C.c_size_t(len(data)), w, h, px, cap))


def read_png8(path):
    """ebo_read_png8: decode_png8 of a file."""
    f = lib().ebo_read_png8
    f.restype = C.c_int
    p = str(path).encode()
    return _png8(lambda w, h, px, cap: f(p, w, h, px, cap))


def write_tracks_txt(path, pts):
    """trajectory.txt as tools::Evaluator::saveFeaturesTrajectory writes it (evaluator.cpp:125-150)."""
    pts = np.ascontiguousarray(pts, dtype=TRACK_DTYPE)
    rc = lib().ebo_write_tracks_txt(str(path).encode(), _vp(pts), C.c_size_t(len(pts)))
    if rc:
        raise EboError(rc, "cannot write %s" % path)


def read_tracks_txt(path, cap=1 << 16):
    """trajectory.txt -> track records; the buffer grows to what the file holds (never a truncated list)."""
    while True:
        out = np.zeros(cap, dtype=TRACK_DTYPE)
        n = C.c_size_t()
        rc = lib().ebo_read_tracks_txt(str(path).encode(), _vp(out), C.c_size_t(cap), C.byref(n))
        if rc == ERR_ARG and n.value > cap:
            cap = n.value
            continue
        if rc:
            raise EboError(rc, "cannot parse %s (parsed %d records before the error)" % (path, n.value))
        return out[: n.value].copy()


def pack_events8(ev, t_base, out=None):
    """EventSamples of one window -> compact 8-byte records relative to t_base."""
    ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
    if out is None:
        out = np.zeros(len(ev), dtype=EVENT8_DTYPE)
    rc = lib().ebo_pack_events8(_vp(ev), C.c_size_t(len(ev)), C.c_int64(int(t_base)), _vp(out))
    if rc:
        raise EboError(rc, "event does not fit the compact record")
    return out


def make_events(x, y, t_us, sign=None):
    ev = np.zeros(len(x), dtype=EVENT_DTYPE)
    ev["x"] = x
    ev["y"] = y
    ev["t_us"] = t_us
    ev["sign"] = 1 if sign is None else sign
    return ev


class Graph:
    """A recorded step (ebo_graph): launch(times) replays it back to back on the context's stream."""

    def __init__(self, ctx, handle):
        self._ctx, self._g = ctx, handle

    def launch(self, times=1):
        self._ctx._check(lib().ebo_graph_launch(self._ctx._h, self._g, int(times)))

    def close(self):
        if self._g:
            lib().ebo_graph_destroy(self._g)
            self._g = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


class Context:
    """Owns one ebo_ctx (one device, one stream).  Mirrors include/ebo.h 1:1."""

    def __init__(self, params=None, **kw):
        self._h = C.c_void_p()
        self.params = params if params is not None else default_params(**kw)
        rc = lib().ebo_create(C.byref(self.params), C.byref(self._h))
        if rc:
            raise EboError(rc, lib().ebo_last_error(None).decode())
        npx, npy = C.c_int(), C.c_int()
        self._check(lib().ebo_grid(self._h, C.byref(npx), C.byref(npy)))
        self.npx, self.npy = npx.value, npy.value
        self.P = self.npx * self.npy
        self.n_windows = 0

    def _check(self, rc):
        if rc:
            raise EboError(rc, lib().ebo_last_error(self._h).decode())

    def close(self):
        if self._h:
            lib().ebo_destroy(self._h)
            self._h = C.c_void_p()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()

    # -- setup ---------------------------------------------------------------
    def set_stream(self, hip_stream):
        self._check(lib().ebo_set_stream(self._h, C.c_void_p(int(hip_stream))))

    def synchronize(self):
        self._check(lib().ebo_synchronize(self._h))

    def record(self, fn):
        """Record the asynchronous *_device calls fn() makes into a HIP graph (ebo_graph_begin / _end).
        Run fn() once before (work tables are allocated on first use).  -> Graph"""
        self._check(lib().ebo_graph_begin(self._h))
        try:
            fn()
        finally:
            g = C.c_void_p()
            rc = lib().ebo_graph_end(self._h, C.byref(g))
        self._check(rc)
        return Graph(self, g)

    def patch_rect(self, px, py):
        v = [C.c_int() for _ in range(4)]
        self._check(lib().ebo_patch_rect(self._h, int(px), int(py), *[C.byref(a) for a in v]))
        return tuple(a.value for a in v)

    def set_window(self, ev):
        ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
        self._check(lib().ebo_set_window(self._h, _vp(ev), C.c_size_t(len(ev))))
        self.n_windows = 1
        self._custom = None

    def set_windows(self, ev, offsets):
        ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        self._check(lib().ebo_set_windows(self._h, _vp(ev), _vp(offsets), int(n)))
        self.n_windows = n
        self._custom = None

    def set_windows_device(self, d_events, offsets):
        """Raw ebo_event records already in device memory (pointer as int); offsets: host."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        self._check(lib().ebo_set_windows_device(self._h, C.c_void_p(int(d_events)), _vp(offsets), int(n)))
        self.n_windows = n
        self._custom = None

    def set_windows8(self, ev8, t_base, offsets, device=False):
        """Compact 8-byte records (EVENT8_DTYPE array or, with device=True, a device pointer)."""
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        t_base = np.ascontiguousarray(t_base, dtype=np.int64)
        n = len(offsets) - 1
        assert len(t_base) == n
        if device:
            self._check(lib().ebo_set_windows8_device(self._h, C.c_void_p(int(ev8)), _vp(t_base), _vp(offsets), int(n)))
        else:
            if isinstance(ev8, np.ndarray):
                ev8 = np.ascontiguousarray(ev8, dtype=EVENT8_DTYPE)
                ptr = _vp(ev8)
            else:
                ptr = C.c_void_p(int(ev8))  # e.g. the address of page-locked memory
            self._check(lib().ebo_set_windows8(self._h, ptr, _vp(t_base), _vp(offsets), int(n)))
        self.n_windows = n
        self._custom = None

    def set_patches(self, ev, offsets, rects):
        """Arbitrary patches (contrastFunctor instances): rects [n][4] = (x, y, w, h)."""
        ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        rects = np.ascontiguousarray(rects, dtype=np.int32).reshape(-1, 4)
        self._check(lib().ebo_set_patches(self._h, _vp(ev), _vp(offsets), _vp(rects), len(rects)))
        self.n_windows = 1
        self._custom = [tuple(int(v) for v in r) for r in rects]

    @property
    def cur_patches(self):
        """Flows per window: grid patches, or the number given to set_patches."""
        return len(self._custom) if getattr(self, "_custom", None) else self.P

    def window_info(self, w=0):
        t, n = C.c_int64(), C.c_uint64()
        self._check(lib().ebo_window_info(self._h, int(w), C.byref(t), C.byref(n)))
        return t.value, n.value

    def patch_info(self, p, w=0):
        n, a, t = C.c_int32(), C.c_int32(), C.c_int64()
        self._check(lib().ebo_patch_info(self._h, int(w), int(p), C.byref(n), C.byref(a), C.byref(t)))
        return n.value, bool(a.value), t.value

    # -- objective -----------------------------------------------------------
    def eval(self, flows, want_jac=True):
        P = self.cur_patches
        flows = np.ascontiguousarray(flows, dtype=np.float64).reshape(self.n_windows, P, 2)
        r = np.zeros((self.n_windows, P))
        J = np.zeros((self.n_windows, P, 2)) if want_jac else None
        self._check(lib().ebo_eval(self._h, _dp(flows), _dp(r), _dp(J) if want_jac else None))
        return r, J

    def eval_device(self, d_flows, want_jac, d_out):
        self._check(lib().ebo_eval_device(
            self._h, C.c_void_p(int(d_flows)), int(want_jac), C.c_void_p(int(d_out))))

    def contrast_image(self, patch, flow, channels=3, window=0):
        if getattr(self, "_custom", None):
            x, y, w, h = self._custom[patch]
        else:
            x, y, w, h = self.patch_rect(patch % self.npx, patch // self.npx)
        flow = np.ascontiguousarray(flow, dtype=np.float64)
        img = np.zeros((channels, 3 * h, 3 * w))
        self._check(lib().ebo_contrast_image(
            self._h, int(window), int(patch), _dp(flow), int(channels), _dp(img)))
        return img

    # -- solve ---------------------------------------------------------------
    def solve(self, opts=None, **kw):
        opts = opts if opts is not None else default_solver(**kw)
        flows = np.zeros((self.n_windows, self.cur_patches, 2))
        summ = (Summary * self.n_windows)()
        self._check(lib().ebo_solve(self._h, C.byref(opts), _dp(flows), summ))
        return flows, list(summ)

    def solve_device(self, opts, d_flows_out, d_stats=0):
        self._check(lib().ebo_solve_device(
            self._h, C.byref(opts), C.c_void_p(int(d_flows_out)),
            C.c_void_p(int(d_stats)) if d_stats else None))

    # -- count images --------------------------------------------------------
    def count_image(self, mode, aux=None):
        img = np.zeros((self.n_windows, self.params.image_h, self.params.image_w))
        a = None
        if mode == COUNT_WARPED:
            aux = np.ascontiguousarray(aux, dtype=np.float64).reshape(self.n_windows, self.P, 2)
            a = _vp(aux)
        elif mode == COUNT_FIELD and aux is not None:
            aux = np.ascontiguousarray(aux, dtype=np.float32).reshape(
                self.n_windows, self.params.image_h, self.params.image_w, 2)
            a = _vp(aux)
        self._check(lib().ebo_count_image(self._h, int(mode), a, _dp(img)))
        return img

    def count_image_shard(self, n_windows, t_ref_us, flows_grid):
        """Partial final image (this context's events only) of n_windows windows whose patches are
        sharded: flows_grid [n_windows][P][2] = flows of ALL grid patches, t_ref_us [n_windows] = the
        windows' reference times.  Needs set_patches."""
        t_ref = np.ascontiguousarray(t_ref_us, dtype=np.int64).reshape(n_windows)
        flows = np.ascontiguousarray(flows_grid, dtype=np.float64).reshape(n_windows, self.P, 2)
        img = np.zeros((n_windows, self.params.image_h, self.params.image_w))
        self._check(lib().ebo_count_image_shard(self._h, int(n_windows), _vp(t_ref), _dp(flows), _dp(img)))
        return img

    def count_image_shard_device(self, n_windows, t_ref_us, d_flows_grid, d_image):
        t_ref = np.ascontiguousarray(t_ref_us, dtype=np.int64).reshape(n_windows)
        self._check(lib().ebo_count_image_shard_device(self._h, int(n_windows), _vp(t_ref),
                                                       C.c_void_p(int(d_flows_grid)), C.c_void_p(int(d_image))))

    def edge_work_stats(self, d_flows, want_jac=True):
        """diagnostic: one edge-loss evaluation that counts its work -> dict of totals over the units"""
        out = (C.c_uint64 * 6)()
        self._check(lib().ebo_edge_work_stats(self._h, C.c_void_p(int(d_flows)), 1 if want_jac else 0, out))
        keys = ("units", "events", "box_pixels", "eigen_pixels", "nms_windows", "argmax_entries")
        return dict(zip(keys, [int(v) for v in out]))

    def lds_rates(self):
        """diagnostic: (G atomics/s, G reads/s) of 64-bit LDS operations at random addresses, measured now"""
        out = (C.c_double * 2)()
        self._check(lib().ebo_lds_rates(self._h, out))
        return float(out[0]), float(out[1])

    def unit_records(self, w, b):
        """diagnostic: the packed records of one unit as they lie in device memory -> np.uint64[n]
        (b = 0 .. P-1 the grid patches, P the stray bucket; after set_patches w = 0 and b = the patch index)"""
        f = lib().ebo_unit_records
        f.argtypes = [C.c_void_p, C.c_int, C.c_int, C.c_void_p, C.c_size_t, C.c_void_p]
        n = C.c_size_t()
        rc = f(self._h, int(w), int(b), None, C.c_size_t(0), C.byref(n))
        if rc and not (rc == ERR_ARG and n.value > 0):
            self._check(rc)
        out = np.zeros(n.value, dtype=np.uint64)
        if n.value:
            self._check(f(self._h, int(w), int(b), _vp(out), C.c_size_t(n.value), C.byref(n)))
        return out

    def launch_order(self):
        """diagnostic: the launch-order table as it lies in device memory -> np.uint32[units]"""
        f = lib().ebo_launch_order
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        n = C.c_size_t()
        rc = f(self._h, None, C.c_size_t(0), C.byref(n))
        if rc and not (rc == ERR_ARG and n.value > 0):
            self._check(rc)
        out = np.zeros(n.value, dtype=np.uint32)
        if n.value:
            self._check(f(self._h, _vp(out), C.c_size_t(n.value), C.byref(n)))
        return out

    def unit_extents(self):
        """diagnostic: the time-extent table as it lies in device memory -> np.int32[units, 258]
        (status, 0, then (dtMin, dtMax) per source column and per source row; ebo.h: ebo_unit_extents)"""
        f = lib().ebo_unit_extents
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        n = C.c_size_t()
        rc = f(self._h, None, C.c_size_t(0), C.byref(n))
        if rc and not (rc == ERR_ARG and n.value > 0):
            self._check(rc)
        out = np.zeros(n.value, dtype=np.int32)
        if n.value:
            self._check(f(self._h, _vp(out), C.c_size_t(n.value), C.byref(n)))
        return out.reshape(-1, 258)

    def box_path_counts(self):
        """diagnostic, A/B library only: (units whose box came from the event pass, from the table) in the last
        variance evaluation"""
        f = lib().ebo_box_path_counts
        f.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p]
        a, b = C.c_uint(), C.c_uint()
        self._check(f(self._h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def interior_path_counts(self):
        """diagnostic, A/B library only: units that took the all-interior path (csrc/eval_interior.h) in the last
        variance evaluation"""
        f = lib().ebo_interior_path_counts
        f.argtypes = [C.c_void_p, C.c_void_p]
        a = C.c_uint()
        self._check(f(self._h, C.byref(a)))
        return a.value

    def unit_deal(self, unit, d_flows, want_jac, d_out):
        """diagnostic, A/B library only: the dealt list of one unit (index as in launch_order) in one variance evaluation
        at the device flows d_flows into d_out -> np.uint16[events of the unit], empty where the unit is not dealt
        (ebo.h: ebo_unit_deal)"""
        f = lib().ebo_unit_deal
        f.argtypes = [C.c_void_p, C.c_int, C.c_void_p, C.c_int, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
        out = np.zeros(65536, dtype=np.uint16)
        n = C.c_size_t()
        self._check(f(self._h, int(unit), C.c_void_p(int(d_flows)), int(want_jac), C.c_void_p(int(d_out)), _vp(out),
                      C.c_size_t(len(out)), C.byref(n)))
        return out[:n.value].copy()

    def eval_launch_shape(self, want_jac=True):
        """diagnostic: (row tiles per unit, lanes per workgroup, flow sets) of the variance evaluation's launch"""
        v = [C.c_int() for _ in range(3)]
        self._check(lib().ebo_eval_launch_shape(self._h, int(want_jac), *[C.byref(a) for a in v]))
        return tuple(a.value for a in v)

    def eval_resident_workgroups(self, want_jac=True):
        """diagnostic: (planned, actual) workgroups of the variance evaluation's launch resident on one CU"""
        v = [C.c_int() for _ in range(2)]
        self._check(lib().ebo_eval_resident_workgroups(self._h, int(want_jac), *[C.byref(a) for a in v]))
        return tuple(a.value for a in v)

    def stream_yardstick_device(self, d_image):
        """diagnostic: the bytes of a count-image launch with no work; returns the bytes moved"""
        n = C.c_uint64()
        self._check(lib().ebo_stream_yardstick_device(self._h, C.c_void_p(int(d_image)), C.byref(n)))
        return n.value

    def count_image_device(self, mode, d_aux, d_image):
        self._check(lib().ebo_count_image_device(
            self._h, int(mode), C.c_void_p(int(d_aux)) if d_aux else None,
            C.c_void_p(int(d_image))))

    def compensate_events_contrast(self, ev, opts=None, want_image=True):
        ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
        opts = opts if opts is not None else default_solver()
        flows = np.zeros((self.P, 2))
        img = np.zeros((self.params.image_h, self.params.image_w)) if want_image else None
        s = Summary()
        self._check(lib().ebo_compensate_events_contrast(
            self._h, _vp(ev), C.c_size_t(len(ev)), C.byref(opts), _dp(flows),
            _dp(img) if want_image else None, C.byref(s)))
        self.n_windows = 1
        self._custom = None
        return flows, img, s

    def compensate_windows(self, ev, offsets, opts=None, images=True):
        """ebo_compensate_windows: window w = ev[offsets[w]:offsets[w+1]], in chunks of what the context holds.
        -> (flows [Wn][P][2], warped [Wn][H][W], integrated [Wn][H][W] (both None without images), summaries,
        status int32 [Wn]).  A refused window has its EBO_ERR_* in status and zeros in its outputs; only an error
        of the call itself (bad arguments, recording a graph) raises."""
        ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        n = len(offsets) - 1
        opts = opts if opts is not None else default_solver()
        flows = np.zeros((n, self.P, 2))
        shape = (n, self.params.image_h, self.params.image_w)
        warped = np.zeros(shape) if images else None
        integrated = np.zeros(shape) if images else None
        summ = (Summary * max(n, 1))()
        status = np.zeros(max(n, 1), dtype=np.int32)
        rc = lib().ebo_compensate_windows(
            self._h, _vp(ev), _vp(offsets), int(n), C.byref(opts), _dp(flows),
            _dp(warped) if images else None, _dp(integrated) if images else None, summ, _vp(status))
        if rc and not status[:n].any():
            self._check(rc)
        self.n_windows = 0  # the context holds the last chunk, not these windows
        self._custom = None
        return flows, warped, integrated, list(summ)[:n], status[:n]

    def init_motion_field(self, timestamp, trajectories, use_average=True):
        """FeatureDetector::initMotionField. trajectories: list of [(x, y, t_us), ...] per patch.
        Returns (field float32 [H][W][2], fixed points [n][2])."""
        offs = np.zeros(len(trajectories) + 1, dtype=np.uint64)
        offs[1:] = np.cumsum([len(t) for t in trajectories])
        flat = [s for t in trajectories for s in t]
        xy = np.ascontiguousarray([[s[0], s[1]] for s in flat], dtype=np.float64).reshape(-1, 2)
        tt = np.ascontiguousarray([int(s[2]) for s in flat], dtype=np.int64)
        field = np.zeros((self.params.image_h, self.params.image_w, 2), dtype=np.float32)
        nfix = C.c_int32()
        fixed = np.zeros((max(len(trajectories), 1), 2), dtype=np.int32)
        self._check(lib().ebo_init_motion_field(
            self._h, C.c_int64(int(timestamp)), int(bool(use_average)), len(trajectories), _vp(offs),
            _vp(xy), _vp(tt), _vp(field), C.byref(nfix), _vp(fixed)))
        return field, fixed[: nfix.value].copy()

    def interpolate_motion_field(self, use_l1=False, opts=None):
        """FeatureDetector::interpolateMotionField on the field of the last init_motion_field.
        Returns (field float32 [H][W][2], Summary, total CG iterations)."""
        field = np.zeros((self.params.image_h, self.params.image_w, 2), dtype=np.float32)
        s = Summary()
        cg = C.c_int32()
        self._check(lib().ebo_interpolate_motion_field(
            self._h, int(bool(use_l1)), C.byref(opts) if opts is not None else None, _vp(field),
            C.byref(s), C.byref(cg)))
        return field, s, cg.value

    # -- per-feature tracker objective (Optimizer / OptimizerCostFunctor) ------
    def optimizer_set_grad(self, grad_x, grad_y):
        gx = np.ascontiguousarray(grad_x, dtype=np.float64)
        gy = np.ascontiguousarray(grad_y, dtype=np.float64)
        assert gx.shape == gy.shape == (self.params.image_h, self.params.image_w)
        self._check(lib().ebo_optimizer_set_grad(self._h, _dp(gx), _dp(gy)))

    @staticmethod
    def _opt_inputs(rects, nablas, poses, flow_dirs):
        rects = np.ascontiguousarray(rects, dtype=np.float64).reshape(-1, 4)
        nabla = np.ascontiguousarray(np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in nablas])
                                     if len(nablas) else np.zeros(0))
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4).copy()
        flow_dirs = np.ascontiguousarray(flow_dirs, dtype=np.float64).reshape(-1).copy()
        sizes = [int(r[2]) * int(r[3]) for r in rects]
        assert nabla.size == sum(sizes)
        return rects, nabla, poses, flow_dirs, sizes

    def optimizer_eval(self, rects, nablas, poses, flow_dirs, want_jac=True):
        """OptimizerCostFunctor for n patches.  Returns lists (residuals, jac_pose, jac_flow)."""
        rects, nabla, poses, flow_dirs, sizes = self._opt_inputs(rects, nablas, poses, flow_dirs)
        total = sum(sizes)
        res = np.zeros(total)
        jp = np.zeros((total, 4)) if want_jac else None
        jf = np.zeros(total) if want_jac else None
        self._check(lib().ebo_optimizer_eval(
            self._h, len(rects), _dp(rects), _dp(nabla), _dp(poses), _dp(flow_dirs), _dp(res),
            _dp(jp) if want_jac else None, _dp(jf) if want_jac else None))
        offs = np.concatenate([[0], np.cumsum(sizes)]).astype(int)
        cut = lambda a: [a[offs[i]:offs[i + 1]] for i in range(len(sizes))]
        return cut(res), (cut(jp) if want_jac else None), (cut(jf) if want_jac else None)

    def optimizer_solve(self, rects, nablas, poses, flow_dirs, normalize=False, huber=0.3, opts=None):
        """Optimizer::optimize's ceres::Solve for n patches.  Returns (poses, flow_dirs, summaries)."""
        rects, nabla, poses, flow_dirs, sizes = self._opt_inputs(rects, nablas, poses, flow_dirs)
        n = len(rects)
        sums = (Summary * max(n, 1))()
        self._check(lib().ebo_optimizer_solve(
            self._h, n, _dp(rects), _dp(nabla), int(bool(normalize)), C.c_double(huber),
            C.byref(opts) if opts is not None else None, _dp(poses), _dp(flow_dirs), sums))
        return poses, flow_dirs, list(sums)[:n]

    def optimizer_cost_map(self, rects, nablas, poses, flow_dirs, map_w=11, map_h=11, normalize=False):
        """Optimizer::drawCostMap for n patches: -> [n][map_h][map_w] (the L2 norm of the functor's residual image
        at the map's translation offsets around each pose)."""
        rects, nabla, poses, flow_dirs, sizes = self._opt_inputs(rects, nablas, poses, flow_dirs)
        n = len(rects)
        out = np.zeros((max(n, 1), map_h, map_w))
        self._check(lib().ebo_optimizer_cost_map(
            self._h, n, _dp(rects), _dp(nabla), int(bool(normalize)), _dp(poses), _dp(flow_dirs), int(map_w), int(map_h),
            _dp(out)))
        return out[:n]

    def estimate_num_events(self, rects, poses, flow_dirs):
        """FeatureDetector::updateNumOfEvents' event-count estimate for n tracked patches."""
        rects = np.ascontiguousarray(rects, dtype=np.float64).reshape(-1, 4)
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4)
        flow_dirs = np.ascontiguousarray(flow_dirs, dtype=np.float64).reshape(-1)
        n = len(rects)
        out = np.zeros(max(n, 1), dtype=np.uint64)
        self._check(lib().ebo_estimate_num_events(self._h, n, _dp(rects), _dp(poses), _dp(flow_dirs), _vp(out)))
        return out[:n]

    def patch_warp_image(self, rects, poses, flow_dirs):
        """Patch::warpImage for n tracked patches: -> list of predictedNabla arrays [h][w] (None where the
        reference returns early because the rect touches the image border)."""
        rects = np.ascontiguousarray(rects, dtype=np.float64).reshape(-1, 4)
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 4)
        flow_dirs = np.ascontiguousarray(flow_dirs, dtype=np.float64).reshape(-1)
        n = len(rects)
        # a size the entry refuses (NaN, outside 0..32767) takes no room here: the call reports it
        dim = lambda v: int(np.rint(v)) if np.isfinite(v) and 0 <= np.rint(v) <= 32767 else 0
        shapes = [(dim(r[3]), dim(r[2])) for r in rects]
        sizes = [h * w for h, w in shapes]
        noff = np.zeros(max(n, 1), dtype=np.uint64)
        noff[1:n] = np.cumsum(sizes[:-1])
        out = np.zeros(max(int(sum(sizes)), 1))
        upd = np.zeros(max(n, 1), dtype=np.int32)
        self._check(lib().ebo_patch_warp_image(self._h, n, _dp(rects), _dp(poses), _dp(flow_dirs), _vp(noff), _dp(out),
                                               _vp(upd)))
        return [out[int(noff[i]):int(noff[i]) + sizes[i]].reshape(shapes[i]).copy() if upd[i] else None for i in range(n)]

    # -- tracked-feature patches (Patch::integrate*) --------------------------
    def patch_integrate(self, ev, offsets, rects):
        ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        rects = np.ascontiguousarray(rects, dtype=np.float64).reshape(-1, 4)
        n = len(rects)
        sizes = [int(r[3]) * int(r[2]) for r in rects]
        noff = np.zeros(n, dtype=np.uint64)
        noff[1:] = np.cumsum(sizes[:-1])
        nabla = np.zeros(int(sum(sizes)))
        cur = np.zeros(n, dtype=np.int64)
        last = np.zeros(n, dtype=np.int64)
        self._check(lib().ebo_patch_integrate(
            self._h, _vp(ev), _vp(offsets), n, _dp(rects), _vp(noff), _dp(nabla), _vp(cur), _vp(last)))
        imgs = [nabla[int(noff[i]):int(noff[i]) + sizes[i]].reshape(int(rects[i][3]), int(rects[i][2]))
                for i in range(n)]
        return imgs, cur, last

    def patch_integrate_mc(self, ev, offsets, rects, traj, mid_time, init=None):
        ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
        offsets = np.ascontiguousarray(offsets, dtype=np.uint64)
        rects = np.ascontiguousarray(rects, dtype=np.float64).reshape(-1, 4)
        traj = np.ascontiguousarray(traj, dtype=np.float64).reshape(-1, 6)
        mid_time = np.ascontiguousarray(mid_time, dtype=np.int64)
        n = len(rects)
        sizes = [int(r[3]) * int(r[2]) for r in rects]
        noff = np.zeros(n, dtype=np.uint64)
        noff[1:] = np.cumsum(sizes[:-1])
        nabla = np.zeros(int(sum(sizes))) if init is None else np.ascontiguousarray(init, dtype=np.float64).copy()
        upd = np.zeros(n, dtype=np.int32)
        self._check(lib().ebo_patch_integrate_mc(
            self._h, _vp(ev), _vp(offsets), n, _dp(rects), _dp(traj), _vp(mid_time), _vp(noff),
            _dp(nabla), _vp(upd)))
        imgs = [nabla[int(noff[i]):int(noff[i]) + sizes[i]].reshape(int(rects[i][3]), int(rects[i][2]))
                for i in range(n)]
        return imgs, upd

    # -- event -> tracked-patch routing (FeatureDetector::updatePatches) --------
    def route_set_events(self, ev):
        ev = np.ascontiguousarray(ev, dtype=EVENT_DTYPE)
        self._check(lib().ebo_route_set_events(self._h, _vp(ev), C.c_size_t(len(ev))))

    def route_events(self, rects, start, max_take, cap):
        """-> (list of index arrays per patch, next index per patch)."""
        rects = np.ascontiguousarray(rects, dtype=np.float64).reshape(-1, 4)
        n = len(rects)
        start = np.ascontiguousarray(start, dtype=np.uint32)
        max_take = np.ascontiguousarray(max_take, dtype=np.uint32)
        idx = np.zeros((n, max(int(cap), 1)), dtype=np.uint32)
        cnt = np.zeros(n, dtype=np.uint32)
        nxt = np.zeros(n, dtype=np.uint32)
        self._check(lib().ebo_route_events(self._h, n, _dp(rects), _vp(start), _vp(max_take), C.c_uint32(int(cap)),
                                           _vp(idx), _vp(cnt), _vp(nxt)))
        return [idx[i, :cnt[i]].copy() for i in range(n)], nxt

    # -- RCCL exchange (no framework) -----------------------------------------
    def comm_init(self, comm_id, rank, nranks):
        buf = (C.c_char * 128).from_buffer_copy(bytes(comm_id))
        self._check(lib().ebo_comm_init(self._h, C.byref(buf), int(rank), int(nranks)))
        self._nranks = int(nranks)

    def allgather_device(self, d_send, d_recv, count_per_rank):
        self._check(lib().ebo_allgather_device(
            self._h, C.c_void_p(int(d_send)), C.c_void_p(int(d_recv)), C.c_size_t(int(count_per_rank))))

    def comm_size(self):
        """(rank, nranks) of the context's communicator; (0, 1) without one."""
        r, n = C.c_int(), C.c_int()
        self._check(lib().ebo_comm_size(self._h, C.byref(r), C.byref(n)))
        return r.value, n.value

    def reduce_sum_device(self, d_send, d_recv, count, root=-1):
        """Sum of `count` doubles over the ranks into d_recv on `root` (every rank when root < 0)."""
        self._check(lib().ebo_reduce_sum_device(
            self._h, C.c_void_p(int(d_send)), C.c_void_p(int(d_recv)) if d_recv else None, C.c_size_t(int(count)),
            int(root)))

    def allgather_tracks(self, local):
        """Every rank's track records on every rank (rank order): -> (records, counts per rank).  ONE counts
        collective + ONE gather per call: the result buffer is kept between calls and grows by a rule that
        depends only on the gathered total (4096 records, then the next power of two), so every rank finds it
        too small -- and repeats the exchange -- in the same call."""
        local = np.ascontiguousarray(local, dtype=TRACK_DTYPE)
        nr = C.c_size_t()
        counts = np.zeros(self.comm_size()[1], dtype=np.uint64)
        buf = getattr(self, "_track_buf", None)
        if buf is None:
            buf = self._track_buf = np.zeros(4096, dtype=TRACK_DTYPE)
        rc = lib().ebo_allgather_tracks(self._h, _vp(local), C.c_size_t(len(local)), _vp(buf), C.c_size_t(len(buf)),
                                        C.byref(nr), _vp(counts))
        if rc == ERR_ARG and nr.value > len(buf):  # the same on every rank: all of them repeat
            buf = self._track_buf = np.zeros(1 << int(nr.value - 1).bit_length(), dtype=TRACK_DTYPE)
            rc = lib().ebo_allgather_tracks(self._h, _vp(local), C.c_size_t(len(local)), _vp(buf), C.c_size_t(len(buf)),
                                            C.byref(nr), _vp(counts))
        self._check(rc)
        return buf[:nr.value].copy(), counts.astype(np.int64)

    # -- band-limited final image of row-sharded windows -------------------------
    def band_plan(self, row_bounds, rank, halo):
        """-> Band for `rank` of the partition row_bounds [nranks + 1] (image rows); EboError(ERR_UNSUPPORTED) when a
        halo would not fit inside a neighbour's rows."""
        return band_plan(self.params.image_h, row_bounds, rank, halo)

    def count_image_band_device(self, n_windows, t_ref_us, d_flows_grid, band, d_top, d_own, d_bottom, d_escaped):
        t_ref = np.ascontiguousarray(t_ref_us, dtype=np.int64).reshape(n_windows)
        self._check(lib().ebo_count_image_band_device(
            self._h, int(n_windows), _vp(t_ref), C.c_void_p(int(d_flows_grid)), C.byref(band),
            C.c_void_p(int(d_top)) if d_top else None, C.c_void_p(int(d_own)) if d_own else None,
            C.c_void_p(int(d_bottom)) if d_bottom else None, C.c_void_p(int(d_escaped))))

    def band_exchange_device(self, n_windows, band, d_top, d_bottom, d_from_above, d_from_below, d_escaped):
        p = lambda v: C.c_void_p(int(v)) if v else None
        self._check(lib().ebo_band_exchange_device(self._h, int(n_windows), C.byref(band), p(d_top), p(d_bottom),
                                                   p(d_from_above), p(d_from_below), p(d_escaped)))

    def band_finish_device(self, n_windows, band, d_own, d_from_above, d_from_below, d_image_own):
        p = lambda v: C.c_void_p(int(v)) if v else None
        self._check(lib().ebo_band_finish_device(self._h, int(n_windows), C.byref(band), p(d_own), p(d_from_above),
                                                 p(d_from_below), p(d_image_own)))

    def band_gather_device(self, n_windows, row_bounds, d_image_own, root, d_full):
        rb = np.ascontiguousarray(row_bounds, dtype=np.int32)
        self._check(lib().ebo_band_gather_device(self._h, int(n_windows), _vp(rb), C.c_void_p(int(d_image_own)) if d_image_own else None,
                                                 int(root), C.c_void_p(int(d_full)) if d_full else None))

    def comm_destroy(self):
        self._check(lib().ebo_comm_destroy(self._h))

    # -- image front end (FeatureDetector::newImage without OpenCV) -----------
    def _image(self, image):
        img = np.ascontiguousarray(image, dtype=np.uint8)
        assert img.shape == (self.params.image_h, self.params.image_w), img.shape
        return img

    def image_gradients(self, image):
        """getLogImage + getGradients: uint8 [h][w] -> (grad_x, grad_y), float64 [h][w]."""
        img = self._image(image)
        gx = np.zeros(img.shape)
        gy = np.zeros(img.shape)
        self._check(lib().ebo_image_gradients(self._h, _vp(img), _dp(gx), _dp(gy)))
        return gx, gy

    def good_features(self, image, mask=None, max_corners=100, quality_level=0.01, min_distance=10.0, block_size=3,
                      harris_k=0.04):
        """goodFeaturesToTrack in Harris mode: -> float32 [n][2] corners (x, y), in selection order."""
        img = self._image(image)
        m = None if mask is None else self._image(mask)
        out = np.zeros((int(max_corners), 2), dtype=np.float32)
        n = C.c_int()
        self._check(lib().ebo_good_features(self._h, _vp(img), _vp(m) if m is not None else None, int(max_corners),
                                            C.c_double(quality_level), C.c_double(min_distance), int(block_size),
                                            C.c_double(harris_k), _vp(out), C.byref(n)))
        return out[:n.value].copy()

    def lk_add_image(self, image):
        """FlowEstimator::addImage: pyramid + derivatives on the device; the last two images are kept."""
        img = self._image(image)
        self._check(lib().ebo_lk_add_image(self._h, _vp(img)))

    def lk_track(self, prev_xy, win=(21, 21), max_level=3, max_count=30, epsilon=0.01, min_eig_threshold=1e-4):
        """calcOpticalFlowPyrLK from the older image to the newer one: -> (next_xy float32 [n][2], status uint8 [n],
        err float32 [n])."""
        pts = np.ascontiguousarray(prev_xy, dtype=np.float32).reshape(-1, 2)
        n = len(pts)
        nxt = np.zeros((max(n, 1), 2), dtype=np.float32)
        st = np.zeros(max(n, 1), dtype=np.uint8)
        err = np.zeros(max(n, 1), dtype=np.float32)
        self._check(lib().ebo_lk_track(self._h, n, _vp(pts), _vp(nxt), _vp(st), _vp(err), int(win[0]), int(win[1]),
                                       int(max_level), int(max_count), C.c_double(epsilon),
                                       C.c_double(min_eig_threshold)))
        return nxt[:n], st[:n], err[:n]

    # -- camera model (common::CameraModel) -----------------------------------
    def camera_unproject(self, cam, uv):
        """CameraModel::unproject for many points: float64 [n][2] pixels -> float64 [n][3] unit bearing vectors."""
        cam = camera(cam)
        uv = np.ascontiguousarray(uv, dtype=np.float64).reshape(-1, 2)
        out = np.zeros((len(uv), 3))
        self._check(lib().ebo_camera_unproject(self._h, C.byref(cam), len(uv), _dp(uv), _dp(out)))
        return out

    def camera_unproject_device(self, cam, n, d_uv, d_bearing):
        """The same on device arrays (pointers as int), asynchronous on the context's stream."""
        cam = camera(cam)
        self._check(lib().ebo_camera_unproject_device(self._h, C.byref(cam), int(n), C.c_void_p(int(d_uv)),
                                                      C.c_void_p(int(d_bearing))))

    def set_rectification(self, cam):
        """Every later window load reads its events through the camera's rectification table."""
        cam = camera(cam)
        self._check(lib().ebo_set_rectification(self._h, C.byref(cam)))

    def clear_rectification(self):
        self._check(lib().ebo_clear_rectification(self._h))

    def rectification_map(self):
        """-> (map float64 [h][w][2] = (u, v), table int16 [h][w][2] = (round(u), round(v)))."""
        h, w = self.params.image_h, self.params.image_w
        m = np.zeros((h, w, 2))
        lut = np.zeros((h, w, 2), dtype=np.int16)
        self._check(lib().ebo_rectification_map(self._h, _dp(m), _vp(lut)))
        return m, lut

    def camera_project(self, cam, xyz):
        """CameraModel::project for many points: float64 [n][3] camera-frame points -> float64 [n][2] pixels."""
        cam = camera(cam)
        xyz = np.ascontiguousarray(xyz, dtype=np.float64).reshape(-1, 3)
        out = np.zeros((len(xyz), 2))
        self._check(lib().ebo_camera_project(self._h, C.byref(cam), len(xyz), _dp(xyz), _dp(out)))
        return out

    def camera_project_device(self, cam, n, d_xyz, d_uv):
        """The same on device arrays (pointers as int), asynchronous on the context's stream."""
        cam = camera(cam)
        self._check(lib().ebo_camera_project_device(self._h, C.byref(cam), int(n), C.c_void_p(int(d_xyz)),
                                                    C.c_void_p(int(d_uv))))

    def fit_rectified_camera(self, cam):
        """-> the Camera (zero distortion) into which the sensor's undistorted border fits exactly."""
        cam = camera(cam)
        out = Camera()
        self._check(lib().ebo_fit_rectified_camera(self._h, C.byref(cam), C.byref(out)))
        return out

    def set_rectification_camera(self, cam, rectified):
        """set_rectification with an explicit rectified camera (zero distortion)."""
        cam, rectified = camera(cam), camera(rectified)
        self._check(lib().ebo_set_rectification_camera(self._h, C.byref(cam), C.byref(rectified)))

    def rectified_camera(self):
        """The rectified Camera of the rectification that is set."""
        out = Camera()
        self._check(lib().ebo_rectified_camera(self._h, C.byref(out)))
        return out

    def rectification_source_map(self):
        """-> float64 [h][w][2]: where in the raw frame each pixel of the rectified frame is sampled."""
        m = np.zeros((self.params.image_h, self.params.image_w, 2))
        self._check(lib().ebo_rectification_source_map(self._h, _dp(m)))
        return m

    def rectify_image(self, image):
        """uint8 [h][w] raw frame -> uint8 [h][w] rectified frame (bilinear, constant border 0)."""
        h, w = self.params.image_h, self.params.image_w
        img = np.ascontiguousarray(image, dtype=np.uint8)
        if img.shape != (h, w):
            raise ValueError("rectify_image: the image must be uint8 [%d][%d]" % (h, w))
        out = np.zeros((h, w), dtype=np.uint8)
        self._check(lib().ebo_rectify_image(self._h, _vp(img), _vp(out)))
        return out

    def rectify_image_device(self, d_image, d_out):
        """The same on device arrays (pointers as int), asynchronous on the context's stream."""
        self._check(lib().ebo_rectify_image_device(self._h, C.c_void_p(int(d_image)), C.c_void_p(int(d_out))))

    # -- two-view geometry (eight-point RANSAC, triangulation, the epipolar test) ---------------------
    def relative_pose_ransac(self, offsets, f1, f2, params=None, diagnostics=False, device=False):
        """ebo_relative_pose_ransac over len(offsets) - 1 keyframe pairs.  f1, f2: float64 [total][3] unit bearing
        vectors (device=True: device pointers as int, and the _device entry).  -> list of dicts (found, model [3][4],
        winner, iterations, n_inliers, inliers int32 [n_inliers]); with diagnostics=True also a dict of every
        hypothesis's counts [pairs][H], models [pairs][H][3][4] and samples [pairs][H][8]."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
        n_pairs = len(offsets) - 1
        prm = params if params is not None else two_view_params()
        total = int(offsets[-1]) if n_pairs >= 0 and len(offsets) else 0
        if device:
            p1, p2 = C.c_void_p(int(f1)), C.c_void_p(int(f2))
            fn = lib().ebo_relative_pose_ransac_device
        else:
            f1 = np.ascontiguousarray(f1, dtype=np.float64).reshape(-1, 3)
            f2 = np.ascontiguousarray(f2, dtype=np.float64).reshape(-1, 3)
            if len(f1) != total or len(f2) != total:
                raise ValueError("f1 / f2 must hold offsets[-1] bearing vectors")
            p1, p2 = _vp(f1), _vp(f2)
            fn = lib().ebo_relative_pose_ransac
        res = (TwoViewResult * max(n_pairs, 1))()
        idx = np.zeros(max(total, 1), dtype=np.int32)
        H = max(int(prm.max_iterations), 1)
        diag = None
        if diagnostics:
            diag = dict(counts=np.zeros((max(n_pairs, 0), H), dtype=np.int32), models=np.zeros((max(n_pairs, 0), H, 3, 4)),
                        samples=np.zeros((max(n_pairs, 0), H, 8), dtype=np.int32))
        self._check(fn(self._h, n_pairs, _vp(offsets), p1, p2, C.byref(prm), res, _vp(idx),
                       _vp(diag["counts"]) if diag else None, _vp(diag["models"]) if diag else None,
                       _vp(diag["samples"]) if diag else None))
        out = []
        for p in range(n_pairs):
            r = res[p]
            out.append(dict(found=bool(r.found), model=np.array(r.model[:]).reshape(3, 4), winner=r.winner,
                            iterations=r.iterations, n_inliers=r.n_inliers,
                            inliers=idx[r.inlier_offset:r.inlier_offset + r.n_inliers].copy()))
        return (out, diag) if diagnostics else out

    def two_view_timing(self, enable=True):
        """ebo_two_view_timing: -> the last timed RANSAC call's (hypotheses, counting, host walk, inlier list, whole call)
        in ms, and switches the timing on or off for the calls that follow."""
        ms = (C.c_float * 5)()
        self._check(lib().ebo_two_view_timing(self._h, 1 if enable else 0, ms))
        return tuple(ms)

    def relative_pose_scores(self, model, f1, f2, threshold=5e-5):
        """ebo_relative_pose_scores: -> (scores float64 [n], inlier flags bool [n]) of a given model [3][4]."""
        model = np.ascontiguousarray(model, dtype=np.float64).reshape(3, 4)
        f1 = np.ascontiguousarray(f1, dtype=np.float64).reshape(-1, 3)
        f2 = np.ascontiguousarray(f2, dtype=np.float64).reshape(-1, 3)
        n = len(f1)
        sc = np.zeros(n)
        fl = np.zeros(n, dtype=np.uint8)
        self._check(lib().ebo_relative_pose_scores(self._h, _vp(model), n, _vp(f1), _vp(f2), C.c_double(threshold), _vp(sc),
                                                   _vp(fl)))
        return sc, fl.astype(bool)

    def relative_pose_scores_device(self, model, n, d_f1, d_f2, threshold, d_scores=0, d_flags=0):
        """The same on device arrays (pointers as int; either output may be 0), asynchronous on the context's stream."""
        model = np.ascontiguousarray(model, dtype=np.float64).reshape(3, 4)
        p = lambda v: C.c_void_p(int(v)) if v else None
        self._check(lib().ebo_relative_pose_scores_device(self._h, _vp(model), int(n), p(d_f1), p(d_f2), C.c_double(threshold),
                                                          p(d_scores), p(d_flags)))

    # -- absolute pose (three-point RANSAC on bearing vectors and landmarks) --------------------------
    def absolute_pose_ransac(self, offsets, f, points, params, diagnostics=False, device=False):
        """ebo_absolute_pose_ransac over len(offsets) - 1 keyframes.  f: float64 [total][3] unit bearing vectors,
        points: float64 [total][3] landmarks in world coordinates (device=True: device pointers as int, and the _device
        entry); params: a TwoViewParams whose threshold the caller has set.  -> list of dicts (found, model [3][4] =
        the camera-to-world pose, winner, iterations, n_inliers, inliers int32 [n_inliers]); with diagnostics=True also
        a dict of every hypothesis's counts [frames][H], models [frames][H][3][4] and samples [frames][H][4]."""
        offsets = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
        n_frames = len(offsets) - 1
        total = int(offsets[-1]) if n_frames >= 0 and len(offsets) else 0
        if device:
            p1, p2 = C.c_void_p(int(f)), C.c_void_p(int(points))
            fn = lib().ebo_absolute_pose_ransac_device
        else:
            f = np.ascontiguousarray(f, dtype=np.float64).reshape(-1, 3)
            points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
            if len(f) != total or len(points) != total:
                raise ValueError("f / points must hold offsets[-1] rows")
            p1, p2 = _vp(f), _vp(points)
            fn = lib().ebo_absolute_pose_ransac
        res = (TwoViewResult * max(n_frames, 1))()
        idx = np.zeros(max(total, 1), dtype=np.int32)
        H = max(int(params.max_iterations), 1)
        diag = None
        if diagnostics:
            diag = dict(counts=np.zeros((max(n_frames, 0), H), dtype=np.int32), models=np.zeros((max(n_frames, 0), H, 3, 4)),
                        samples=np.zeros((max(n_frames, 0), H, 4), dtype=np.int32))
        self._check(fn(self._h, n_frames, _vp(offsets), p1, p2, C.byref(params), res, _vp(idx),
                       _vp(diag["counts"]) if diag else None, _vp(diag["models"]) if diag else None,
                       _vp(diag["samples"]) if diag else None))
        out = []
        for k in range(n_frames):
            r = res[k]
            out.append(dict(found=bool(r.found), model=np.array(r.model[:]).reshape(3, 4), winner=r.winner,
                            iterations=r.iterations, n_inliers=r.n_inliers,
                            inliers=idx[r.inlier_offset:r.inlier_offset + r.n_inliers].copy()))
        return (out, diag) if diagnostics else out

    def absolute_pose_scores(self, pose, f, points, threshold):
        """ebo_absolute_pose_scores: -> (scores float64 [n], inlier flags bool [n]) of a given pose [3][4]."""
        pose = np.ascontiguousarray(pose, dtype=np.float64).reshape(3, 4)
        f = np.ascontiguousarray(f, dtype=np.float64).reshape(-1, 3)
        points = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        n = len(f)
        sc = np.zeros(n)
        fl = np.zeros(n, dtype=np.uint8)
        self._check(lib().ebo_absolute_pose_scores(self._h, _vp(pose), n, _vp(f), _vp(points), C.c_double(threshold), _vp(sc),
                                                   _vp(fl)))
        return sc, fl.astype(bool)

    def absolute_pose_scores_device(self, pose, n, d_f, d_points, threshold, d_scores=0, d_flags=0):
        """The same on device arrays (pointers as int; either output may be 0), asynchronous on the context's stream."""
        pose = np.ascontiguousarray(pose, dtype=np.float64).reshape(3, 4)
        p = lambda v: C.c_void_p(int(v)) if v else None
        self._check(lib().ebo_absolute_pose_scores_device(self._h, _vp(pose), int(n), p(d_f), p(d_points), C.c_double(threshold),
                                                          p(d_scores), p(d_flags)))

    # -- bundle adjustment (Schur-complement LM over many windows) -------------------------------------
    def bundle_adjust(self, problems, cam, huber, fix_points=False, opts=None, trace=False):
        """ebo_bundle_adjust over a list of problems, each a dict of poses float64 [F][3][4] (camera to world), fixed
        [F], points [P][3], of / op int [N] (frame and point of an observation, local indices) and uv [N][2].
        -> list of dicts (poses, points, summary = dict of the ebo_summary fields, and with trace=True trace
        [max_num_iterations + 1][4])."""
        o = opts if opts is not None else default_ba_opts()
        n = len(problems)

        def cat(key, dt, shape):
            parts = [np.asarray(p[key], dtype=dt).reshape(shape) for p in problems]
            return np.ascontiguousarray(np.concatenate(parts), dtype=dt) if parts else np.zeros((0,) + tuple(shape[1:]), dt)

        off = lambda key, div: np.ascontiguousarray(np.concatenate(
            [[0], np.cumsum([np.asarray(p[key]).size // div for p in problems])]), dtype=np.int32)
        fo, po, oo = off("poses", 12), off("points", 3), off("of", 1)
        poses, fixed, points = cat("poses", np.float64, (-1, 12)), cat("fixed", np.uint8, (-1,)), cat("points", np.float64, (-1, 3))
        of, op, uv = cat("of", np.int32, (-1,)), cat("op", np.int32, (-1,)), cat("uv", np.float64, (-1, 2))
        summ = (Summary * max(n, 1))()
        rows = int(o.max_num_iterations) + 1
        tr = np.zeros((max(n, 1), max(rows, 1), 4)) if trace else None
        cam = camera(cam)
        self._check(lib().ebo_bundle_adjust(self._h, n, _vp(fo), _vp(po), _vp(oo), _vp(poses), _vp(fixed), _vp(points), _vp(of),
                                            _vp(op), _vp(uv), C.addressof(cam), C.c_double(huber), 1 if fix_points else 0,
                                            C.addressof(o), C.addressof(summ), _vp(tr) if trace else None))
        out = []
        for k in range(n):
            s = summ[k]
            d = dict(poses=poses[fo[k]:fo[k + 1]].reshape(-1, 3, 4).copy(), points=points[po[k]:po[k + 1]].copy(),
                     summary={f: getattr(s, f) for f, _ in Summary._fields_})
            if trace:
                d["trace"] = tr[k].copy()
            out.append(d)
        return out

    def bundle_adjust_device(self, frame_offsets, point_offsets, obs_offsets, d_poses, d_fixed, d_points, d_of, d_op, d_uv, cam,
                             huber, fix_points=False, opts=None, d_trace=0):
        """ebo_bundle_adjust_device: host int32 offsets, device pointers as int (observations already in (point, frame)
        order); poses and points are updated in place on the device.  -> list of summary dicts."""
        o = opts if opts is not None else default_ba_opts()
        fo, po, oo = (np.ascontiguousarray(v, dtype=np.int32).reshape(-1) for v in (frame_offsets, point_offsets, obs_offsets))
        n = len(fo) - 1
        summ = (Summary * max(n, 1))()
        cam = camera(cam)
        p = lambda v: C.c_void_p(int(v)) if v else None
        self._check(lib().ebo_bundle_adjust_device(self._h, n, _vp(fo), _vp(po), _vp(oo), p(d_poses), p(d_fixed), p(d_points),
                                                   p(d_of), p(d_op), p(d_uv), C.addressof(cam), C.c_double(huber),
                                                   1 if fix_points else 0, C.addressof(o), C.addressof(summ), p(d_trace)))
        return [{f: getattr(summ[k], f) for f, _ in Summary._fields_} for k in range(n)]

    # -- relative-pose refinement (five-variable LM over each pair's RANSAC inliers) ---------------------
    def relative_pose_refine(self, pairs, opts=None, trace=False):
        """ebo_relative_pose_refine over a list of pairs, each a dict of model float64 [3][4], f1 / f2 [n][3] and idx
        int [m] (the listed inliers, indices within the pair).  -> list of dicts (model, summary = dict of the
        ebo_summary fields, and with trace=True trace [max_num_iterations + 1][4])."""
        o = opts if opts is not None else default_ba_opts()
        n = len(pairs)
        sizes = [np.asarray(p["f1"]).size // 3 for p in pairs]
        off = np.ascontiguousarray(np.concatenate([[0], np.cumsum(sizes)]), dtype=np.int32)
        total = int(off[-1])
        f1 = np.zeros((max(total, 1), 3))
        f2 = np.zeros((max(total, 1), 3))
        idx = np.zeros(max(total, 1), dtype=np.int32)
        cnt = np.zeros(max(n, 1), dtype=np.int32)
        models = np.zeros((max(n, 1), 12))
        for k, p in enumerate(pairs):
            f1[off[k]:off[k + 1]] = np.asarray(p["f1"], dtype=np.float64).reshape(-1, 3)
            f2[off[k]:off[k + 1]] = np.asarray(p["f2"], dtype=np.float64).reshape(-1, 3)
            li = np.asarray(p["idx"], dtype=np.int32).reshape(-1)
            if len(li) > sizes[k]:
                raise ValueError("a pair lists more inliers than it holds correspondences")
            idx[off[k]:off[k] + len(li)] = li
            cnt[k] = len(li)
            models[k] = np.asarray(p["model"], dtype=np.float64).reshape(12)
        summ = (Summary * max(n, 1))()
        rows = int(o.max_num_iterations) + 1
        tr = np.zeros((max(n, 1), max(rows, 1), 4)) if trace else None
        self._check(lib().ebo_relative_pose_refine(self._h, n, _vp(off), _vp(f1), _vp(f2), _vp(models), _vp(cnt), _vp(idx),
                                                   C.addressof(o), C.addressof(summ), _vp(tr) if trace else None))
        out = []
        for k in range(n):
            d = dict(model=models[k].reshape(3, 4).copy(), summary={f: getattr(summ[k], f) for f, _ in Summary._fields_})
            if trace:
                d["trace"] = tr[k].copy()
            out.append(d)
        return out

    def relative_pose_refine_device(self, offsets, d_f1, d_f2, d_models, n_inliers, d_inlier_idx, opts=None, d_trace=0):
        """ebo_relative_pose_refine_device: host int32 offsets and inlier counts, device pointers as int; the models are
        updated in place on the device.  -> list of summary dicts."""
        o = opts if opts is not None else default_ba_opts()
        off = np.ascontiguousarray(offsets, dtype=np.int32).reshape(-1)
        cnt = np.ascontiguousarray(n_inliers, dtype=np.int32).reshape(-1)
        n = len(off) - 1
        if len(cnt) != n:
            raise ValueError("n_inliers must hold one count per pair")
        summ = (Summary * max(n, 1))()
        p = lambda v: C.c_void_p(int(v)) if v else None
        self._check(lib().ebo_relative_pose_refine_device(self._h, n, _vp(off), p(d_f1), p(d_f2), p(d_models), _vp(cnt),
                                                          p(d_inlier_idx), C.addressof(o), C.addressof(summ), p(d_trace)))
        return [{f: getattr(summ[k], f) for f, _ in Summary._fields_} for k in range(n)]

    # -- trajectory alignment (Sim3 / SE3 of estimated centres onto ground truth, and the ATE) -------------
    @staticmethod
    def _align_out(res, n):
        return [dict(scale=np.float64(r.scale), R=np.array(r.R[:], dtype=np.float64).reshape(3, 3),
                     t=np.array(r.t[:], dtype=np.float64), rmse=np.float64(r.rmse), mean=np.float64(r.mean),
                     min=np.float64(r.min), max=np.float64(r.max), count=int(r.count), status=int(r.status))
                for r in res[:n]]

    def align_sim3(self, data, model, segments, fix_scale=False):
        """ebo_align_sim3: data (the ground-truth centres) and model (the estimated centres) float64 [n][3]; segments a
        list of (begin, end) over both, which may overlap.  The fit is data ~ s R model + t.  -> one dict per segment:
        scale, R [3][3], t [3], rmse, mean, min, max, count, status (0 aligned, 1 fewer than 3 points, 2 a non-finite
        input, 3 degenerate)."""
        data = np.ascontiguousarray(data, dtype=np.float64).reshape(-1, 3)
        model = np.ascontiguousarray(model, dtype=np.float64).reshape(-1, 3)
        if len(data) != len(model):
            raise ValueError("data and model must hold the same number of points")
        seg = np.asarray(segments, dtype=np.int32).reshape(-1, 2)
        sb, se = np.ascontiguousarray(seg[:, 0]), np.ascontiguousarray(seg[:, 1])
        n = len(seg)
        res = (AlignResult * max(n, 1))()
        self._check(lib().ebo_align_sim3(self._h, len(data), _vp(data) if len(data) else None,
                                         _vp(model) if len(model) else None, n, _vp(sb) if n else None,
                                         _vp(se) if n else None, 1 if fix_scale else 0, C.addressof(res)))
        return self._align_out(res, n)

    def align_sim3_device(self, n_points, d_data, d_model, segments, fix_scale=False):
        """ebo_align_sim3_device: device pointers as int for data and model; the segments and the results stay on the
        host.  -> as align_sim3."""
        seg = np.asarray(segments, dtype=np.int32).reshape(-1, 2)
        sb, se = np.ascontiguousarray(seg[:, 0]), np.ascontiguousarray(seg[:, 1])
        n = len(seg)
        res = (AlignResult * max(n, 1))()
        p = lambda v: C.c_void_p(int(v)) if v else None
        self._check(lib().ebo_align_sim3_device(self._h, int(n_points), p(d_data), p(d_model), n, _vp(sb) if n else None,
                                                _vp(se) if n else None, 1 if fix_scale else 0, C.addressof(res)))
        return self._align_out(res, n)

    # -- relative pose error (the drift per step of an estimated trajectory, beside the ATE) -----------------
    RPE_FIELDS = ("trans_rmse", "trans_mean", "trans_min", "trans_max", "rot_rmse", "rot_mean", "rot_min", "rot_max")

    @staticmethod
    def _rpe_args(segments, deltas, scales):
        seg = np.asarray(segments, dtype=np.int32).reshape(-1, 2)
        sb, se = np.ascontiguousarray(seg[:, 0]), np.ascontiguousarray(seg[:, 1])
        dl = np.ascontiguousarray(deltas, dtype=np.int32).reshape(-1)
        sc = None
        if scales is not None:
            sc = np.ascontiguousarray(scales, dtype=np.float64).reshape(-1)
            if len(sc) != len(seg):
                raise ValueError("one scale per segment")
        return sb, se, dl, sc

    @classmethod
    def _rpe_out(cls, res, n, deltas):
        nd = len(deltas)
        out = []
        for u in range(n * nd):
            r = res[u]
            d = {f: np.float64(getattr(r, f)) for f in cls.RPE_FIELDS}
            d.update(count=int(r.count), status=int(r.status), segment=u // nd, delta=int(deltas[u % nd]))
            out.append(d)
        return out

    def trajectory_rpe(self, gt, est, segments, deltas, scales=None):
        """ebo_trajectory_rpe: gt (the ground-truth poses) and est (the estimated poses) float64 [n][3][4], camera to
        world; segments a list of (begin, end) over both, which may overlap; deltas the steps (>= 1) every segment is
        evaluated at; scales one factor per segment for the estimate's translations (None: 1).  -> one dict per
        (segment, delta), segment-major: trans_rmse, trans_mean, trans_min, trans_max, rot_rmse, rot_mean, rot_min,
        rot_max (radians), count (pairs), status (0 evaluated, 1 no pair, 2 a non-finite input), segment, delta."""
        gt = np.ascontiguousarray(gt, dtype=np.float64).reshape(-1, 3, 4)
        est = np.ascontiguousarray(est, dtype=np.float64).reshape(-1, 3, 4)
        if len(gt) != len(est):
            raise ValueError("gt and est must hold the same number of poses")
        sb, se, dl, sc = self._rpe_args(segments, deltas, scales)
        n, nd = len(sb), len(dl)
        res = (RpeResult * max(n * nd, 1))()
        self._check(lib().ebo_trajectory_rpe(self._h, len(gt), _vp(gt) if len(gt) else None, _vp(est) if len(est) else None, n,
                                             _vp(sb) if n else None, _vp(se) if n else None, _vp(sc) if sc is not None and n else None,
                                             nd, _vp(dl) if nd else None, C.addressof(res)))
        return self._rpe_out(res, n, dl)

    def trajectory_rpe_device(self, n_poses, d_gt, d_est, segments, deltas, scales=None):
        """ebo_trajectory_rpe_device: device pointers as int for gt and est; the segments, deltas, scales and the results
        stay on the host.  -> as trajectory_rpe."""
        sb, se, dl, sc = self._rpe_args(segments, deltas, scales)
        n, nd = len(sb), len(dl)
        res = (RpeResult * max(n * nd, 1))()
        p = lambda v: C.c_void_p(int(v)) if v else None
        self._check(lib().ebo_trajectory_rpe_device(self._h, int(n_poses), p(d_gt), p(d_est), n, _vp(sb) if n else None,
                                                    _vp(se) if n else None, _vp(sc) if sc is not None and n else None, nd,
                                                    _vp(dl) if nd else None, C.addressof(res)))
        return self._rpe_out(res, n, dl)

    # -- landmark maintenance (N-view triangulation of whole observation lists, the audit of landmarks) --------
    LANDMARK_DOUBLES = ("parallax", "score_max")
    LANDMARK_INTS = ("status", "n_obs", "n_inliers", "winner", "hypotheses")

    @staticmethod
    def landmark_params(**kw):
        """ebo_default_landmark_params with the given fields replaced -> LandmarkParams."""
        p = LandmarkParams()
        lib().ebo_default_landmark_params(C.byref(p))
        for k, v in kw.items():
            if not hasattr(p, k):
                raise ValueError("no landmark parameter " + k)
            setattr(p, k, v)
        return p

    LANDMARK_DTYPE = np.dtype([("point", np.float64, 3), ("parallax", np.float64), ("score_max", np.float64), ("status", np.int32),
                               ("n_obs", np.int32), ("n_inliers", np.int32), ("winner", np.int32), ("hypotheses", np.int32),
                               ("reserved", np.int32)])

    @classmethod
    def _landmark_out(cls, res, n):
        rec = np.frombuffer(res, dtype=cls.LANDMARK_DTYPE, count=n)
        return {f: rec[f].copy() for f in ("point",) + cls.LANDMARK_DOUBLES + cls.LANDMARK_INTS}

    def _landmarks(self, solve, poses, obs_offsets, obs_pose, obs_f, points, params, want_scores, want_flags):
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3, 4)
        off = np.ascontiguousarray(obs_offsets, dtype=np.int32).reshape(-1)
        if len(off) < 1:
            raise ValueError("obs_offsets holds n_landmarks + 1 entries")
        n = len(off) - 1
        idx = np.ascontiguousarray(obs_pose, dtype=np.int32).reshape(-1)
        f = np.ascontiguousarray(obs_f, dtype=np.float64).reshape(-1, 3)
        total = max(int(off[-1]), 0)
        if len(idx) < total or len(f) < total:
            raise ValueError("obs_pose and obs_f hold obs_offsets[-1] observations")
        prm = params if params is not None else self.landmark_params()
        res = (LandmarkResult * max(n, 1))()
        scores = np.zeros(total) if want_scores else None
        flags = np.zeros(total, dtype=np.uint8) if want_flags else None
        args = [self._h, len(poses), _vp(poses) if len(poses) else None, n, _vp(off), _vp(idx) if total else None,
                _vp(f) if total else None]
        if not solve:
            pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
            if len(pts) != n:
                raise ValueError("one point per landmark")
            args.append(_vp(pts) if n else None)
        args += [C.byref(prm), C.addressof(res), _vp(scores) if want_scores and total else None,
                 _vp(flags) if want_flags and total else None]
        self._check((lib().ebo_triangulate_tracks if solve else lib().ebo_landmark_scores)(*args))
        out = self._landmark_out(res, n)
        if want_scores:
            out["scores"] = scores
        if want_flags:
            out["flags"] = flags
        return out

    def triangulate_tracks(self, poses, obs_offsets, obs_pose, obs_f, params=None, scores=True, flags=True):
        """ebo_triangulate_tracks: poses float64 [n_poses][3][4], camera to world; landmark l owns observations
        obs_offsets[l] .. obs_offsets[l + 1] - 1 of obs_pose (int32 pose indices) and obs_f (float64 [.][3] bearing
        vectors).  Consensus over two-observation hypotheses, least squares over the winner's inliers (L1-L6 of
        include/ebo.h).  -> dict of arrays with one row per landmark: point [n][3], parallax, score_max, status, n_obs,
        n_inliers, winner, hypotheses; and per observation `scores` and `flags` (unless switched off)."""
        return self._landmarks(True, poses, obs_offsets, obs_pose, obs_f, None, params, scores, flags)

    def landmark_scores(self, poses, obs_offsets, obs_pose, obs_f, points, params=None, scores=True, flags=True):
        """ebo_landmark_scores: the audit (L7) of the given points float64 [n_landmarks][3] against their observations
        under the given poses.  -> as triangulate_tracks; status 0 keeps a landmark."""
        return self._landmarks(False, poses, obs_offsets, obs_pose, obs_f, points, params, scores, flags)

    def _landmarks_device(self, solve, n_poses, d_poses, obs_offsets, d_obs_pose, d_obs_f, d_points, params, d_results, d_scores, d_flags):
        off = np.ascontiguousarray(obs_offsets, dtype=np.int32).reshape(-1)
        if len(off) < 1:
            raise ValueError("obs_offsets holds n_landmarks + 1 entries")
        prm = params if params is not None else self.landmark_params()
        p = lambda v: C.c_void_p(int(v)) if v else None
        args = [self._h, int(n_poses), p(d_poses), len(off) - 1, _vp(off), p(d_obs_pose), p(d_obs_f)]
        if not solve:
            args.append(p(d_points))
        args += [C.byref(prm), p(d_results), p(d_scores), p(d_flags)]
        self._check((lib().ebo_triangulate_tracks_device if solve else lib().ebo_landmark_scores_device)(*args))

    def triangulate_tracks_device(self, n_poses, d_poses, obs_offsets, d_obs_pose, d_obs_f, d_results, params=None, d_scores=None,
                                  d_flags=None):
        """ebo_triangulate_tracks_device: device pointers as int; obs_offsets and params stay on the host; d_results
        receives n_landmarks ebo_landmark_result records (64 bytes each).  Asynchronous on the context's stream."""
        self._landmarks_device(True, n_poses, d_poses, obs_offsets, d_obs_pose, d_obs_f, None, params, d_results, d_scores, d_flags)

    def landmark_scores_device(self, n_poses, d_poses, obs_offsets, d_obs_pose, d_obs_f, d_points, d_results, params=None,
                               d_scores=None, d_flags=None):
        """ebo_landmark_scores_device: as triangulate_tracks_device with the points on the device."""
        self._landmarks_device(False, n_poses, d_poses, obs_offsets, d_obs_pose, d_obs_f, d_points, params, d_results, d_scores, d_flags)

    @classmethod
    def landmark_results(cls, raw):
        """The bytes of n ebo_landmark_result records (a uint8 array copied back from the device) -> the dict of
        triangulate_tracks without scores and flags."""
        raw = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1)
        n = raw.size // cls.LANDMARK_DTYPE.itemsize
        return cls._landmark_out(raw[:n * cls.LANDMARK_DTYPE.itemsize].tobytes(), n)

    # -- angular velocity from events (rotational contrast maximisation, rules V1-V9 / N1-N5) ----------------
    def _rot_args(self, cam, params):
        return camera(cam), params if params is not None else RotationParams()

    def eval_rotation(self, cam, omegas, params=None, want_grad=True):
        """ebo_eval_rotation: omegas float64 [Wn][3] in rad/s -> (r [Wn], g [Wn][3] or None)."""
        k, prm = self._rot_args(cam, params)
        om = np.ascontiguousarray(omegas, dtype=np.float64).reshape(self.n_windows, 3)
        r = np.zeros(self.n_windows)
        g = np.zeros((self.n_windows, 3)) if want_grad else None
        self._check(lib().ebo_eval_rotation(self._h, C.addressof(k), C.addressof(prm), _dp(om), _dp(r), _dp(g) if want_grad else None))
        return r, g

    def eval_rotation_device(self, cam, d_omegas, d_r, d_g=0, params=None):
        """ebo_eval_rotation_device: device pointers as int; asynchronous on the context's stream."""
        k, prm = self._rot_args(cam, params)
        p = lambda v: C.c_void_p(int(v)) if v else None
        self._check(lib().ebo_eval_rotation_device(self._h, C.addressof(k), C.addressof(prm), p(d_omegas), p(d_r), p(d_g)))

    def rotation_image(self, cam, omegas, votes=True, image=True):
        """ebo_rotation_image -> (H int64 [Wn][h][w] or None, F float64 [Wn][h][w] or None)."""
        k = camera(cam)
        om = np.ascontiguousarray(omegas, dtype=np.float64).reshape(self.n_windows, 3)
        shape = (self.n_windows, self.params.image_h, self.params.image_w)
        Hq = np.zeros(shape, dtype=np.int64) if votes else None
        F = np.zeros(shape) if image else None
        self._check(lib().ebo_rotation_image(self._h, C.addressof(k), _dp(om), _vp(Hq) if votes else None, _dp(F) if image else None))
        return Hq, F

    def solve_rotation(self, cam, params=None, opts=None, omega0=None):
        """ebo_solve_rotation from omega0 ([Wn][3], None: zeros) -> (omega [Wn][3], [RotSummary] * Wn)."""
        k, prm = self._rot_args(cam, params)
        o0 = None if omega0 is None else np.ascontiguousarray(omega0, dtype=np.float64).reshape(self.n_windows, 3)
        out = np.zeros((self.n_windows, 3))
        summ = (RotSummary * self.n_windows)()
        self._check(lib().ebo_solve_rotation(self._h, C.addressof(k), C.addressof(prm), C.byref(opts) if opts is not None else None,
                                             _dp(o0) if o0 is not None else None, _dp(out), summ))
        return out, list(summ)

    # -- pose from events against a map (map-to-event-image alignment, rules E1-E9) ------------------------
    def event_images(self, cam, omegas=None, params=None):
        """ebo_event_images: the blurred event image B float64 [Wn][h][w] of every resident window at omegas [Wn][3]
        (None: zeros, the un-warped count image blurred)."""
        k, prm = self._rot_args(cam, params)
        om = None if omegas is None else np.ascontiguousarray(omegas, dtype=np.float64).reshape(self.n_windows, 3)
        out = np.zeros((self.n_windows, self.params.image_h, self.params.image_w))
        self._check(lib().ebo_event_images(self._h, C.addressof(k), C.addressof(prm), _dp(om) if om is not None else None, _dp(out)))
        return out

    def event_images_device(self, cam, d_images, d_omegas=0, params=None):
        """ebo_event_images_device: device pointers as int; asynchronous on the context's stream."""
        k, prm = self._rot_args(cam, params)
        p = lambda v: C.c_void_p(int(v)) if v else None
        self._check(lib().ebo_event_images_device(self._h, C.addressof(k), C.addressof(prm), p(d_omegas), p(d_images)))

    def map_track(self, cam, images, points, unit_image, poses, z_min=0.05, opts=None, trace=False):
        """ebo_map_track: images float64 [n][h][w], points [P][3], unit_image int [U], poses [U][12] (camera to world, R
        row-major, then t) -> (poses [U][12], list of result dicts, trace [U][max_num_iterations + 1][4] or None)."""
        o = opts if opts is not None else default_map_track_opts()
        k = camera(cam)
        im = np.ascontiguousarray(images, dtype=np.float64)
        assert im.ndim == 3, im.shape
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        ui = np.ascontiguousarray(unit_image, dtype=np.int32).reshape(-1)
        po = np.array(poses, dtype=np.float64).reshape(-1, 12)
        n = len(ui)
        if len(po) != n:
            raise ValueError("one pose per unit")
        res = (MapTrackResult * max(n, 1))()
        tr = np.zeros((max(n, 1), int(o.max_num_iterations) + 1, 4)) if trace else None
        self._check(lib().ebo_map_track(self._h, C.addressof(k), im.shape[2], im.shape[1], im.shape[0], _dp(im) if im.size else None,
                                        len(pts), _dp(pts) if len(pts) else None, n, _vp(ui) if n else None, _dp(po) if n else None,
                                        C.c_double(z_min), C.addressof(o), C.addressof(res), _dp(tr) if trace else None))
        out = [{f: getattr(res[u], f) for f in MAP_TRACK_FIELDS} for u in range(n)]
        return po, out, (tr[:n] if trace else None)

    def map_track_resident(self, cam, points, unit_window, poses, make_images=True, omegas=None, params=None, z_min=0.05, opts=None,
                           trace=False):
        """ebo_map_track_resident: map_track against the blurred event images of the RESIDENT windows, which are made on the
        device (make_images) and kept there for later calls; unit_window names a resident window per unit."""
        o = opts if opts is not None else default_map_track_opts()
        k, prm = self._rot_args(cam, params)
        om = None if omegas is None else np.ascontiguousarray(omegas, dtype=np.float64).reshape(self.n_windows, 3)
        pts = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
        ui = np.ascontiguousarray(unit_window, dtype=np.int32).reshape(-1)
        po = np.array(poses, dtype=np.float64).reshape(-1, 12)
        n = len(ui)
        res = (MapTrackResult * max(n, 1))()
        tr = np.zeros((max(n, 1), int(o.max_num_iterations) + 1, 4)) if trace else None
        self._check(lib().ebo_map_track_resident(self._h, C.addressof(k), C.addressof(prm), _dp(om) if om is not None else None,
                                                 1 if make_images else 0, len(pts), _dp(pts) if len(pts) else None, n,
                                                 _vp(ui) if n else None, _dp(po) if n else None, C.c_double(z_min), C.addressof(o),
                                                 C.addressof(res), _dp(tr) if trace else None))
        out = [{f: getattr(res[u], f) for f in MAP_TRACK_FIELDS} for u in range(n)]
        return po, out, (tr[:n] if trace else None)

    def map_track_device(self, cam, w, h, n_images, d_images, n_points, d_points, n_units, d_unit_image, d_poses, d_results,
                         z_min=0.05, opts=None, d_trace=0):
        """ebo_map_track_device: device pointers as int; poses are updated in place, d_results receives n_units
        ebo_map_track_result records (MAP_TRACK_DTYPE, 64 bytes each).  Asynchronous on the context's stream."""
        o = opts if opts is not None else default_map_track_opts()
        k = camera(cam)
        p = lambda v: C.c_void_p(int(v)) if v else None
        self._check(lib().ebo_map_track_device(self._h, C.addressof(k), int(w), int(h), int(n_images), p(d_images), int(n_points),
                                               p(d_points), int(n_units), p(d_unit_image), p(d_poses), C.c_double(z_min),
                                               C.addressof(o), p(d_results), p(d_trace)))

    @staticmethod
    def map_track_results(raw):
        """The bytes of ebo_map_track_result records copied back from the device -> list of result dicts."""
        a = np.ascontiguousarray(raw, dtype=np.uint8).reshape(-1).view(MAP_TRACK_DTYPE)
        return [{f: a[f][u].item() for f in MAP_TRACK_FIELDS} for u in range(len(a))]

    # -- depth from events (space-sweep voting, rules M1-M9) --------------------------------------------------
    def dsi_begin(self, cam, ref_pose, params=None):
        """ebo_dsi_begin: opens and clears the volume of a reference view; ref_pose 12 doubles (R row-major, t)."""
        k = camera(cam)
        ref = np.ascontiguousarray(ref_pose, dtype=np.float64).reshape(12)
        prm = params if params is not None else default_depth_params()
        self._check(lib().ebo_dsi_begin(self._h, C.addressof(k), _dp(ref), C.addressof(prm)))
        self._dsi_prm = prm  # a refused begin leaves the open volume, and its shape, as they were

    def dsi_add_windows(self, poses, use=None):
        """ebo_dsi_add_windows: votes the resident windows; poses [Wn][12], use [Wn] (None: all)."""
        po = np.ascontiguousarray(poses, dtype=np.float64).reshape(self.n_windows, 12)
        u = None if use is None else np.ascontiguousarray(use, dtype=np.uint8).reshape(self.n_windows)
        self._check(lib().ebo_dsi_add_windows(self._h, _dp(po), _vp(u) if u is not None else None))

    def dsi_volume(self):
        """ebo_dsi_volume -> H uint32 [nz][h][w]"""
        prm = getattr(self, "_dsi_prm", None)  # None: no begin yet, the call is refused before it writes
        Hq = np.zeros((prm.nz if prm else 1, self.params.image_h, self.params.image_w), dtype=np.uint32)
        self._check(lib().ebo_dsi_volume(self._h, _vp(Hq)))
        return Hq

    def dsi_depth(self, max_points=None):
        """ebo_dsi_depth -> (index int32 [h][w], conf uint32 [h][w], depth [h][w], points [min(n, max_points)][3], n);
        max_points None: every kept pixel."""
        h, w = self.params.image_h, self.params.image_w
        cap = h * w if max_points is None else int(max_points)
        index = np.zeros((h, w), dtype=np.int32)
        conf = np.zeros((h, w), dtype=np.uint32)
        depth = np.zeros((h, w))
        points = np.zeros((max(cap, 1), 3))
        n = C.c_int(0)
        self._check(lib().ebo_dsi_depth(self._h, _vp(index), _vp(conf), _dp(depth), _dp(points), cap, C.byref(n)))
        return index, conf, depth, points[:min(n.value, cap)], n.value

    def dsi_end(self):
        self._check(lib().ebo_dsi_end(self._h))

    # -- track evaluation (KLT reference tracks on the frames, track error and feature age) ------------------
    def reference_tracks(self, frames, frame_t_us, seed_frame, seed_xy, win=(21, 21), max_level=3, max_count=30, epsilon=0.01,
                         min_eig_threshold=1e-4):
        """ebo_reference_tracks: frames uint8 [F][h][w] at the context's size, seeds as track_seeds returns them; the
        others are lk_track's parameters.  -> (first int32 [n], last int32 [n], xy float64 [n][F][2], 0 outside
        [first, last]).  The context's last two images are then the last two frames."""
        fr = np.ascontiguousarray(frames, dtype=np.uint8)
        assert fr.ndim == 3 and fr.shape[1:] == (self.params.image_h, self.params.image_w), fr.shape
        ft = np.ascontiguousarray(frame_t_us, dtype=np.int64).reshape(-1)
        if len(ft) != len(fr):
            raise ValueError("one time per frame")
        sf = np.ascontiguousarray(seed_frame, dtype=np.int32).reshape(-1)
        sx = np.ascontiguousarray(seed_xy, dtype=np.float32).reshape(-1, 2)
        if len(sf) != len(sx):
            raise ValueError("one position per seed")
        n, F = len(sf), len(fr)
        first = np.zeros(max(n, 1), dtype=np.int32)
        last = np.zeros(max(n, 1), dtype=np.int32)
        xy = np.zeros((max(n, 1), max(F, 1), 2), dtype=np.float64)
        lk = LkParams(int(win[0]), int(win[1]), int(max_level), int(max_count), float(epsilon), float(min_eig_threshold))
        self._check(lib().ebo_reference_tracks(self._h, F, _vp(fr) if F else None, _vp(ft) if F else None, n, _vp(sf), _vp(sx),
                                               C.addressof(lk), _vp(first), _vp(last), _vp(xy)))
        return first[:n], last[:n], xy[:n, :F]

    @staticmethod
    def _track_error_out(res, n, taus):
        nt = len(taus)
        out = []
        for u in range(n * nt):
            r = res[u]
            d = {f: np.float64(getattr(r, f)) for f in TRACK_ERROR_FIELDS}
            d.update({f: int(getattr(r, f)) for f in TRACK_ERROR_INTS})
            d.update(track=u // nt, tau=np.float64(taus[u % nt]))
            out.append(d)
        return out

    def track_errors(self, est_tracks, gt_tracks, taus, sample_errors=False):
        """ebo_track_errors: est_tracks and gt_tracks lists of (t_us int64 [n], xy float64 [n][2]), one ground-truth
        track per estimated track; taus the thresholds in pixels (at most 8).  -> one dict per (track, tau),
        track-major: err_mean, err_rmse, err_max (over the inliers), age_us, t_first_us, n_inliers, n_comparable, first,
        cut (-1: never beyond tau), status (0 evaluated, 1 nothing to compare, 2 a non-finite coordinate), track, tau;
        with sample_errors also float64 [n_est], each estimated sample's error, -1 where it has none."""
        if len(est_tracks) != len(gt_tracks):
            raise ValueError("one ground-truth track per estimated track")
        eo, et, exy = _pack_tracks(est_tracks)
        go, gt, gxy = _pack_tracks(gt_tracks)
        ta = np.ascontiguousarray(taus, dtype=np.float64).reshape(-1)
        n, nt = len(est_tracks), len(ta)
        res = (TrackErrorResult * max(n * nt, 1))()
        per = np.zeros(max(len(et), 1), dtype=np.float64) if sample_errors else None
        self._check(lib().ebo_track_errors(self._h, n, _vp(eo), _vp(et) if len(et) else None, _vp(exy) if len(et) else None,
                                           _vp(go), _vp(gt) if len(gt) else None, _vp(gxy) if len(gt) else None, nt,
                                           _vp(ta) if nt else None, C.addressof(res), _vp(per) if sample_errors else None))
        out = self._track_error_out(res, n, ta)
        return (out, per[:len(et)]) if sample_errors else out

    def track_errors_device(self, est_off, d_est_t, d_est_xy, gt_off, d_gt_t, d_gt_xy, taus, d_sample_err=0):
        """ebo_track_errors_device: device pointers as int for the four sample arrays (int64 times, float64 [.][2]
        positions) and the per-sample errors; the offsets (int32 [n_tracks + 1]), taus and the results stay on the host.
        -> as track_errors."""
        eo = np.ascontiguousarray(est_off, dtype=np.int32).reshape(-1)
        go = np.ascontiguousarray(gt_off, dtype=np.int32).reshape(-1)
        if len(eo) != len(go) or len(eo) < 1:
            raise ValueError("est_off and gt_off hold n_tracks + 1 entries each")
        ta = np.ascontiguousarray(taus, dtype=np.float64).reshape(-1)
        n, nt = len(eo) - 1, len(ta)
        res = (TrackErrorResult * max(n * nt, 1))()
        p = lambda v: C.c_void_p(int(v)) if v else None
        self._check(lib().ebo_track_errors_device(self._h, n, _vp(eo), p(d_est_t), p(d_est_xy), _vp(go), p(d_gt_t), p(d_gt_xy), nt,
                                                  _vp(ta) if nt else None, C.addressof(res), p(d_sample_err)))
        return self._track_error_out(res, n, ta)

    def triangulate(self, poses, pose_pair, f1, f2):
        """ebo_triangulate: poses float64 [n_poses][3][4] camera-to-world, pose_pair int [n][2] -> world points [n][3]."""
        poses = np.ascontiguousarray(poses, dtype=np.float64).reshape(-1, 3, 4)
        pose_pair = np.ascontiguousarray(pose_pair, dtype=np.int32).reshape(-1, 2)
        f1 = np.ascontiguousarray(f1, dtype=np.float64).reshape(-1, 3)
        f2 = np.ascontiguousarray(f2, dtype=np.float64).reshape(-1, 3)
        n = len(f1)
        out = np.zeros((n, 3))
        self._check(lib().ebo_triangulate(self._h, len(poses), _vp(poses), n, _vp(pose_pair), _vp(f1), _vp(f2), _vp(out)))
        return out

    def triangulate_device(self, n_poses, d_poses, n, d_pose_pair, d_f1, d_f2, d_points):
        p = lambda v: C.c_void_p(int(v)) if v else None
        self._check(lib().ebo_triangulate_device(self._h, int(n_poses), p(d_poses), int(n), p(d_pose_pair), p(d_f1), p(d_f2),
                                                 p(d_points)))

    def epipolar_inliers(self, model, f1, f2, threshold):
        """ebo_epipolar_inliers: |f1^T E f2| < threshold with E = hat(t / |t|) R -> bool [n]."""
        model = np.ascontiguousarray(model, dtype=np.float64).reshape(3, 4)
        f1 = np.ascontiguousarray(f1, dtype=np.float64).reshape(-1, 3)
        f2 = np.ascontiguousarray(f2, dtype=np.float64).reshape(-1, 3)
        fl = np.zeros(len(f1), dtype=np.uint8)
        self._check(lib().ebo_epipolar_inliers(self._h, _vp(model), len(f1), _vp(f1), _vp(f2), C.c_double(threshold), _vp(fl)))
        return fl.astype(bool)

    # -- timing --------------------------------------------------------------
    def timer_begin(self):
        self._check(lib().ebo_timer_begin(self._h))

    def timer_end(self):
        ms = C.c_float()
        self._check(lib().ebo_timer_end(self._h, C.byref(ms)))
        return ms.value
