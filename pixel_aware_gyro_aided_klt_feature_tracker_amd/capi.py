"""ctypes binding of include/pagk.h (libpagk_hip.so, built by __graft_entry__.build()).

This is the only way Python reaches the product.  There is no CPU fallback: if the
shared library is missing, or no HIP device can be opened, the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

PKG_DIR = os.path.dirname(os.path.abspath(__file__))
# PAGK_LIB: an alternative build of the same library (same-session A/B runs of tools/ab_lib.py; never a CPU path)
LIB_PATH = os.environ.get("PAGK_LIB") or os.path.join(PKG_DIR, "libpagk_hip.so")

PAGK_OK = 0
PAGK_E_ARG = -1
PAGK_E_HIP = -2
PAGK_E_NOMEM = -3
PAGK_E_UNSUPPORTED = -4
PAGK_E_NODEVICE = -5
PAGK_E_NCCL = -6
PAGK_E_CAPACITY = -7
PAGK_INVERSE_TEMPLATE = 2   # pagk_params::inverse: the template-Jacobian mode (include/pagk.h)


class Image(C.Structure):
    _fields_ = [("data", C.c_void_p), ("width", C.c_int32), ("height", C.c_int32), ("step", C.c_int64)]


class Params(C.Structure):
    _fields_ = [
        ("half_patch", C.c_int32), ("iterations", C.c_int32), ("pyramids", C.c_int32),
        ("has_gyro_predict_initial", C.c_uint8), ("inverse", C.c_uint8),
        ("consider_illumination", C.c_uint8), ("consider_affine", C.c_uint8),
        ("regularization_penalty", C.c_uint8), ("calculate_ncc", C.c_uint8),
        ("predict_method", C.c_uint8), ("solver_variant", C.c_uint8),
        ("lambda_", C.c_float), ("alpha", C.c_float), ("max_distance", C.c_int32),
        ("inv_log_max_dist", C.c_float),
        ("fx", C.c_float), ("fy", C.c_float), ("cx", C.c_float), ("cy", C.c_float),
        ("dist_coef", C.c_float * 5), ("n_dist_coef", C.c_int32),
    ]


class FitParams(C.Structure):
    """pagk_fit_params (include/pagk.h)."""
    _fields_ = [("seed", C.c_uint64), ("iters_H", C.c_int32), ("iters_F", C.c_int32), ("thresh_H", C.c_double),
                ("thresh_F", C.c_double), ("conf_H", C.c_double), ("conf_F", C.c_double)]


class PoseParams(C.Structure):
    """pagk_pose_params (include/pagk.h): the budget and thresholds of the essential matrix and the pose, and the
    pagk_fit_params of the H and F of the same call."""
    _fields_ = [("seed", C.c_uint64), ("iters_E", C.c_int32), ("reserved", C.c_int32), ("thresh_E", C.c_double),
                ("conf_E", C.c_double), ("max_depth", C.c_double), ("fit", FitParams)]


class DetectParams(C.Structure):
    """pagk_detect_params (include/pagk.h): the arguments of the reference's goodFeaturesToTrack call."""
    _fields_ = [("quality_level", C.c_double), ("min_distance", C.c_double), ("harris_k", C.c_double),
                ("raw_cap", C.c_int32)]


class FastParams(C.Structure):
    """pagk_fast_params (include/pagk.h): the ORBextractor constructor arguments the FAST-and-quadtree detector reads."""
    _fields_ = [("ini_threshold", C.c_int32), ("min_threshold", C.c_int32), ("n_features", C.c_int32),
                ("n_levels", C.c_int32)]


class RectifyParams(C.Structure):
    """pagk_rectify_params (include/pagk.h): source channels and the integer RGB-to-gray step behind the remap."""
    _fields_ = [("channels", C.c_int32), ("gray_weight", C.c_int32 * 3), ("gray_shift", C.c_int32)]


class OrbParams(C.Structure):
    """pagk_orb_params (include/pagk.h): the Q8 blur taps, the matcher's distance floor, the number of levels (1)."""
    _fields_ = [("blur_weights", C.c_int32 * 4), ("match_floor", C.c_int32), ("n_levels", C.c_int32)]


class OrbExtractor(C.Structure):
    """pagk_orb_extractor (include/pagk.h): the five constructor arguments of ORBextractor (src/ORBextractor.cc:434-437)."""
    _fields_ = [("n_features", C.c_int32), ("scale_factor", C.c_float), ("n_levels", C.c_int32),
                ("ini_threshold", C.c_int32), ("min_threshold", C.c_int32)]


class LkParams(C.Structure):
    """pagk_lk_params (include/pagk.h): the constants of the reference's calcOpticalFlowPyrLK call and its error filter."""
    _fields_ = [("half_patch", C.c_int32), ("max_level", C.c_int32), ("max_count", C.c_int32), ("epsilon", C.c_double),
                ("min_eig_threshold", C.c_double), ("err_threshold", C.c_float)]


class AssocParams(C.Structure):
    """pagk_assoc_params (include/pagk.h): the constants of MatchFeatures, of the retry of SearchByGyroPredict and of
    SearchByOpencvKLT's association."""
    _fields_ = [("th_ncc_high", C.c_float), ("th_ncc_low", C.c_float), ("th_ratio", C.c_float), ("use_ncc", C.c_int32),
                ("min_matches", C.c_int32), ("klt_max_distance", C.c_float), ("klt_ratio", C.c_double),
                ("klt_disparity_factor", C.c_double)]


ASSOC_INFO_WORDS = 8
ASSOC_STATS_WORDS = 8
ASSOC_MATCH_INFO_FIELDS = ("chosen", "overlong", "out_of_range", "claimed_twice", "matches", "level2_ran")
ASSOC_KLT_INFO_FIELDS = ("live", "no_neighbour", "one_neighbour", "more_neighbours", "ratio_rejects", "lost_to_earlier",
                         "dropped_by_disparity", "matches")
ASSOC_STATS_FIELDS = ("avg1", "avg2", "max1", "max2", "threshold", "sum1", "sum2")
DETECT_INFO_WORDS = 8
ORB_INFO_WORDS = 8
LK_INFO_WORDS = 8


class SequenceParams(C.Structure):
    """pagk_sequence_params (include/pagk.h): the configuration of the sequence a context owns."""
    _fields_ = [("track", Params), ("lk", LkParams), ("fit", FitParams), ("harris", DetectParams), ("fast", FastParams),
                ("new_point_threshold", C.c_double), ("tracker", C.c_int32), ("lk_initial_flow", C.c_int32),
                ("width", C.c_int32), ("height", C.c_int32), ("cap", C.c_int32), ("target_n", C.c_int32),
                ("detector", C.c_int32), ("cand_cap", C.c_int32), ("validate", C.c_int32), ("sigma", C.c_float)]


class ImuWindow(C.Structure):
    """pagk_imu_window (include/pagk.h "Gyro integration"): the gyroscope samples between two frames."""
    _fields_ = [("t_ref", C.c_double), ("t_cur", C.c_double), ("n", C.c_int32), ("t", C.c_void_p), ("w", C.c_void_p),
                ("bias", C.c_float * 3)]


class SequenceSensor(C.Structure):
    """pagk_sequence_sensor (include/pagk.h): what a sensor sequence adds to pagk_sequence_params."""
    _fields_ = [("rectify", RectifyParams), ("raw", C.c_int32), ("src_width", C.c_int32), ("src_height", C.c_int32),
                ("imu_cap", C.c_int32), ("Rbc", C.c_float * 9), ("flow_velocity", C.c_int32)]


RESULTS_PARTS = ("header", "state", "info", "keys", "keys_un", "keys_normal", "index_in_last", "live", "track_id", "age",
                 "velocity", "status", "pt_predict", "pt_predict_un", "err")


class ResultsLayout(C.Structure):
    """pagk_results_layout (include/pagk.h "The result ring of a sequence"): the byte offsets of a record's parts, its size."""
    _fields_ = [(name, C.c_int64) for name in RESULTS_PARTS] + [("bytes", C.c_int64), ("cap", C.c_int32), ("sensor", C.c_int32)]


class SequenceResult(C.Structure):
    """pagk_sequence_result (include/pagk.h): the header of a frame's record and views into its pinned block."""
    _fields_ = [("frame", C.c_int32), ("cap", C.c_int32), ("n_live", C.c_int32), ("n_new", C.c_int32), ("next_id", C.c_int64),
                ("t", C.c_double)] + [(name, C.c_void_p) for name in RESULTS_PARTS[1:]]


# part of a record -> (dtype, columns): what Context.sequence_fetch copies out of the views
RESULTS_ARRAYS = {"keys": (np.float32, 2), "keys_un": (np.float32, 2), "keys_normal": (np.float32, 2),
                  "index_in_last": (np.int32, 1), "live": (np.uint8, 1), "track_id": (np.int64, 1), "age": (np.int32, 1),
                  "velocity": (np.float32, 2), "status": (np.uint8, 1), "pt_predict": (np.float32, 2),
                  "pt_predict_un": (np.float32, 2), "err": (np.float32, 1)}

IMU_MAX_SAMPLES = 64
SEQ_PATCHMATCH, SEQ_LK = 0, 1
SEQ_GRAPH, SEQ_DIRECT = 0, 1
SEQ_STATUS_WORDS = 4
ORB_MAX_LEVELS = 8
ORB_LEVELS_INFO_WORDS = 32
LK_INFO_FIELDS = ("n", "raw", "kept", "top_level", "lost_min_eig", "lost_out_of_range")
ORB_DESCRIBE_INFO_FIELDS = ("described", "outside")
ORB_MATCH_INFO_FIELDS = ("nq", "matches", "kept", "min_dist", "max_dist", "threshold")
DETECT_INFO_FIELDS = ("n_corners", "raw", "overflow", "rmax_bits", "visited")
FAST_INFO_FIELDS = ("n_keypoints", "raw", "first_pass_empty", "empty_cells", "nodes", "passes")
FIT_INFO_WORDS = 12
FIT_INFO_FIELDS = ("status", "best", "best_count", "refit_count", "valid", "adaptive")
POSE_INFO_WORDS = 16
POSE_INFO_FIELDS = ("status", "m", "best_hyp", "best_root", "best_count", "valid_samples", "valid_candidates", "adaptive",
                    "pose", "good0", "good1", "good2", "good3")


class Outputs(C.Structure):
    _fields_ = [("pt_un", C.c_void_p), ("pt_dist", C.c_void_p), ("status", C.c_void_p),
                ("pix_err", C.c_void_p), ("dist_pred", C.c_void_p), ("ncc", C.c_void_p),
                ("iters", C.c_void_p)]


def make_params(*, half_patch=5, iterations=10, pyramids=3, has_gyro=True, illumination=True,
                affine=True, penalty=False, ncc=False, inverse=False, camera=None, predict_method=1,
                solver_variant=0) -> Params:
    """pagk_params_default() (reference call site src/gyro_aided_tracker.cpp:276-282)
    with overrides.  `camera` is a synth.Camera or None."""
    p = Params()
    p.half_patch, p.iterations, p.pyramids = half_patch, iterations, pyramids
    p.has_gyro_predict_initial = int(has_gyro)
    p.inverse = int(inverse)
    p.consider_illumination = int(illumination)
    p.consider_affine = int(affine)
    p.regularization_penalty = int(penalty)
    p.calculate_ncc = int(ncc)
    p.predict_method = int(predict_method)   # 1 PIXEL_AWARE_PREDICTION, 2 SINGLE_HOMOGRAPHY (gyro prediction only)
    p.solver_variant = int(solver_variant)   # Eigen association switches (include/pagk.h); 0 = Eigen 3.3 + SSE2
    p.lambda_, p.alpha, p.max_distance = 1.0, 0.5, 25
    p.inv_log_max_dist = 0.0
    if camera is not None:
        p.fx, p.fy, p.cx, p.cy = camera.fx, camera.fy, camera.cx, camera.cy
        for i, v in enumerate(camera.dist[:5]):
            p.dist_coef[i] = v
        p.n_dist_coef = max(4, len(camera.dist))
    else:
        p.fx = p.fy = 1.0
        p.n_dist_coef = 4
    return p


def params_check(p: Params) -> int:
    """pagk_params_check: the code every tracking entry point returns for these parameters (no device needed)."""
    return int(load().pagk_params_check(C.byref(p)))


def image_view(a: np.ndarray) -> Image:
    assert a.dtype == np.uint8 and a.ndim == 2 and a.strides[1] == 1
    return Image(a.ctypes.data, a.shape[1], a.shape[0], a.strides[0])


def alloc_outputs(n: int, with_iters: bool = True) -> dict:
    nn = max(n, 1)
    d = dict(pt_un=np.zeros((nn, 2), np.float32), pt_dist=np.zeros((nn, 2), np.float32),
             status=np.zeros(nn, np.uint8), pix_err=np.zeros(nn, np.float64),
             dist_pred=np.zeros(nn, np.float64), ncc=np.zeros(nn, np.float32))
    if with_iters:
        d["iters"] = np.zeros(nn, np.int32)
    return d


def outputs_struct(d: dict) -> Outputs:
    o = Outputs()
    for k in ("pt_un", "pt_dist", "status", "pix_err", "dist_pred", "ncc", "iters"):
        v = d.get(k)
        if v is None:
            setattr(o, k, None)
        elif isinstance(v, np.ndarray):
            setattr(o, k, v.ctypes.data)
        else:  # torch tensor (device pointer)
            setattr(o, k, v.data_ptr())
    return o


def _ptr(a):
    """Raw address of a numpy array or a torch tensor.  The C ABI takes dense row-major arrays: anything
    else (a transposed view, a column-major array) is refused here rather than silently mis-read."""
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        if not a.flags.c_contiguous:
            raise ValueError("array must be C-contiguous")
        return a.ctypes.data
    if not a.is_contiguous():
        raise ValueError("tensor must be contiguous")
    return a.data_ptr()


_P = C.POINTER
_lib = None


def declare(lib) -> None:
    """argtypes/restype for every symbol include/pagk.h declares."""
    vp, i32 = C.c_void_p, C.c_int32
    lib.pagk_version.restype = C.c_int
    lib.pagk_version.argtypes = []
    lib.pagk_strerror.restype = C.c_char_p
    lib.pagk_strerror.argtypes = [C.c_int]
    lib.pagk_last_error.restype = C.c_char_p
    lib.pagk_last_error.argtypes = [vp]
    lib.pagk_params_default.restype = None
    lib.pagk_params_default.argtypes = [_P(Params)]
    if hasattr(lib, "pagk_params_check"):   # (an older build given through PAGK_LIB for an A/B run has no such check)
        lib.pagk_params_check.restype = C.c_int
        lib.pagk_params_check.argtypes = [_P(Params)]
    lib.pagk_inv_log_max_dist.restype = C.c_float
    lib.pagk_inv_log_max_dist.argtypes = [C.c_float, i32]
    lib.pagk_create.restype = C.c_int
    lib.pagk_create.argtypes = [_P(vp), C.c_int]
    lib.pagk_destroy.restype = None
    lib.pagk_destroy.argtypes = [vp]
    lib.pagk_track.restype = C.c_int
    lib.pagk_track.argtypes = [vp, _P(Params), _P(Image), _P(Image), i32, vp, vp, vp, vp, _P(Outputs)]
    lib.pagk_track_pyr.restype = C.c_int
    lib.pagk_track_pyr.argtypes = [vp, _P(Params), i32, _P(Image), _P(Image), i32, vp, vp, vp, vp, _P(Outputs)]
    lib.pagk_frame_upload.restype = C.c_int
    lib.pagk_frame_upload.argtypes = [vp, i32, _P(Image), i32]
    if hasattr(lib, "pagk_frame_upload_pinned"):   # (absent from older builds that tools/ab_lib.py loads for A/B runs)
        lib.pagk_frame_upload_pinned.restype = C.c_int
        lib.pagk_frame_upload_pinned.argtypes = [vp, i32, _P(Image), i32]
    lib.pagk_frame_set_device.restype = C.c_int
    lib.pagk_frame_set_device.argtypes = [vp, i32, vp, i32, i32, C.c_int64, i32]
    lib.pagk_frame_download_level.restype = C.c_int
    lib.pagk_frame_download_level.argtypes = [vp, i32, i32, vp, _P(i32), _P(i32)]
    lib.pagk_track_device.restype = C.c_int
    lib.pagk_track_device.argtypes = [vp, _P(Params), i32, i32, i32, vp, vp, vp, vp, _P(Outputs)]
    if hasattr(lib, "pagk_frame_set_device_batch"):
        lib.pagk_frame_set_device_batch.restype = C.c_int
        lib.pagk_frame_set_device_batch.argtypes = [vp, i32, vp, vp, vp, vp, vp, i32]
    if hasattr(lib, "pagk_track_device_batch"):
        lib.pagk_track_device_batch.restype = C.c_int
        lib.pagk_track_device_batch.argtypes = [vp, i32, _P(Params), vp, vp, vp, vp, vp, vp, vp, vp]
    lib.pagk_track_device_fused.restype = C.c_int
    lib.pagk_track_device_fused.argtypes = [vp, _P(Params), i32, i32, i32, vp, vp, vp, vp, _P(Outputs), i32, vp, i32, i32,
                                            C.c_int64, i32]
    lib.pagk_sync.restype = C.c_int
    lib.pagk_sync.argtypes = [vp]
    lib.pagk_set_stream.restype = C.c_int
    lib.pagk_set_stream.argtypes = [vp, vp]
    lib.pagk_set_kernel.restype = C.c_int
    lib.pagk_set_kernel.argtypes = [vp, i32]
    lib.pagk_last_variant.restype = C.c_int
    lib.pagk_last_variant.argtypes = [vp]
    lib.pagk_set_concurrency.restype = C.c_int
    lib.pagk_set_concurrency.argtypes = [vp, i32]
    lib.pagk_last_handover.restype = C.c_int
    lib.pagk_last_handover.argtypes = [vp]
    lib.pagk_last_kernel_ms.restype = C.c_int
    lib.pagk_last_kernel_ms.argtypes = [vp, _P(C.c_float), _P(C.c_float)]
    lib.pagk_gyro_predict_device.restype = C.c_int
    lib.pagk_gyro_predict_device.argtypes = [vp, _P(Params), i32, i32, vp, vp, i32, vp, vp, vp, vp, vp]
    lib.pagk_gyro_predict_device_rot.restype = C.c_int
    lib.pagk_gyro_predict_device_rot.argtypes = [vp, _P(Params), i32, i32, vp, i32, vp, vp, vp, vp, vp]
    lib.pagk_post_filter.restype = C.c_int
    lib.pagk_post_filter.argtypes = [i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "pagk_frame_handover_device"):   # (absent from older builds that tools/ab_lib.py loads for A/B runs)
        lib.pagk_post_filter_device.restype = C.c_int
        lib.pagk_post_filter_device.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.pagk_gyro_predict_device_live.restype = C.c_int
        lib.pagk_gyro_predict_device_live.argtypes = [vp, _P(Params), i32, i32, vp, i32, vp, vp, vp, vp, vp, vp]
        for name in ("pagk_frame_handover_device", "pagk_frame_handover"):
            getattr(lib, name).restype = C.c_int
            getattr(lib, name).argtypes = [vp, _P(Params), i32, i32, i32, i32, C.c_double, vp, vp, vp, i32, vp, vp, vp,
                                           vp, vp, vp, vp, vp, vp]
    if hasattr(lib, "pagk_detect_corners_device"):   # (absent from older builds that tools/ab_lib.py loads for A/B runs)
        lib.pagk_detect_params_default.restype = None
        lib.pagk_detect_params_default.argtypes = [_P(DetectParams)]
        lib.pagk_detect_corners_device.restype = C.c_int
        lib.pagk_detect_corners_device.argtypes = [vp, _P(DetectParams), i32, vp, i32, vp, vp, vp]
        lib.pagk_detect_corners.restype = C.c_int
        lib.pagk_detect_corners.argtypes = [vp, _P(DetectParams), _P(Image), vp, i32, vp, vp]
        lib.pagk_frame_handover_detect_device.restype = C.c_int
        lib.pagk_frame_handover_detect_device.argtypes = [vp, _P(Params), i32, i32, i32, i32, C.c_double, vp, vp, vp,
                                                          _P(DetectParams), i32, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.pagk_frame_handover_detect.restype = C.c_int
        lib.pagk_frame_handover_detect.argtypes = [vp, _P(Params), i32, i32, i32, i32, C.c_double, vp, vp, vp,
                                                   _P(DetectParams), _P(Image), vp, vp, vp, vp, vp, vp, vp, vp]
        lib.pagk_selftest_corner_response.restype = C.c_int
        lib.pagk_selftest_corner_response.argtypes = [vp, _P(Image), vp]
    if hasattr(lib, "pagk_detect_fast_device"):   # (absent from older builds that tools/ab_lib.py loads for A/B runs)
        lib.pagk_fast_params_default.restype = None
        lib.pagk_fast_params_default.argtypes = [_P(FastParams)]
        lib.pagk_fast_params_check.restype = C.c_int
        lib.pagk_fast_params_check.argtypes = [_P(FastParams)]
        lib.pagk_detect_fast_bounds.restype = C.c_int
        lib.pagk_detect_fast_bounds.argtypes = [i32, i32, i32, _P(i32), _P(i32)]
        lib.pagk_detect_fast_device.restype = C.c_int
        lib.pagk_detect_fast_device.argtypes = [vp, _P(FastParams), i32, vp, i32, vp, vp, vp]
        lib.pagk_detect_fast.restype = C.c_int
        lib.pagk_detect_fast.argtypes = [vp, _P(FastParams), _P(Image), vp, i32, vp, vp, vp]
        lib.pagk_frame_handover_fast_device.restype = C.c_int
        lib.pagk_frame_handover_fast_device.argtypes = [vp, _P(Params), i32, i32, i32, i32, C.c_double, vp, vp, vp,
                                                        _P(FastParams), i32, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.pagk_frame_handover_fast.restype = C.c_int
        lib.pagk_frame_handover_fast.argtypes = [vp, _P(Params), i32, i32, i32, i32, C.c_double, vp, vp, vp,
                                                 _P(FastParams), _P(Image), vp, vp, vp, vp, vp, vp, vp, vp]
        lib.pagk_selftest_fast_cells.restype = C.c_int
        lib.pagk_selftest_fast_cells.argtypes = [vp, _P(FastParams), _P(Image), vp, vp, _P(i32)]
    if hasattr(lib, "pagk_frame_rectify_device"):   # (absent from older builds that tools/ab_lib.py loads for A/B runs)
        lib.pagk_rectify_params_default.restype = None
        lib.pagk_rectify_params_default.argtypes = [_P(RectifyParams)]
        lib.pagk_rectify_params_check.restype = C.c_int
        lib.pagk_rectify_params_check.argtypes = [_P(RectifyParams)]
        lib.pagk_rectify_set_maps.restype = C.c_int
        lib.pagk_rectify_set_maps.argtypes = [vp, vp, vp, i32, i32, C.c_int64]
        for name in ("pagk_frame_rectify_device", "pagk_frame_rectify_pinned"):
            getattr(lib, name).restype = C.c_int
            getattr(lib, name).argtypes = [vp, i32, _P(RectifyParams), vp, i32, i32, C.c_int64, i32]
        lib.pagk_rectify.restype = C.c_int
        lib.pagk_rectify.argtypes = [vp, _P(RectifyParams), vp, i32, i32, C.c_int64, vp, C.c_int64]
        f64 = C.c_double
        lib.pagk_undistort_maps.restype = C.c_int
        lib.pagk_undistort_maps.argtypes = [f64, f64, f64, f64, vp, i32, f64, f64, f64, f64, i32, i32, vp, vp]
    if hasattr(lib, "pagk_orb_describe_device"):   # (absent from older builds that tools/ab_lib.py loads for A/B runs)
        lib.pagk_orb_params_default.restype = None
        lib.pagk_orb_params_default.argtypes = [_P(OrbParams)]
        lib.pagk_orb_params_check.restype = C.c_int
        lib.pagk_orb_params_check.argtypes = [_P(OrbParams)]
        lib.pagk_orb_pattern_check.restype = C.c_int
        lib.pagk_orb_pattern_check.argtypes = [vp]
        lib.pagk_orb_set_pattern.restype = C.c_int
        lib.pagk_orb_set_pattern.argtypes = [vp, vp]
        lib.pagk_orb_describe_device.restype = C.c_int
        lib.pagk_orb_describe_device.argtypes = [vp, _P(OrbParams), i32, i32, vp, vp, vp, vp, vp]
        lib.pagk_orb_describe.restype = C.c_int
        lib.pagk_orb_describe.argtypes = [vp, _P(OrbParams), _P(Image), i32, vp, vp, vp, vp]
        lib.pagk_orb_match_device.restype = C.c_int
        lib.pagk_orb_match_device.argtypes = [vp, _P(OrbParams), i32, vp, vp, i32, vp, vp, vp, vp, vp, vp]
        lib.pagk_orb_match.restype = C.c_int
        lib.pagk_orb_match.argtypes = [vp, _P(OrbParams), i32, vp, i32, vp, vp, vp, vp, vp]
    if hasattr(lib, "pagk_orb_extract_slot"):   # (absent from older builds that tools/ab_lib.py loads for A/B runs)
        lib.pagk_orb_extractor_default.restype = None
        lib.pagk_orb_extractor_default.argtypes = [_P(OrbExtractor)]
        lib.pagk_orb_extractor_check.restype = C.c_int
        lib.pagk_orb_extractor_check.argtypes = [_P(OrbExtractor)]
        lib.pagk_orb_extractor_levels.restype = C.c_int
        lib.pagk_orb_extractor_levels.argtypes = [_P(OrbExtractor), i32, i32, vp, vp, vp, vp, vp, vp]
        lib.pagk_orb_extract_slot.restype = C.c_int
        lib.pagk_orb_extract_slot.argtypes = [vp, _P(OrbExtractor), _P(OrbParams), i32]
        lib.pagk_orb_slot_read.restype = C.c_int
        lib.pagk_orb_slot_read.argtypes = [vp, i32, i32, vp, vp, vp, vp, vp, vp]
        lib.pagk_orb_match_slots.restype = C.c_int
        lib.pagk_orb_match_slots.argtypes = [vp, _P(OrbParams), i32, i32]
        lib.pagk_orb_match_slots_read.restype = C.c_int
        lib.pagk_orb_match_slots_read.argtypes = [vp, i32, i32, vp, vp, vp, vp]
        lib.pagk_orb_extract_levels.restype = C.c_int
        lib.pagk_orb_extract_levels.argtypes = [vp, _P(OrbExtractor), _P(OrbParams), _P(Image), i32, vp, vp, vp, vp, vp, vp]
        lib.pagk_orb_detect_levels.restype = C.c_int
        lib.pagk_orb_detect_levels.argtypes = [vp, _P(OrbExtractor), _P(Image), vp, i32, vp, vp, vp, vp]
        lib.pagk_selftest_orb_level.restype = C.c_int
        lib.pagk_selftest_orb_level.argtypes = [vp, i32, i32, vp, C.c_int64]
    if hasattr(lib, "pagk_lk_track_device"):   # (absent from older builds that tools/ab_lib.py loads for A/B runs)
        lib.pagk_lk_params_default.restype = None
        lib.pagk_lk_params_default.argtypes = [_P(LkParams)]
        lib.pagk_lk_params_check.restype = C.c_int
        lib.pagk_lk_params_check.argtypes = [_P(LkParams)]
        lib.pagk_lk_levels.restype = C.c_int
        lib.pagk_lk_levels.argtypes = [i32, i32, _P(LkParams)]
        lib.pagk_lk_pyramid_device.restype = C.c_int
        lib.pagk_lk_pyramid_device.argtypes = [vp, _P(LkParams), i32]
        lib.pagk_lk_track_device.restype = C.c_int
        lib.pagk_lk_track_device.argtypes = [vp, _P(LkParams), i32, i32, i32, vp, vp, vp, vp, vp, vp, vp, vp]
        lib.pagk_lk_track.restype = C.c_int
        lib.pagk_lk_track.argtypes = [vp, _P(LkParams), _P(Image), _P(Image), i32, vp, vp, vp, vp, vp, vp, vp]
        lib.pagk_selftest_lk_level.restype = C.c_int
        lib.pagk_selftest_lk_level.argtypes = [vp, i32, i32, vp, C.c_int64]
    if hasattr(lib, "pagk_sequence_create"):
        sp = _P(SequenceParams)
        lib.pagk_sequence_params_default.restype = None
        lib.pagk_sequence_params_default.argtypes = [sp]
        for name, args in (("pagk_sequence_params_check", [sp]), ("pagk_sequence_create", [vp, sp]),
                           ("pagk_sequence_destroy", [vp]), ("pagk_sequence_start", [vp, _P(Image), vp, i32]),
                           ("pagk_sequence_step", [vp, _P(Image), vp, vp, i32, i32]),
                           ("pagk_sequence_read", [vp, i32, vp, vp, vp, vp, vp, vp, vp]),
                           ("pagk_sequence_read_pair", [vp, i32, vp, vp, vp, vp]), ("pagk_sequence_status", [vp, vp])):
            getattr(lib, name).restype = C.c_int
            getattr(lib, name).argtypes = args
    if hasattr(lib, "pagk_sequence_create_sensor"):
        sp, ss, iw = _P(SequenceParams), _P(SequenceSensor), _P(ImuWindow)
        lib.pagk_sequence_sensor_default.restype = None
        lib.pagk_sequence_sensor_default.argtypes = [ss]
        for name, args in (("pagk_sequence_sensor_check", [ss]), ("pagk_sequence_create_sensor", [vp, sp, ss]),
                           ("pagk_sequence_start_sensor", [vp, _P(Image), C.c_double, vp, i32]),
                           ("pagk_sequence_step_sensor", [vp, _P(Image), iw, vp, i32, i32]),
                           ("pagk_sequence_read_velocity", [vp, i32, vp]), ("pagk_imu_window_check", [iw, i32]),
                           ("pagk_gyro_integrate", [vp, vp, _P(Params), iw, vp, vp])):
            getattr(lib, name).restype = C.c_int
            getattr(lib, name).argtypes = args
    if hasattr(lib, "pagk_sequence_group_create"):
        sp = _P(SequenceParams)
        for name, args in (("pagk_sequence_group_check", [sp]), ("pagk_sequence_group_create", [vp, i32]),
                           ("pagk_sequence_group_destroy", [vp]), ("pagk_sequence_group_start", [vp, vp, vp, vp]),
                           ("pagk_sequence_group_step", [vp, vp, vp, vp, vp, i32]), ("pagk_sequence_group_status", [vp, vp])):
            getattr(lib, name).restype = C.c_int
            getattr(lib, name).argtypes = args
    if hasattr(lib, "pagk_sequence_group_create_sensor"):
        sp, ss = _P(SequenceParams), _P(SequenceSensor)
        for name, args in (("pagk_sequence_group_sensor_check", [sp, ss]), ("pagk_sequence_group_create_sensor", [vp, i32]),
                           ("pagk_sequence_group_start_sensor", [vp, vp, vp, vp, vp]),
                           ("pagk_sequence_group_step_sensor", [vp, vp, vp, vp, vp, i32])):
            getattr(lib, name).restype = C.c_int
            getattr(lib, name).argtypes = args
    if hasattr(lib, "pagk_sequence_group_create_lk"):
        for name, args in (("pagk_sequence_group_lk_check", [_P(SequenceParams), _P(SequenceSensor)]),
                           ("pagk_sequence_group_create_lk", [vp, i32])):
            getattr(lib, name).restype = C.c_int
            getattr(lib, name).argtypes = args
    if hasattr(lib, "pagk_sequence_results_create"):
        for name, args in (("pagk_sequence_results_layout", [i32, i32, _P(ResultsLayout)]),
                           ("pagk_sequence_results_create", [vp, i32]), ("pagk_sequence_fetch", [vp, i32, _P(SequenceResult)]),
                           ("pagk_sequence_poll", [vp, i32])):
            getattr(lib, name).restype = C.c_int
            getattr(lib, name).argtypes = args
    if hasattr(lib, "pagk_lk_track_flow"):
        lib.pagk_lk_track_flow.restype = C.c_int
        lib.pagk_lk_track_flow.argtypes = [vp, _P(LkParams), _P(Params), _P(Image), _P(Image), i32, vp, vp, vp, vp, vp, vp, vp,
                                           vp, vp, vp]
    f32 = C.c_float
    for name in ("pagk_graph_begin",):
        getattr(lib, name).restype = C.c_int
        getattr(lib, name).argtypes = [vp]
    lib.pagk_graph_end.restype = C.c_int
    lib.pagk_graph_end.argtypes = [vp, _P(i32)]
    lib.pagk_graph_launch.restype = C.c_int
    lib.pagk_graph_launch.argtypes = [vp, i32]
    lib.pagk_graph_destroy.restype = C.c_int
    lib.pagk_graph_destroy.argtypes = [vp, i32]
    lib.pagk_geometry_scores_device.restype = C.c_int
    lib.pagk_geometry_scores_device.argtypes = [vp, vp, vp, vp, i32, vp, vp, f32, vp, vp, vp]
    lib.pagk_geometry_scores.restype = C.c_int
    lib.pagk_geometry_scores.argtypes = [vp, vp, vp, vp, i32, vp, vp, f32, vp, vp, _P(f32), _P(f32)]
    lib.pagk_geometry_select.restype = C.c_int
    lib.pagk_geometry_select.argtypes = [f32, f32]
    lib.pagk_geometry_validation.restype = C.c_int
    lib.pagk_geometry_validation.argtypes = [vp, vp, vp, vp, i32, vp, vp, vp, f32, _P(f32)]
    if hasattr(lib, "pagk_search_klt_device"):   # (absent from older builds that tools/ab_lib.py loads for A/B runs)
        ap, lp, f32_ = _P(AssocParams), _P(LkParams), C.c_float
        lib.pagk_assoc_params_default.restype = None
        lib.pagk_assoc_params_default.argtypes = [ap]
        lib.pagk_assoc_params_check.restype = C.c_int
        lib.pagk_assoc_params_check.argtypes = [ap]
        lib.pagk_match_features_device.restype = C.c_int
        lib.pagk_match_features_device.argtypes = [vp, ap, i32, i32, i32] + [vp] * 10
        lib.pagk_search_gyro_predict_device.restype = C.c_int
        lib.pagk_search_gyro_predict_device.argtypes = ([vp, ap, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, f32_, i32]
                                                        + [vp] * 11)
        lib.pagk_search_gyro_predict.restype = C.c_int
        lib.pagk_search_gyro_predict.argtypes = ([vp, ap, _P(Image), _P(Image), i32, i32, vp, vp, vp, vp, i32, vp, vp, f32_, i32]
                                                 + [vp] * 10)
        lib.pagk_search_klt_device.restype = C.c_int
        lib.pagk_search_klt_device.argtypes = [vp, lp, ap, i32, i32, i32, vp, vp, i32, vp, vp] + [vp] * 11
        lib.pagk_search_klt.restype = C.c_int
        lib.pagk_search_klt.argtypes = [vp, lp, ap, _P(Image), _P(Image), i32, vp, i32, vp] + [vp] * 10
    lib.pagk_fit_params_default.restype = None
    lib.pagk_fit_params_default.argtypes = [_P(FitParams)]
    lib.pagk_geometry_fit_device.restype = C.c_int
    lib.pagk_geometry_fit_device.argtypes = [vp, _P(FitParams), i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.pagk_geometry_fit.restype = C.c_int
    lib.pagk_geometry_fit.argtypes = [vp, _P(FitParams), i32, vp, vp, vp, vp, vp, vp, vp, vp]
    lib.pagk_geometry_validation_device.restype = C.c_int
    lib.pagk_geometry_validation_device.argtypes = [vp, _P(FitParams), i32, vp, vp, vp, f32, vp, vp]
    lib.pagk_geometry_validation_fit.restype = C.c_int
    lib.pagk_geometry_validation_fit.argtypes = [vp, _P(FitParams), i32, vp, vp, vp, f32, _P(f32)]
    lib.pagk_selftest_fit_samples.restype = C.c_int
    lib.pagk_selftest_fit_samples.argtypes = [vp, C.c_uint64, i32, i32, i32, i32, vp]
    f64 = C.c_double
    lib.pagk_pose_params_default.restype = None
    lib.pagk_pose_params_default.argtypes = [_P(PoseParams)]
    lib.pagk_pose_params_check.restype = C.c_int
    lib.pagk_pose_params_check.argtypes = [_P(PoseParams)]
    lib.pagk_pose_2d2d_device.restype = C.c_int
    lib.pagk_pose_2d2d_device.argtypes = [vp, _P(PoseParams), f64, f64, f64, i32] + [vp] * 12
    lib.pagk_pose_from_matches_device.restype = C.c_int
    lib.pagk_pose_from_matches_device.argtypes = [vp, _P(PoseParams), f64, f64, f64, i32, vp, vp, i32] + [vp] * 12
    lib.pagk_pose_2d2d.restype = C.c_int
    lib.pagk_pose_2d2d.argtypes = [vp, _P(PoseParams), f64, f64, f64, i32] + [vp] * 12
    lib.pagk_near_neighbors_device.restype = C.c_int
    lib.pagk_near_neighbors_device.argtypes = [vp, i32, i32, i32, i32, vp, vp, vp, vp, i32, vp, vp, i32, f32, i32, i32,
                                               vp, vp, vp, vp]
    lib.pagk_find_near_neighbors.restype = C.c_int
    lib.pagk_find_near_neighbors.argtypes = [vp, _P(Image), _P(Image), i32, i32, vp, vp, vp, vp, i32, vp, vp, i32, f32,
                                             i32, i32, vp, vp, vp, vp]
    lib.pagk_ncc_free.restype = C.c_int
    lib.pagk_ncc_free.argtypes = [vp, _P(Image), _P(Image), i32, i32, vp, vp, vp, vp]
    if hasattr(lib, "pagk_selftest_divide"):   # (absent from older builds that tools/ab_lib.py loads for A/B runs)
        lib.pagk_selftest_divide.restype = C.c_int
        lib.pagk_selftest_divide.argtypes = [vp, i32, vp, vp, vp, vp, vp, vp]
        lib.pagk_selftest_solve.restype = C.c_int
        lib.pagk_selftest_solve.argtypes = [vp, i32, vp, vp, C.c_uint32, vp, vp, vp, vp]
    if hasattr(lib, "pagk_prio_hint_reset"):   # (an older build given through PAGK_LIB for an A/B run has no hint)
        lib.pagk_prio_hint_threshold.restype = C.c_int
        lib.pagk_prio_hint_threshold.argtypes = [vp]
        lib.pagk_prio_hint_reset.restype = C.c_int
        lib.pagk_prio_hint_reset.argtypes = [vp]
        lib.pagk_prio_hint_get.restype = C.c_int
        lib.pagk_prio_hint_get.argtypes = [vp, i32, vp]
        lib.pagk_prio_hint_set.restype = C.c_int
        lib.pagk_prio_hint_set.argtypes = [vp, i32, vp]
    if hasattr(lib, "pagk_dispatch_order_get"):   # (likewise: an older build has no dispatch order)
        lib.pagk_dispatch_order_enabled.restype = C.c_int
        lib.pagk_dispatch_order_enabled.argtypes = [vp]
        lib.pagk_dispatch_order_get.restype = C.c_int
        lib.pagk_dispatch_order_get.argtypes = [vp, i32, vp, vp]
    if hasattr(lib, "pagk_priority_threshold"):
        lib.pagk_priority_threshold.restype = C.c_int
        lib.pagk_priority_threshold.argtypes = [vp]
    if hasattr(lib, "pagk_check_launch"):
        lib.pagk_check_launch.restype = C.c_int
        lib.pagk_check_launch.argtypes = [vp]
    if hasattr(lib, "pagk_selftest_repeat_sum"):
        lib.pagk_selftest_repeat_sum.restype = C.c_int
        lib.pagk_selftest_repeat_sum.argtypes = [vp, i32, vp, i32, vp, vp]
    if hasattr(lib, "pagk_selftest_sample"):
        lib.pagk_selftest_sample.restype = C.c_int
        lib.pagk_selftest_sample.argtypes = [vp, i32, i32, i32, i32, vp, vp]
    if hasattr(lib, "pagk_selftest_fill_workspaces"):
        lib.pagk_selftest_fill_workspaces.restype = C.c_int
        lib.pagk_selftest_fill_workspaces.argtypes = [vp, C.c_uint32, i32]
    lib.pagk_match_features.restype = C.c_int
    lib.pagk_match_features.argtypes = [i32, i32, vp, vp, vp, vp, i32, vp, vp, vp, vp]
    # the sharded path
    lib.pagk_multi_create.restype = C.c_int
    lib.pagk_multi_create.argtypes = [_P(vp), _P(i32), i32]
    lib.pagk_multi_unique_id.restype = C.c_int
    lib.pagk_multi_unique_id.argtypes = [vp]
    lib.pagk_multi_create_rank.restype = C.c_int
    lib.pagk_multi_create_rank.argtypes = [_P(vp), vp, i32, i32, i32]
    lib.pagk_multi_destroy.restype = None
    lib.pagk_multi_destroy.argtypes = [vp]
    lib.pagk_multi_world.restype = i32
    lib.pagk_multi_world.argtypes = [vp]
    if hasattr(lib, "pagk_multi_comm_count"):
        lib.pagk_multi_comm_count.restype = i32
        lib.pagk_multi_comm_count.argtypes = [vp]
    lib.pagk_multi_local.restype = i32
    lib.pagk_multi_local.argtypes = [vp]
    lib.pagk_multi_ctx.restype = vp
    lib.pagk_multi_ctx.argtypes = [vp, i32]
    lib.pagk_multi_last_error.restype = C.c_char_p
    lib.pagk_multi_last_error.argtypes = [vp]
    lib.pagk_shard_range.restype = None
    lib.pagk_shard_range.argtypes = [i32, i32, i32, _P(i32), _P(i32)]
    lib.pagk_shard_layout.restype = C.c_size_t
    lib.pagk_shard_layout.argtypes = [i32, _P(C.c_size_t)]
    lib.pagk_multi_allgather.restype = C.c_int
    lib.pagk_multi_allgather.argtypes = [vp, _P(vp), _P(vp), C.c_size_t, _P(vp)]
    lib.pagk_track_sharded.restype = C.c_int
    lib.pagk_track_sharded.argtypes = [vp, _P(Params), _P(Image), _P(Image), i32, vp, vp, vp, vp, _P(Outputs)]


EXPORTED_SYMBOLS = [
    "pagk_version", "pagk_strerror", "pagk_last_error", "pagk_params_default", "pagk_params_check", "pagk_inv_log_max_dist",
    "pagk_create", "pagk_destroy", "pagk_track", "pagk_track_pyr", "pagk_frame_upload", "pagk_frame_upload_pinned",
    "pagk_frame_set_device", "pagk_frame_download_level", "pagk_track_device", "pagk_track_device_fused", "pagk_sync",
    "pagk_set_stream", "pagk_set_kernel", "pagk_last_variant", "pagk_set_concurrency", "pagk_last_handover", "pagk_last_kernel_ms", "pagk_post_filter", "pagk_gyro_predict_device",
    "pagk_gyro_predict_device_rot",
    "pagk_geometry_scores_device", "pagk_geometry_scores", "pagk_geometry_select", "pagk_geometry_validation",
    "pagk_graph_begin", "pagk_graph_end", "pagk_graph_launch", "pagk_graph_destroy",
    "pagk_near_neighbors_device", "pagk_find_near_neighbors", "pagk_ncc_free", "pagk_match_features",
    "pagk_multi_create", "pagk_multi_unique_id", "pagk_multi_create_rank", "pagk_multi_destroy", "pagk_multi_world",
    "pagk_multi_local", "pagk_multi_ctx", "pagk_multi_last_error", "pagk_shard_range", "pagk_shard_layout",
    "pagk_multi_allgather", "pagk_track_sharded", "pagk_selftest_divide", "pagk_selftest_solve",
    "pagk_selftest_repeat_sum", "pagk_check_launch", "pagk_track_device_batch", "pagk_frame_set_device_batch", "pagk_priority_threshold",
    "pagk_multi_comm_count", "pagk_has_variant",
    "pagk_prio_hint_threshold", "pagk_prio_hint_reset", "pagk_prio_hint_get", "pagk_prio_hint_set",
    "pagk_dispatch_order_enabled", "pagk_dispatch_order_get",
    "pagk_fit_params_default", "pagk_geometry_fit_device", "pagk_geometry_fit", "pagk_geometry_validation_device",
    "pagk_geometry_validation_fit", "pagk_selftest_fit_samples",
    "pagk_pose_params_default", "pagk_pose_params_check", "pagk_pose_2d2d_device", "pagk_pose_from_matches_device",
    "pagk_pose_2d2d",
    "pagk_post_filter_device", "pagk_gyro_predict_device_live", "pagk_frame_handover_device", "pagk_frame_handover",
    "pagk_detect_params_default", "pagk_detect_corners_device", "pagk_detect_corners",
    "pagk_frame_handover_detect_device", "pagk_frame_handover_detect", "pagk_selftest_corner_response",
    "pagk_fast_params_default", "pagk_fast_params_check", "pagk_detect_fast_bounds", "pagk_detect_fast_device",
    "pagk_detect_fast", "pagk_frame_handover_fast_device", "pagk_frame_handover_fast", "pagk_selftest_fast_cells",
    "pagk_rectify_params_default", "pagk_rectify_params_check", "pagk_rectify_set_maps", "pagk_frame_rectify_device",
    "pagk_frame_rectify_pinned", "pagk_rectify", "pagk_undistort_maps",
    "pagk_orb_params_default", "pagk_orb_params_check", "pagk_orb_pattern_check", "pagk_orb_set_pattern",
    "pagk_orb_describe_device", "pagk_orb_describe", "pagk_orb_match_device", "pagk_orb_match",
    "pagk_selftest_sample", "pagk_selftest_fill_workspaces",
    "pagk_orb_extractor_default", "pagk_orb_extractor_check", "pagk_orb_extractor_levels", "pagk_orb_extract_slot",
    "pagk_orb_slot_read", "pagk_orb_match_slots", "pagk_orb_match_slots_read", "pagk_orb_extract_levels",
    "pagk_orb_detect_levels", "pagk_selftest_orb_level",
    "pagk_lk_params_default", "pagk_lk_params_check", "pagk_lk_levels", "pagk_lk_pyramid_device", "pagk_lk_track_device",
    "pagk_lk_track", "pagk_selftest_lk_level", "pagk_lk_track_flow",
    "pagk_sequence_params_default", "pagk_sequence_params_check", "pagk_sequence_create", "pagk_sequence_destroy",
    "pagk_sequence_start", "pagk_sequence_step", "pagk_sequence_read", "pagk_sequence_read_pair", "pagk_sequence_status",
    "pagk_imu_window_check", "pagk_gyro_integrate", "pagk_sequence_sensor_default", "pagk_sequence_sensor_check",
    "pagk_sequence_create_sensor", "pagk_sequence_start_sensor", "pagk_sequence_step_sensor", "pagk_sequence_read_velocity",
    "pagk_sequence_group_check", "pagk_sequence_group_create", "pagk_sequence_group_destroy", "pagk_sequence_group_start",
    "pagk_sequence_group_step", "pagk_sequence_group_status",
    "pagk_sequence_group_sensor_check", "pagk_sequence_group_create_sensor", "pagk_sequence_group_start_sensor",
    "pagk_sequence_group_step_sensor",
    "pagk_sequence_group_lk_check", "pagk_sequence_group_create_lk",
    "pagk_sequence_results_layout", "pagk_sequence_results_create", "pagk_sequence_fetch", "pagk_sequence_poll",
    "pagk_assoc_params_default", "pagk_assoc_params_check", "pagk_match_features_device", "pagk_search_gyro_predict_device",
    "pagk_search_gyro_predict", "pagk_search_klt_device", "pagk_search_klt",
]

HANDOVER_STATE_WORDS = 8
HANDOVER_STATE_FIELDS = ("total", "reach_flag", "survivors", "added", "rejected")


def fit_params_default(**overrides) -> FitParams:
    """pagk_fit_params_default() with overrides (seed, iters_H, iters_F, thresh_H, thresh_F, conf_H, conf_F)."""
    p = FitParams()
    load().pagk_fit_params_default(C.byref(p))
    for k, v in overrides.items():
        if k not in dict(FitParams._fields_):
            raise TypeError(f"pagk_fit_params has no field {k}")
        setattr(p, k, v)
    return p


def pose_params_default(**overrides) -> PoseParams:
    """pagk_pose_params_default() with overrides (seed, iters_E, thresh_E, conf_E, max_depth, fit: a FitParams)."""
    p = PoseParams()
    load().pagk_pose_params_default(C.byref(p))
    for k, v in overrides.items():
        if k not in dict(PoseParams._fields_):
            raise TypeError(f"pagk_pose_params has no field {k}")
        setattr(p, k, v)
    return p


def pose_params_check(p: PoseParams) -> int:
    """pagk_pose_params_check: PAGK_OK or PAGK_E_ARG.  Needs no device."""
    return load().pagk_pose_params_check(C.byref(p))


def detect_params_default(**overrides) -> DetectParams:
    """pagk_detect_params_default() with overrides (quality_level, min_distance, harris_k, raw_cap)."""
    p = DetectParams()
    load().pagk_detect_params_default(C.byref(p))
    for k, v in overrides.items():
        if k not in dict(DetectParams._fields_):
            raise TypeError(f"pagk_detect_params has no field {k}")
        setattr(p, k, v)
    return p


def fast_params_default(**overrides) -> FastParams:
    """pagk_fast_params_default() with overrides (ini_threshold, min_threshold, n_features, n_levels)."""
    p = FastParams()
    load().pagk_fast_params_default(C.byref(p))
    for k, v in overrides.items():
        if k not in dict(FastParams._fields_):
            raise TypeError(f"pagk_fast_params has no field {k}")
        setattr(p, k, v)
    return p


def fast_params_check(p: FastParams) -> int:
    """pagk_fast_params_check: PAGK_OK, PAGK_E_ARG or PAGK_E_UNSUPPORTED (needs no device)."""
    return int(load().pagk_fast_params_check(C.byref(p)))


def detect_fast_bounds(width: int, height: int, n_features: int):
    """pagk_detect_fast_bounds -> (raw_bound, out_bound); PagkError for a size the definition excludes (needs no device)."""
    raw, out = C.c_int32(0), C.c_int32(0)
    rc = load().pagk_detect_fast_bounds(int(width), int(height), int(n_features), C.byref(raw), C.byref(out))
    if rc != 0:
        raise PagkError(rc, "pagk_detect_fast_bounds")
    return raw.value, out.value


def orb_params_default(**overrides) -> OrbParams:
    """pagk_orb_params_default() with overrides (blur_weights = four integers, match_floor, n_levels)."""
    p = OrbParams()
    load().pagk_orb_params_default(C.byref(p))
    for k, v in overrides.items():
        if k not in dict(OrbParams._fields_):
            raise TypeError(f"pagk_orb_params has no field {k}")
        if k == "blur_weights":
            v = (C.c_int32 * 4)(*[int(x) for x in v])
        setattr(p, k, v)
    return p


def orb_params_check(p: OrbParams) -> int:
    """pagk_orb_params_check: PAGK_OK, PAGK_E_ARG or PAGK_E_UNSUPPORTED (needs no device)."""
    return int(load().pagk_orb_params_check(C.byref(p)))


def _orb_pattern(pattern) -> np.ndarray:
    pat = np.ascontiguousarray(pattern, np.int32).reshape(-1)
    if pat.shape[0] != 1024:
        raise ValueError("a sampling pattern is 512 points: 1024 integers, x then y")
    return pat


def orb_pattern_check(pattern) -> int:
    """pagk_orb_pattern_check: PAGK_OK if every coordinate lies in [-13, 13] (needs no device)."""
    return int(load().pagk_orb_pattern_check(_orb_pattern(pattern).ctypes.data))


def orb_extractor_default(**overrides) -> OrbExtractor:
    """pagk_orb_extractor_default() with overrides (n_features, scale_factor, n_levels, ini_threshold, min_threshold)."""
    e = OrbExtractor()
    load().pagk_orb_extractor_default(C.byref(e))
    for k, v in overrides.items():
        if k not in dict(OrbExtractor._fields_):
            raise TypeError(f"pagk_orb_extractor has no field {k}")
        setattr(e, k, v)
    return e


def orb_extractor_check(e: OrbExtractor) -> int:
    """pagk_orb_extractor_check: PAGK_OK or PAGK_E_ARG (needs no device)."""
    return int(load().pagk_orb_extractor_check(C.byref(e)))


def orb_extractor_levels(e: OrbExtractor, width: int, height: int):
    """pagk_orb_extractor_levels (needs no device) -> dict(rc, and for rc == 0: n_levels, width, height, scale, quota, size
    (arrays of n_levels entries) and out_bound)."""
    lw, lh = np.zeros(ORB_MAX_LEVELS, np.int32), np.zeros(ORB_MAX_LEVELS, np.int32)
    sc, quota, size = np.zeros(ORB_MAX_LEVELS, np.float32), np.zeros(ORB_MAX_LEVELS, np.int32), np.zeros(ORB_MAX_LEVELS, np.int32)
    ob = C.c_int32(0)
    rc = int(load().pagk_orb_extractor_levels(C.byref(e), int(width), int(height), lw.ctypes.data, lh.ctypes.data,
                                              sc.ctypes.data, quota.ctypes.data, size.ctypes.data, C.addressof(ob)))
    if rc:
        return dict(rc=rc)
    n = int(e.n_levels)
    return dict(rc=0, n_levels=n, width=lw[:n], height=lh[:n], scale=sc[:n], quota=quota[:n], size=size[:n],
                out_bound=int(ob.value))


def _orb_set_dict(cap, kp, octave, resp, ang, desc, info) -> dict:
    """The arrays of a keypoint set cut to its count, with the whole-capacity arrays under full_*."""
    n = int(info[0])
    out = dict(n=n, cap=cap, keypoints=kp[:n], octave=octave[:n], response=resp[:n], info=info,
               full_keypoints=kp, full_octave=octave, full_response=resp, outside=int(info[1]), n_levels=int(info[2]),
               level_counts=info[8:16].copy(), level_raw=info[16:24].copy(), level_quota=info[24:32].copy())
    if ang is not None:
        out.update(angle=ang[:n], desc=desc[:n], full_angle=ang, full_desc=desc)
    return out


def lk_params_default(**overrides) -> LkParams:
    """pagk_lk_params_default() with overrides (half_patch, max_level, max_count, epsilon, min_eig_threshold, err_threshold)."""
    p = LkParams()
    load().pagk_lk_params_default(C.byref(p))
    for k, v in overrides.items():
        if k not in dict(LkParams._fields_):
            raise TypeError(f"pagk_lk_params has no field {k}")
        setattr(p, k, v)
    return p


def sequence_params_default(**overrides) -> SequenceParams:
    """pagk_sequence_params_default() with overrides (any field of pagk_sequence_params; nested blocks as their structures)."""
    p = SequenceParams()
    load().pagk_sequence_params_default(C.byref(p))
    for k, v in overrides.items():
        if k not in dict(SequenceParams._fields_):
            raise TypeError(f"pagk_sequence_params has no field {k}")
        setattr(p, k, v)
    return p


def sequence_params_check(p: SequenceParams) -> int:
    """pagk_sequence_params_check: PAGK_OK, or the code pagk_sequence_create refuses these parameters with (needs no device)."""
    return int(load().pagk_sequence_params_check(C.byref(p)))


def sequence_results_layout(cap: int, sensor: int = 0) -> ResultsLayout:
    """pagk_sequence_results_layout: where the parts of a frame's record lie (needs no device).  ValueError when refused."""
    lay = ResultsLayout()
    rc = int(load().pagk_sequence_results_layout(int(cap), int(sensor), C.byref(lay)))
    if rc != PAGK_OK:
        raise ValueError(f"pagk_sequence_results_layout refuses cap {cap}, sensor {sensor}")
    return lay


def sequence_group_check(p: SequenceParams) -> int:
    """pagk_sequence_group_check: PAGK_OK if sequences of these parameters can form a group (needs no device)."""
    return int(load().pagk_sequence_group_check(C.byref(p)))


def sequence_group_sensor_check(p: SequenceParams, s: "SequenceSensor") -> int:
    """pagk_sequence_group_sensor_check: PAGK_OK if sensor sequences of these blocks can form a sensor group (needs no device)."""
    return int(load().pagk_sequence_group_sensor_check(C.byref(p), C.byref(s)))


def sequence_group_lk_check(p: SequenceParams, s: "SequenceSensor | None" = None) -> int:
    """pagk_sequence_group_lk_check: PAGK_OK if Lucas-Kanade sequences of these blocks (s: the sensor block of sensor
    sequences, None for plain ones) can form a group (needs no device)."""
    return int(load().pagk_sequence_group_lk_check(C.byref(p), C.byref(s) if s is not None else None))


class SequenceGroup:
    """pagk_sequence_group_*: k contexts, each with a plain sequence of the same parameters, stepped together.  contexts[0] is
    the lead; per camera the results are those of its sequence stepped alone (Context.sequence_read / sequence_read_pair).
    With sensor=True the contexts hold sensor sequences (pagk_sequence_group_*_sensor): start_sensor and step_sensor take the
    raw frames, time stamps and IMU windows; with detector 2 candidates is None.
    With lk=True the contexts hold Lucas-Kanade sequences (pagk_sequence_group_create_lk), plain ones or, with sensor=True,
    sensor sequences; the same start and step calls drive the group."""

    def __init__(self, contexts, sensor: bool = False, lk: bool = False):
        self.ctxs = list(contexts)
        self.lib = load()
        self.lead = self.ctxs[0]
        self.k = len(self.ctxs)
        self.sensor = bool(sensor)
        handles = (C.c_void_p * self.k)(*(c.h for c in self.ctxs))
        self.lk = bool(lk)
        if self.lk:
            self.lead._check(self.lib.pagk_sequence_group_create_lk(handles, self.k), "pagk_sequence_group_create_lk")
        elif self.sensor:
            self.lead._check(self.lib.pagk_sequence_group_create_sensor(handles, self.k), "pagk_sequence_group_create_sensor")
        else:
            self.lead._check(self.lib.pagk_sequence_group_create(handles, self.k), "pagk_sequence_group_create")
        self.alive = True

    def _inputs(self, frames, candidates, view=None):
        if len(frames) != self.k or (candidates is not None and len(candidates) != self.k):
            raise ValueError("one frame and one candidate list per camera")
        views = (Image * self.k)(*((view or image_view)(f) for f in frames))
        if candidates is None:                     # (a detecting sensor group takes no lists)
            return (frames, None), views, None, None
        lists = [Context._seq_cand(c if c is not None else np.zeros((0, 2), np.float32)) for c in candidates]
        ptrs = (C.c_void_p * self.k)(*(l[1] for l in lists))
        counts = (C.c_int32 * self.k)(*(l[2] for l in lists))
        return (frames, lists), views, ptrs, counts

    def start(self, frames, candidates):
        """pagk_sequence_group_start: the k first frames (host images) and candidate lists."""
        keep, views, ptrs, counts = self._inputs(frames, candidates if candidates is not None else [None] * self.k)
        self.lead._check(self.lib.pagk_sequence_group_start(self.lead.h, views, ptrs, counts), "pagk_sequence_group_start")

    def step(self, frames, rot9s=None, candidates=None, mode: int = SEQ_GRAPH):
        """pagk_sequence_group_step: frame k >= 1 of every camera; rot9s is k x 9 floats or None; nothing is synchronised."""
        keep, views, ptrs, counts = self._inputs(frames, candidates if candidates is not None else [None] * self.k)
        rot = None if rot9s is None else np.ascontiguousarray(rot9s, np.float32).reshape(self.k, 9)
        self.lead._check(self.lib.pagk_sequence_group_step(self.lead.h, views, _ptr(rot), ptrs, counts, int(mode)),
                         "pagk_sequence_group_step")

    def start_sensor(self, raws, times, candidates=None):
        """pagk_sequence_group_start_sensor: the k first raw frames, their time stamps and (detector 0) candidate lists."""
        keep, views, ptrs, counts = self._inputs(raws, candidates, Context._raw_view)
        t = np.ascontiguousarray(times, np.float64).reshape(-1)
        if t.shape[0] != self.k:
            raise ValueError("one time stamp per camera")
        self.lead._check(self.lib.pagk_sequence_group_start_sensor(self.lead.h, views, _ptr(t), ptrs, counts),
                         "pagk_sequence_group_start_sensor")

    def step_sensor(self, raws, windows, candidates=None, mode: int = SEQ_GRAPH):
        """pagk_sequence_group_step_sensor: raw frame k >= 1 of every camera with its ImuWindow; nothing is synchronised."""
        keep, views, ptrs, counts = self._inputs(raws, candidates, Context._raw_view)
        if len(windows) != self.k:
            raise ValueError("one window per camera")
        wins = (ImuWindow * self.k)(*windows)
        self.lead._check(self.lib.pagk_sequence_group_step_sensor(self.lead.h, views, wins, ptrs, counts, int(mode)),
                         "pagk_sequence_group_step_sensor")

    def status(self) -> dict:
        """pagk_sequence_group_status -> dict(frames, last_was_graph, graphs, k); nothing is synchronised."""
        w = np.zeros(SEQ_STATUS_WORDS, np.int32)
        self.lead._check(self.lib.pagk_sequence_group_status(self.lead.h, _ptr(w)), "pagk_sequence_group_status")
        return dict(frames=int(w[0]), last_was_graph=bool(w[1]), graphs=int(w[2]), k=int(w[3]))

    def destroy(self):
        """pagk_sequence_group_destroy: every member is an ordinary sequence again."""
        if self.alive:
            self.alive = False
            self.lead._check(self.lib.pagk_sequence_group_destroy(self.lead.h), "pagk_sequence_group_destroy")


def sequence_sensor_default(**overrides) -> SequenceSensor:
    """pagk_sequence_sensor_default() with overrides (rectify as a RectifyParams, Rbc as nine numbers, the scalars)."""
    s = SequenceSensor()
    load().pagk_sequence_sensor_default(C.byref(s))
    for k, v in overrides.items():
        if k not in dict(SequenceSensor._fields_):
            raise TypeError(f"pagk_sequence_sensor has no field {k}")
        if k == "Rbc":
            v = (C.c_float * 9)(*[float(x) for x in np.asarray(v, np.float32).reshape(9)])
        setattr(s, k, v)
    return s


def sequence_sensor_check(s: SequenceSensor) -> int:
    """pagk_sequence_sensor_check: PAGK_OK or PAGK_E_ARG (needs no device)."""
    return int(load().pagk_sequence_sensor_check(C.byref(s)))


def imu_window(t_ref: float, t_cur: float, t, w, bias=(0.0, 0.0, 0.0)):
    """A pagk_imu_window over host arrays: t (n doubles), w (n x 3 floats, rad/s).  Returns (window, keep): `keep` holds the
    arrays the window points into and must live as long as the window is used."""
    tt = np.ascontiguousarray(t, np.float64).reshape(-1)
    ww = np.ascontiguousarray(w, np.float32).reshape(-1, 3)
    if ww.shape[0] != tt.shape[0]:
        raise ValueError("one rate per time stamp")
    win = ImuWindow(float(t_ref), float(t_cur), int(tt.shape[0]), tt.ctypes.data if tt.size else None,
                    ww.ctypes.data if ww.size else None, (C.c_float * 3)(*[float(b) for b in bias]))
    return win, (tt, ww)


def imu_window_check(win: ImuWindow, imu_cap: int = IMU_MAX_SAMPLES) -> int:
    """pagk_imu_window_check: PAGK_OK or PAGK_E_ARG (needs no device)."""
    return int(load().pagk_imu_window_check(C.byref(win), int(imu_cap)))


def lk_params_check(p: LkParams) -> int:
    """pagk_lk_params_check: PAGK_OK or PAGK_E_ARG (needs no device)."""
    return int(load().pagk_lk_params_check(C.byref(p)))


def lk_levels(width: int, height: int, lk: LkParams | None = None) -> int:
    """pagk_lk_levels: the effective top level of the Lucas-Kanade pyramid of a width x height image, or PAGK_E_ARG
    (needs no device)."""
    lk = lk if lk is not None else lk_params_default()
    return int(load().pagk_lk_levels(int(width), int(height), C.byref(lk)))


def assoc_params_default(**overrides) -> AssocParams:
    """pagk_assoc_params_default() with overrides (th_ncc_high, th_ncc_low, th_ratio, use_ncc, min_matches, klt_max_distance,
    klt_ratio, klt_disparity_factor)."""
    p = AssocParams()
    load().pagk_assoc_params_default(C.byref(p))
    for k, v in overrides.items():
        if k not in dict(AssocParams._fields_):
            raise TypeError(f"pagk_assoc_params has no field {k}")
        setattr(p, k, v)
    return p


def assoc_params_check(p: AssocParams) -> int:
    """pagk_assoc_params_check: PAGK_OK or PAGK_E_ARG (needs no device)."""
    return int(load().pagk_assoc_params_check(C.byref(p)))


def rectify_params_default(**overrides) -> RectifyParams:
    """pagk_rectify_params_default() with overrides (channels, gray_weight = three integers, gray_shift)."""
    p = RectifyParams()
    load().pagk_rectify_params_default(C.byref(p))
    for k, v in overrides.items():
        if k not in dict(RectifyParams._fields_):
            raise TypeError(f"pagk_rectify_params has no field {k}")
        if k == "gray_weight":
            v = (C.c_int32 * 3)(*[int(x) for x in v])
        setattr(p, k, v)
    return p


def undistort_maps(fx, fy, cx, cy, dist, width: int, height: int, new_camera=None):
    """pagk_undistort_maps (host, no device): the float32 planes map_x, map_y (height x width) of the Brown-Conrady camera
    (fx fy cx cy, dist = k1 k2 p1 p2 [k3]) seen through new_camera = (fx, fy, cx, cy), the same camera by default."""
    d = np.ascontiguousarray(dist, np.float64).ravel()
    nfx, nfy, ncx, ncy = new_camera if new_camera is not None else (fx, fy, cx, cy)
    mx, my = np.zeros((height, width), np.float32), np.zeros((height, width), np.float32)
    rc = load().pagk_undistort_maps(fx, fy, cx, cy, d.ctypes.data if d.size else None, int(d.size), nfx, nfy, ncx, ncy,
                                    int(width), int(height), mx.ctypes.data, my.ctypes.data)
    if rc != PAGK_OK:
        raise PagkError(rc, "pagk_undistort_maps")
    return mx, my


def load():
    """Load libpagk_hip.so.  Raises if it has not been built: there is no fallback."""
    global _lib
    if _lib is None:
        if not os.path.exists(LIB_PATH):
            raise RuntimeError(
                f"{LIB_PATH} is missing: run `python -c 'import __graft_entry__ as g; g.build()'` "
                "(hipcc --offload-arch=gfx950). The HIP path is the product; there is no CPU fallback.")
        lib = C.CDLL(LIB_PATH, mode=C.RTLD_GLOBAL)
        declare(lib)
        _lib = lib
    return _lib


def has_variant(which: int) -> bool:
    """Can pagk_set_kernel select `which` in the library that is loaded?  (Variants 2 and 6 need -DPAGK_ALL_VARIANTS.)"""
    lib = load()
    if not hasattr(lib, "pagk_has_variant"):
        return True   # (an older build, loaded for an A/B run)
    lib.pagk_has_variant.restype = C.c_int
    lib.pagk_has_variant.argtypes = [C.c_int32]
    return bool(lib.pagk_has_variant(int(which)))


class PagkError(RuntimeError):
    def __init__(self, code: int, where: str, detail: str = ""):
        self.code = code
        msg = load().pagk_strerror(code).decode()
        super().__init__(f"{where}: {msg} ({code}){': ' + detail if detail else ''}")


def _handover_args(h, params: Params, width, height, cap, target_n, new_point_threshold, status, pt_predict, pt_predict_un,
                   *outs, device: bool = True):
    """(head, tail) of the arguments of every pagk_frame_handover* entry point; the candidates' source goes between them.
    outs: keys, keys_un, keys_normal, index_in_last, live, mask, state and, for a detecting form, info.  The device forms
    share one guard."""
    if device and cap < target_n:
        raise ValueError("cap must be at least target_n")
    head = (h, C.byref(params), width, height, cap, target_n, float(new_point_threshold), _ptr(status), _ptr(pt_predict),
            _ptr(pt_predict_un))
    return head, tuple(_ptr(a) for a in outs)


def _handover_host_arrays(width, height, cap, status, pt_predict, pt_predict_un, state, with_info: bool):
    """The host forms' shared part -> ((status, pt_predict, pt_predict_un) padded to cap, the dictionary that the call fills
    and returns: its values in the order of _handover_args' outs, `state` a copy)."""
    def pad(a, dtype, width_):
        out = np.zeros((cap, width_) if width_ > 1 else (cap,), dtype)
        a = np.asarray(a, dtype).reshape((-1, width_) if width_ > 1 else (-1,))
        if a.shape[0] > cap:
            raise ValueError("more entries than cap")
        out[:a.shape[0]] = a
        return out
    ins = pad(status, np.uint8, 1), pad(pt_predict, np.float32, 2), pad(pt_predict_un, np.float32, 2)
    state = np.zeros(HANDOVER_STATE_WORDS, np.int32) if state is None else np.array(state, np.int32, copy=True)
    out = dict(keys=np.zeros((cap, 2), np.float32), keys_un=np.zeros((cap, 2), np.float32),
               keys_normal=np.zeros((cap, 2), np.float32), index_in_last=np.zeros(cap, np.int32),
               live=np.zeros(cap, np.uint8), mask=np.zeros((height, width), np.uint8), state=state)
    if with_info:
        out["info"] = np.zeros(DETECT_INFO_WORDS, np.int32)
    return ins, out


class Context:
    """pagk_ctx owner.  One per GPU / host thread."""

    def __init__(self, device: int = 0, _borrowed=None):
        self.lib = load()
        self._owned = _borrowed is None
        if _borrowed is not None:          # a member context of a Multi group: the group destroys it
            self.h = C.c_void_p(_borrowed)
            return
        h = C.c_void_p()
        rc = self.lib.pagk_create(C.byref(h), device)
        if rc != PAGK_OK:
            raise PagkError(rc, "pagk_create")
        self.h = h

    def close(self):
        if getattr(self, "h", None):
            if self._owned:
                self.lib.pagk_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _check(self, rc: int, where: str):
        if rc != PAGK_OK:
            raise PagkError(rc, where, self.lib.pagk_last_error(self.h).decode())

    # host-buffer path ------------------------------------------------------------------
    def track(self, params: Params, img_ref, img_cur, pt_ref, pt_init, affine, status_in, out: dict | None = None):
        n = int(pt_ref.shape[0])
        out = out if out is not None else alloc_outputs(n)
        ir, ic = image_view(img_ref), image_view(img_cur)
        o = outputs_struct(out)
        self._check(self.lib.pagk_track(self.h, C.byref(params), C.byref(ir), C.byref(ic), n, _ptr(pt_ref),
                                        _ptr(pt_init), _ptr(affine), _ptr(status_in), C.byref(o)), "pagk_track")
        return out

    def track_pyr(self, params: Params, ref_levels, cur_levels, pt_ref, pt_init, affine, status_in, out=None):
        n = int(pt_ref.shape[0])
        out = out if out is not None else alloc_outputs(n)
        L = len(ref_levels)
        r = (Image * L)(*[image_view(a) for a in ref_levels])
        c = (Image * L)(*[image_view(a) for a in cur_levels])
        o = outputs_struct(out)
        self._check(self.lib.pagk_track_pyr(self.h, C.byref(params), L, r, c, n, _ptr(pt_ref), _ptr(pt_init),
                                            _ptr(affine), _ptr(status_in), C.byref(o)), "pagk_track_pyr")
        return out

    # device-resident path --------------------------------------------------------------
    def frame_upload(self, slot: int, img: np.ndarray, pyramids: int):
        iv = image_view(img)
        self._check(self.lib.pagk_frame_upload(self.h, slot, C.byref(iv), pyramids), "pagk_frame_upload")

    def frame_upload_pinned(self, slot: int, host_ptr: int, width: int, height: int, step: int, pyramids: int):
        """pagk_frame_upload_pinned: asynchronous / capturable upload of a frame that lives in pinned host memory."""
        iv = Image(host_ptr, width, height, step)
        self._check(self.lib.pagk_frame_upload_pinned(self.h, slot, C.byref(iv), pyramids), "pagk_frame_upload_pinned")

    def frame_set_device(self, slot: int, d_ptr: int, width: int, height: int, step: int, pyramids: int):
        self._check(self.lib.pagk_frame_set_device(self.h, slot, d_ptr, width, height, step, pyramids),
                    "pagk_frame_set_device")

    def frame_download_level(self, slot: int, level: int, width: int, height: int) -> np.ndarray:
        w, h = C.c_int32(0), C.c_int32(0)
        buf = np.zeros((height >> level, width >> level), np.uint8)
        self._check(self.lib.pagk_frame_download_level(self.h, slot, level, buf.ctypes.data, C.byref(w), C.byref(h)),
                    "pagk_frame_download_level")
        assert (h.value, w.value) == buf.shape
        return buf

    def track_device(self, params: Params, slot_ref: int, slot_cur: int, n: int, d_pt_ref, d_pt_init, d_affine,
                     d_status, d_out: dict):
        o = outputs_struct(d_out)
        self._check(self.lib.pagk_track_device(self.h, C.byref(params), slot_ref, slot_cur, n, _ptr(d_pt_ref),
                                               _ptr(d_pt_init), _ptr(d_affine), _ptr(d_status), C.byref(o)),
                    "pagk_track_device")

    @staticmethod
    def frame_set_device_batch(ctxs, slots, d_ptrs, widths, heights, steps, pyramids: int):
        """pagk_frame_set_device_batch: the pyramids of k contexts' frames (device images) as ONE launch on ctxs[0]'s
        stream; per frame the same bytes as frame_set_device."""
        k = len(ctxs)
        lib = ctxs[0].lib
        hs = (C.c_void_p * k)(*[c.h for c in ctxs])
        sl = (C.c_int32 * k)(*slots)
        pp = (C.c_void_p * k)(*[int(p) for p in d_ptrs])
        ww, hh = (C.c_int32 * k)(*widths), (C.c_int32 * k)(*heights)
        st = (C.c_int64 * k)(*steps)
        ctxs[0]._check(lib.pagk_frame_set_device_batch(hs, k, sl, pp, ww, hh, st, pyramids), "pagk_frame_set_device_batch")

    @staticmethod
    def track_device_batch(ctxs, params: Params, slots_ref, slots_cur, ns, d_pt_ref, d_pt_init, d_affine, d_status, d_outs):
        """pagk_track_device_batch: k camera streams (contexts `ctxs`, all on one device) as ONE launch, issued on
        ctxs[0]'s stream.  Per stream j: frame slots, feature count and device arrays (torch tensors / addresses) as for
        track_device; d_pt_init / d_affine may be None."""
        k = len(ctxs)
        lib = ctxs[0].lib
        hs = (C.c_void_p * k)(*[c.h for c in ctxs])
        sr, sc, nn = (C.c_int32 * k)(*slots_ref), (C.c_int32 * k)(*slots_cur), (C.c_int32 * k)(*ns)

        def ptrs(lst):
            return None if lst is None else (C.c_void_p * k)(*[_ptr(t) for t in lst])
        outs = (Outputs * k)(*[outputs_struct(o) for o in d_outs])
        rc = lib.pagk_track_device_batch(hs, k, C.byref(params), sr, sc, nn, ptrs(d_pt_ref), ptrs(d_pt_init), ptrs(d_affine),
                                         ptrs(d_status), outs)
        ctxs[0]._check(rc, "pagk_track_device_batch")

    def track_device_fused(self, params: Params, slot_ref: int, slot_cur: int, n: int, d_pt_ref, d_pt_init, d_affine,
                           d_status, d_out: dict, slot_next: int, d_next_ptr: int, width: int, height: int, step: int,
                           pyramids: int):
        """pagk_track_device + the pyramid of another frame into slot_next, one launch when possible."""
        o = outputs_struct(d_out)
        self._check(self.lib.pagk_track_device_fused(self.h, C.byref(params), slot_ref, slot_cur, n, _ptr(d_pt_ref),
                                                     _ptr(d_pt_init), _ptr(d_affine), _ptr(d_status), C.byref(o),
                                                     slot_next, d_next_ptr, width, height, step, pyramids),
                    "pagk_track_device_fused")

    def gyro_predict_device(self, params: Params, width: int, height: int, KRKinv, r3, n: int, d_pt_ref,
                            d_pt_predict_un, d_pt_predict, d_status, d_affine):
        K = np.ascontiguousarray(KRKinv, np.float32)
        r = np.ascontiguousarray(r3, np.float32)
        self._check(self.lib.pagk_gyro_predict_device(self.h, C.byref(params), width, height, K.ctypes.data,
                                                      r.ctypes.data, n, _ptr(d_pt_ref), _ptr(d_pt_predict_un),
                                                      _ptr(d_pt_predict), _ptr(d_status), _ptr(d_affine)),
                    "pagk_gyro_predict_device")

    @staticmethod
    def _mat3(M):
        M = np.ascontiguousarray(M, np.float64)
        if M.size != 9:
            raise ValueError("expected a 3x3 matrix")
        return M

    def geometry_scores_device(self, H21, H12, F21, n: int, d_pts1, d_pts2, sigma: float, d_inl_H, d_inl_F,
                               d_scores):
        """CheckHomography / CheckFundamental scoring loops on device arrays (asynchronous)."""
        H21, H12, F21 = self._mat3(H21), self._mat3(H12), self._mat3(F21)
        self._check(self.lib.pagk_geometry_scores_device(self.h, H21.ctypes.data, H12.ctypes.data, F21.ctypes.data,
                                                         n, _ptr(d_pts1), _ptr(d_pts2), sigma, _ptr(d_inl_H),
                                                         _ptr(d_inl_F), _ptr(d_scores)),
                    "pagk_geometry_scores_device")

    def geometry_scores(self, H21, H12, F21, pts1, pts2, sigma: float = 1.0):
        """Host buffers -> (inliers_H, inliers_F, score_H, score_F); reference
        src/gyro_aided_tracker.cpp:620-676, 704-768."""
        H21, H12, F21 = self._mat3(H21), self._mat3(H12), self._mat3(F21)
        pts1 = np.ascontiguousarray(pts1, np.float32).reshape(-1, 2)
        pts2 = np.ascontiguousarray(pts2, np.float32).reshape(-1, 2)
        n = pts1.shape[0]
        if pts2.shape[0] != n:
            raise ValueError("pts1 / pts2 differ in length")
        inH, inF = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
        sH, sF = C.c_float(0), C.c_float(0)
        self._check(self.lib.pagk_geometry_scores(self.h, H21.ctypes.data, H12.ctypes.data, F21.ctypes.data, n,
                                                  _ptr(pts1), _ptr(pts2), sigma, _ptr(inH), _ptr(inF),
                                                  C.byref(sH), C.byref(sF)), "pagk_geometry_scores")
        return inH[:n], inF[:n], np.float32(sH.value), np.float32(sF.value)

    def geometry_validation(self, H21, H12, F21, pt_ref_un, pt_predict_un, status, sigma: float = 1.0):
        """GyroAidedTracker::GeometryValidation around externally fitted models
        (src/gyro_aided_tracker.cpp:429-480) -> (cnt_inlier, status, track_score)."""
        H21, H12, F21 = self._mat3(H21), self._mat3(H12), self._mat3(F21)
        p1 = np.ascontiguousarray(pt_ref_un, np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(pt_predict_un, np.float32).reshape(-1, 2)
        st = np.array(status, np.uint8, copy=True)
        n = st.shape[0]
        ts = C.c_float(0)
        rc = self.lib.pagk_geometry_validation(self.h, H21.ctypes.data, H12.ctypes.data, F21.ctypes.data, n,
                                               _ptr(p1), _ptr(p2), _ptr(st), sigma, C.byref(ts))
        if rc < 0:
            self._check(rc, "pagk_geometry_validation")
        return rc, st, np.float32(ts.value)

    # the RANSAC fits of GeometryValidation on the device (src/gyro_aided_tracker.cpp:429-480, 589-768) ------------
    fit_params_default = staticmethod(fit_params_default)

    def geometry_fit(self, pts1, pts2, status=None, params: FitParams | None = None, hyp_counts: bool = False):
        """Deterministic RANSAC fits of H21 and F21 (include/pagk.h pagk_geometry_fit), host buffers -> dict(H21, H12,
        F21, mask_H, mask_F, info, H / F: the info words by name, hyp_counts when asked for)."""
        params = params if params is not None else fit_params_default()
        pts1 = np.ascontiguousarray(pts1, np.float32).reshape(-1, 2)
        pts2 = np.ascontiguousarray(pts2, np.float32).reshape(-1, 2)
        n = pts1.shape[0]
        if pts2.shape[0] != n:
            raise ValueError("pts1 / pts2 differ in length")
        st = None if status is None else np.ascontiguousarray(status, np.uint8)
        if st is not None and st.shape[0] != n:
            raise ValueError("status has the wrong length")
        models = np.zeros(27, np.float64)
        mH, mF = np.zeros(max(n, 1), np.uint8), np.zeros(max(n, 1), np.uint8)
        info = np.zeros(FIT_INFO_WORDS, np.int32)
        hc = np.zeros(params.iters_H + params.iters_F, np.int32) if hyp_counts else None
        self._check(self.lib.pagk_geometry_fit(self.h, C.byref(params), n, _ptr(pts1), _ptr(pts2), _ptr(st),
                                               _ptr(models), _ptr(mH), _ptr(mF), _ptr(info), _ptr(hc)),
                    "pagk_geometry_fit")
        out = dict(models=models, H21=models[:9].reshape(3, 3), H12=models[9:18].reshape(3, 3),
                   F21=models[18:].reshape(3, 3), mask_H=mH[:n], mask_F=mF[:n], info=info,
                   H=dict(zip(FIT_INFO_FIELDS, info[:6].tolist())), F=dict(zip(FIT_INFO_FIELDS, info[6:].tolist())))
        if hc is not None:
            out["hyp_counts"] = hc
        return out

    def geometry_fit_device(self, params: FitParams, n: int, d_pts1, d_pts2, d_status, d_models, d_mask_H, d_mask_F,
                            d_info, d_hyp_counts=None):
        """pagk_geometry_fit_device on device arrays (asynchronous, capturable)."""
        self._check(self.lib.pagk_geometry_fit_device(self.h, C.byref(params), n, _ptr(d_pts1), _ptr(d_pts2),
                                                      _ptr(d_status), _ptr(d_models), _ptr(d_mask_H), _ptr(d_mask_F),
                                                      _ptr(d_info), _ptr(d_hyp_counts)), "pagk_geometry_fit_device")

    def geometry_validation_fit(self, pt_ref_un, pt_predict_un, status, sigma: float = 1.0,
                                params: FitParams | None = None):
        """GyroAidedTracker::GeometryValidation with the device fits (src/gyro_aided_tracker.cpp:429-480)
        -> (cnt_inlier, status, track_score)."""
        params = params if params is not None else fit_params_default()
        p1 = np.ascontiguousarray(pt_ref_un, np.float32).reshape(-1, 2)
        p2 = np.ascontiguousarray(pt_predict_un, np.float32).reshape(-1, 2)
        st = np.array(status, np.uint8, copy=True)
        ts = C.c_float(0)
        rc = self.lib.pagk_geometry_validation_fit(self.h, C.byref(params), st.shape[0], _ptr(p1), _ptr(p2), _ptr(st),
                                                   sigma, C.byref(ts))
        if rc < 0:
            self._check(rc, "pagk_geometry_validation_fit")
        return rc, st, np.float32(ts.value)

    def geometry_validation_device(self, params: FitParams, n: int, d_pt_ref_un, d_pt_predict_un, d_status,
                                   sigma: float, d_cnt, d_score):
        """pagk_geometry_validation_device: d_status updated in place, d_cnt (int32) and d_score (float32) written;
        asynchronous, capturable."""
        self._check(self.lib.pagk_geometry_validation_device(self.h, C.byref(params), n, _ptr(d_pt_ref_un),
                                                             _ptr(d_pt_predict_un), _ptr(d_status), sigma, _ptr(d_cnt),
                                                             _ptr(d_score)), "pagk_geometry_validation_device")

    def selftest_fit_samples(self, seed: int, model: int, m: int, first: int, count: int) -> np.ndarray:
        """The drawn index sets of hypotheses [first, first + count) of model 0 (H, 4 each), 1 (F, 8 each) or 2 (E, 5 each)."""
        out = np.zeros((max(count, 1), 5 if model == 2 else 8 if model else 4), np.int32)
        self._check(self.lib.pagk_selftest_fit_samples(self.h, seed, model, m, first, count, _ptr(out)),
                    "pagk_selftest_fit_samples")
        return out[:count]

    # the two-view pose (src/ORBDetectAndDespMatcher.cpp:84-108) ----------------------------------------------------
    pose_params_default = staticmethod(pose_params_default)

    def pose_2d2d(self, pts1, pts2, f: float, cx: float, cy: float, status=None, params: PoseParams | None = None,
                  cand_counts: bool = False) -> dict:
        """PoseEstimation2d2d (include/pagk.h pagk_pose_2d2d), host buffers -> dict(models, H21, H12, F21, pose, E, R, t,
        mask_H, mask_F, mask_E, mask_pose, fit_info, pose_info, info: the pose words by name, cand_counts when asked for)."""
        params = params if params is not None else pose_params_default()
        pts1 = np.ascontiguousarray(pts1, np.float32).reshape(-1, 2)
        pts2 = np.ascontiguousarray(pts2, np.float32).reshape(-1, 2)
        n = pts1.shape[0]
        if pts2.shape[0] != n:
            raise ValueError("pts1 / pts2 differ in length")
        st = None if status is None else np.ascontiguousarray(status, np.uint8)
        if st is not None and st.shape[0] != n:
            raise ValueError("status has the wrong length")
        models, pose = np.zeros(27, np.float64), np.zeros(21, np.float64)
        masks = [np.zeros(max(n, 1), np.uint8) for _ in range(4)]
        fi, pi = np.zeros(FIT_INFO_WORDS, np.int32), np.zeros(POSE_INFO_WORDS, np.int32)
        cc = np.zeros((params.iters_E, 10), np.int32) if cand_counts else None
        self._check(self.lib.pagk_pose_2d2d(self.h, C.byref(params), f, cx, cy, n, _ptr(pts1), _ptr(pts2), _ptr(st),
                                            _ptr(models), _ptr(pose), *[_ptr(m) for m in masks], _ptr(fi), _ptr(pi),
                                            _ptr(cc)), "pagk_pose_2d2d")
        out = dict(models=models, H21=models[:9].reshape(3, 3), H12=models[9:18].reshape(3, 3), F21=models[18:].reshape(3, 3),
                   pose=pose, E=pose[:9].reshape(3, 3), R=pose[9:18].reshape(3, 3), t=pose[18:], mask_H=masks[0][:n],
                   mask_F=masks[1][:n], mask_E=masks[2][:n], mask_pose=masks[3][:n], fit_info=fi, pose_info=pi,
                   info=dict(zip(POSE_INFO_FIELDS, pi.tolist())))
        if cc is not None:
            out["cand_counts"] = cc
        return out

    def pose_2d2d_device(self, params: PoseParams, f: float, cx: float, cy: float, n: int, d_pts1, d_pts2, d_status, d_models,
                         d_pose, d_mask_H, d_mask_F, d_mask_E, d_mask_pose, d_fit_info, d_pose_info, d_cand_counts=None):
        """pagk_pose_2d2d_device on device arrays (asynchronous, capturable)."""
        self._check(self.lib.pagk_pose_2d2d_device(self.h, C.byref(params), f, cx, cy, n, _ptr(d_pts1), _ptr(d_pts2),
                                                   _ptr(d_status), _ptr(d_models), _ptr(d_pose), _ptr(d_mask_H),
                                                   _ptr(d_mask_F), _ptr(d_mask_E), _ptr(d_mask_pose), _ptr(d_fit_info),
                                                   _ptr(d_pose_info), _ptr(d_cand_counts)), "pagk_pose_2d2d_device")

    def pose_from_matches_device(self, params: PoseParams, f: float, cx: float, cy: float, cap_q: int, d_kp_ref, d_nq,
                                 cap_t: int, d_kp_cur, d_nt, d_train_idx, d_keep, d_models, d_pose, d_mask_H, d_mask_F,
                                 d_mask_E, d_mask_pose, d_fit_info, d_pose_info):
        """pagk_pose_from_matches_device behind pagk_orb_match_device (asynchronous, capturable)."""
        self._check(self.lib.pagk_pose_from_matches_device(self.h, C.byref(params), f, cx, cy, cap_q, _ptr(d_kp_ref),
                                                           _ptr(d_nq), cap_t, _ptr(d_kp_cur), _ptr(d_nt), _ptr(d_train_idx),
                                                           _ptr(d_keep), _ptr(d_models), _ptr(d_pose), _ptr(d_mask_H),
                                                           _ptr(d_mask_F), _ptr(d_mask_E), _ptr(d_mask_pose),
                                                           _ptr(d_fit_info), _ptr(d_pose_info)),
                    "pagk_pose_from_matches_device")

    # NCC nearest-neighbour matching ------------------------------
    def find_near_neighbors(self, img_ref, img_cur, half_patch, keys_ref, pt_predict_un, status, affine, keys_cur,
                            keys_cur_un, level=1, radius_unit=None, use_ncc=True, cap=64, count=None):
        """FindAndSortNearNeighbor (reference src/gyro_aided_tracker.cpp:788-851), host buffers ->
        dict(count, idx, dist, ncc, rc); rc is PAGK_OK or PAGK_E_CAPACITY (count then holds the sizes needed)."""
        n, m = int(keys_ref.shape[0]), int(keys_cur.shape[0])
        ir, ic = image_view(img_ref), image_view(img_cur)
        count = np.zeros(max(n, 1), np.int32) if count is None else np.array(count, np.int32, copy=True)
        idx = np.full((max(n, 1), cap), -1, np.int32)
        dist = np.zeros((max(n, 1), cap), np.float32)
        ncc = np.zeros((max(n, 1), cap), np.float32)
        ru = float(2 * half_patch) if radius_unit is None else float(radius_unit)
        rc = self.lib.pagk_find_near_neighbors(self.h, C.byref(ir), C.byref(ic), half_patch, n, _ptr(keys_ref),
                                               _ptr(pt_predict_un), _ptr(status), _ptr(affine), m, _ptr(keys_cur),
                                               _ptr(keys_cur_un), level, ru, int(use_ncc), cap, _ptr(count), _ptr(idx),
                                               _ptr(dist), _ptr(ncc))
        if rc not in (PAGK_OK, PAGK_E_CAPACITY):
            self._check(rc, "pagk_find_near_neighbors")
        return dict(count=count[:n], idx=idx[:n], dist=dist[:n], ncc=ncc[:n], rc=rc)

    def near_neighbors_device(self, slot_ref, slot_cur, half_patch, n, d_keys_ref, d_pt_predict_un, d_status, d_affine,
                              m, d_keys_cur, d_keys_cur_un, level, radius_unit, use_ncc, cap, d_count, d_idx, d_dist,
                              d_ncc):
        self._check(self.lib.pagk_near_neighbors_device(self.h, slot_ref, slot_cur, half_patch, n, _ptr(d_keys_ref),
                                                        _ptr(d_pt_predict_un), _ptr(d_status), _ptr(d_affine), m,
                                                        _ptr(d_keys_cur), _ptr(d_keys_cur_un), level, float(radius_unit),
                                                        int(use_ncc), cap, _ptr(d_count), _ptr(d_idx), _ptr(d_dist),
                                                        _ptr(d_ncc)), "pagk_near_neighbors_device")

    def ncc_free(self, img_ref, img_cur, half_patch, pt_ref, pt_cur, affine=None) -> np.ndarray:
        """The free NCC of reference src/utils.cpp:166-200 for n point pairs (host buffers)."""
        n = int(pt_ref.shape[0])
        ir, ic = image_view(img_ref), image_view(img_cur)
        out = np.zeros(max(n, 1), np.float32)
        self._check(self.lib.pagk_ncc_free(self.h, C.byref(ir), C.byref(ic), half_patch, n, _ptr(pt_ref), _ptr(pt_cur),
                                           _ptr(affine), _ptr(out)), "pagk_ncc_free")
        return out[:n]

    def selftest_divide(self, num: np.ndarray, den: np.ndarray):
        """(num / den, the same through the prepared-denominator form, sqrt(num), sqrt(num) through the solve's lean form)
        computed on the device."""
        num, den = np.ascontiguousarray(num, np.float64), np.ascontiguousarray(den, np.float64)
        n = int(num.shape[0])
        qp, qq, rt, rl = (np.zeros(max(n, 1), np.float64) for _ in range(4))
        self._check(self.lib.pagk_selftest_divide(self.h, n, _ptr(num), _ptr(den), _ptr(qp), _ptr(qq), _ptr(rt), _ptr(rl)),
                    "pagk_selftest_divide")
        return qp[:n], qq[:n], rt[:n], rl[:n]

    def selftest_repeat_sum(self, c: np.ndarray, count: int):
        """(closed form, loop) of the ordered sum of `count` copies of c*c on the device (pagk_selftest_repeat_sum)."""
        c = np.ascontiguousarray(c, dtype=np.float32)
        n = c.shape[0]
        closed, loop = np.empty(n, np.float64), np.empty(n, np.float64)
        self._check(self.lib.pagk_selftest_repeat_sum(self.h, n, _ptr(c), int(count), _ptr(closed), _ptr(loop)),
                    "pagk_selftest_repeat_sum")
        return closed, loop

    def selftest_sample(self, slot: int, level: int, mode: int, xy: np.ndarray) -> np.ndarray:
        """pagk_selftest_sample: the device sampler on a built slot's level at the (x, y) rows of `xy`.  mode 0 / 1: the
        clamped / clamp-free sample, n floats; mode 2 / 3: the five samples of a Gauss-Newton pixel, n x 5 floats."""
        xy = np.ascontiguousarray(xy, np.float32).reshape(-1, 2)
        n = int(xy.shape[0])
        out = np.zeros((max(n, 1), 5) if mode >= 2 else max(n, 1), np.float32)
        self._check(self.lib.pagk_selftest_sample(self.h, int(slot), int(level), int(mode), n, _ptr(xy), _ptr(out)),
                    "pagk_selftest_sample")
        return out[:n]

    def selftest_fill_workspaces(self, word: int, also_new: bool = False) -> None:
        """pagk_selftest_fill_workspaces: the scratch this context owns becomes the 32-bit `word` (no frame slot is valid and no
        slot has a Lucas-Kanade pyramid afterwards); also_new: so does every block the library allocates from now on."""
        self._check(self.lib.pagk_selftest_fill_workspaces(self.h, int(word) & 0xFFFFFFFF, int(bool(also_new))),
                    "pagk_selftest_fill_workspaces")

    def selftest_solve(self, H: np.ndarray, b: np.ndarray, solver_variant: int = 0):
        """H.llt().solve(b) and the update's norm for n 4x4 systems: (x, norm) of the one-lane form and
        (x, squared norm) of the four-lane form."""
        H, b = np.ascontiguousarray(H, np.float64), np.ascontiguousarray(b, np.float64)
        n = int(H.shape[0])
        xs, xl = np.zeros((max(n, 1), 4)), np.zeros((max(n, 1), 4))
        ns, nl = np.zeros(max(n, 1)), np.zeros(max(n, 1))
        self._check(self.lib.pagk_selftest_solve(self.h, n, _ptr(H), _ptr(b), int(solver_variant), _ptr(xs), _ptr(ns),
                                                 _ptr(xl), _ptr(nl)), "pagk_selftest_solve")
        return xs[:n], ns[:n], xl[:n], nl[:n]

    def gyro_predict_device_rot(self, params: Params, width: int, height: int, d_rot, n: int, d_pt_ref,
                                d_pt_predict_un, d_pt_predict, d_status, d_affine):
        """Prediction with the rotation (KRKinv rows 0-1, r3: 9 floats) in device memory: capturable per frame."""
        self._check(self.lib.pagk_gyro_predict_device_rot(self.h, C.byref(params), width, height, _ptr(d_rot), n,
                                                          _ptr(d_pt_ref), _ptr(d_pt_predict_un), _ptr(d_pt_predict),
                                                          _ptr(d_status), _ptr(d_affine)),
                    "pagk_gyro_predict_device_rot")

    def gyro_predict_device_live(self, params: Params, width: int, height: int, d_rot, n: int, d_pt_ref, d_live,
                                 d_pt_predict_un, d_pt_predict, d_status, d_affine):
        """pagk_gyro_predict_device_rot with a live mask: dead slots (d_live[i] == 0) come out as status 0, points (0,0)."""
        if d_rot is None or (n > 0 and d_live is None):
            raise ValueError("d_rot and d_live are required")
        self._check(self.lib.pagk_gyro_predict_device_live(self.h, C.byref(params), width, height, _ptr(d_rot), n,
                                                           _ptr(d_pt_ref), _ptr(d_live), _ptr(d_pt_predict_un),
                                                           _ptr(d_pt_predict), _ptr(d_status), _ptr(d_affine)),
                    "pagk_gyro_predict_device_live")

    # Step 3 and the frame hand-over on the device (include/pagk.h) -----------------------------
    def post_filter_device(self, n: int, half_patch: int, d_status_pm, d_pix_err, d_dist_pred, d_pt_pm, d_pt_pm_un,
                           d_status_out, d_pt_predict, d_pt_predict_un, d_kept, d_thresholds=None):
        """pagk_post_filter_device on device arrays (asynchronous, capturable); d_status_out may be d_status_pm."""
        if d_kept is None:
            raise ValueError("d_kept is required")
        self._check(self.lib.pagk_post_filter_device(self.h, n, half_patch, _ptr(d_status_pm), _ptr(d_pix_err),
                                                     _ptr(d_dist_pred), _ptr(d_pt_pm), _ptr(d_pt_pm_un),
                                                     _ptr(d_status_out), _ptr(d_pt_predict), _ptr(d_pt_predict_un),
                                                     _ptr(d_kept), _ptr(d_thresholds)), "pagk_post_filter_device")

    def frame_handover_device(self, params: Params, width: int, height: int, cap: int, target_n: int,
                              new_point_threshold: float, d_status, d_pt_predict, d_pt_predict_un, cand_cap: int,
                              d_n_cand, d_cand_un, d_keys, d_keys_un, d_keys_normal, d_index_in_last, d_live, d_mask,
                              d_state):
        """pagk_frame_handover_device on device arrays (asynchronous, capturable)."""
        head, tail = _handover_args(self.h, params, width, height, cap, target_n, new_point_threshold, d_status, d_pt_predict,
                                    d_pt_predict_un, d_keys, d_keys_un, d_keys_normal, d_index_in_last, d_live, d_mask, d_state)
        self._check(self.lib.pagk_frame_handover_device(*head, cand_cap, _ptr(d_n_cand), _ptr(d_cand_un), *tail),
                    "pagk_frame_handover_device")

    def frame_handover(self, params: Params, width: int, height: int, cap: int, target_n: int,
                       new_point_threshold: float, status, pt_predict, pt_predict_un, candidates, state=None,
                       cand_cap: int | None = None) -> dict:
        """pagk_frame_handover, host buffers -> dict(keys, keys_un, keys_normal, index_in_last, live, mask, state).
        `state` (8 int32, reach_flag in [1]) is copied, not updated in place; status / points are padded to cap."""
        ins, out = _handover_host_arrays(width, height, cap, status, pt_predict, pt_predict_un, state, False)
        cand = np.ascontiguousarray(candidates, np.float32).reshape(-1, 2)
        cc = cand.shape[0] if cand_cap is None else int(cand_cap)
        if cc < cand.shape[0]:
            raise ValueError("cand_cap is smaller than the candidate list")
        cbuf = np.zeros((max(cc, 1), 2), np.float32)
        cbuf[:cand.shape[0]] = cand
        ncand = np.array([cand.shape[0]], np.int32)
        head, tail = _handover_args(self.h, params, width, height, cap, target_n, new_point_threshold, *ins, *out.values(),
                                    device=False)
        self._check(self.lib.pagk_frame_handover(*head, cc, _ptr(ncand), _ptr(cbuf), *tail), "pagk_frame_handover")
        return out

    # the corner detector (reference src/frame.cpp:156-218: goodFeaturesToTrack with the Harris response) -------
    detect_params_default = staticmethod(detect_params_default)

    def detect_corners_device(self, det: DetectParams, slot: int, d_mask, cap: int, d_max_corners, d_corners, d_info):
        """pagk_detect_corners_device on level 0 of frame slot `slot` (asynchronous, capturable).  d_mask / d_max_corners
        may be None (all ones / cap)."""
        if d_corners is None or d_info is None:
            raise ValueError("d_corners and d_info are required")
        self._check(self.lib.pagk_detect_corners_device(self.h, C.byref(det), slot, _ptr(d_mask), cap, _ptr(d_max_corners),
                                                        _ptr(d_corners), _ptr(d_info)), "pagk_detect_corners_device")

    def detect_corners(self, img: np.ndarray, mask, max_corners: int, det: DetectParams | None = None) -> dict:
        """pagk_detect_corners, host buffers -> dict(corners (the accepted ones, n x 2), buffer (max_corners x 2, zero
        beyond n), info, and the info words by name)."""
        det = det if det is not None else detect_params_default()
        iv = image_view(img)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        if m is not None and m.shape != img.shape:
            raise ValueError("the mask has the wrong shape")
        buf = np.zeros((max(int(max_corners), 1), 2), np.float32)
        info = np.zeros(DETECT_INFO_WORDS, np.int32)
        self._check(self.lib.pagk_detect_corners(self.h, C.byref(det), C.byref(iv), _ptr(m), int(max_corners), _ptr(buf),
                                                 _ptr(info)), "pagk_detect_corners")
        out = dict(corners=buf[:int(info[0])], buffer=buf, info=info)
        out.update(zip(DETECT_INFO_FIELDS, (int(v) for v in info[:5])))
        return out

    def selftest_corner_response(self, img: np.ndarray) -> np.ndarray:
        """The detector's response map R (float32, harris_k = 0.04) of an image, computed on the device."""
        iv = image_view(img)
        R = np.zeros(img.shape, np.float32)
        self._check(self.lib.pagk_selftest_corner_response(self.h, C.byref(iv), _ptr(R)), "pagk_selftest_corner_response")
        return R

    def frame_handover_detect_device(self, params: Params, width: int, height: int, cap: int, target_n: int,
                                     new_point_threshold: float, d_status, d_pt_predict, d_pt_predict_un,
                                     det: DetectParams, slot: int, d_keys, d_keys_un, d_keys_normal, d_index_in_last,
                                     d_live, d_mask, d_state, d_info):
        """pagk_frame_handover_detect_device on device arrays (asynchronous, capturable): the hand-over with the
        candidates detected on level 0 of frame slot `slot` under the mask the call builds."""
        head, tail = _handover_args(self.h, params, width, height, cap, target_n, new_point_threshold, d_status, d_pt_predict,
                                    d_pt_predict_un, d_keys, d_keys_un, d_keys_normal, d_index_in_last, d_live, d_mask, d_state,
                                    d_info)
        self._check(self.lib.pagk_frame_handover_detect_device(*head, C.byref(det), slot, *tail),
                    "pagk_frame_handover_detect_device")

    def frame_handover_detect(self, params: Params, img: np.ndarray, cap: int, target_n: int, new_point_threshold: float,
                              status, pt_predict, pt_predict_un, det: DetectParams | None = None, state=None) -> dict:
        """pagk_frame_handover_detect, host buffers -> dict(keys, keys_un, keys_normal, index_in_last, live, mask, state,
        info).  `state` is copied, not updated in place; status / points are padded to cap."""
        det = det if det is not None else detect_params_default()
        height, width = img.shape
        ins, out = _handover_host_arrays(width, height, cap, status, pt_predict, pt_predict_un, state, True)
        iv = image_view(img)
        head, tail = _handover_args(self.h, params, width, height, cap, target_n, new_point_threshold, *ins, *out.values(),
                                    device=False)
        self._check(self.lib.pagk_frame_handover_detect(*head, C.byref(det), C.byref(iv), *tail), "pagk_frame_handover_detect")
        return out

    # the detector of the reference's front-ends (src/ORBextractor.cc:1148-1205: FAST in cells, then the quadtree) ----
    fast_params_default = staticmethod(fast_params_default)
    detect_fast_bounds = staticmethod(detect_fast_bounds)

    def detect_fast_device(self, fast: FastParams, slot: int, d_mask, cap: int, d_keypoints, d_response, d_info):
        """pagk_detect_fast_device on level 0 of frame slot `slot` (asynchronous, capturable).  d_mask / d_response may be
        None.  cap >= detect_fast_bounds(...)[1]."""
        if d_keypoints is None or d_info is None:
            raise ValueError("d_keypoints and d_info are required")
        self._check(self.lib.pagk_detect_fast_device(self.h, C.byref(fast), slot, _ptr(d_mask), cap, _ptr(d_keypoints),
                                                     _ptr(d_response), _ptr(d_info)), "pagk_detect_fast_device")

    def detect_fast(self, img: np.ndarray, mask, n_features: int, fast: FastParams | None = None, cap: int | None = None) -> dict:
        """pagk_detect_fast, host buffers -> dict(keypoints (the returned ones, n x 2), response (n), buffer and
        response_buffer (cap entries, zero beyond n), info, and the info words by name)."""
        fast = fast if fast is not None else fast_params_default()
        fp = FastParams(fast.ini_threshold, fast.min_threshold, int(n_features), fast.n_levels)
        iv = image_view(img)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        if m is not None and m.shape != img.shape:
            raise ValueError("the mask has the wrong shape")
        if cap is None:
            cap = detect_fast_bounds(img.shape[1], img.shape[0], n_features)[1]
        buf, resp = np.zeros((max(int(cap), 1), 2), np.float32), np.zeros(max(int(cap), 1), np.float32)
        info = np.zeros(DETECT_INFO_WORDS, np.int32)
        self._check(self.lib.pagk_detect_fast(self.h, C.byref(fp), C.byref(iv), _ptr(m), int(cap), _ptr(buf), _ptr(resp),
                                              _ptr(info)), "pagk_detect_fast")
        n = int(info[0])
        out = dict(keypoints=buf[:n], response=resp[:n], buffer=buf, response_buffer=resp, info=info)
        out.update(zip(FAST_INFO_FIELDS, (int(v) for v in info[:6])))
        return out

    def selftest_fast_cells(self, img: np.ndarray, fast: FastParams | None = None) -> dict:
        """pagk_selftest_fast_cells -> dict(xy (n x 2, relative to minBorder), score (n), n): the raw list in its order."""
        fast = fast if fast is not None else fast_params_default()
        iv = image_view(img)
        rb = detect_fast_bounds(img.shape[1], img.shape[0], 1)[0]
        xy, sc, n = np.zeros((rb, 2), np.float32), np.zeros(rb, np.int32), C.c_int32(0)
        self._check(self.lib.pagk_selftest_fast_cells(self.h, C.byref(fast), C.byref(iv), _ptr(xy), _ptr(sc), C.byref(n)),
                    "pagk_selftest_fast_cells")
        return dict(xy=xy[:n.value].copy(), score=sc[:n.value].copy(), n=n.value)

    def frame_handover_fast_device(self, params: Params, width: int, height: int, cap: int, target_n: int,
                                   new_point_threshold: float, d_status, d_pt_predict, d_pt_predict_un, fast: FastParams,
                                   slot: int, d_keys, d_keys_un, d_keys_normal, d_index_in_last, d_live, d_mask, d_state,
                                   d_info):
        """pagk_frame_handover_fast_device on device arrays (asynchronous, capturable): the hand-over with the
        candidates = the FAST-and-quadtree detector's output on level 0 of frame slot `slot`."""
        head, tail = _handover_args(self.h, params, width, height, cap, target_n, new_point_threshold, d_status, d_pt_predict,
                                    d_pt_predict_un, d_keys, d_keys_un, d_keys_normal, d_index_in_last, d_live, d_mask, d_state,
                                    d_info)
        self._check(self.lib.pagk_frame_handover_fast_device(*head, C.byref(fast), slot, *tail),
                    "pagk_frame_handover_fast_device")

    def frame_handover_fast(self, params: Params, img: np.ndarray, cap: int, target_n: int, new_point_threshold: float,
                            status, pt_predict, pt_predict_un, fast: FastParams | None = None, state=None) -> dict:
        """pagk_frame_handover_fast, host buffers -> dict(keys, keys_un, keys_normal, index_in_last, live, mask, state,
        info).  `state` is copied, not updated in place; status / points are padded to cap."""
        fast = fast if fast is not None else fast_params_default()
        height, width = img.shape
        ins, out = _handover_host_arrays(width, height, cap, status, pt_predict, pt_predict_un, state, True)
        iv = image_view(img)
        head, tail = _handover_args(self.h, params, width, height, cap, target_n, new_point_threshold, *ins, *out.values(),
                                    device=False)
        self._check(self.lib.pagk_frame_handover_fast(*head, C.byref(fast), C.byref(iv), *tail), "pagk_frame_handover_fast")
        return out

    # rectification: a raw camera frame (distorted, 1 / 3 / 4 channels) into a frame slot ----
    def rectify_set_maps(self, map_x: np.ndarray, map_y: np.ndarray):
        """pagk_rectify_set_maps: two float32 planes of one shape (rows may be strided, elements not)."""
        if map_x.dtype != np.float32 or map_y.dtype != np.float32 or map_x.ndim != 2 or map_x.shape != map_y.shape:
            raise ValueError("the maps are two float32 planes of one shape")
        if map_x.strides != map_y.strides or map_x.strides[1] != 4:
            raise ValueError("the maps must share one row step and have dense rows")
        self._check(self.lib.pagk_rectify_set_maps(self.h, map_x.ctypes.data, map_y.ctypes.data, map_x.shape[1],
                                                   map_x.shape[0], map_x.strides[0]), "pagk_rectify_set_maps")
        self._rect_shape = map_x.shape

    def frame_rectify_device(self, slot: int, rp: RectifyParams, d_raw_ptr: int, src_width: int, src_height: int,
                             src_step: int, pyramids: int):
        """pagk_frame_rectify_device: raw frame in device memory -> rectified gray level 0 of `slot` -> its pyramid
        (asynchronous, capturable)."""
        self._check(self.lib.pagk_frame_rectify_device(self.h, slot, C.byref(rp), d_raw_ptr, src_width, src_height,
                                                       src_step, pyramids), "pagk_frame_rectify_device")

    def frame_rectify_pinned(self, slot: int, rp: RectifyParams, host_ptr: int, src_width: int, src_height: int,
                             src_step: int, pyramids: int):
        """pagk_frame_rectify_pinned: the same for a raw frame in pinned host memory (asynchronous, capturable)."""
        self._check(self.lib.pagk_frame_rectify_pinned(self.h, slot, C.byref(rp), host_ptr, src_width, src_height,
                                                       src_step, pyramids), "pagk_frame_rectify_pinned")

    def rectify(self, rp: RectifyParams, raw: np.ndarray) -> np.ndarray:
        """pagk_rectify, host buffers: raw is Hs x Ws (channels 1) or Hs x Ws x channels uint8, rows may be strided;
        returns the rectified gray image of the maps' size (rectify_set_maps)."""
        cn = int(rp.channels)
        if raw.dtype != np.uint8 or raw.ndim not in (2, 3) or (raw.ndim == 3 and raw.shape[2] != cn) or (raw.ndim == 2 and cn != 1):
            raise ValueError("raw must be uint8, Hs x Ws or Hs x Ws x channels")
        if raw.strides[-1] != 1 or (raw.ndim == 3 and raw.strides[1] != cn):
            raise ValueError("the pixels of a row must be dense")
        if not getattr(self, "_rect_shape", None):
            raise ValueError("rectify_set_maps first")
        dst = np.zeros(self._rect_shape, np.uint8)
        self._check(self.lib.pagk_rectify(self.h, C.byref(rp), raw.ctypes.data, raw.shape[1], raw.shape[0], raw.strides[0],
                                          dst.ctypes.data, dst.strides[0]), "pagk_rectify")
        return dst

    # ORB descriptors and matching (src/ORBextractor.cc:101-171, 1113-1130; src/ORBDetectAndDespMatcher.cpp:55-91) ----
    orb_params_default = staticmethod(orb_params_default)

    def orb_set_pattern(self, pattern):
        """pagk_orb_set_pattern: 512 sampling points as 1024 integers (x then y), every one in [-13, 13]."""
        self._check(self.lib.pagk_orb_set_pattern(self.h, _orb_pattern(pattern).ctypes.data), "pagk_orb_set_pattern")

    def orb_describe_device(self, orb: OrbParams, slot: int, cap: int, d_keypoints, d_n, d_angle, d_desc, d_info):
        """pagk_orb_describe_device on level 0 of frame slot `slot` (asynchronous, capturable): d_keypoints cap x 2 float
        and the device count d_n as pagk_detect_fast_device writes them; d_angle may be None."""
        if d_keypoints is None or d_n is None or d_desc is None or d_info is None:
            raise ValueError("d_keypoints, d_n, d_desc and d_info are required")
        self._check(self.lib.pagk_orb_describe_device(self.h, C.byref(orb), slot, cap, _ptr(d_keypoints), _ptr(d_n),
                                                      _ptr(d_angle), _ptr(d_desc), _ptr(d_info)), "pagk_orb_describe_device")

    def orb_describe(self, img: np.ndarray, keypoints, orb: OrbParams | None = None) -> dict:
        """pagk_orb_describe, host buffers -> dict(angle (n), desc (n x 32), info, and the info words by name)."""
        orb = orb if orb is not None else orb_params_default()
        kp = np.ascontiguousarray(keypoints, np.float32).reshape(-1, 2)
        n = int(kp.shape[0])
        iv = image_view(img)
        ang, desc = np.zeros(max(n, 1), np.float32), np.zeros((max(n, 1), 32), np.uint8)
        info = np.zeros(ORB_INFO_WORDS, np.int32)
        self._check(self.lib.pagk_orb_describe(self.h, C.byref(orb), C.byref(iv), n, _ptr(kp) if n else None, _ptr(ang),
                                               _ptr(desc), _ptr(info)), "pagk_orb_describe")
        out = dict(angle=ang[:n], desc=desc[:n], info=info)
        out.update(zip(ORB_DESCRIBE_INFO_FIELDS, (int(v) for v in info[:2])))
        return out

    def orb_match_device(self, orb: OrbParams, cap_q: int, d_desc_q, d_nq, cap_t: int, d_desc_t, d_nt, d_train_idx,
                         d_distance, d_keep, d_info):
        """pagk_orb_match_device (asynchronous, capturable): best train row per query row by Hamming distance, the lowest
        index on a tie, and the reference's distance filter; counts are device words."""
        self._check(self.lib.pagk_orb_match_device(self.h, C.byref(orb), cap_q, _ptr(d_desc_q), _ptr(d_nq), cap_t,
                                                   _ptr(d_desc_t), _ptr(d_nt), _ptr(d_train_idx), _ptr(d_distance),
                                                   _ptr(d_keep), _ptr(d_info)), "pagk_orb_match_device")

    def orb_match(self, desc_q, desc_t, orb: OrbParams | None = None) -> dict:
        """pagk_orb_match, host buffers -> dict(train_idx (nq), distance (nq), keep (nq), info, and the info words by name)."""
        orb = orb if orb is not None else orb_params_default()
        dq = np.ascontiguousarray(desc_q, np.uint8).reshape(-1, 32)
        dt = np.ascontiguousarray(desc_t, np.uint8).reshape(-1, 32)
        nq, nt = int(dq.shape[0]), int(dt.shape[0])
        idx, dist = np.zeros(max(nq, 1), np.int32), np.zeros(max(nq, 1), np.int32)
        keep, info = np.zeros(max(nq, 1), np.uint8), np.zeros(ORB_INFO_WORDS, np.int32)
        self._check(self.lib.pagk_orb_match(self.h, C.byref(orb), nq, _ptr(dq) if nq else None, nt, _ptr(dt) if nt else None,
                                            _ptr(idx), _ptr(dist), _ptr(keep), _ptr(info)), "pagk_orb_match")
        out = dict(train_idx=idx[:nq], distance=dist[:nq], keep=keep[:nq], info=info)
        out.update(zip(ORB_MATCH_INFO_FIELDS, (int(v) for v in info[:6])))
        return out

    # ORB over a scale pyramid (src/ORBextractor.cc:434-470, 789-875, 1066-1232) --------------------------------------
    orb_extractor_default = staticmethod(orb_extractor_default)

    def orb_extract_slot(self, ex: OrbExtractor, slot: int, orb: OrbParams | None = None):
        """pagk_orb_extract_slot: ORBextractor::operator() on frame slot `slot` into the slot's keypoint set (asynchronous,
        capturable)."""
        orb = orb if orb is not None else orb_params_default()
        self._check(self.lib.pagk_orb_extract_slot(self.h, C.byref(ex), C.byref(orb), slot), "pagk_orb_extract_slot")

    def orb_slot_read(self, slot: int, cap: int) -> dict:
        """pagk_orb_slot_read (synchronous) -> dict(n, keypoints, octave, response, angle, desc (cut to n), info and its
        words by name, full_* (cap rows))."""
        cap = int(cap)
        kp, octave = np.full((max(cap, 1), 2), 7, np.float32), np.full(max(cap, 1), 7, np.int32)
        resp, ang = np.full(max(cap, 1), 7, np.float32), np.full(max(cap, 1), 7, np.float32)
        desc, info = np.full((max(cap, 1), 32), 7, np.uint8), np.zeros(ORB_LEVELS_INFO_WORDS, np.int32)
        self._check(self.lib.pagk_orb_slot_read(self.h, slot, cap, _ptr(kp), _ptr(octave), _ptr(resp), _ptr(ang), _ptr(desc),
                                                _ptr(info)), "pagk_orb_slot_read")
        return _orb_set_dict(cap, kp, octave, resp, ang, desc, info)

    def orb_match_slots(self, slot_q: int, slot_t: int, orb: OrbParams | None = None):
        """pagk_orb_match_slots: the matcher and the distance filter between two slots' sets (asynchronous, capturable)."""
        orb = orb if orb is not None else orb_params_default()
        self._check(self.lib.pagk_orb_match_slots(self.h, C.byref(orb), slot_q, slot_t), "pagk_orb_match_slots")

    def orb_match_slots_read(self, slot_q: int, cap: int) -> dict:
        """pagk_orb_match_slots_read (synchronous) -> dict(train_idx, distance, keep (cap rows), info and its words by name)."""
        cap = int(cap)
        idx, dist = np.full(max(cap, 1), 7, np.int32), np.full(max(cap, 1), 7, np.int32)
        keep, info = np.full(max(cap, 1), 7, np.uint8), np.zeros(ORB_INFO_WORDS, np.int32)
        self._check(self.lib.pagk_orb_match_slots_read(self.h, slot_q, cap, _ptr(idx), _ptr(dist), _ptr(keep), _ptr(info)),
                    "pagk_orb_match_slots_read")
        out = dict(train_idx=idx, distance=dist, keep=keep, info=info)
        out.update(zip(ORB_MATCH_INFO_FIELDS, (int(v) for v in info[:6])))
        return out

    def orb_extract_levels(self, img: np.ndarray, ex: OrbExtractor, orb: OrbParams | None = None, cap: int | None = None) -> dict:
        """pagk_orb_extract_levels, host buffers -> the dict of orb_slot_read.  cap defaults to the table's out_bound."""
        orb = orb if orb is not None else orb_params_default()
        iv = image_view(img)
        if cap is None:
            cap = orb_extractor_levels(ex, iv.width, iv.height).get("out_bound", 1)
        cap = int(cap)
        kp, octave = np.full((max(cap, 1), 2), 7, np.float32), np.full(max(cap, 1), 7, np.int32)
        resp, ang = np.full(max(cap, 1), 7, np.float32), np.full(max(cap, 1), 7, np.float32)
        desc, info = np.full((max(cap, 1), 32), 7, np.uint8), np.zeros(ORB_LEVELS_INFO_WORDS, np.int32)
        self._check(self.lib.pagk_orb_extract_levels(self.h, C.byref(ex), C.byref(orb), C.byref(iv), cap, _ptr(kp), _ptr(octave),
                                                     _ptr(resp), _ptr(ang), _ptr(desc), _ptr(info)), "pagk_orb_extract_levels")
        return _orb_set_dict(cap, kp, octave, resp, ang, desc, info)

    def orb_detect_levels(self, img: np.ndarray, ex: OrbExtractor, mask=None, cap: int | None = None) -> dict:
        """pagk_orb_detect_levels, host buffers -> dict(n, keypoints, octave, response (cut to n), info and its words by name,
        full_* (cap rows)).  mask: height x width bytes or None."""
        iv = image_view(img)
        if cap is None:
            cap = orb_extractor_levels(ex, iv.width, iv.height).get("out_bound", 1)
        cap = int(cap)
        m = None if mask is None else np.ascontiguousarray(mask, np.uint8)
        if m is not None and m.shape != (iv.height, iv.width):
            raise ValueError("mask must be height x width")
        kp, octave = np.full((max(cap, 1), 2), 7, np.float32), np.full(max(cap, 1), 7, np.int32)
        resp, info = np.full(max(cap, 1), 7, np.float32), np.zeros(ORB_LEVELS_INFO_WORDS, np.int32)
        self._check(self.lib.pagk_orb_detect_levels(self.h, C.byref(ex), C.byref(iv), _ptr(m), cap, _ptr(kp), _ptr(octave),
                                                    _ptr(resp), _ptr(info)), "pagk_orb_detect_levels")
        return _orb_set_dict(cap, kp, octave, resp, None, None, info)

    def selftest_orb_level(self, slot: int, level: int, width: int, height: int, pitch: int | None = None) -> np.ndarray:
        """pagk_selftest_orb_level: level `level` of the slot's ORB scale pyramid, height x width."""
        pitch = width if pitch is None else int(pitch)
        buf = np.zeros((height, pitch), np.uint8)
        self._check(self.lib.pagk_selftest_orb_level(self.h, slot, level, buf.ctypes.data, pitch), "pagk_selftest_orb_level")
        return buf[:, :width]

    # pyramidal Lucas-Kanade, tracker type 0 (src/gyro_aided_tracker.cpp:353-380) -------------------------------------
    lk_params_default = staticmethod(lk_params_default)

    def lk_pyramid_device(self, lk: LkParams, slot: int):
        """pagk_lk_pyramid_device: the pyrDown levels of frame slot `slot` (asynchronous, capturable)."""
        self._check(self.lib.pagk_lk_pyramid_device(self.h, C.byref(lk), slot), "pagk_lk_pyramid_device")

    def lk_track_device(self, lk: LkParams, slot_ref: int, slot_cur: int, cap: int, d_pt_ref, d_n, d_pt_out, d_status,
                        d_status_raw, d_err, d_flow, d_info):
        """pagk_lk_track_device (asynchronous, capturable): d_n, d_status_raw and d_flow may be None."""
        if d_pt_ref is None or d_pt_out is None or d_status is None or d_err is None or d_info is None:
            raise ValueError("d_pt_ref, d_pt_out, d_status, d_err and d_info are required")
        self._check(self.lib.pagk_lk_track_device(self.h, C.byref(lk), slot_ref, slot_cur, cap, _ptr(d_pt_ref), _ptr(d_n),
                                                  _ptr(d_pt_out), _ptr(d_status), _ptr(d_status_raw), _ptr(d_err),
                                                  _ptr(d_flow), _ptr(d_info)), "pagk_lk_track_device")

    def lk_track(self, img_ref: np.ndarray, img_cur: np.ndarray, pts, lk: LkParams | None = None) -> dict:
        """pagk_lk_track, host buffers -> dict(pt_out (n x 2), status (n), status_raw (n), err (n), flow (n x 2), info, and
        the info words by name)."""
        lk = lk if lk is not None else lk_params_default()
        pt = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        n = int(pt.shape[0])
        nn = max(n, 1)
        ir, ic = image_view(img_ref), image_view(img_cur)
        out = dict(pt_out=np.zeros((nn, 2), np.float32), status=np.zeros(nn, np.uint8), status_raw=np.zeros(nn, np.uint8),
                   err=np.zeros(nn, np.float32), flow=np.zeros((nn, 2), np.float32))
        info = np.zeros(LK_INFO_WORDS, np.int32)
        self._check(self.lib.pagk_lk_track(self.h, C.byref(lk), C.byref(ir), C.byref(ic), n, _ptr(pt) if n else None,
                                           _ptr(out["pt_out"]), _ptr(out["status"]), _ptr(out["status_raw"]),
                                           _ptr(out["err"]), _ptr(out["flow"]), _ptr(info)), "pagk_lk_track")
        out = {k: v[:n] for k, v in out.items()}
        out["info"] = info
        out.update(zip(LK_INFO_FIELDS, (int(v) for v in info[:6])))
        return out

    def lk_track_flow(self, img_ref: np.ndarray, img_cur: np.ndarray, pts, lk: LkParams | None = None, cam: Params | None = None,
                      pt_init=None, status_in=None) -> dict:
        """pagk_lk_track_flow, host buffers: Lucas-Kanade started from pt_init (None: pts), rows with status_in == 0 (None:
        all 1) left out, the distorted point with the camera of `cam` (None: no pt_out_dist) -> the dict of lk_track plus
        pt_out_dist (n x 2, with cam) and the info word `skipped`."""
        lk = lk if lk is not None else lk_params_default()
        pt = np.ascontiguousarray(pts, np.float32).reshape(-1, 2)
        n = int(pt.shape[0])
        nn = max(n, 1)
        init = None if pt_init is None else np.ascontiguousarray(pt_init, np.float32).reshape(-1, 2)
        live = None if status_in is None else np.ascontiguousarray(status_in, np.uint8).reshape(-1)
        if (init is not None and init.shape[0] != n) or (live is not None and live.shape[0] != n):
            raise ValueError("pt_init and status_in have one row per point")
        ir, ic = image_view(img_ref), image_view(img_cur)
        out = dict(pt_out=np.zeros((nn, 2), np.float32), status=np.zeros(nn, np.uint8), status_raw=np.zeros(nn, np.uint8),
                   err=np.zeros(nn, np.float32), flow=np.zeros((nn, 2), np.float32))
        if cam is not None:
            out["pt_out_dist"] = np.zeros((nn, 2), np.float32)
        info = np.zeros(LK_INFO_WORDS, np.int32)
        opt = lambda a: _ptr(a) if (a is not None and n) else None     # noqa: E731
        self._check(self.lib.pagk_lk_track_flow(self.h, C.byref(lk), C.byref(cam) if cam is not None else None, C.byref(ir),
                                                C.byref(ic), n, opt(pt), opt(init), opt(live), _ptr(out["pt_out"]),
                                                _ptr(out["pt_out_dist"]) if cam is not None else None, _ptr(out["status"]),
                                                _ptr(out["status_raw"]), _ptr(out["err"]), _ptr(out["flow"]), _ptr(info)),
                    "pagk_lk_track_flow")
        out = {k: v[:n] for k, v in out.items()}
        out["info"] = info
        out.update(zip(LK_INFO_FIELDS, (int(v) for v in info[:6])))
        out["skipped"] = int(info[6])
        return out

    # the sequence the context owns (Examples/Demo/RealSenseD435i.cpp:199-321) -------------------------------------------
    def sequence_create(self, sp: SequenceParams):
        """pagk_sequence_create: one sequence per context; its buffers are the context's."""
        self._check(self.lib.pagk_sequence_create(self.h, C.byref(sp)), "pagk_sequence_create")
        self._seq_params = sp

    def sequence_destroy(self):
        self._check(self.lib.pagk_sequence_destroy(self.h), "pagk_sequence_destroy")

    @staticmethod
    def _seq_cand(candidates):
        if candidates is None:
            return None, None, 0
        cand = np.ascontiguousarray(candidates, np.float32).reshape(-1, 2)
        n = int(cand.shape[0])
        if n == 0:
            cand = np.zeros((1, 2), np.float32)   # (an empty list is still a list: the pointer is required)
        return cand, cand.ctypes.data, n

    def sequence_start(self, frame: np.ndarray, candidates=None):
        """pagk_sequence_start: the first frame (host image); candidates (n x 2) for a sequence without a detector."""
        iv = image_view(frame)
        keep, ptr, n = self._seq_cand(candidates)
        self._check(self.lib.pagk_sequence_start(self.h, C.byref(iv), ptr, n), "pagk_sequence_start")

    def sequence_step(self, frame: np.ndarray, rot9=None, candidates=None, mode: int = SEQ_GRAPH):
        """pagk_sequence_step: frame k >= 1 with its nine rotation floats; nothing is synchronised."""
        iv = image_view(frame)
        rot = None if rot9 is None else np.ascontiguousarray(rot9, np.float32).reshape(9)
        keep, ptr, n = self._seq_cand(candidates)
        self._check(self.lib.pagk_sequence_step(self.h, C.byref(iv), _ptr(rot), ptr, n, int(mode)), "pagk_sequence_step")

    def sequence_read(self, cap: int) -> dict:
        """pagk_sequence_read -> dict(keys, keys_un, keys_normal, index_in_last, live (cap rows), state, info and the state
        words by name)."""
        out = dict(keys=np.zeros((cap, 2), np.float32), keys_un=np.zeros((cap, 2), np.float32),
                   keys_normal=np.zeros((cap, 2), np.float32), index_in_last=np.zeros(cap, np.int32), live=np.zeros(cap, np.uint8),
                   state=np.zeros(HANDOVER_STATE_WORDS, np.int32), info=np.zeros(DETECT_INFO_WORDS, np.int32))
        self._check(self.lib.pagk_sequence_read(self.h, cap, *(_ptr(out[k]) for k in ("keys", "keys_un", "keys_normal",
                                                                                       "index_in_last", "live", "state", "info"))),
                    "pagk_sequence_read")
        out.update(zip(HANDOVER_STATE_FIELDS, (int(v) for v in out["state"][:5])))
        return out

    def sequence_read_pair(self, cap: int) -> dict:
        """pagk_sequence_read_pair -> dict(status, pt_predict, pt_predict_un, err), cap rows: what the last pair handed over."""
        out = dict(status=np.zeros(cap, np.uint8), pt_predict=np.zeros((cap, 2), np.float32),
                   pt_predict_un=np.zeros((cap, 2), np.float32), err=np.zeros(cap, np.float32))
        self._check(self.lib.pagk_sequence_read_pair(self.h, cap, *(_ptr(out[k]) for k in ("status", "pt_predict", "pt_predict_un",
                                                                                            "err"))), "pagk_sequence_read_pair")
        return out

    def sequence_status(self) -> dict:
        """pagk_sequence_status -> dict(frames, last_was_graph, graphs); nothing is synchronised."""
        w = np.zeros(SEQ_STATUS_WORDS, np.int32)
        self._check(self.lib.pagk_sequence_status(self.h, _ptr(w)), "pagk_sequence_status")
        return dict(frames=int(w[0]), last_was_graph=bool(w[1]), graphs=int(w[2]), results_depth=int(w[3]))

    # the result ring of the sequence (include/pagk.h "The result ring of a sequence") ------------------------------------
    def sequence_results_create(self, depth: int):
        """pagk_sequence_results_create: `depth` (2 .. 8) pinned result blocks, in front of the first start."""
        self._check(self.lib.pagk_sequence_results_create(self.h, int(depth)), "pagk_sequence_results_create")

    def sequence_fetch(self, frame: int) -> dict:
        """pagk_sequence_fetch -> the record of `frame` as a dict of COPIES (the views die with the block's next frame): the
        header's scalars (frame, cap, n_live, n_new, next_id, t), state, info and every array on all cap rows."""
        r = SequenceResult()
        self._check(self.lib.pagk_sequence_fetch(self.h, int(frame), C.byref(r)), "pagk_sequence_fetch")
        cap = int(r.cap)
        out = dict(frame=int(r.frame), cap=cap, n_live=int(r.n_live), n_new=int(r.n_new), next_id=int(r.next_id), t=float(r.t))

        def view(name, dtype, count):
            buf = (C.c_uint8 * (count * np.dtype(dtype).itemsize)).from_address(getattr(r, name))
            return np.frombuffer(buf, dtype).copy()
        out["state"] = view("state", np.int32, HANDOVER_STATE_WORDS)
        out["info"] = view("info", np.int32, DETECT_INFO_WORDS)
        for name, (dtype, cols) in RESULTS_ARRAYS.items():
            a = view(name, dtype, cap * cols)
            out[name] = a.reshape(cap, 2) if cols == 2 else a
        return out

    def sequence_poll(self, frame: int) -> bool:
        """pagk_sequence_poll: has the copy of `frame` completed?  Nothing is waited for."""
        rc = int(self.lib.pagk_sequence_poll(self.h, int(frame)))
        if rc < 0:
            self._check(rc, "pagk_sequence_poll")
        return rc == 1

    # the sensor form of the sequence and the gyro integration (src/gyro_aided_tracker.cpp:511-587) ------------------------
    def gyro_integrate(self, Rbc, camera: Params, window: ImuWindow):
        """pagk_gyro_integrate -> (Rcl (3 x 3), rot9): the window's rotation by k_gyro_integrate."""
        rbc = np.ascontiguousarray(Rbc, np.float32).reshape(9)
        rcl, rot9 = np.zeros(9, np.float32), np.zeros(9, np.float32)
        self._check(self.lib.pagk_gyro_integrate(self.h, _ptr(rbc), C.byref(camera), C.byref(window), _ptr(rcl), _ptr(rot9)),
                    "pagk_gyro_integrate")
        return rcl.reshape(3, 3), rot9

    def sequence_create_sensor(self, sp: SequenceParams, sensor: SequenceSensor):
        """pagk_sequence_create_sensor: a sequence fed raw frames and IMU windows."""
        self._check(self.lib.pagk_sequence_create_sensor(self.h, C.byref(sp), C.byref(sensor)), "pagk_sequence_create_sensor")
        self._seq_params = sp

    @staticmethod
    def _raw_view(frame: np.ndarray) -> Image:
        """height x width (x channels) bytes, rows possibly padded: width and height in pixels, step in bytes"""
        assert frame.dtype == np.uint8 and frame.ndim in (2, 3) and frame.strides[-1] == 1
        assert frame.ndim == 2 or frame.strides[1] == frame.shape[2]
        return Image(frame.ctypes.data, frame.shape[1], frame.shape[0], frame.strides[0])

    def sequence_start_sensor(self, raw: np.ndarray, t: float, candidates=None):
        """pagk_sequence_start_sensor: the first raw frame and its time stamp."""
        iv = self._raw_view(raw)
        keep, ptr, n = self._seq_cand(candidates)
        self._check(self.lib.pagk_sequence_start_sensor(self.h, C.byref(iv), float(t), ptr, n), "pagk_sequence_start_sensor")

    def sequence_step_sensor(self, raw: np.ndarray, window: ImuWindow, candidates=None, mode: int = SEQ_GRAPH):
        """pagk_sequence_step_sensor: raw frame k >= 1 with the samples since the previous frame; nothing is synchronised."""
        iv = self._raw_view(raw)
        keep, ptr, n = self._seq_cand(candidates)
        self._check(self.lib.pagk_sequence_step_sensor(self.h, C.byref(iv), C.byref(window), ptr, n, int(mode)),
                    "pagk_sequence_step_sensor")

    def sequence_read_velocity(self, cap: int) -> np.ndarray:
        """pagk_sequence_read_velocity -> cap x 2 floats: mvFlowVelocityInNormalPlane of the current key set."""
        v = np.zeros((cap, 2), np.float32)
        self._check(self.lib.pagk_sequence_read_velocity(self.h, cap, _ptr(v)), "pagk_sequence_read_velocity")
        return v

    def selftest_lk_level(self, slot: int, level: int, width: int, height: int, pitch: int | None = None) -> np.ndarray:
        """pagk_selftest_lk_level: level `level` (>= 1) of the slot's Lucas-Kanade pyramid, height x width."""
        pitch = width if pitch is None else int(pitch)
        buf = np.zeros((height, pitch), np.uint8)
        self._check(self.lib.pagk_selftest_lk_level(self.h, slot, level, buf.ctypes.data, pitch), "pagk_selftest_lk_level")
        return buf[:, :width]

    # track-to-detection association (src/gyro_aided_tracker.cpp:859-939, :1017-1136) ---------------------------------------
    assoc_params_default = staticmethod(assoc_params_default)

    def match_features_device(self, ap: AssocParams, n: int, m: int, cap: int, d_count, d_idx, d_dist, d_ncc, d_match_query,
                              d_match_train, d_match_dist, d_match_ncc, d_n_matches, d_info):
        """pagk_match_features_device (asynchronous, capturable): d_match_dist and d_match_ncc may be None."""
        self._check(self.lib.pagk_match_features_device(self.h, C.byref(ap), n, m, cap, _ptr(d_count), _ptr(d_idx), _ptr(d_dist),
                                                        _ptr(d_ncc), _ptr(d_match_query), _ptr(d_match_train),
                                                        _ptr(d_match_dist), _ptr(d_match_ncc), _ptr(d_n_matches), _ptr(d_info)),
                    "pagk_match_features_device")

    def search_gyro_predict_device(self, ap: AssocParams, slot_ref: int, slot_cur: int, half_patch: int, n: int, d_keys_ref,
                                   d_pt_predict_un, d_status, d_affine, m: int, d_keys_cur, d_keys_cur_un, d_m,
                                   radius_unit: float, cap: int, d_count, d_idx, d_dist, d_ncc, d_match_query, d_match_train,
                                   d_match_dist, d_match_ncc, d_n_matches, d_flows_err, d_info):
        """pagk_search_gyro_predict_device (asynchronous, capturable): d_affine, d_m, d_match_dist, d_match_ncc and
        d_flows_err may be None."""
        self._check(self.lib.pagk_search_gyro_predict_device(
            self.h, C.byref(ap), slot_ref, slot_cur, half_patch, n, _ptr(d_keys_ref), _ptr(d_pt_predict_un), _ptr(d_status),
            _ptr(d_affine), m, _ptr(d_keys_cur), _ptr(d_keys_cur_un), _ptr(d_m), float(radius_unit), cap, _ptr(d_count),
            _ptr(d_idx), _ptr(d_dist), _ptr(d_ncc), _ptr(d_match_query), _ptr(d_match_train), _ptr(d_match_dist),
            _ptr(d_match_ncc), _ptr(d_n_matches), _ptr(d_flows_err), _ptr(d_info)), "pagk_search_gyro_predict_device")

    def search_gyro_predict(self, img_ref, img_cur, half_patch, keys_ref, pt_predict_un, status, affine, keys_cur, keys_cur_un,
                            ap: AssocParams | None = None, radius_unit=None, cap=64) -> dict:
        """pagk_search_gyro_predict, host buffers -> dict(rc, n_matches, query, train, dist, ncc (n_matches rows),
        flows_err (n x 2), count, idx, dist_lists, ncc_lists, info and the info words by name); rc is the number of matches or
        PAGK_E_CAPACITY (count then holds the sizes needed)."""
        ap = ap if ap is not None else assoc_params_default()
        n, m = int(keys_ref.shape[0]), int(keys_cur.shape[0])
        nn = max(n, 1)
        ir, ic = image_view(img_ref), image_view(img_cur)
        count = np.zeros(nn, np.int32)
        idx = np.full((nn, cap), -1, np.int32)
        dist, ncc = np.zeros((nn, cap), np.float32), np.zeros((nn, cap), np.float32)
        q, t = np.full(nn, -1, np.int32), np.full(nn, -1, np.int32)
        md, mc = np.zeros(nn, np.float32), np.zeros(nn, np.float32)
        flows = np.zeros((nn, 2), np.float32)
        info = np.zeros(ASSOC_INFO_WORDS, np.int32)
        ru = float(2 * half_patch) if radius_unit is None else float(radius_unit)
        rc = self.lib.pagk_search_gyro_predict(self.h, C.byref(ap), C.byref(ir), C.byref(ic), half_patch, n, _ptr(keys_ref),
                                               _ptr(pt_predict_un), _ptr(status), _ptr(affine), m, _ptr(keys_cur),
                                               _ptr(keys_cur_un), ru, cap, _ptr(count), _ptr(idx), _ptr(dist), _ptr(ncc),
                                               _ptr(q), _ptr(t), _ptr(md), _ptr(mc), _ptr(flows), _ptr(info))
        if rc < 0 and rc != PAGK_E_CAPACITY:
            self._check(rc, "pagk_search_gyro_predict")
        k = int(info[4])
        out = dict(rc=rc, n_matches=k, query=q[:k], train=t[:k], dist=md[:k], ncc=mc[:k], flows_err=flows[:n], count=count[:n],
                   idx=idx[:n], dist_lists=dist[:n], ncc_lists=ncc[:n], info=info)
        out.update(zip(ASSOC_MATCH_INFO_FIELDS, (int(v) for v in info[:6])))
        return out

    def search_klt_device(self, lk: LkParams, ap: AssocParams, slot_ref: int, slot_cur: int, cap: int, d_keys_ref, d_n, m: int,
                          d_keys_cur, d_m, d_pt_out, d_status, d_err, d_match_query, d_match_train, d_match_dist, d_disparity,
                          d_n_matches, d_stats, d_info, d_lk_info):
        """pagk_search_klt_device (asynchronous, capturable): d_n, d_m and d_match_dist may be None."""
        self._check(self.lib.pagk_search_klt_device(
            self.h, C.byref(lk), C.byref(ap), slot_ref, slot_cur, cap, _ptr(d_keys_ref), _ptr(d_n), m, _ptr(d_keys_cur), _ptr(d_m),
            _ptr(d_pt_out), _ptr(d_status), _ptr(d_err), _ptr(d_match_query), _ptr(d_match_train), _ptr(d_match_dist),
            _ptr(d_disparity), _ptr(d_n_matches), _ptr(d_stats), _ptr(d_info), _ptr(d_lk_info)), "pagk_search_klt_device")

    def search_klt(self, img_ref, img_cur, keys_ref, keys_cur, lk: LkParams | None = None, ap: AssocParams | None = None) -> dict:
        """pagk_search_klt, host buffers -> dict(n_matches, query, train, dist, disparity (n_matches rows), pt_out, status, err
        (n rows), stats, info, lk_info and the info words and statistics by name)."""
        lk = lk if lk is not None else lk_params_default()
        ap = ap if ap is not None else assoc_params_default()
        kr = np.ascontiguousarray(keys_ref, np.float32).reshape(-1, 2)
        kc = np.ascontiguousarray(keys_cur, np.float32).reshape(-1, 2)
        n, m = int(kr.shape[0]), int(kc.shape[0])
        nn = max(n, 1)
        ir, ic = image_view(img_ref), image_view(img_cur)
        pt_out, status, err = np.zeros((nn, 2), np.float32), np.zeros(nn, np.uint8), np.zeros(nn, np.float32)
        q, t = np.full(nn, -1, np.int32), np.full(nn, -1, np.int32)
        md, disp = np.zeros(nn, np.float32), np.zeros(nn, np.float64)
        stats = np.zeros(ASSOC_STATS_WORDS, np.float64)
        info, lk_info = np.zeros(ASSOC_INFO_WORDS, np.int32), np.zeros(LK_INFO_WORDS, np.int32)
        k = self.lib.pagk_search_klt(self.h, C.byref(lk), C.byref(ap), C.byref(ir), C.byref(ic), n, _ptr(kr) if n else None, m,
                                     _ptr(kc) if m else None, _ptr(pt_out), _ptr(status), _ptr(err), _ptr(q), _ptr(t), _ptr(md),
                                     _ptr(disp), _ptr(stats), _ptr(info), _ptr(lk_info))
        self._check(min(k, 0), "pagk_search_klt")
        out = dict(n_matches=k, query=q[:k], train=t[:k], dist=md[:k], disparity=disp[:k], pt_out=pt_out[:n], status=status[:n],
                   err=err[:n], stats=stats, info=info, lk_info=lk_info)
        out.update(zip(ASSOC_KLT_INFO_FIELDS, (int(v) for v in info)))
        out.update(zip(ASSOC_STATS_FIELDS, (float(v) for v in stats[:7])))
        return out

    # hipGraph capture of the *_device calls issued on the context stream --------------------
    def graph_begin(self):
        self._check(self.lib.pagk_graph_begin(self.h), "pagk_graph_begin")

    def graph_end(self) -> int:
        gid = C.c_int32(-1)
        self._check(self.lib.pagk_graph_end(self.h, C.byref(gid)), "pagk_graph_end")
        return gid.value

    def graph_launch(self, graph_id: int):
        self._check(self.lib.pagk_graph_launch(self.h, graph_id), "pagk_graph_launch")

    def graph_destroy(self, graph_id: int):
        self._check(self.lib.pagk_graph_destroy(self.h, graph_id), "pagk_graph_destroy")

    def sync(self):
        self._check(self.lib.pagk_sync(self.h), "pagk_sync")

    def check_launch(self):
        """The error state pagk_sync would return, without synchronising: for callers that synchronise the stream
        themselves (a torch stream).  Raises PAGK_E_HIP once for a launch in which a wave gave up its wait
        (kernel 7's level hand-off, the 4-wave kernel's solve)."""
        self._check(self.lib.pagk_check_launch(self.h), "pagk_check_launch")

    def set_stream(self, stream_ptr: int | None):
        self._check(self.lib.pagk_set_stream(self.h, stream_ptr), "pagk_set_stream")

    def set_kernel(self, which: int):
        self._check(self.lib.pagk_set_kernel(self.h, which), "pagk_set_kernel")

    VARIANT_NAMES = {0: "4-wave workgroup per feature, DPP row chains", 1: "one thread per feature (cross-check)",
                     2: "2-wave workgroup per feature, f64 MFMA chain", 3: "one wave per feature, f64 MFMA chain",
                     4: "relaxed order (experiment)", 5: "four features per wave, f64 MFMA blocks",
                     6: "four independent rows per wave + work queue",
                     7: "four features per wave, one pyramid level per wave"}

    def priority_threshold(self) -> int:
        """K of the next 4-wave launch's issue priorities (csrc/pagk_prio.h); synchronises."""
        rc = int(self.lib.pagk_priority_threshold(self.h))
        if rc < 0:
            self._check(rc, "pagk_priority_threshold")
        return rc

    def prio_hint_threshold(self) -> int:
        """Threshold of the 4-wave kernels' hint (csrc/pagk_prio.h; PAGK_PRIO_HINT, 0 = off)."""
        return int(self.lib.pagk_prio_hint_threshold(self.h))

    def prio_hint_reset(self):
        """New features were written into the device arrays: forget what the slots' previous features ran (stream order)."""
        if hasattr(self.lib, "pagk_prio_hint_reset"):   # (an older build through PAGK_LIB: nothing to forget)
            self._check(self.lib.pagk_prio_hint_reset(self.h), "pagk_prio_hint_reset")

    def prio_hint_get(self, n: int) -> np.ndarray:
        out = np.zeros(max(n, 0), np.int32)
        self._check(self.lib.pagk_prio_hint_get(self.h, n, out.ctypes.data_as(C.c_void_p)), "pagk_prio_hint_get")
        return out

    def prio_hint_set(self, hints) -> None:
        h = np.ascontiguousarray(hints, np.int32)
        self._check(self.lib.pagk_prio_hint_set(self.h, int(h.shape[0]), h.ctypes.data_as(C.c_void_p)), "pagk_prio_hint_set")

    def dispatch_order_enabled(self) -> bool:
        """The 4-wave kernels' dispatch order (csrc/pagk_order.h) is on (PAGK_DISPATCH_ORDER=0 in the environment of the context's
        creation switches it off)."""
        return bool(self.lib.pagk_dispatch_order_enabled(self.h))

    def dispatch_order_get(self, n: int):
        """(order, in_force): the first n entries of the order array as they are on the device, and whether a 4-wave launch of n
        features enqueued next on the current stream would use it.  Synchronises."""
        out = np.zeros(max(n, 0), np.int32)
        in_force = C.c_int32(0)
        self._check(self.lib.pagk_dispatch_order_get(self.h, n, out.ctypes.data_as(C.c_void_p), C.byref(in_force)),
                    "pagk_dispatch_order_get")
        return out, bool(in_force.value)

    def last_variant(self) -> int:
        return int(self.lib.pagk_last_variant(self.h))

    def last_handover(self) -> int:
        """Features the last launch handed from the throughput kernel to the latency kernel (0: hand-over not used)."""
        rc = int(self.lib.pagk_last_handover(self.h))
        if rc < 0:
            self._check(rc, "pagk_last_handover")
        return rc

    def set_concurrency(self, streams: int):
        """`streams` contexts like this one run at the same time on the device: the automatic variant thresholds are
        applied to streams * n (pagk_set_concurrency)."""
        self._check(self.lib.pagk_set_concurrency(self.h, streams), "pagk_set_concurrency")

    def last_kernel_ms(self):
        t, p = C.c_float(0), C.c_float(0)
        self._check(self.lib.pagk_last_kernel_ms(self.h, C.byref(t), C.byref(p)), "pagk_last_kernel_ms")
        return t.value, p.value


def post_filter(half_patch: int, status_pm, pix_err, dist_pred, pt_pm, pt_pm_un):
    """pagk_post_filter: the tracker-side inlier mask (reference src/gyro_aided_tracker.cpp:289-341)."""
    lib = load()
    n = int(status_pm.shape[0])
    status = np.zeros(max(n, 1), np.uint8)
    pp = np.zeros((max(n, 1), 2), np.float32)
    ppu = np.zeros((max(n, 1), 2), np.float32)
    rc = lib.pagk_post_filter(n, half_patch, _ptr(status_pm), _ptr(pix_err), _ptr(dist_pred), _ptr(pt_pm),
                              _ptr(pt_pm_un), _ptr(status), _ptr(pp), _ptr(ppu))
    if rc < 0:
        raise PagkError(rc, "pagk_post_filter")
    return rc, status[:n], pp[:n], ppu[:n]


def geometry_select(score_H: float, score_F: float) -> bool:
    """True = homography chosen (RH > 0.45, reference src/gyro_aided_tracker.cpp:462-470)."""
    return bool(load().pagk_geometry_select(float(score_H), float(score_F)))


def match_features(count, idx, dist, ncc, use_ncc=True):
    """pagk_match_features: GyroAidedTracker::MatchFeatures (reference src/gyro_aided_tracker.cpp:949-1008)
    -> (query, train, dist, ncc) of the accepted matches."""
    n = int(count.shape[0])
    cap = int(idx.shape[1])
    q, t = np.zeros(max(n, 1), np.int32), np.zeros(max(n, 1), np.int32)
    d, c = np.zeros(max(n, 1), np.float32), np.zeros(max(n, 1), np.float32)
    count = np.ascontiguousarray(count, np.int32)
    idx, dist, ncc = np.ascontiguousarray(idx), np.ascontiguousarray(dist), np.ascontiguousarray(ncc)
    k = load().pagk_match_features(n, cap, _ptr(count), _ptr(idx), _ptr(dist), _ptr(ncc), int(use_ncc), _ptr(q), _ptr(t),
                                   _ptr(d), _ptr(c))
    if k < 0:
        raise PagkError(k, "pagk_match_features")
    return q[:k], t[:k], d[:k], c[:k]


def shard_range(n: int, rank: int, world: int) -> tuple[int, int]:
    """pagk_shard_range: the contiguous feature block of a rank."""
    lo, hi = C.c_int32(0), C.c_int32(0)
    load().pagk_shard_range(n, rank, world, C.byref(lo), C.byref(hi))
    return lo.value, hi.value


def shard_layout(m: int) -> tuple[list[int], int]:
    """pagk_shard_layout: byte offsets of the seven SoA blocks of a rank's packed slice, and its size."""
    offs = (C.c_size_t * 7)()
    total = load().pagk_shard_layout(m, offs)
    return [int(v) for v in offs], int(total)


class Multi:
    """pagk_multi owner: the group of GPUs one tracking call is sharded over, and its RCCL communicator.
    Multi(devices=[...]) drives all devices from this process; Multi(uid=..., rank=, world=, device=) joins a
    one-process-per-GPU group (uid from Multi.unique_id() on rank 0, handed over by the application)."""

    def __init__(self, devices=None, *, uid: bytes | None = None, rank: int = 0, world: int = 1, device: int = 0):
        self.lib = load()
        self._lent = []   # Contexts handed out by ctx(): invalidated by close()
        h = C.c_void_p()
        if uid is None:
            if devices is None or len(devices) == 0 or any(int(d) < 0 for d in devices):
                raise ValueError("Multi(devices=[...]) needs a non-empty list of device indices (or uid=, rank=, world=)")
            devs = (C.c_int32 * len(devices))(*devices)
            rc = self.lib.pagk_multi_create(C.byref(h), devs, len(devices))
            where = "pagk_multi_create"
        else:
            if len(uid) != 128:
                raise ValueError("the RCCL unique id is 128 bytes")
            buf = (C.c_uint8 * 128).from_buffer_copy(uid)
            rc = self.lib.pagk_multi_create_rank(C.byref(h), buf, rank, world, device)
            where = "pagk_multi_create_rank"
        if rc != PAGK_OK:
            raise PagkError(rc, where)
        self.h = h
        self.world = self.lib.pagk_multi_world(h)
        self.n_local = self.lib.pagk_multi_local(h)
        self.rank = rank if uid is not None else 0

    def comm_count(self) -> int | None:
        """Ranks of the communicator as RCCL reports them (ncclCommCount); None when the library cannot tell."""
        c = int(self.lib.pagk_multi_comm_count(self.h))
        return c if c >= 0 else None

    @staticmethod
    def unique_id() -> bytes:
        buf = (C.c_uint8 * 128)()
        rc = load().pagk_multi_unique_id(buf)
        if rc != PAGK_OK:
            raise PagkError(rc, "pagk_multi_unique_id")
        return bytes(buf)

    def ctx(self, local_index: int = 0) -> Context:
        if not getattr(self, "h", None):
            raise RuntimeError("this Multi has been closed")
        p = self.lib.pagk_multi_ctx(self.h, local_index)
        if not p:
            raise IndexError(local_index)
        c = Context(_borrowed=p)
        self._lent.append(c)
        return c

    def _check(self, rc: int, where: str):
        if rc != PAGK_OK:
            raise PagkError(rc, where, self.lib.pagk_multi_last_error(self.h).decode())

    def allgather(self, d_send, d_recv, nbytes: int, streams=None):
        """One all-gather of `nbytes` bytes per rank; d_send / d_recv: one device buffer per local member."""
        k = self.n_local
        snd = (C.c_void_p * k)(*[_ptr(a) for a in d_send])
        rcv = (C.c_void_p * k)(*[_ptr(a) for a in d_recv])
        st = None if streams is None else (C.c_void_p * k)(*streams)
        self._check(self.lib.pagk_multi_allgather(self.h, snd, rcv, nbytes, st), "pagk_multi_allgather")

    def track_sharded(self, params: Params, img_ref, img_cur, pt_ref, pt_init, affine, status_in, out: dict | None = None):
        n = int(pt_ref.shape[0])
        out = out if out is not None else alloc_outputs(n)
        ir, ic = image_view(img_ref), image_view(img_cur)
        o = outputs_struct(out)
        self._check(self.lib.pagk_track_sharded(self.h, C.byref(params), C.byref(ir), C.byref(ic), n, _ptr(pt_ref),
                                                _ptr(pt_init), _ptr(affine), _ptr(status_in), C.byref(o)),
                    "pagk_track_sharded")
        return out

    def close(self):
        if getattr(self, "h", None):
            for c in getattr(self, "_lent", []):
                c.h = None    # the group owns its member contexts: a borrowed handle must not outlive it
            self._lent = []
            self.lib.pagk_multi_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
