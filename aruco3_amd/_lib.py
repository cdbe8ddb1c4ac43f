"""ctypes binding of libaruco3_hip.so (the C ABI of include/aruco3_hip.h).

There is no CPU implementation behind this module: if the shared library is missing, or
no MI355X is visible, every entry point raises.  Build with `python __graft_entry__.py`
(or `make -C aruco3_amd/csrc`).
"""
import ctypes as C
from pathlib import Path

import numpy as np

import os

_HERE = Path(__file__).resolve().parent
# A3_HIP_LIB: the A/B scripts under tools/ (ab_libs.sh, r6_ab.sh) point this at another build of the library;
# everything else loads the product library next to this file.
LIB_PATH = Path(os.environ["A3_HIP_LIB"]).resolve() if os.environ.get("A3_HIP_LIB") else _HERE / "libaruco3_hip.so"

OK, ERR_INVALID, ERR_HIP, ERR_CAPACITY, ERR_INTERNAL, ERR_NO_DEVICE, ERR_LIMIT = 0, -1, -2, -3, -4, -5, -6
FMT_RGB8, FMT_RGBA8, FMT_L8, FMT_BGRA8 = 0, 1, 2, 3
FMT_YUYV8, FMT_UYVY8 = 5, 6   # packed 4:2:2, 2 bytes per pixel, the luma byte is the grey level (4 is unassigned and refused)
MEM_HOST, MEM_DEVICE = 0, 1
PROFILE_OFF, PROFILE_STAGES, PROFILE_THRESHOLD_ONLY, PROFILE_THRESHOLD_SAMPLED = 0, 1, 2, 3
STAGE_THRESHOLD, STAGE_CONTOUR, STAGE_DECODE = 0, 1, 2
# a3_stats.stepping & 0xFF (include/aruco3_hip.h A3_STEP_*)
STEP_WHOLE, STEP_DECODE_DEFERRED, STEP_HELD_RELEASED_BY_LAST, STEP_HELD_RELEASED_EARLY, STEP_BURST_LAST, STEP_HELD = 0, 1, 2, 3, 4, 5
REFINE_NONE, REFINE_SUBPIX, REFINE_EDGES = 0, 1, 2
BOARD_NONE, BOARD_OK = 0, 1
BOARD_MAX_MARKERS = 1024
DIST_NONE, DIST_RATIONAL = 0, 1
DIST_FISHEYE = 3   # (2 is unassigned)
CHARUCO_MAX_CORNERS = 2048
CHARUCO_NO_ADJ = 0xFFFFFFFF
# a3_calibrate_cameras (include/aruco3_hip.h A3_CALIB_*)
CALIB_FIX_PRINCIPAL_POINT, CALIB_ZERO_TANGENT_DIST, CALIB_FIX_K3, CALIB_RATIONAL_MODEL, CALIB_USE_INTRINSIC_GUESS = 1, 2, 4, 8, 16
CALIB_OK, CALIB_TOO_FEW, CALIB_NO_INIT, CALIB_NOT_FINITE = 1, 2, 3, 4
CALIB_VIEW_USED, CALIB_VIEW_TOO_FEW_POINTS, CALIB_VIEW_DEGENERATE = 1, 2, 3
CALIB_MAX_POINTS, CALIB_MAX_VIEWS, CALIB_MAX_CAMERAS, CALIB_MAX_CALL_VIEWS = 4096, 4096, 1024, 65536
# a3_calibrate_fisheye_cameras (include/aruco3_hip.h A3_FISHEYE_*): the flags of its a3_calib_camera records
FISHEYE_FIX_PRINCIPAL_POINT, FISHEYE_FIX_K1, FISHEYE_FIX_K2, FISHEYE_FIX_K3, FISHEYE_FIX_K4, FISHEYE_USE_INTRINSIC_GUESS = 1, 2, 4, 8, 16, 32
FISHEYE_START_MAX_R = 4.0
# a3_calibrate_rigs (include/aruco3_hip.h A3_RIG_*)
RIG_USE_EXTRINSIC_GUESS, RIG_FIX_EXTRINSICS = 1, 2
RIG_OK, RIG_NOT_CONNECTED, RIG_NOT_FINITE = 1, 2, 3
RIG_OBS_USED, RIG_OBS_TOO_FEW_POINTS, RIG_OBS_DEGENERATE = 1, 2, 3
RIG_FRAME_USED, RIG_FRAME_UNUSED = 1, 2
RIG_MAX_CAMERAS, RIG_MAX_FRAMES, RIG_MAX_RIGS, RIG_MAX_CALL_FRAMES, RIG_MAX_CALL_OBSERVATIONS = 8, 4096, 1024, 65536, 262144
# a3_calibrate_hand_eyes (include/aruco3_hip.h A3_HANDEYE_*)
HANDEYE_USE_GUESS, HANDEYE_FIX_X = 1, 2
HANDEYE_OK, HANDEYE_TOO_FEW_FRAMES, HANDEYE_NO_MOTION, HANDEYE_NOT_FINITE = 1, 2, 3, 4
HANDEYE_FRAME_USED, HANDEYE_FRAME_TOO_FEW_POINTS, HANDEYE_FRAME_DEGENERATE = 1, 2, 3
HANDEYE_MAX_FRAMES, HANDEYE_MAX_PROBLEMS, HANDEYE_MAX_CALL_FRAMES = 256, 1024, 65536
HANDEYE_MIN_PIVOT_RATIO = 1e-4
# a3_build_marker_maps (include/aruco3_hip.h A3_MAP_*)
MAP_USE_GUESS, MAP_FIX_MAP = 1, 2
MAP_OK, MAP_NOT_CONNECTED, MAP_NOT_FINITE = 1, 2, 3
MAP_MARKER_USED, MAP_MARKER_UNSEEN, MAP_MARKER_UNREACHED = 1, 2, 3
MAP_FRAME_USED, MAP_FRAME_UNUSED = 1, 2
MAP_OBS_USED, MAP_OBS_DEGENERATE, MAP_OBS_UNREACHED = 1, 2, 3
MAP_MAX_MARKERS, MAP_MAX_FRAMES, MAP_MAX_MAPS, MAP_MAX_CALL_FRAMES, MAP_MAX_CALL_OBSERVATIONS, MAP_START_OBSERVATIONS = 128, 4096, 1024, 65536, 262144, 8
MAX_THRESHOLD_WINDOWS = 4   # A3_MAX_THRESHOLD_WINDOWS
POLARITY_DARK, POLARITY_BOTH = 0, 1   # A3_POLARITY_*
MARKER_INVERTED = 1                   # A3_MARKER_INVERTED
STEP_NAMES = {0: "whole", 1: "decode_deferred", 2: "held_released_by_last", 3: "held_released_early", 4: "burst_last", 5: "held"}

# every symbol include/aruco3_hip.h declares
SYMBOLS = [
    "a3_abi_version", "a3_default_config", "a3_create", "a3_destroy", "a3_last_error", "a3_set_stream", "a3_get_stream", "a3_set_pool_limits",
    "a3_get_tau", "a3_order_after", "a3_set_debug_taps", "a3_detect_batch", "a3_detect_batch_pose", "a3_detect_batch_submit", "a3_detect_batch_collect", "a3_detect_batch_pose_submit", "a3_detect_batch_pose_collect",
    "a3_host_alloc", "a3_host_free", "a3_host_register", "a3_host_unregister", "a3_get_stats", "a3_synth_render", "a3_download_grey", "a3_download_thresholded",
    "a3_candidate_count", "a3_download_candidates", "a3_download_homographies", "a3_estimate_pose", "a3_estimate_pose_normalized",
    "a3_find_nearest", "a3_calculate_tau", "a3_set_profiling", "a3_get_profile",
    "a3_contour_count", "a3_download_contours", "a3_detection_record_bytes", "a3_pack_detections",
    "a3_default_refine_config", "a3_set_corner_refinement", "a3_get_refined_corners", "a3_refine_corners",
    "a3_set_board", "a3_get_board_poses", "a3_estimate_board_pose", "a3_set_board3d",
    "a3_default_recover_config", "a3_set_board_recovery", "a3_get_board_recovery", "a3_get_recovered_counts", "a3_recover_markers",
    "a3_default_distortion", "a3_set_distortion", "a3_get_undistorted_corners", "a3_undistort_points",
    "a3_default_charuco_config", "a3_set_charuco", "a3_get_charuco_corners", "a3_get_charuco_poses", "a3_interpolate_charuco",
    "a3_calibrate_cameras", "a3_calibrate_fisheye_cameras", "a3_calibrate_rigs", "a3_calibrate_hand_eyes", "a3_build_marker_maps",
    "a3_default_rectify", "a3_rectify_frames", "a3_set_rectification", "a3_get_rectification",
    "a3_reduce_frames", "a3_set_reduction", "a3_get_reduction",
    "a3_set_threshold_windows", "a3_get_threshold_windows",
    "a3_set_marker_polarity", "a3_get_marker_polarity", "a3_get_marker_flags",
]
CAND_DTYPE = np.dtype([("start_key", "<u4"), ("xy", "<u2", (8,))])      # a3_debug_cand (a3_internal.h)
PROJ_DTYPE = np.dtype([("inv", "<f4", (9,)), ("ok", "<i4")])            # A3_DEBUG_PROJ_BYTES
CONTOUR_DTYPE = np.dtype([("frame", "<u4"), ("start_key", "<u4"), ("point_base", "<u4"), ("n", "<u4")])   # a3_debug_contour
# aruco3_amd/csrc/a3_internal.h: probes and single-stage hooks for this repository's tests and tools, not for bindings
INTERNAL_SYMBOLS = ["a3_debug_set_overlap", "a3_debug_build_flags", "a3_debug_spin", "a3_debug_set_hold", "a3_debug_set_jump_rounds", "a3_debug_launch_threshold", "a3_debug_kernel_time", "a3_selftest_ieee", "a3_debug_clockwise", "a3_debug_rotate_bits", "a3_debug_discard_too_near", "a3_debug_inject_candidates", "a3_debug_sample_frames", "a3_debug_frame_candidates", "a3_debug_contour_quads", "a3_debug_merge_candidates"]


class A3Error(RuntimeError):
    def __init__(self, code, message):
        super().__init__(f"aruco3_hip error {code}: {message}")
        self.code = code


class Config(C.Structure):
    _fields_ = [
        ("threshold_window", C.c_uint32),
        ("contour_simplification_epsilon", C.c_double),
        ("min_side_length_factor", C.c_float),
        ("min_corner_separation_factor", C.c_float),
        ("homography_sample_size", C.c_uint32),
        ("filter_high_bit_errors", C.c_uint8),
    ]


class MarkerRec(C.Structure):
    _fields_ = [
        ("frame", C.c_uint32),
        ("id", C.c_uint32),
        ("code", C.c_uint64),
        ("corners", C.c_uint32 * 8),
        ("hamming_distance", C.c_uint8),
        ("rotation", C.c_uint8),
        ("candidate_index", C.c_uint16),
    ]


MARKER_DTYPE = np.dtype([("frame", "<u4"), ("id", "<u4"), ("code", "<u8"), ("corners", "<u4", (8,)), ("hamming_distance", "u1"),
                         ("rotation", "u1"), ("candidate_index", "<u2")], align=True)
assert MARKER_DTYPE.itemsize == C.sizeof(MarkerRec) == 56


class PoseRec(C.Structure):
    _fields_ = [("error", C.c_float), ("rotation", C.c_float * 9), ("translation", C.c_float * 3)]


class Intrinsics(C.Structure):
    _fields_ = [("image_width", C.c_uint32), ("image_height", C.c_uint32), ("focal_x", C.c_float), ("focal_y", C.c_float),
                ("principal_x", C.c_float), ("principal_y", C.c_float)]


class RefineConfig(C.Structure):
    """a3_refine_config: sub-pixel corner refinement (an extension beyond the reference; include/aruco3_hip.h states the algorithm)"""
    _fields_ = [("method", C.c_uint32), ("win_half", C.c_uint32), ("relative_win", C.c_float), ("max_iterations", C.c_uint32),
                ("min_shift", C.c_float)]


class BoardPoseRec(C.Structure):
    """a3_board_pose: one board pose per frame (an extension beyond the reference; include/aruco3_hip.h states the solve)"""
    _fields_ = [("status", C.c_uint32), ("markers_used", C.c_uint32), ("markers_rejected", C.c_uint32), ("iterations", C.c_uint32),
                ("rms_px", C.c_float), ("alt_rms_px", C.c_float), ("rotation", C.c_float * 9), ("translation", C.c_float * 3)]


class RecoverConfig(C.Structure):
    """a3_recover_config: board-aided recovery of rejected markers (an extension beyond the reference; include/aruco3_hip.h states it)"""
    _fields_ = [("mode", C.c_uint32), ("min_markers", C.c_uint32), ("max_distance_px", C.c_float), ("max_hamming", C.c_uint8),
                ("reserved", C.c_uint8 * 3)]


RECOVER_NO_BITS = 255   # a3_recover_config.max_hamming: bits are not compared


class DistortionRec(C.Structure):
    """a3_distortion: lens distortion, OpenCV's rational model (an extension beyond the reference; include/aruco3_hip.h states it)"""
    _fields_ = [("model", C.c_uint32), ("iterations", C.c_uint32), ("k1", C.c_float), ("k2", C.c_float), ("p1", C.c_float),
                ("p2", C.c_float), ("k3", C.c_float), ("k4", C.c_float), ("k5", C.c_float), ("k6", C.c_float),
                ("max_residual_px", C.c_float)]


class CharucoConfig(C.Structure):
    """a3_charuco_config: ChArUco corners (an extension beyond the reference; include/aruco3_hip.h states the algorithm)"""
    _fields_ = [("min_markers", C.c_uint32), ("refine", C.c_uint32), ("win_half", C.c_uint32), ("relative_win", C.c_float),
                ("max_iterations", C.c_uint32), ("min_shift", C.c_float)]


CHARUCO_CORNER_DTYPE = np.dtype([("frame", "<u4"), ("id", "<u4"), ("x", "<f4"), ("y", "<f4"), ("interp_x", "<f4"), ("interp_y", "<f4"),
                                 ("markers_used", "<u4"), ("window", "<u4")])
CHARUCO_POSE_DTYPE = np.dtype([("status", "<u4"), ("corners_used", "<u4"), ("iterations", "<u4"), ("reserved", "<u4"), ("rms_px", "<f4"),
                               ("alt_rms_px", "<f4"), ("rotation", "<f4", (9,)), ("translation", "<f4", (3,))])
BOARD_POSE_DTYPE = np.dtype([("status", "<u4"), ("markers_used", "<u4"), ("markers_rejected", "<u4"), ("iterations", "<u4"),
                             ("rms_px", "<f4"), ("alt_rms_px", "<f4"), ("rotation", "<f4", (9,)), ("translation", "<f4", (3,))])


class CalibCamera(C.Structure):
    """a3_calib_camera: one calibration problem (an extension beyond the reference; include/aruco3_hip.h states the algorithm)"""
    _fields_ = [("image_width", C.c_uint32), ("image_height", C.c_uint32), ("first_view", C.c_uint32), ("n_views", C.c_uint32),
                ("flags", C.c_uint32), ("max_iterations", C.c_uint32), ("guess", Intrinsics), ("guess_distortion", DistortionRec)]


class CalibResult(C.Structure):
    _fields_ = [("status", C.c_uint32), ("views_used", C.c_uint32), ("points_used", C.c_uint32), ("iterations", C.c_uint32),
                ("converged", C.c_uint32), ("reserved", C.c_uint32), ("fx", C.c_double), ("fy", C.c_double), ("cx", C.c_double),
                ("cy", C.c_double), ("dist", C.c_double * 8), ("std_dev", C.c_double * 12), ("rms_px", C.c_double),
                ("intrinsics", Intrinsics), ("distortion", DistortionRec), ("reserved2", C.c_uint32)]


class CalibView(C.Structure):
    _fields_ = [("status", C.c_uint32), ("points", C.c_uint32), ("rms_px", C.c_float), ("rotation", C.c_float * 9), ("translation", C.c_float * 3)]


class Rig(C.Structure):
    """a3_rig: one rig calibration problem (an extension beyond the reference; include/aruco3_hip.h states the algorithm)"""
    _fields_ = [("first_camera", C.c_uint32), ("n_cameras", C.c_uint32), ("first_frame", C.c_uint32), ("n_frames", C.c_uint32),
                ("first_obs", C.c_uint32), ("n_obs", C.c_uint32), ("flags", C.c_uint32), ("max_iterations", C.c_uint32)]


class RigCamera(C.Structure):
    _fields_ = [("a", C.c_double * 12), ("guess_rotation", C.c_double * 9), ("guess_translation", C.c_double * 3)]


class RigObservation(C.Structure):
    _fields_ = [("camera", C.c_uint32), ("frame", C.c_uint32), ("first_point", C.c_uint32), ("n_points", C.c_uint32)]


class RigResult(C.Structure):
    _fields_ = [("status", C.c_uint32), ("frames_used", C.c_uint32), ("obs_used", C.c_uint32), ("points_used", C.c_uint32),
                ("iterations", C.c_uint32), ("converged", C.c_uint32), ("rms_px", C.c_double)]


class RigCameraResult(C.Structure):
    _fields_ = [("rotation", C.c_double * 9), ("translation", C.c_double * 3), ("std_dev", C.c_double * 6), ("rms_px", C.c_double),
                ("rotation_f", C.c_float * 9), ("translation_f", C.c_float * 3), ("obs_used", C.c_uint32), ("points_used", C.c_uint32)]


class RigFrame(C.Structure):
    _fields_ = [("status", C.c_uint32), ("obs_used", C.c_uint32), ("points_used", C.c_uint32), ("rms_px", C.c_float),
                ("rotation", C.c_double * 9), ("translation", C.c_double * 3), ("rotation_f", C.c_float * 9), ("translation_f", C.c_float * 3)]


class RigObservationResult(C.Structure):
    _fields_ = [("status", C.c_uint32), ("points", C.c_uint32), ("rms_px", C.c_float), ("reserved", C.c_uint32)]


class HandEyeProblem(C.Structure):
    """a3_handeye_problem: one hand-eye calibration problem (an extension beyond the reference; include/aruco3_hip.h states the algorithm)"""
    _fields_ = [("first_frame", C.c_uint32), ("n_frames", C.c_uint32), ("flags", C.c_uint32), ("max_iterations", C.c_uint32),
                ("a", C.c_double * 12), ("guess_x_rotation", C.c_double * 9), ("guess_x_translation", C.c_double * 3),
                ("guess_y_rotation", C.c_double * 9), ("guess_y_translation", C.c_double * 3)]


class HandEyeFrame(C.Structure):
    _fields_ = [("rotation", C.c_double * 9), ("translation", C.c_double * 3), ("first_point", C.c_uint32), ("n_points", C.c_uint32)]


class HandEyeResult(C.Structure):
    _fields_ = [("status", C.c_uint32), ("frames_used", C.c_uint32), ("points_used", C.c_uint32), ("pairs_used", C.c_uint32),
                ("iterations", C.c_uint32), ("converged", C.c_uint32), ("rms_px", C.c_double),
                ("x_rotation", C.c_double * 9), ("x_translation", C.c_double * 3), ("y_rotation", C.c_double * 9),
                ("y_translation", C.c_double * 3), ("std_dev", C.c_double * 12),
                ("x_rotation_f", C.c_float * 9), ("x_translation_f", C.c_float * 3), ("y_rotation_f", C.c_float * 9),
                ("y_translation_f", C.c_float * 3)]


class HandEyeFrameResult(C.Structure):
    _fields_ = [("status", C.c_uint32), ("points", C.c_uint32), ("rms_px", C.c_float), ("reserved", C.c_uint32),
                ("rotation", C.c_double * 9), ("translation", C.c_double * 3), ("rotation_f", C.c_float * 9), ("translation_f", C.c_float * 3)]


class Map(C.Structure):
    """a3_map: one marker map problem (an extension beyond the reference; include/aruco3_hip.h states the algorithm)"""
    _fields_ = [("first_marker", C.c_uint32), ("n_markers", C.c_uint32), ("first_frame", C.c_uint32), ("n_frames", C.c_uint32),
                ("first_obs", C.c_uint32), ("n_obs", C.c_uint32), ("flags", C.c_uint32), ("max_iterations", C.c_uint32),
                ("a", C.c_double * 12), ("marker_length", C.c_float), ("reserved", C.c_uint32)]


class MapMarker(C.Structure):
    _fields_ = [("guess_rotation", C.c_double * 9), ("guess_translation", C.c_double * 3)]


class MapObservation(C.Structure):
    _fields_ = [("marker", C.c_uint32), ("frame", C.c_uint32)]


class MapResult(C.Structure):
    _fields_ = [("status", C.c_uint32), ("markers_used", C.c_uint32), ("frames_used", C.c_uint32), ("obs_used", C.c_uint32),
                ("iterations", C.c_uint32), ("converged", C.c_uint32), ("rms_px", C.c_double)]


class MapMarkerResult(C.Structure):
    _fields_ = [("rotation", C.c_double * 9), ("translation", C.c_double * 3), ("std_dev", C.c_double * 6), ("rms_px", C.c_double),
                ("corners", C.c_double * 12), ("rotation_f", C.c_float * 9), ("translation_f", C.c_float * 3), ("status", C.c_uint32),
                ("obs_used", C.c_uint32)]


class MapFrame(C.Structure):
    _fields_ = [("status", C.c_uint32), ("obs_used", C.c_uint32), ("rms_px", C.c_float), ("reserved", C.c_uint32),
                ("rotation", C.c_double * 9), ("translation", C.c_double * 3), ("rotation_f", C.c_float * 9), ("translation_f", C.c_float * 3)]


class MapObservationResult(C.Structure):
    _fields_ = [("status", C.c_uint32), ("rms_px", C.c_float), ("start_rms_px", C.c_float * 2)]


class RectifyRec(C.Structure):
    """a3_rectify: one rectification (an extension beyond the reference; include/aruco3_hip.h states the map and the blend)"""
    _fields_ = [("src", Intrinsics), ("distortion", DistortionRec), ("dst", Intrinsics), ("rotation", C.c_float * 9), ("fill", C.c_uint8),
                ("reserved", C.c_uint8 * 3)]


class ReductionRec(C.Structure):
    """a3_reduction: detection on frames reduced by `factor` (an extension beyond the reference; include/aruco3_hip.h states the plane)"""
    _fields_ = [("factor", C.c_uint32), ("reserved", C.c_uint32 * 3)]


class RectifyInfo(C.Structure):
    _fields_ = [("tiles", C.c_uint32), ("path_tiles", C.c_uint32 * 4), ("reserved", C.c_uint32 * 3)]


class Stats(C.Structure):
    _fields_ = [("darts", C.c_uint64), ("contours_traced", C.c_uint64), ("contours_materialised", C.c_uint64),
                ("candidates_pre", C.c_uint64), ("candidates", C.c_uint64), ("markers", C.c_uint64),
                ("resolve_iterations", C.c_uint32), ("jump_rounds", C.c_uint32), ("chunks", C.c_uint32), ("stepping", C.c_uint32)]

    def as_dict(self):
        d = {k: int(getattr(self, k)) for k, _ in self._fields_}
        d["released_others"] = (d["stepping"] >> 8) & 0xFF     # (a3_stats.stepping: bits 8-15 = chains of other contexts this batch's submit released)
        d["reruns"] = (d["stepping"] >> 16) & 0xFF              # (bits 16-23: synchronous re-runs the device asked for)
        d["stepping"] = STEP_NAMES.get(d["stepping"] & 0xFF, d["stepping"] & 0xFF)
        return d


_lib = None


def load():
    """dlopen the library and declare the prototypes.  Raises if it has not been built."""
    global _lib
    if _lib is not None:
        return _lib
    # One HIP/HSA runtime per process: PyTorch-ROCm wheels bundle their own libamdhip64.so.7 / libhsa-runtime64,
    # and a second copy (from /opt/rocm) initialised in the same process finds no device.  Importing torch first
    # makes the dynamic linker bind this library's NEEDED libamdhip64.so.7 to the copy torch already loaded.
    try:
        import torch  # noqa: F401
    except ImportError:  # a host without PyTorch: the system ROCm runtime is used
        pass
    if not LIB_PATH.exists():
        raise ImportError(f"{LIB_PATH} is missing: build the HIP library first (python -c 'import __graft_entry__ as g; g.build()'). "
                          "aruco3_amd has no CPU fallback.")
    L = C.CDLL(str(LIB_PATH))
    vp, u8p, u32p, u64p, f32p, f64p = C.c_void_p, C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_float), C.POINTER(C.c_double)
    L.a3_abi_version.restype = C.c_int
    L.a3_default_config.restype = None
    L.a3_default_config.argtypes = [C.POINTER(Config)]
    L.a3_create.restype = C.c_int
    L.a3_create.argtypes = [C.c_int, C.POINTER(Config), u64p, C.c_size_t, C.c_uint8, C.c_uint8, C.POINTER(vp)]
    L.a3_destroy.restype = None
    L.a3_destroy.argtypes = [vp]
    L.a3_last_error.restype = C.c_char_p
    L.a3_last_error.argtypes = [vp]
    L.a3_set_stream.restype = C.c_int
    L.a3_set_stream.argtypes = [vp, vp]
    L.a3_get_stream.restype = C.c_int
    L.a3_get_stream.argtypes = [vp, C.POINTER(vp)]
    L.a3_detect_batch_pose_submit.restype = C.c_int
    L.a3_detect_batch_pose_submit.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, C.c_uint32, C.c_float,
                                              C.POINTER(Intrinsics), C.c_size_t]
    L.a3_detect_batch_pose_collect.restype = C.c_int
    L.a3_detect_batch_pose_collect.argtypes = [vp, vp, vp, C.c_size_t, u32p, C.POINTER(C.c_size_t)]
    L.a3_order_after.restype = C.c_int
    L.a3_order_after.argtypes = [vp, vp]
    L.a3_host_alloc.restype = C.c_int
    L.a3_host_alloc.argtypes = [C.c_size_t, C.POINTER(vp)]
    L.a3_host_free.restype = C.c_int
    L.a3_host_free.argtypes = [vp]
    L.a3_host_register.restype = C.c_int
    L.a3_host_register.argtypes = [vp, C.c_size_t]
    L.a3_host_unregister.restype = C.c_int
    L.a3_host_unregister.argtypes = [vp]
    L.a3_set_pool_limits.restype = C.c_int
    L.a3_set_pool_limits.argtypes = [vp, C.c_uint64, C.c_uint64]
    L.a3_get_tau.restype = C.c_int
    L.a3_get_tau.argtypes = [vp, u8p]
    L.a3_set_debug_taps.restype = C.c_int
    L.a3_set_debug_taps.argtypes = [vp, C.c_int]
    L.a3_detect_batch.restype = C.c_int
    L.a3_detect_batch.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, C.c_uint32, vp, C.c_size_t, u32p,
                                  C.POINTER(C.c_size_t)]
    L.a3_detect_batch_submit.restype = C.c_int
    L.a3_detect_batch_submit.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, C.c_uint32, C.c_size_t]
    L.a3_detect_batch_collect.restype = C.c_int
    L.a3_detect_batch_collect.argtypes = [vp, vp, C.c_size_t, u32p, C.POINTER(C.c_size_t)]
    L.a3_detect_batch_pose.restype = C.c_int
    L.a3_detect_batch_pose.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, C.c_uint32, C.c_float,
                                       C.POINTER(Intrinsics), vp, vp, C.c_size_t, u32p, C.POINTER(C.c_size_t)]
    L.a3_synth_render.restype = C.c_int
    L.a3_synth_render.argtypes = [C.c_int, vp, vp, C.c_uint32, vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_int, C.c_float, C.c_float, C.c_int,
                                  vp, C.c_size_t, C.c_size_t]
    if hasattr(L, "a3_debug_set_overlap"):      # (older builds loaded through A3_HIP_LIB for A/B runs lack it)
        L.a3_debug_set_overlap.restype = C.c_int
        L.a3_debug_set_overlap.argtypes = [C.c_int]
    if hasattr(L, "a3_debug_launch_threshold"):
        L.a3_debug_launch_threshold.restype = C.c_int
        L.a3_debug_launch_threshold.argtypes = [vp, vp, C.c_int, C.c_uint32, C.c_uint32, C.c_uint32]
    if hasattr(L, "a3_debug_set_hold"):
        L.a3_debug_set_hold.restype = C.c_int
        L.a3_debug_set_hold.argtypes = [C.c_int]
    if hasattr(L, "a3_debug_set_jump_rounds"):
        L.a3_debug_set_jump_rounds.restype = C.c_int
        L.a3_debug_set_jump_rounds.argtypes = [C.c_int]
    if hasattr(L, "a3_debug_spin"):
        L.a3_debug_spin.restype = C.c_int
        L.a3_debug_spin.argtypes = [vp, C.c_int, C.c_int, C.c_int]
    if hasattr(L, "a3_debug_build_flags"):
        L.a3_debug_build_flags.restype = C.c_int
        L.a3_debug_build_flags.argtypes = []
    L.a3_debug_kernel_time.restype = C.c_int
    L.a3_debug_kernel_time.argtypes = [vp, C.c_int, C.c_int, C.c_int, C.POINTER(C.c_float)]
    L.a3_get_stats.restype = C.c_int
    L.a3_get_stats.argtypes = [vp, C.POINTER(Stats)]
    L.a3_download_grey.restype = C.c_int
    L.a3_download_grey.argtypes = [vp, C.c_uint32, u8p]
    L.a3_download_thresholded.restype = C.c_int
    L.a3_download_thresholded.argtypes = [vp, C.c_uint32, u8p]
    L.a3_candidate_count.restype = C.c_int
    L.a3_candidate_count.argtypes = [vp, C.c_uint32, u32p, u32p]
    L.a3_download_candidates.restype = C.c_int
    L.a3_download_candidates.argtypes = [vp, C.c_uint32, C.c_int, u32p, C.c_size_t]
    L.a3_download_homographies.restype = C.c_int
    L.a3_download_homographies.argtypes = [vp, C.c_uint32, u8p, u8p, u64p, C.POINTER(C.c_int32), C.c_size_t]
    L.a3_estimate_pose.restype = C.c_int
    L.a3_estimate_pose.argtypes = [vp, u32p, C.c_size_t, C.c_float, C.POINTER(Intrinsics), C.c_uint32, C.c_uint32, C.POINTER(PoseRec)]
    L.a3_estimate_pose_normalized.restype = C.c_int
    L.a3_estimate_pose_normalized.argtypes = [vp, f32p, C.c_size_t, C.c_float, C.POINTER(PoseRec)]
    L.a3_find_nearest.restype = C.c_int
    L.a3_find_nearest.argtypes = [vp, u64p, C.c_size_t, u32p, u8p]
    L.a3_calculate_tau.restype = C.c_int
    L.a3_calculate_tau.argtypes = [C.c_int, u64p, C.c_size_t, u8p]
    L.a3_set_profiling.restype = C.c_int
    L.a3_set_profiling.argtypes = [vp, C.c_int]
    L.a3_get_profile.restype = C.c_int
    L.a3_get_profile.argtypes = [vp, C.c_int, f64p, u64p, C.c_int]
    L.a3_selftest_ieee.restype = C.c_int
    L.a3_selftest_ieee.argtypes = [vp, f64p, f64p, C.c_size_t, f64p, f64p, f32p, f32p]
    L.a3_contour_count.restype = C.c_int
    L.a3_contour_count.argtypes = [vp, C.c_uint32, u32p, u64p]
    L.a3_download_contours.restype = C.c_int
    L.a3_download_contours.argtypes = [vp, C.c_uint32, u32p, u32p, u32p, C.c_size_t, C.c_size_t]
    L.a3_detection_record_bytes.restype = C.c_size_t
    L.a3_detection_record_bytes.argtypes = [C.c_uint32, C.c_int]
    L.a3_pack_detections.restype = C.c_int
    L.a3_pack_detections.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_int, vp, C.c_size_t]
    L.a3_debug_clockwise.restype = C.c_int
    L.a3_debug_clockwise.argtypes = [vp, C.POINTER(C.c_int32), C.c_size_t, C.POINTER(C.c_int32)]
    L.a3_debug_rotate_bits.restype = C.c_int
    L.a3_debug_rotate_bits.argtypes = [vp, u8p, C.c_uint32, C.c_uint32, u8p]
    L.a3_debug_inject_candidates.restype = C.c_int
    L.a3_debug_inject_candidates.argtypes = [vp, u32p, C.c_size_t]
    if hasattr(L, "a3_debug_sample_frames"):    # (older builds loaded through A3_HIP_LIB for A/B runs lack it)
        L.a3_debug_sample_frames.restype = C.c_int
        L.a3_debug_sample_frames.argtypes = [vp, C.c_int]
    if hasattr(L, "a3_refine_corners"):      # (older builds loaded through A3_HIP_LIB for A/B runs lack corner refinement)
        L.a3_default_refine_config.restype = None
        L.a3_default_refine_config.argtypes = [C.POINTER(RefineConfig)]
        L.a3_set_corner_refinement.restype = C.c_int
        L.a3_set_corner_refinement.argtypes = [vp, C.POINTER(RefineConfig)]
        L.a3_get_refined_corners.restype = C.c_int
        L.a3_get_refined_corners.argtypes = [vp, f32p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.a3_refine_corners.restype = C.c_int
        L.a3_refine_corners.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_size_t, f32p, f32p, C.c_size_t]
    if hasattr(L, "a3_set_board"):      # (older builds loaded through A3_HIP_LIB for A/B runs lack the board pose)
        L.a3_set_board.restype = C.c_int
        L.a3_set_board.argtypes = [vp, u32p, f32p, C.c_size_t]
        L.a3_get_board_poses.restype = C.c_int
        L.a3_get_board_poses.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.a3_estimate_board_pose.restype = C.c_int
        L.a3_estimate_board_pose.argtypes = [vp, u32p, f32p, C.c_size_t, C.POINTER(Intrinsics), C.c_uint32, C.c_uint32, C.POINTER(BoardPoseRec)]
    if hasattr(L, "a3_set_board3d"):      # (older builds loaded through A3_HIP_LIB for A/B runs lack 3-D boards)
        L.a3_set_board3d.restype = C.c_int
        L.a3_set_board3d.argtypes = [vp, u32p, f32p, C.c_size_t]
    if hasattr(L, "a3_set_board_recovery"):      # (older builds loaded through A3_HIP_LIB for A/B runs lack board recovery)
        u64p, u8p = C.POINTER(C.c_uint64), C.POINTER(C.c_uint8)
        L.a3_default_recover_config.restype = C.c_int
        L.a3_default_recover_config.argtypes = [vp, C.POINTER(RecoverConfig)]
        L.a3_set_board_recovery.restype = C.c_int
        L.a3_set_board_recovery.argtypes = [vp, C.POINTER(RecoverConfig)]
        L.a3_get_board_recovery.restype = C.c_int
        L.a3_get_board_recovery.argtypes = [vp, C.POINTER(RecoverConfig)]
        L.a3_get_recovered_counts.restype = C.c_int
        L.a3_get_recovered_counts.argtypes = [vp, u32p, C.c_size_t]
        L.a3_recover_markers.restype = C.c_int
        L.a3_recover_markers.argtypes = [vp, u32p, u32p, C.c_size_t, u32p, u64p, u8p, C.c_size_t, C.POINTER(RecoverConfig), vp, C.c_size_t,
                                         C.POINTER(C.c_size_t)]
    if hasattr(L, "a3_set_distortion"):      # (older builds loaded through A3_HIP_LIB for A/B runs lack lens distortion)
        L.a3_default_distortion.restype = None
        L.a3_default_distortion.argtypes = [C.POINTER(DistortionRec)]
        L.a3_set_distortion.restype = C.c_int
        L.a3_set_distortion.argtypes = [vp, C.POINTER(DistortionRec)]
        L.a3_get_undistorted_corners.restype = C.c_int
        L.a3_get_undistorted_corners.argtypes = [vp, f32p, f32p, C.c_size_t, C.POINTER(C.c_size_t)]
        L.a3_undistort_points.restype = C.c_int
        L.a3_undistort_points.argtypes = [vp, f32p, C.c_size_t, C.POINTER(Intrinsics), C.POINTER(DistortionRec), f32p, f32p]
    if hasattr(L, "a3_set_charuco"):      # (older builds loaded through A3_HIP_LIB for A/B runs lack ChArUco)
        L.a3_default_charuco_config.restype = None
        L.a3_default_charuco_config.argtypes = [C.POINTER(CharucoConfig)]
        L.a3_set_charuco.restype = C.c_int
        L.a3_set_charuco.argtypes = [vp, f32p, u32p, C.c_size_t, C.POINTER(CharucoConfig)]
        L.a3_get_charuco_corners.restype = C.c_int
        L.a3_get_charuco_corners.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.a3_get_charuco_poses.restype = C.c_int
        L.a3_get_charuco_poses.argtypes = [vp, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        L.a3_interpolate_charuco.restype = C.c_int
        L.a3_interpolate_charuco.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_size_t, u32p, f32p, C.c_size_t, vp,
                                             C.c_size_t, C.POINTER(C.c_size_t)]
    if hasattr(L, "a3_calibrate_rigs"):
        L.a3_calibrate_rigs.restype = C.c_int
        L.a3_calibrate_rigs.argtypes = [vp, C.POINTER(Rig), C.c_size_t, C.POINTER(RigCamera), C.c_size_t, C.POINTER(RigObservation), C.c_size_t,
                                        f32p, f32p, C.POINTER(RigResult), C.POINTER(RigCameraResult), C.POINTER(RigFrame),
                                        C.POINTER(RigObservationResult)]
    if hasattr(L, "a3_calibrate_hand_eyes"):
        L.a3_calibrate_hand_eyes.restype = C.c_int
        L.a3_calibrate_hand_eyes.argtypes = [vp, C.POINTER(HandEyeProblem), C.c_size_t, C.POINTER(HandEyeFrame), C.c_size_t, f32p, f32p,
                                             C.POINTER(HandEyeResult), C.POINTER(HandEyeFrameResult)]
    if hasattr(L, "a3_build_marker_maps"):
        L.a3_build_marker_maps.restype = C.c_int
        L.a3_build_marker_maps.argtypes = [vp, C.POINTER(Map), C.c_size_t, C.POINTER(MapMarker), C.c_size_t, C.POINTER(MapObservation),
                                           C.c_size_t, f32p, C.POINTER(MapResult), C.POINTER(MapMarkerResult), C.POINTER(MapFrame),
                                           C.POINTER(MapObservationResult)]
    if hasattr(L, "a3_calibrate_cameras"):      # (older builds loaded through A3_HIP_LIB for A/B runs lack calibration)
        L.a3_calibrate_cameras.restype = C.c_int
        L.a3_calibrate_cameras.argtypes = [vp, C.POINTER(CalibCamera), C.c_size_t, u32p, C.c_size_t, f32p, f32p, C.POINTER(CalibResult),
                                           C.POINTER(CalibView)]
    if hasattr(L, "a3_calibrate_fisheye_cameras"):      # (older builds loaded through A3_HIP_LIB for A/B runs lack it)
        L.a3_calibrate_fisheye_cameras.restype = C.c_int
        L.a3_calibrate_fisheye_cameras.argtypes = [vp, C.POINTER(CalibCamera), C.c_size_t, u32p, C.c_size_t, f32p, f32p, C.POINTER(CalibResult),
                                                   C.POINTER(CalibView)]
    if hasattr(L, "a3_rectify_frames"):      # (older builds loaded through A3_HIP_LIB for A/B runs lack rectification)
        L.a3_default_rectify.restype = None
        L.a3_default_rectify.argtypes = [C.POINTER(RectifyRec), C.POINTER(Intrinsics), C.POINTER(DistortionRec)]
        L.a3_rectify_frames.restype = C.c_int
        L.a3_rectify_frames.argtypes = [vp, vp, C.c_int, C.c_int, C.c_size_t, C.c_size_t, C.c_uint32, C.POINTER(RectifyRec), vp, C.c_int,
                                        C.c_size_t, C.c_size_t, C.POINTER(RectifyInfo)]
    if hasattr(L, "a3_reduce_frames"):       # (likewise detection on reduced frames)
        L.a3_reduce_frames.restype = C.c_int
        L.a3_reduce_frames.argtypes = [vp, vp, C.c_int, C.c_int, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, C.c_uint32, C.c_uint32, vp, C.c_int,
                                       C.c_size_t, C.c_size_t]
        L.a3_set_reduction.restype = C.c_int
        L.a3_set_reduction.argtypes = [vp, C.POINTER(ReductionRec)]
        L.a3_get_reduction.restype = C.c_int
        L.a3_get_reduction.argtypes = [vp, C.POINTER(ReductionRec), C.POINTER(C.c_int)]
    if hasattr(L, "a3_set_marker_polarity"):   # (likewise inverted markers)
        L.a3_set_marker_polarity.restype = C.c_int
        L.a3_set_marker_polarity.argtypes = [vp, C.c_int]
        L.a3_get_marker_polarity.restype = C.c_int
        L.a3_get_marker_polarity.argtypes = [vp, C.POINTER(C.c_int)]
        L.a3_get_marker_flags.restype = C.c_int
        L.a3_get_marker_flags.argtypes = [vp, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t)]
    if hasattr(L, "a3_set_threshold_windows"):   # (likewise several threshold windows)
        L.a3_set_threshold_windows.restype = C.c_int
        L.a3_set_threshold_windows.argtypes = [vp, C.POINTER(C.c_uint32), C.c_size_t]
        L.a3_get_threshold_windows.restype = C.c_int
        L.a3_get_threshold_windows.argtypes = [vp, C.POINTER(C.c_uint32), C.c_size_t, C.POINTER(C.c_size_t)]
    if hasattr(L, "a3_set_rectification"):   # (likewise rectification inside the detect calls)
        L.a3_set_rectification.restype = C.c_int
        L.a3_set_rectification.argtypes = [vp, C.POINTER(RectifyRec)]
        L.a3_get_rectification.restype = C.c_int
        L.a3_get_rectification.argtypes = [vp, C.POINTER(RectifyRec), C.POINTER(C.c_int)]
    L.a3_debug_discard_too_near.restype = C.c_int
    L.a3_debug_discard_too_near.argtypes = [vp, u32p, C.c_size_t, C.c_float, u32p, C.POINTER(C.c_size_t)]
    if hasattr(L, "a3_debug_merge_candidates"):      # (likewise)
        L.a3_debug_merge_candidates.restype = C.c_int
        L.a3_debug_merge_candidates.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, u32p, vp, C.c_float, C.c_uint32, C.POINTER(C.c_uint16),
                                                C.POINTER(C.c_uint16), u32p, u32p, u32p, vp, u32p, u32p]
    if hasattr(L, "a3_debug_frame_candidates"):      # (older builds loaded through A3_HIP_LIB for A/B runs lack it)
        L.a3_debug_frame_candidates.restype = C.c_int
        L.a3_debug_frame_candidates.argtypes = [vp, C.c_uint32, C.c_uint32, u32p, vp, C.c_float, C.c_uint32, C.POINTER(C.c_uint16),
                                                C.POINTER(C.c_uint16), u32p, u32p, u32p, vp]
    if hasattr(L, "a3_debug_contour_quads"):         # (likewise)
        L.a3_debug_contour_quads.restype = C.c_int
        L.a3_debug_contour_quads.argtypes = [vp, C.c_uint32, C.c_uint32, C.c_uint32, C.c_double, C.c_uint32, C.c_uint32, C.c_uint32, C.c_uint32,
                                             C.c_uint32, C.c_uint32, C.c_uint32, vp, C.c_uint32, vp, C.c_size_t, u32p, vp, u32p]
    _lib = L
    return L


def library_info() -> dict:
    """which shared library this process runs on (bench.py and the GPU tests put it into their output: a leftover A3_HIP_LIB
    pointing at a tuning build must not pass for the product)"""
    L = load()
    flags = int(L.a3_debug_build_flags()) if hasattr(L, "a3_debug_build_flags") else -1
    return {"path": str(LIB_PATH), "from_A3_HIP_LIB": bool(os.environ.get("A3_HIP_LIB")), "tuning_build": bool(flags & 1) if flags >= 0 else None,
            "non_default_kernel_build": bool(flags & 2) if flags >= 0 else None, "abi": int(L.a3_abi_version())}


class PinnedBuffer:
    """a3_host_alloc as a numpy uint8 array (`.array`): frames placed here cross the link asynchronously and at its full rate"""

    def __init__(self, nbytes: int):
        p = C.c_void_p()
        rc = load().a3_host_alloc(nbytes, C.byref(p))
        if rc != OK:
            raise A3Error(rc, load().a3_last_error(None).decode("utf-8", "replace"))
        self.ptr, self.nbytes = p.value, nbytes
        self.array = np.ctypeslib.as_array((C.c_uint8 * nbytes).from_address(p.value))

    def close(self):
        if getattr(self, "ptr", None):
            self.array = None
            load().a3_host_free(C.c_void_p(self.ptr))
            self.ptr = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _f32(a, cols: int) -> np.ndarray:
    """a contiguous float32 (n, cols) view or copy of `a`"""
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(-1, cols))


def _symbol(name: str):
    """an entry point that a library built before it was added does not have"""
    fn = getattr(load(), name, None)
    if fn is None:
        raise A3Error(-1, f"this libaruco3_hip.so has no {name}")
    return fn


def check(rc, ctx=None):
    if rc != OK:
        raise A3Error(rc, load().a3_last_error(ctx).decode("utf-8", "replace"))


def default_config() -> Config:
    cfg = Config()
    load().a3_default_config(C.byref(cfg))
    return cfg


def default_refine_config() -> RefineConfig:
    cfg = RefineConfig()
    load().a3_default_refine_config(C.byref(cfg))
    return cfg


def default_distortion() -> DistortionRec:
    d = DistortionRec()
    load().a3_default_distortion(C.byref(d))
    return d


def default_rectify(src: Intrinsics, d: DistortionRec = None) -> RectifyRec:
    r = RectifyRec()
    load().a3_default_rectify(C.byref(r), C.byref(src), C.byref(d) if d is not None else None)
    return r


def default_charuco_config() -> CharucoConfig:
    cfg = CharucoConfig()
    load().a3_default_charuco_config(C.byref(cfg))
    return cfg


def synth_render(device: int, frames: np.ndarray, markers: np.ndarray, width: int, height: int, paper: bool, black: float, white: float,
                 supersample: int, out_ptr: int, row_stride: int = 0, frame_stride: int = 0, stream: int = 0) -> None:
    """a3_synth_render: frames / markers are the record arrays of aruco3_amd.synth.device_layout, out_ptr a device pointer."""
    frames = np.ascontiguousarray(frames)
    markers = np.ascontiguousarray(markers)
    rc = load().a3_synth_render(device, C.c_void_p(stream), frames.ctypes.data_as(C.c_void_p), len(frames),
                                markers.ctypes.data_as(C.c_void_p) if len(markers) else None, len(markers), width, height, int(paper),
                                black, white, supersample, C.c_void_p(out_ptr), row_stride, frame_stride)
    if rc != 0:
        raise A3Error(rc, "a3_synth_render failed")


class Context:
    """Owns one a3_ctx (one device, one stream)."""

    def __init__(self, config: Config, codes: np.ndarray, num_bits: int, tau: int, device: int = 0):
        L = load()
        self._codes = np.ascontiguousarray(codes, dtype=np.uint64)
        h = C.c_void_p()
        rc = L.a3_create(device, C.byref(config), _p(self._codes, C.c_uint64), self._codes.size, num_bits, tau, C.byref(h))
        check(rc, None)
        self.handle = h
        self.device = device
        self.sample = int(config.homography_sample_size)

    def close(self):
        if getattr(self, "handle", None):
            load().a3_destroy(self.handle)
            self.handle = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    @property
    def tau(self) -> int:
        t = C.c_uint8()
        check(load().a3_get_tau(self.handle, C.byref(t)), self.handle)
        return int(t.value)

    def set_stream(self, stream_ptr: int):
        check(load().a3_set_stream(self.handle, C.c_void_p(stream_ptr)), self.handle)

    @property
    def stream_ptr(self) -> int:
        """hipStream_t the context enqueues on (a3_get_stream): wrap it with torch.cuda.ExternalStream to order torch work after it"""
        p = C.c_void_p()
        check(load().a3_get_stream(self.handle, C.byref(p)), self.handle)
        return int(p.value or 0)

    def order_after(self, other: "Context"):
        """a3_order_after: this context's next batch starts only after `other`'s work in flight has finished (burst stepping)"""
        check(load().a3_order_after(self.handle, other.handle), self.handle)

    def set_debug_taps(self, on: bool):
        check(load().a3_set_debug_taps(self.handle, int(on)), self.handle)

    def set_pool_limits(self, max_darts: int = 0, max_points: int = 0):
        check(load().a3_set_pool_limits(self.handle, max_darts, max_points), self.handle)

    def set_profiling(self, mode):
        """False / 0 off, True / 1 every stage, PROFILE_THRESHOLD_ONLY (2): the threshold stage only (two event records per batch)"""
        check(load().a3_set_profiling(self.handle, int(mode)), self.handle)

    def profile(self, stage: int, reset: bool = False):
        ms, n = C.c_double(), C.c_uint64()
        check(load().a3_get_profile(self.handle, stage, C.byref(ms), C.byref(n), int(reset)), self.handle)
        return float(ms.value), int(n.value)

    def debug_kernel_time(self, kernel: int, dbg: int = 0, reps: int = 5) -> float:
        ms = C.c_float()
        check(load().a3_debug_kernel_time(self.handle, kernel, dbg, reps, C.byref(ms)), self.handle)
        return ms.value

    def stats(self) -> dict:
        s = Stats()
        check(load().a3_get_stats(self.handle, C.byref(s)), self.handle)
        return s.as_dict()

    def detect_batch(self, pixels_ptr: int, memory: int, fmt: int, width: int, height: int, row_stride: int, frame_stride: int, n_frames: int,
                     out_cap: int = 0):
        """-> (markers structured array, per-frame counts)"""
        cap = out_cap or max(64 * n_frames, 64)
        out = np.empty(cap, dtype=MARKER_DTYPE)   # only the first n records are written and returned
        per = np.zeros(max(n_frames, 1), dtype=np.uint32)
        n = C.c_size_t()
        rc = load().a3_detect_batch(self.handle, C.c_void_p(pixels_ptr), memory, fmt, width, height, row_stride, frame_stride, n_frames,
                                    out.ctypes.data_as(C.c_void_p), cap, _p(per, C.c_uint32), C.byref(n))
        check(rc, self.handle)
        return out[: n.value], per[:n_frames]

    def submit(self, pixels_ptr: int, memory: int, fmt: int, width: int, height: int, row_stride: int, frame_stride: int, n_frames: int,
               out_cap: int = 0):
        """Enqueue a batch without waiting (a3_detect_batch_submit); `collect()` returns what detect_batch would."""
        self._pending = (out_cap or max(64 * n_frames, 64), n_frames)
        check(load().a3_detect_batch_submit(self.handle, C.c_void_p(pixels_ptr), memory, fmt, width, height, row_stride, frame_stride, n_frames,
                                            self._pending[0]), self.handle)

    def collect(self):
        cap, n_frames = self._pending
        out = np.empty(cap, dtype=MARKER_DTYPE)
        per = np.zeros(max(n_frames, 1), dtype=np.uint32)
        n = C.c_size_t()
        check(load().a3_detect_batch_collect(self.handle, out.ctypes.data_as(C.c_void_p), cap, _p(per, C.c_uint32), C.byref(n)), self.handle)
        return out[: n.value], per[:n_frames]

    def detect_batch_pose(self, pixels_ptr: int, memory: int, fmt: int, width: int, height: int, row_stride: int, frame_stride: int,
                          n_frames: int, marker_size_mm: float, intrinsics: "Intrinsics" = None, out_cap: int = 0):
        """-> (markers, per-frame counts, poses float32 [n_markers, 2, 13] = error, 9 rotation row-major, 3 translation)"""
        cap = out_cap or max(64 * n_frames, 64)
        out = np.zeros(cap, dtype=MARKER_DTYPE)
        poses = np.zeros((cap, 2, 13), dtype=np.float32)
        per = np.zeros(max(n_frames, 1), dtype=np.uint32)
        n = C.c_size_t()
        rc = load().a3_detect_batch_pose(self.handle, C.c_void_p(pixels_ptr), memory, fmt, width, height, row_stride, frame_stride, n_frames,
                                         marker_size_mm, C.byref(intrinsics) if intrinsics else None, out.ctypes.data_as(C.c_void_p),
                                         poses.ctypes.data_as(C.c_void_p), cap, _p(per, C.c_uint32), C.byref(n))
        check(rc, self.handle)
        return out[: n.value], per[:n_frames], poses[: n.value]

    def submit_pose(self, pixels_ptr: int, memory: int, fmt: int, width: int, height: int, row_stride: int, frame_stride: int, n_frames: int,
                    marker_size_mm: float, intrinsics: "Intrinsics" = None, out_cap: int = 0):
        """a3_detect_batch_pose_submit; `collect_pose()` returns what detect_batch_pose would."""
        self._pending = (out_cap or max(64 * n_frames, 64), n_frames)
        check(load().a3_detect_batch_pose_submit(self.handle, C.c_void_p(pixels_ptr), memory, fmt, width, height, row_stride, frame_stride, n_frames,
                                                 marker_size_mm, C.byref(intrinsics) if intrinsics else None, self._pending[0]), self.handle)

    def collect_pose(self):
        cap, n_frames = self._pending
        out = np.empty(cap, dtype=MARKER_DTYPE)
        poses = np.zeros((cap, 2, 13), dtype=np.float32)
        per = np.zeros(max(n_frames, 1), dtype=np.uint32)
        n = C.c_size_t()
        check(load().a3_detect_batch_pose_collect(self.handle, out.ctypes.data_as(C.c_void_p), poses.ctypes.data_as(C.c_void_p), cap,
                                                  _p(per, C.c_uint32), C.byref(n)), self.handle)
        return out[: n.value], per[:n_frames], poses[: n.value]

    # ---- sub-pixel corner refinement ----
    def set_corner_refinement(self, cfg: "RefineConfig" = None):
        """a3_set_corner_refinement: None (or method REFINE_NONE) turns it off; applies to batches submitted afterwards"""
        check(load().a3_set_corner_refinement(self.handle, C.byref(cfg) if cfg is not None else None), self.handle)

    def refined_corners(self) -> np.ndarray:
        """a3_get_refined_corners: float32 [n_markers, 4, 2] of the last collected batch, in marker order"""
        n = C.c_size_t()
        L = load()
        rc = L.a3_get_refined_corners(self.handle, None, 0, C.byref(n))
        if rc not in (OK, ERR_CAPACITY):
            check(rc, self.handle)
        out = np.zeros((max(n.value, 1), 4, 2), dtype=np.float32)
        check(L.a3_get_refined_corners(self.handle, _p(out, C.c_float), max(n.value, 1), C.byref(n)), self.handle)
        return out[: n.value]

    def refine_corners(self, pixels_ptr: int, memory: int, fmt: int, width: int, height: int, row_stride: int, corners: np.ndarray,
                       cell_px: np.ndarray = None) -> np.ndarray:
        """a3_refine_corners (stand-alone, one frame): corners (..., 2) -> refined float32 (n, 2).  With the context's method REFINE_EDGES
        the corners are quads (a multiple of 4, a3_marker order) and cell_px is read at each quad's first corner."""
        xy = _f32(corners, 2).copy()
        cp = None if cell_px is None else np.ascontiguousarray(np.asarray(cell_px, dtype=np.float32).reshape(-1))
        if cp is not None and cp.size != xy.shape[0]:
            raise ValueError("cell_px needs one value per corner")
        check(load().a3_refine_corners(self.handle, C.c_void_p(pixels_ptr), memory, fmt, width, height, row_stride, _p(xy, C.c_float),
                                       None if cp is None else _p(cp, C.c_float), xy.shape[0]), self.handle)
        return xy

    # ---- board pose ----
    def set_board(self, ids=None, corners=None):
        """a3_set_board: ids (n,), corners (n, 4, 2) float in board units; None / empty clears it; applies to batches submitted afterwards"""
        if ids is None or len(ids) == 0:
            check(load().a3_set_board(self.handle, None, None, 0), self.handle)
            return
        i = np.ascontiguousarray(np.asarray(ids, dtype=np.uint32).reshape(-1))
        c = _f32(corners, 8)
        if c.shape[0] != i.size:
            raise ValueError("set_board needs four corners per id")
        check(load().a3_set_board(self.handle, _p(i, C.c_uint32), _p(c, C.c_float), i.size), self.handle)

    def set_board3d(self, ids=None, corners=None):
        """a3_set_board3d: ids (n,), corners (n, 4, 3) float in board units; None / empty clears the board; applies to batches submitted
        afterwards"""
        if ids is None or len(ids) == 0:
            check(load().a3_set_board3d(self.handle, None, None, 0), self.handle)
            return
        i = np.ascontiguousarray(np.asarray(ids, dtype=np.uint32).reshape(-1))
        c = _f32(corners, 12)
        if c.shape[0] != i.size:
            raise ValueError("set_board3d needs four corners per id")
        check(load().a3_set_board3d(self.handle, _p(i, C.c_uint32), _p(c, C.c_float), i.size), self.handle)

    def board_poses(self) -> np.ndarray:
        """a3_get_board_poses: BOARD_POSE_DTYPE records of the last collected batch, one per frame"""
        n = C.c_size_t()
        L = load()
        rc = L.a3_get_board_poses(self.handle, None, 0, C.byref(n))
        if rc not in (OK, ERR_CAPACITY):
            check(rc, self.handle)
        out = np.zeros(max(n.value, 1), dtype=BOARD_POSE_DTYPE)
        check(L.a3_get_board_poses(self.handle, out.ctypes.data_as(C.c_void_p), max(n.value, 1), C.byref(n)), self.handle)
        return out[: n.value]

    def estimate_board_pose(self, ids, corners, image_size=None, intrinsics: "Intrinsics" = None) -> np.ndarray:
        """a3_estimate_board_pose (stand-alone, one frame): ids (n,), image corners (n, 4, 2) in pixels -> one BOARD_POSE_DTYPE record"""
        i = np.ascontiguousarray(np.asarray(ids, dtype=np.uint32).reshape(-1))
        c = _f32(corners, 8)
        if c.shape[0] != i.size:
            raise ValueError("estimate_board_pose needs four corners per id")
        iw, ih = image_size if image_size else (0, 0)
        rec = BoardPoseRec()
        check(load().a3_estimate_board_pose(self.handle, _p(i, C.c_uint32), _p(c, C.c_float), i.size, C.byref(intrinsics) if intrinsics else None,
                                            iw, ih, C.byref(rec)), self.handle)
        out = np.zeros(1, dtype=BOARD_POSE_DTYPE)
        C.memmove(out.ctypes.data, C.addressof(rec), C.sizeof(rec))
        return out[0]

    # ---- board-aided recovery ----
    def default_recover_config(self) -> "RecoverConfig":
        """a3_default_recover_config: on, min_markers 2, max_distance_px 10, max_hamming derived from the dictionary's bit count"""
        cfg = RecoverConfig()
        check(load().a3_default_recover_config(self.handle, C.byref(cfg)), self.handle)
        return cfg

    def set_board_recovery(self, cfg: "RecoverConfig" = None):
        """a3_set_board_recovery: None (or mode 0) clears it; applies to batches submitted afterwards"""
        check(load().a3_set_board_recovery(self.handle, C.byref(cfg) if cfg is not None else None), self.handle)

    def board_recovery(self):
        """a3_get_board_recovery -> the RecoverConfig in force, or None"""
        cfg = RecoverConfig()
        check(load().a3_get_board_recovery(self.handle, C.byref(cfg)), self.handle)
        return cfg if cfg.mode else None

    def recovered_counts(self, n_frames: int) -> np.ndarray:
        """a3_get_recovered_counts: how many markers at the tail of each frame's segment of the last collected batch are recovered ones"""
        out = np.zeros(max(n_frames, 1), dtype=np.uint32)
        check(load().a3_get_recovered_counts(self.handle, _p(out, C.c_uint32), n_frames), self.handle)
        return out[:n_frames]

    def recover_markers(self, detected_ids, detected_corners, candidate_corners, codes4, has_codes, cfg: "RecoverConfig", out_cap: int = None) -> np.ndarray:
        """a3_recover_markers (stand-alone, one frame): detected ids (n,) and integer corners (n, 4, 2); rejected candidates' integer
        corners (m, 4, 2), their four rotated codes (m, 4) and has-codes flags (m,) -> MARKER_DTYPE records, in candidate order"""
        i = np.ascontiguousarray(np.asarray(detected_ids, dtype=np.uint32).reshape(-1))
        d = np.ascontiguousarray(np.asarray(detected_corners, dtype=np.uint32).reshape(-1, 8))
        q = np.ascontiguousarray(np.asarray(candidate_corners, dtype=np.uint32).reshape(-1, 8))
        k = np.ascontiguousarray(np.asarray(codes4, dtype=np.uint64).reshape(-1, 4))
        h = np.ascontiguousarray(np.asarray(has_codes, dtype=np.uint8).reshape(-1))
        if d.shape[0] != i.size:
            raise ValueError("recover_markers needs four corners per detected id")
        if k.shape[0] != q.shape[0] or h.size != q.shape[0]:
            raise ValueError("recover_markers needs four codes and one flag per candidate")
        cap = q.shape[0] if out_cap is None else int(out_cap)
        out = np.zeros(max(cap, 1), dtype=MARKER_DTYPE)
        n = C.c_size_t()
        check(load().a3_recover_markers(self.handle, _p(i, C.c_uint32), _p(d, C.c_uint32), i.size, _p(q, C.c_uint32), _p(k, C.c_uint64), _p(h, C.c_uint8),
                                        q.shape[0], C.byref(cfg), out.ctypes.data_as(C.c_void_p), cap, C.byref(n)), self.handle)
        return out[: n.value]

    # ---- lens distortion ----
    # ---- ChArUco ----
    def set_charuco(self, corners=None, adjacent_ids=None, cfg: "CharucoConfig" = None):
        """a3_set_charuco: chessboard corners (n, 2) in board units and adjacent marker ids (n, 4); None / empty clears it"""
        if corners is None or len(corners) == 0:
            check(load().a3_set_charuco(self.handle, None, None, 0, None), self.handle)
            return
        c = _f32(corners, 2)
        a = np.ascontiguousarray(np.asarray(adjacent_ids, dtype=np.uint32).reshape(-1, 4))
        if a.shape[0] != c.shape[0]:
            raise ValueError("set_charuco needs four adjacent ids per corner")
        check(load().a3_set_charuco(self.handle, _p(c, C.c_float), _p(a, C.c_uint32), c.shape[0], C.byref(cfg) if cfg else None), self.handle)

    def charuco_corners(self) -> np.ndarray:
        """a3_get_charuco_corners: CHARUCO_CORNER_DTYPE records of the last collected batch, ordered by (frame, id)"""
        L = load()
        n = C.c_size_t(0)
        rc = L.a3_get_charuco_corners(self.handle, None, 0, C.byref(n))
        if rc not in (0, ERR_CAPACITY):
            check(rc, self.handle)
        out = np.zeros(max(n.value, 1), dtype=CHARUCO_CORNER_DTYPE)
        check(L.a3_get_charuco_corners(self.handle, out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)), self.handle)
        return out[:n.value]

    def charuco_poses(self) -> np.ndarray:
        """a3_get_charuco_poses: CHARUCO_POSE_DTYPE records of the last collected pose batch, one per frame"""
        L = load()
        n = C.c_size_t(0)
        rc = L.a3_get_charuco_poses(self.handle, None, 0, C.byref(n))
        if rc not in (0, ERR_CAPACITY):
            check(rc, self.handle)
        out = np.zeros(max(n.value, 1), dtype=CHARUCO_POSE_DTYPE)
        check(L.a3_get_charuco_poses(self.handle, out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)), self.handle)
        return out[:n.value]

    def interpolate_charuco(self, pixels_ptr: int, memory: int, fmt: int, width: int, height: int, row_stride: int, ids, corners) -> np.ndarray:
        """a3_interpolate_charuco (stand-alone, one frame): marker ids (n,) and raw pixel corners (n, 4, 2) -> CHARUCO_CORNER_DTYPE records"""
        L = load()
        i = np.ascontiguousarray(np.asarray(ids, dtype=np.uint32).reshape(-1))
        c = _f32(corners, 8)
        if c.shape[0] != i.size:
            raise ValueError("interpolate_charuco needs four corners per id")
        n = C.c_size_t(0)
        args = (self.handle, C.c_void_p(pixels_ptr), memory, fmt, width, height, row_stride, _p(i, C.c_uint32), _p(c, C.c_float), i.size)
        rc = L.a3_interpolate_charuco(*args, None, 0, C.byref(n))
        if rc not in (0, ERR_CAPACITY):
            check(rc, self.handle)
        out = np.zeros(max(n.value, 1), dtype=CHARUCO_CORNER_DTYPE)
        check(L.a3_interpolate_charuco(*args, out.ctypes.data_as(C.c_void_p), out.size, C.byref(n)), self.handle)
        return out[:n.value]

    def set_distortion(self, d: "DistortionRec" = None):
        """a3_set_distortion: None (or model DIST_NONE) clears it; applies to pose batches submitted afterwards"""
        check(load().a3_set_distortion(self.handle, C.byref(d) if d is not None else None), self.handle)

    def undistorted_corners(self):
        """a3_get_undistorted_corners: (float32 [n_markers, 4, 2] corners, float32 [n_markers, 4] residuals in px) of the last
        collected batch, in marker order"""
        n = C.c_size_t()
        L = load()
        rc = L.a3_get_undistorted_corners(self.handle, None, None, 0, C.byref(n))
        if rc not in (OK, ERR_CAPACITY):
            check(rc, self.handle)
        out = np.zeros((max(n.value, 1), 4, 2), dtype=np.float32)
        res = np.zeros((max(n.value, 1), 4), dtype=np.float32)
        check(L.a3_get_undistorted_corners(self.handle, _p(out, C.c_float), _p(res, C.c_float), max(n.value, 1), C.byref(n)), self.handle)
        return out[: n.value], res[: n.value]

    def undistort_points(self, points: np.ndarray, intrinsics: "Intrinsics", d: "DistortionRec"):
        """a3_undistort_points (stand-alone): points (..., 2) pixels -> (float32 (n, 2) undistorted pixels, float32 (n,) residuals)"""
        xy = _f32(points, 2)
        out = np.zeros_like(xy)
        res = np.zeros(xy.shape[0], dtype=np.float32)
        check(load().a3_undistort_points(self.handle, _p(xy, C.c_float), xy.shape[0], C.byref(intrinsics), C.byref(d), _p(out, C.c_float),
                                         _p(res, C.c_float)), self.handle)
        return out, res

    # ---- frame rectification ----
    def set_rectification(self, r: "RectifyRec" = None):
        """a3_set_rectification: every later detect call of this context sees its frames through r (they have r.src's size, the results
        are pixels of r.dst's view); None turns it off.  Refused while a submitted batch is in flight."""
        check(load().a3_set_rectification(self.handle, C.byref(r) if r is not None else None), self.handle)

    def rectification(self):
        """a3_get_rectification -> the RectifyRec in force, or None"""
        r, on = RectifyRec(), C.c_int(0)
        check(load().a3_get_rectification(self.handle, C.byref(r), C.byref(on)), self.handle)
        return r if on.value else None

    def rectify_frames(self, src_ptr: int, src_memory: int, fmt: int, src_row_stride: int, src_frame_stride: int, n_frames: int,
                       r: "RectifyRec", dst_ptr: int, dst_memory: int, dst_row_stride: int, dst_frame_stride: int) -> "RectifyInfo":
        """a3_rectify_frames: n_frames frames at src_ptr (r.src's size) -> rectified frames at dst_ptr (r.dst's size, same format; for
        FMT_YUYV8 / FMT_UYVY8 the rectified luma view, one byte per pixel); synchronous -> the launch's a3_rectify_info"""
        info = RectifyInfo()
        check(load().a3_rectify_frames(self.handle, C.c_void_p(src_ptr), src_memory, fmt, src_row_stride, src_frame_stride, n_frames,
                                       C.byref(r), C.c_void_p(dst_ptr), dst_memory, dst_row_stride, dst_frame_stride, C.byref(info)),
              self.handle)
        return info

    # ---- detection on reduced frames ----
    def set_reduction(self, r: "ReductionRec" = None):
        """a3_set_reduction: every later detect call of this context detects on its frames reduced by r.factor and returns full-size
        corners; None turns it off.  Refused while a submitted batch is in flight, and on a context with a rectification."""
        check(load().a3_set_reduction(self.handle, C.byref(r) if r is not None else None), self.handle)

    def reduction(self):
        """a3_get_reduction -> the ReductionRec in force, or None"""
        r, on = ReductionRec(), C.c_int(0)
        check(load().a3_get_reduction(self.handle, C.byref(r), C.byref(on)), self.handle)
        return r if on.value else None

    def reduce_frames(self, src_ptr: int, src_memory: int, fmt: int, width: int, height: int, src_row_stride: int, src_frame_stride: int,
                      n_frames: int, factor: int, dst_ptr: int, dst_memory: int, dst_row_stride: int, dst_frame_stride: int) -> None:
        """a3_reduce_frames: n_frames frames of width x height at src_ptr -> grey planes of (width // factor) x (height // factor) bytes at
        dst_ptr; synchronous"""
        check(load().a3_reduce_frames(self.handle, C.c_void_p(src_ptr), src_memory, fmt, width, height, src_row_stride, src_frame_stride, n_frames,
                                      factor, C.c_void_p(dst_ptr), dst_memory, dst_row_stride, dst_frame_stride), self.handle)

    # ---- several threshold windows ----
    def set_threshold_windows(self, radii=None):
        """a3_set_threshold_windows: every later detect call of this context thresholds at each radius and merges the candidates on the
        device (one radius: the single-window path with that radius); None or an empty sequence turns it off.  Refused while a
        submitted batch is in flight."""
        r = [int(v) for v in radii] if radii is not None else []
        if any(v < 0 or v > 0xFFFFFFFF for v in r):
            raise ValueError("a threshold window radius is a uint32")
        arr = (C.c_uint32 * max(len(r), 1))(*r)
        check(load().a3_set_threshold_windows(self.handle, arr if r else None, len(r)), self.handle)

    def set_marker_polarity(self, mode: int):
        """a3_set_marker_polarity: POLARITY_DARK (the reference) or POLARITY_BOTH (bright-on-dark markers are read too); applies to
        batches submitted afterwards"""
        check(load().a3_set_marker_polarity(self.handle, int(mode)), self.handle)

    def get_marker_polarity(self) -> int:
        """a3_get_marker_polarity -> the mode in force"""
        mode = C.c_int(0)
        check(load().a3_get_marker_polarity(self.handle, C.byref(mode)), self.handle)
        return int(mode.value)

    def marker_flags(self) -> np.ndarray:
        """a3_get_marker_flags: uint32 [n_markers] of the last collected batch, in marker order (MARKER_INVERTED: read inverted);
        refused when that batch ran in mode POLARITY_DARK"""
        n = C.c_size_t()
        L = load()
        rc = L.a3_get_marker_flags(self.handle, None, 0, C.byref(n))
        if rc not in (OK, ERR_CAPACITY):
            check(rc, self.handle)
        out = np.zeros(max(n.value, 1), dtype=np.uint32)
        check(L.a3_get_marker_flags(self.handle, _p(out, C.c_uint32), max(n.value, 1), C.byref(n)), self.handle)
        return out[: n.value]

    def get_threshold_windows(self):
        """a3_get_threshold_windows -> the radii in force as a tuple (empty: off)"""
        arr, n = (C.c_uint32 * MAX_THRESHOLD_WINDOWS)(), C.c_size_t(0)
        check(load().a3_get_threshold_windows(self.handle, arr, MAX_THRESHOLD_WINDOWS, C.byref(n)), self.handle)
        return tuple(int(arr[i]) for i in range(n.value))

    # ---- camera calibration ----
    def _calibrate(self, symbol, cams, view_offsets, object_xy, image_xy, with_views):
        off = np.ascontiguousarray(np.asarray(view_offsets, dtype=np.uint32).reshape(-1))
        obj, img = _f32(object_xy, 2), _f32(image_xy, 2)
        n_views = max(off.size - 1, 0)
        res = (CalibResult * max(len(cams), 1))()
        views = (CalibView * max(n_views, 1))() if with_views else None
        check(getattr(load(), symbol)(self.handle, cams, len(cams), _p(off, C.c_uint32), n_views, _p(obj, C.c_float), _p(img, C.c_float), res,
                                      views), self.handle)
        return res, views

    def calibrate_cameras(self, cams, view_offsets, object_xy, image_xy, with_views: bool = True):
        """a3_calibrate_cameras: cams (a CalibCamera array), view_offsets (n_views + 1), object / image points (n, 2) ->
        (CalibResult array, CalibView array or None)"""
        return self._calibrate("a3_calibrate_cameras", cams, view_offsets, object_xy, image_xy, with_views)

    def calibrate_fisheye_cameras(self, cams, view_offsets, object_xy, image_xy, with_views: bool = True):
        """a3_calibrate_fisheye_cameras: the arguments of calibrate_cameras, the cameras' flags read as FISHEYE_* ->
        (CalibResult array, CalibView array or None)"""
        return self._calibrate("a3_calibrate_fisheye_cameras", cams, view_offsets, object_xy, image_xy, with_views)

    # ---- camera rig calibration ----
    def calibrate_rigs(self, rigs, cameras, obs, object_xy, image_xy):
        """a3_calibrate_rigs: rigs (a Rig array), cameras (RigCamera array), obs (RigObservation array), object / image points (n, 2) ->
        (RigResult array, RigCameraResult array, RigFrame array, RigObservationResult array)"""
        obj, img = _f32(object_xy, 2), _f32(image_xy, 2)
        n_frames = max([int(r.first_frame) + int(r.n_frames) for r in rigs], default=0)
        res = (RigResult * max(len(rigs), 1))()
        cres = (RigCameraResult * max(len(cameras), 1))()
        frames = (RigFrame * max(n_frames, 1))()
        ores = (RigObservationResult * max(len(obs), 1))()
        check(load().a3_calibrate_rigs(self.handle, rigs, len(rigs), cameras, len(cameras), obs, len(obs), _p(obj, C.c_float), _p(img, C.c_float),
                                       res, cres, frames, ores), self.handle)
        return res, cres, frames, ores

    # ---- hand-eye calibration ----
    def calibrate_hand_eyes(self, problems, frames, object_xy, image_xy):
        """a3_calibrate_hand_eyes: problems (a HandEyeProblem array), frames (HandEyeFrame array), object / image points (n, 2) ->
        (HandEyeResult array, HandEyeFrameResult array)"""
        obj, img = _f32(object_xy, 2), _f32(image_xy, 2)
        res = (HandEyeResult * max(len(problems), 1))()
        fres = (HandEyeFrameResult * max(len(frames), 1))()
        check(_symbol("a3_calibrate_hand_eyes")(self.handle, problems, len(problems), frames, len(frames), _p(obj, C.c_float), _p(img, C.c_float),
                                                res, fres), self.handle)
        return res, fres

    # ---- marker maps ----
    def build_marker_maps(self, maps, markers, obs, image_xy):
        """a3_build_marker_maps: maps (a Map array), markers (MapMarker array), obs (MapObservation array), image corners (n_obs, 8) ->
        (MapResult array, MapMarkerResult array, MapFrame array, MapObservationResult array)"""
        img = _f32(image_xy, 8)
        n_frames = max([int(r.first_frame) + int(r.n_frames) for r in maps], default=0)
        res = (MapResult * max(len(maps), 1))()
        mres = (MapMarkerResult * max(len(markers), 1))()
        frames = (MapFrame * max(n_frames, 1))()
        ores = (MapObservationResult * max(len(obs), 1))()
        check(_symbol("a3_build_marker_maps")(self.handle, maps, len(maps), markers, len(markers), obs, len(obs), _p(img, C.c_float), res, mres,
                                              frames, ores), self.handle)
        return res, mres, frames, ores

    # ---- Detection.grey / thresholded / candidates / homographies of the last batch ----
    def download_grey(self, frame: int, w: int, h: int, thresholded: bool = False) -> np.ndarray:
        out = np.empty((h, w), dtype=np.uint8)
        fn = load().a3_download_thresholded if thresholded else load().a3_download_grey
        check(fn(self.handle, frame, _p(out, C.c_uint8)), self.handle)
        return out

    def candidates(self, frame: int, before_discard: bool = False) -> np.ndarray:
        a, b = C.c_uint32(), C.c_uint32()
        check(load().a3_candidate_count(self.handle, frame, C.byref(a), C.byref(b)), self.handle)
        cnt = a.value if before_discard else b.value
        out = np.zeros((max(cnt, 1), 4, 2), dtype=np.uint32)
        check(load().a3_download_candidates(self.handle, frame, int(before_discard), _p(out, C.c_uint32), max(cnt, 1)), self.handle)
        return out[:cnt]

    def homographies(self, frame: int, with_patches: bool = True):
        a, b = C.c_uint32(), C.c_uint32()
        check(load().a3_candidate_count(self.handle, frame, C.byref(a), C.byref(b)), self.handle)
        cnt, S = b.value, self.sample
        patches = np.zeros((max(cnt, 1), S, S), dtype=np.uint8)
        ok = np.zeros(max(cnt, 1), dtype=np.uint8)
        codes = np.zeros((max(cnt, 1), 4), dtype=np.uint64)
        dec = np.zeros(max(cnt, 1), dtype=np.int32)
        check(load().a3_download_homographies(self.handle, frame, _p(patches, C.c_uint8) if with_patches else None, _p(ok, C.c_uint8),
                                              _p(codes, C.c_uint64), _p(dec, C.c_int32), max(cnt, 1)), self.handle)
        return patches[:cnt], ok[:cnt], codes[:cnt], dec[:cnt]

    def contours(self, frame: int):
        """find_contours of one frame of the last batch (debug taps on): -> (start_keys u32[n], list of int32 [len, 2] point arrays)
        in the reference's discovery order."""
        nc, npts = C.c_uint32(), C.c_uint64()
        check(load().a3_contour_count(self.handle, frame, C.byref(nc), C.byref(npts)), self.handle)
        keys = np.zeros(max(nc.value, 1), dtype=np.uint32)
        lens = np.zeros(max(nc.value, 1), dtype=np.uint32)
        pts = np.zeros((max(npts.value, 1), 2), dtype=np.uint32)
        check(load().a3_download_contours(self.handle, frame, _p(keys, C.c_uint32), _p(lens, C.c_uint32), _p(pts, C.c_uint32),
                                          max(nc.value, 1), max(npts.value, 1)), self.handle)
        keys, lens = keys[: nc.value], lens[: nc.value]
        offs = np.concatenate([[0], np.cumsum(lens, dtype=np.int64)])
        return keys, [pts[offs[i]: offs[i + 1]].astype(np.int64) for i in range(nc.value)]

    def pack_detections(self, first_frame_global: int, max_markers: int, dst_ptr: int, dst_bytes: int, with_poses: bool = False):
        """a3_pack_detections: the last batch's markers (and, after detect_batch_pose, their poses) as fixed-capacity per-frame
        records in device memory at dst_ptr (enqueued on the context's stream)."""
        check(load().a3_pack_detections(self.handle, first_frame_global, max_markers, int(with_poses), C.c_void_p(dst_ptr), dst_bytes), self.handle)

    # ---- a3_internal.h: the reference's small helpers on the device, for its own vectors ----
    def debug_clockwise(self, quads: np.ndarray) -> np.ndarray:
        q = np.ascontiguousarray(quads, dtype=np.int32).reshape(-1, 8)
        out = np.zeros_like(q)
        check(load().a3_debug_clockwise(self.handle, _p(q, C.c_int32), q.shape[0], _p(out, C.c_int32)), self.handle)
        return out.reshape(-1, 4, 2)

    def debug_rotate_bits(self, bits: np.ndarray, times: int = 1) -> np.ndarray:
        b = np.ascontiguousarray(bits, dtype=np.uint8)
        n = b.shape[0]
        assert b.shape == (n, n)
        out = np.zeros_like(b)
        check(load().a3_debug_rotate_bits(self.handle, _p(b, C.c_uint8), n, times, _p(out, C.c_uint8)), self.handle)
        return out

    def debug_inject_candidates(self, quads: np.ndarray):
        """the next one-frame batch decodes THESE quads (n x 4 x 2, in this order) instead of what its contour stage finds"""
        q = np.ascontiguousarray(quads, dtype=np.uint32).reshape(-1, 8)
        check(load().a3_debug_inject_candidates(self.handle, _p(q, C.c_uint32), q.shape[0]), self)

    def debug_sample_frames(self, on: bool):
        """while set, a batch with debug taps on keeps sampling the caller's frames (as one without taps does) and not the grey plane"""
        check(load().a3_debug_sample_frames(self.handle, int(on)), self.handle)

    def debug_discard_too_near(self, quads: np.ndarray, min_distance: float) -> np.ndarray:
        q = np.ascontiguousarray(quads, dtype=np.uint32).reshape(-1, 8)
        out = np.zeros_like(q)
        n = C.c_size_t()
        check(load().a3_debug_discard_too_near(self.handle, _p(q, C.c_uint32), q.shape[0], min_distance, _p(out, C.c_uint32), C.byref(n)),
              self.handle)
        return out[: n.value].reshape(-1, 4, 2)

    def debug_frame_candidates(self, cand_count, records: np.ndarray, max_cand: int, min_distance: float, S: int = 0) -> dict:
        """a3_debug_frame_candidates: one launch of k_frame_candidates, as the pipeline makes it, on hand-made candidate tables.
        cand_count: per frame (may exceed max_cand); records: CAND_DTYPE, frame after frame, min(count, max_cand) each, in table order.
        Returns whole tables -- what the kernel did not write is 0xFF bytes: pre_xy, fin_xy (frames x max_cand x 8 u16), fin_count,
        work (frames * max_cand u32), work_count, and with S != 0 proj (PROJ_DTYPE, frames * max_cand, indexed like work)."""
        cnt = np.ascontiguousarray(cand_count, dtype=np.uint32).reshape(-1)
        rec = np.ascontiguousarray(records, dtype=CAND_DTYPE).reshape(-1)
        n = cnt.shape[0]
        if max_cand >= 1 and rec.shape[0] != int(np.minimum(cnt, max_cand).sum()):
            raise ValueError("records must hold min(cand_count, max_cand) entries per frame")
        slots = n * max_cand if 1 <= max_cand <= 65536 else 0      # (out of range: the library refuses before it writes)
        pre = np.empty((n, slots // max(n, 1), 8), dtype=np.uint16)
        fin = np.empty_like(pre)
        fin_count = np.empty(n, dtype=np.uint32)
        work = np.empty(slots, dtype=np.uint32)
        work_count = np.zeros(1, dtype=np.uint32)
        proj = np.empty(slots if S else 0, dtype=PROJ_DTYPE)
        check(load().a3_debug_frame_candidates(self.handle, n, max_cand, _p(cnt, C.c_uint32), rec.ctypes.data if rec.size else None, min_distance, S,
                                               _p(pre, C.c_uint16), _p(fin, C.c_uint16), _p(fin_count, C.c_uint32), _p(work, C.c_uint32),
                                               _p(work_count, C.c_uint32), proj.ctypes.data if S else None), self.handle)
        return {"pre_xy": pre, "fin_xy": fin, "fin_count": fin_count, "work": work, "work_count": int(work_count[0]), "proj": proj if S else None}

    def debug_merge_candidates(self, n_frames: int, n_windows: int, plane_cand: int, cand_count, records, min_distance: float, S: int = 0) -> dict:
        """a3_debug_merge_candidates: one launch of k_merge_candidates, as the pipeline makes it, on hand-made per-plane tables.
        cand_count: n_windows * n_frames counts at plane index k * n_frames + f; records: CAND_DTYPE, plane after plane in that order.
        Returns whole tables of M = min(n_windows * plane_cand, 65536) slots per frame -- 0xFF bytes where the kernel did not write."""
        cnt = np.ascontiguousarray(cand_count, dtype=np.uint32).reshape(-1)
        rec = np.ascontiguousarray(records, dtype=CAND_DTYPE).reshape(-1)
        assert cnt.size == n_frames * n_windows
        m = min(n_windows * plane_cand, 65536)
        slots = n_frames * m
        pre = np.empty((n_frames, m, 4, 2), dtype=np.uint16)
        fin = np.empty((n_frames, m, 4, 2), dtype=np.uint16)
        fin_count = np.empty(n_frames, dtype=np.uint32)
        merged = np.empty(n_frames, dtype=np.uint32)
        work = np.empty(slots, dtype=np.uint32)
        work_count = np.zeros(1, dtype=np.uint32)
        err = np.zeros(1, dtype=np.uint32)
        proj = np.empty(slots if S else 0, dtype=PROJ_DTYPE)
        check(load().a3_debug_merge_candidates(self.handle, n_frames, n_windows, plane_cand, _p(cnt, C.c_uint32), rec.ctypes.data if rec.size else None,
                                               min_distance, S, _p(pre, C.c_uint16), _p(fin, C.c_uint16), _p(fin_count, C.c_uint32),
                                               _p(work, C.c_uint32), _p(work_count, C.c_uint32), proj.ctypes.data if S else None,
                                               _p(merged, C.c_uint32), _p(err, C.c_uint32)), self.handle)
        return {"pre_xy": pre, "fin_xy": fin, "fin_count": fin_count, "merged_count": merged, "work": work, "work_count": int(work_count[0]),
                "err_flags": int(err[0]), "proj": proj if S else None, "merged_cap": m}

    def debug_contour_quads(self, width: int, height: int, records: np.ndarray, points: np.ndarray, *, eps_factor: float = 0.05,
                            min_edge_length: int = 0, n_darts: int = 0, first_frame: int = 0, n_frames: int = 1, max_cand: int = 1024,
                            max_contours: int = None, ctr_contours: int = None, ctr_err_flags: int = 0) -> dict:
        """a3_debug_contour_quads: one launch of k_contour_quads, as the pipeline makes it, on a hand-made contour table.
        records: CONTOUR_DTYPE in table order; points: the pool, x | y << 16; max_contours and ctr_contours default to the record count.
        Returns whole tables -- what the kernel did not write is 0xFF bytes: cand_count (first_frame + n_frames u32), cands (CAND_DTYPE,
        first_frame + n_frames x max_cand) and the kernel's err_flags word."""
        rec = np.ascontiguousarray(records, dtype=CONTOUR_DTYPE).reshape(-1)
        pts = np.ascontiguousarray(points, dtype=np.uint32).reshape(-1)
        frames = first_frame + n_frames
        ok = 1 <= max_cand <= 65536 and 1 <= n_frames <= 65536 and 0 <= first_frame <= 65536 and frames * max_cand <= 1 << 24
        cnt = np.empty(frames if ok else 1, dtype=np.uint32)      # (out of range: the library refuses before it writes)
        cands = np.empty((frames, max_cand) if ok else (1, 1), dtype=CAND_DTYPE)
        err = np.zeros(1, dtype=np.uint32)
        check(load().a3_debug_contour_quads(self.handle, width, height, n_darts, eps_factor, min_edge_length, first_frame, n_frames, max_cand,
                                            len(rec) if max_contours is None else max_contours, len(rec) if ctr_contours is None else ctr_contours,
                                            ctr_err_flags, rec.ctypes.data if rec.size else None, len(rec), pts.ctypes.data if pts.size else None,
                                            pts.size, _p(cnt, C.c_uint32), cands.ctypes.data, _p(err, C.c_uint32)), self.handle)
        return {"cand_count": cnt, "cands": cands, "err_flags": int(err[0])}

    # ---- pose ----
    def estimate_pose(self, corners: np.ndarray, marker_size_mm: float, image_size=None, intrinsics: Intrinsics = None) -> np.ndarray:
        c = np.ascontiguousarray(corners, dtype=np.uint32).reshape(-1, 8)
        out = (PoseRec * (2 * max(c.shape[0], 1)))()
        iw, ih = image_size if image_size else (1, 1)
        check(load().a3_estimate_pose(self.handle, _p(c, C.c_uint32), c.shape[0], marker_size_mm, C.byref(intrinsics) if intrinsics else None,
                                      iw, ih, out), self.handle)
        return out

    def estimate_pose_normalized(self, points: np.ndarray, marker_size_mm: float):
        p = np.ascontiguousarray(points, dtype=np.float32).reshape(-1, 8)
        out = (PoseRec * (2 * max(p.shape[0], 1)))()
        check(load().a3_estimate_pose_normalized(self.handle, _p(p, C.c_float), p.shape[0], marker_size_mm, out), self.handle)
        return out

    def find_nearest(self, bits: np.ndarray):
        b = np.ascontiguousarray(bits, dtype=np.uint64)
        idx = np.zeros(max(b.size, 1), dtype=np.uint32)
        dist = np.zeros(max(b.size, 1), dtype=np.uint8)
        check(load().a3_find_nearest(self.handle, _p(b, C.c_uint64), b.size, _p(idx, C.c_uint32), _p(dist, C.c_uint8)), self.handle)
        return idx[: b.size], dist[: b.size]

    def selftest_ieee(self, a: np.ndarray, b: np.ndarray):
        a = np.ascontiguousarray(a, dtype=np.float64)
        b = np.ascontiguousarray(b, dtype=np.float64)
        n = a.size
        sq, dv = np.zeros(n), np.zeros(n)
        sqf, dvf = np.zeros(n, dtype=np.float32), np.zeros(n, dtype=np.float32)
        check(load().a3_selftest_ieee(self.handle, _p(a, C.c_double), _p(b, C.c_double), n, _p(sq, C.c_double), _p(dv, C.c_double),
                                      _p(sqf, C.c_float), _p(dvf, C.c_float)), self.handle)
        return sq, dv, sqf, dvf


# ---- dictionary helpers used by ARDictionary (device kernels; no host arithmetic) ----
_dict_ctx = {}


def _ctx_for(codes: np.ndarray) -> Context:
    # keyed by the table's contents: an address can be re-used by another array once the first one is freed
    codes = np.ascontiguousarray(codes, dtype=np.uint64)
    key = codes.tobytes()
    ctx = _dict_ctx.get(key)
    if ctx is None:
        ctx = Context(default_config(), codes, 64, 1)
        _dict_ctx[key] = ctx
    return ctx


def find_nearest(codes: np.ndarray, bits: np.ndarray):
    return _ctx_for(codes).find_nearest(bits)


def calculate_tau(codes: np.ndarray) -> int:
    codes = np.ascontiguousarray(codes, dtype=np.uint64)
    t = C.c_uint8()
    check(load().a3_calculate_tau(0, _p(codes, C.c_uint64), codes.size, C.byref(t)), None)
    return int(t.value)
