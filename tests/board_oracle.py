"""ctypes binding of tests/board_oracle.c: the CPU restatement of the board pose (a3_set_board, include/aruco3_hip.h) that the device
kernel k_board_pose is held to.  TEST INFRASTRUCTURE ONLY -- the tests and tools/board_bench.py load it; aruco3_amd never does.

The library is compiled on first use into a temporary directory of its own (gcc / cc, -ffp-contract=off as the kernels), so the
repository tree is not written to."""
import ctypes as C

import numpy as np

from tests.oracle_build import build

_lib = None

REC_DTYPE = np.dtype([("status", "<u4"), ("markers_used", "<u4"), ("markers_rejected", "<u4"), ("iterations", "<u4"),
                      ("rms_px", "<f4"), ("alt_rms_px", "<f4"), ("rotation", "<f4", (9,)), ("translation", "<f4", (3,))])
CHECK_ERRORS = {0: None, 1: "no size", 2: "sides differ", 3: "not right angles", 4: "wound the wrong way", 5: "not finite"}


def lib():
    global _lib
    if _lib is None:
        L = build("board_oracle")
        u32p, f32p, vp = C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_void_p
        L.a3o_check_marker.restype = C.c_int
        L.a3o_check_marker.argtypes = [f32p]
        L.a3o_ippe.restype = None
        L.a3o_ippe.argtypes = [f32p, C.c_float, vp]
        L.a3o_cayley.restype = None
        L.a3o_cayley.argtypes = [f32p, f32p, f32p]
        L.a3o_board_pose.restype = C.c_int
        L.a3o_board_pose.argtypes = [u32p, f32p, C.c_uint32, u32p, f32p, C.c_uint32, f32p, C.c_uint32, C.c_uint32, vp, f32p]
        L.a3o_refine_from.restype = C.c_uint32
        L.a3o_refine_from.argtypes = [u32p, f32p, C.c_uint32, u32p, f32p, C.c_uint32, f32p, C.c_uint32, C.c_uint32, f32p, f32p, f32p]
        _lib = L
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _f32(a, shape):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(shape))


def _intr(intr):
    """(fx, fy, cx, cy), an aruco3_amd._lib.Intrinsics, or None"""
    if intr is None:
        return None
    if hasattr(intr, "focal_x"):
        intr = (intr.focal_x, intr.focal_y, intr.principal_x, intr.principal_y)
    return _f32(intr, 4)


def check_marker(corners):
    """None for a valid board marker, else the reason a3_set_board refuses it"""
    return CHECK_ERRORS[int(lib().a3o_check_marker(_p(_f32(corners, 8), C.c_float)))]


def ippe(pts_norm, side: float):
    """both IPPE poses (a3_estimate_pose_normalized) -> float32 (2, 13): error, rotation, translation"""
    out = np.zeros((2, 13), np.float32)
    lib().a3o_ippe(_p(_f32(pts_norm, 8), C.c_float), side, out.ctypes.data_as(C.c_void_p))
    return out


def cayley(w, R):
    out = np.zeros(9, np.float32)
    lib().a3o_cayley(_p(_f32(w, 3), C.c_float), _p(_f32(R, 9), C.c_float), _p(out, C.c_float))
    return out.reshape(3, 3)


def board_pose(board, ids, corners_px, image_size=None, intrinsics=None, with_starts=False):
    """the contract's board pose of one frame: ids (n,) and pixel corners (n, 4, 2) in batch order -> a REC_DTYPE record
    (and the two starts, float32 (2, 12): R row-major, t, when with_starts)"""
    bi = np.ascontiguousarray(board.ids, dtype=np.uint32)
    bx = _f32(board.corners, (-1, 8))
    i = np.ascontiguousarray(np.asarray(ids, dtype=np.uint32).reshape(-1))
    px = _f32(corners_px, (-1, 8)) if i.size else np.zeros((1, 8), np.float32)
    w, h = image_size if image_size else (0, 0)
    rec = np.zeros(1, REC_DTYPE)
    starts = np.zeros((2, 12), np.float32)
    ci = _intr(intrinsics)
    rc = lib().a3o_board_pose(_p(bi, C.c_uint32), _p(bx, C.c_float), bi.size, _p(i, C.c_uint32), _p(px, C.c_float), i.size,
                              None if ci is None else _p(ci, C.c_float), w, h, rec.ctypes.data_as(C.c_void_p), _p(starts, C.c_float))
    assert rc == 0
    return (rec[0], starts) if with_starts else rec[0]


def refine_from(board, ids, corners_px, R, t, image_size=None, intrinsics=None):
    """the contract's LM from a given start -> (R, t, evaluations, cost, pixel cost)"""
    bi = np.ascontiguousarray(board.ids, dtype=np.uint32)
    bx = _f32(board.corners, (-1, 8))
    i = np.ascontiguousarray(np.asarray(ids, dtype=np.uint32).reshape(-1))
    px = _f32(corners_px, (-1, 8))
    R = _f32(R, 9).copy()
    t = _f32(t, 3).copy()
    cp = np.zeros(2, np.float32)
    w, h = image_size if image_size else (0, 0)
    ci = _intr(intrinsics)
    ev = lib().a3o_refine_from(_p(bi, C.c_uint32), _p(bx, C.c_float), bi.size, _p(i, C.c_uint32), _p(px, C.c_float), i.size,
                               None if ci is None else _p(ci, C.c_float), w, h, _p(R, C.c_float), _p(t, C.c_float), _p(cp, C.c_float))
    return R.reshape(3, 3), t, int(ev), float(cp[0]), float(cp[1])
