"""ctypes binding of tests/board3d_oracle.c: the CPU restatement of the 3-D board pose (a3_set_board3d, include/aruco3_hip.h) that the
device kernel k_board3d_pose is held to.  TEST INFRASTRUCTURE ONLY -- the tests and tools/board3d_bench.py load it; aruco3_amd never
does.  Compiled together with tests/board_oracle.c, whose IPPE, LM loop and butterfly it links instead of copying."""
import ctypes as C

import numpy as np

from tests.board_oracle import REC_DTYPE, _f32, _intr, _p
from tests.oracle_build import HERE, build

_lib = None

SLOT_DTYPE = np.dtype([("x", "<f4", (4,)), ("y", "<f4", (4,)), ("z", "<f4", (4,)), ("side", "<f4"), ("ex", "<f4", (3,)), ("ey", "<f4", (3,)),
                       ("ez", "<f4", (3,)), ("c", "<f4", (3,))])


def lib():
    global _lib
    if _lib is None:
        L = build("board3d_oracle", [HERE / "board3d_oracle.c", HERE / "board_oracle.c"])
        u32p, f32p, vp = C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_void_p
        L.a3o_board3d_slot.restype = None
        L.a3o_board3d_slot.argtypes = [f32p, vp]
        L.a3o_board3d_pose.restype = C.c_int
        L.a3o_board3d_pose.argtypes = [u32p, f32p, C.c_uint32, u32p, f32p, C.c_uint32, f32p, C.c_uint32, C.c_uint32, vp, f32p]
        L.a3o_board3d_refine_from.restype = C.c_uint32
        L.a3o_board3d_refine_from.argtypes = [u32p, f32p, C.c_uint32, u32p, f32p, C.c_uint32, f32p, C.c_uint32, C.c_uint32, f32p, f32p, f32p]
        L.a3o_board3d_cost_at.restype = None
        L.a3o_board3d_cost_at.argtypes = [u32p, f32p, C.c_uint32, u32p, f32p, C.c_uint32, f32p, C.c_uint32, C.c_uint32, f32p, f32p, f32p]
        _lib = L
    return _lib


def slot(corners_xyz):
    """the contract's slot record of one marker's (4, 3) corners -> a SLOT_DTYPE record"""
    out = np.zeros(1, SLOT_DTYPE)
    lib().a3o_board3d_slot(_p(_f32(corners_xyz, 12), C.c_float), out.ctypes.data_as(C.c_void_p))
    return out[0]


def _frame(board, ids, corners_px, image_size, intrinsics):
    bi = np.ascontiguousarray(board.ids, dtype=np.uint32)
    bx = _f32(board.corners, (-1, 12))
    i = np.ascontiguousarray(np.asarray(ids, dtype=np.uint32).reshape(-1))
    px = _f32(corners_px, (-1, 8)) if i.size else np.zeros((1, 8), np.float32)
    w, h = image_size if image_size else (0, 0)
    ci = _intr(intrinsics)
    keep = (bi, bx, i, px, ci)
    return keep, (_p(bi, C.c_uint32), _p(bx, C.c_float), bi.size, _p(i, C.c_uint32), _p(px, C.c_float), i.size,
                  None if ci is None else _p(ci, C.c_float), w, h)


def board_pose(board, ids, corners_px, image_size=None, intrinsics=None, with_starts=False):
    """the contract's pose of a Board3D in one frame: ids (n,) and pixel corners (n, 4, 2) in batch order -> a REC_DTYPE record (and
    the two starts, float32 (2, 12): R row-major, t, when with_starts)"""
    keep, args = _frame(board, ids, corners_px, image_size, intrinsics)
    rec = np.zeros(1, REC_DTYPE)
    starts = np.zeros((2, 12), np.float32)
    rc = lib().a3o_board3d_pose(*args, rec.ctypes.data_as(C.c_void_p), _p(starts, C.c_float))
    assert rc == 0
    return (rec[0], starts) if with_starts else rec[0]


def refine_from(board, ids, corners_px, R, t, image_size=None, intrinsics=None):
    """the contract's LM from a given start -> (R, t, evaluations, cost, pixel cost)"""
    keep, args = _frame(board, ids, corners_px, image_size, intrinsics)
    R = _f32(R, 9).copy()
    t = _f32(t, 3).copy()
    cp = np.zeros(2, np.float32)
    ev = lib().a3o_board3d_refine_from(*args, _p(R, C.c_float), _p(t, C.c_float), _p(cp, C.c_float))
    return R.reshape(3, 3), t, int(ev), float(cp[0]), float(cp[1])


def cost_at(board, ids, corners_px, R, t, image_size=None, intrinsics=None):
    """the sums' cost and pixel cost at (R, t), no LM step"""
    keep, args = _frame(board, ids, corners_px, image_size, intrinsics)
    cp = np.zeros(2, np.float32)
    lib().a3o_board3d_cost_at(*args, _p(_f32(R, 9), C.c_float), _p(_f32(t, 3), C.c_float), _p(cp, C.c_float))
    return float(cp[0]), float(cp[1])
