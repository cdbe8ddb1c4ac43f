"""ctypes binding of tests/charuco_oracle.c: the CPU restatement of the ChArUco corners and pose (a3_set_charuco, include/aruco3_hip.h)
that the device kernels of k_charuco.hip are held to.  TEST INFRASTRUCTURE ONLY -- the tests and tools/charuco_bench.py load it;
aruco3_amd never does.

Compiled on first use into a temporary directory of its own, with board_oracle.c, refine_oracle.c, lens_oracle.c and oracle/a3_oracle.c (gcc / cc,
-ffp-contract=off as the kernels), so the repository tree is not written to."""
import ctypes as C
from pathlib import Path

import numpy as np

from tests.oracle_build import build

_HERE = Path(__file__).resolve().parent
_lib = None

CORNER_DTYPE = np.dtype([("frame", "<u4"), ("id", "<u4"), ("x", "<f4"), ("y", "<f4"), ("interp_x", "<f4"), ("interp_y", "<f4"),
                         ("markers_used", "<u4"), ("window", "<u4")])
POSE_DTYPE = np.dtype([("status", "<u4"), ("corners_used", "<u4"), ("iterations", "<u4"), ("reserved", "<u4"), ("rms_px", "<f4"),
                       ("alt_rms_px", "<f4"), ("rotation", "<f4", (9,)), ("translation", "<f4", (3,))])


class Config(C.Structure):
    """a3_charuco_config"""
    _fields_ = [("min_markers", C.c_uint32), ("refine", C.c_uint32), ("win_half", C.c_uint32), ("relative_win", C.c_float),
                ("max_iterations", C.c_uint32), ("min_shift", C.c_float)]

    @classmethod
    def default(cls, **kw):
        c = cls(2, 1, 5, 0.5, 30, 0.01)
        for k, v in kw.items():
            setattr(c, k, v)
        return c


def lib():
    global _lib
    if _lib is None:
        srcs = [_HERE / "charuco_oracle.c", _HERE / "board_oracle.c", _HERE / "refine_oracle.c", _HERE / "lens_oracle.c",
                _HERE.parent / "oracle" / "a3_oracle.c"]
        L = build("charuco_oracle", srcs)
        u8p, u32p, f32p, vp = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_float), C.c_void_p
        L.a3o_charuco_corners.restype = C.c_uint32
        L.a3o_charuco_corners.argtypes = [u32p, f32p, C.c_uint32, f32p, u32p, C.c_uint32, C.POINTER(Config), u32p, f32p, C.c_uint32, u8p,
                                          C.c_uint32, C.c_uint32, C.c_uint32, vp]
        L.a3o_charuco_pose.restype = C.c_int
        L.a3o_charuco_pose.argtypes = [u32p, f32p, C.c_uint32, f32p, u32p, f32p, C.c_uint32, vp, C.c_uint32, f32p, f32p, C.c_uint32,
                                       C.c_uint32, vp]
        _lib = L
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _f32(a, shape):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(shape))


def corners(board, ids, corners_px, grey=None, config: Config = None, image_size=None, frame: int = 0) -> np.ndarray:
    """the contract's corners of one frame: the frame's markers (ids (n,), raw pixel corners (n, 4, 2), batch order) on a CharucoBoard;
    grey: the frame's into_luma8 plane (H, W), needed with refine = 1 -> CORNER_DTYPE records in id order"""
    cfg = config or Config.default()
    bi = np.ascontiguousarray(board.ids, dtype=np.uint32)
    bx = _f32(board.corners, (-1, 8))
    cxy = _f32(board.chessboard_corners, (-1, 2))
    adj = np.ascontiguousarray(board.adjacent_ids, dtype=np.uint32).reshape(-1, 4)
    i = np.ascontiguousarray(np.asarray(ids, dtype=np.uint32).reshape(-1))
    px = _f32(corners_px, (-1, 8)) if i.size else np.zeros((1, 8), np.float32)
    if grey is not None:
        g = np.ascontiguousarray(grey, dtype=np.uint8)
        h, w = g.shape
    else:
        assert not cfg.refine, "refinement needs the grey frame"
        g = np.zeros((1, 1), np.uint8)
        w, h = image_size
    out = np.zeros(max(cxy.shape[0], 1), CORNER_DTYPE)
    n = lib().a3o_charuco_corners(_p(bi, C.c_uint32), _p(bx, C.c_float), bi.size, _p(cxy, C.c_float), _p(adj, C.c_uint32), cxy.shape[0],
                                  C.byref(cfg), _p(i, C.c_uint32), _p(px, C.c_float), i.size, _p(g, C.c_uint8), w, h, frame,
                                  out.ctypes.data_as(C.c_void_p))
    return out[:n].copy()


def pose(board, ids, corners_px, records, image_size, intrinsics=None, distortion=None) -> np.ndarray:
    """the contract's ChArUco pose of one frame: ids / corners_px the frame's markers as the board pose reads them (undistorted with a
    distortion), records its CORNER_DTYPE records; intrinsics (fx, fy, cx, cy) or None; distortion (k1 .. k6, iterations, max residual)"""
    bi = np.ascontiguousarray(board.ids, dtype=np.uint32)
    bx = _f32(board.corners, (-1, 8))
    cxy = _f32(board.chessboard_corners, (-1, 2))
    i = np.ascontiguousarray(np.asarray(ids, dtype=np.uint32).reshape(-1))
    px = _f32(corners_px, (-1, 8)) if i.size else np.zeros((1, 8), np.float32)
    rec = np.ascontiguousarray(records, dtype=CORNER_DTYPE)
    if rec.size == 0:
        rec = np.zeros(1, CORNER_DTYPE)[:0]
    ci = None if intrinsics is None else _f32(intrinsics, 4)
    di = None if distortion is None else _f32(distortion, 10)
    out = np.zeros(1, POSE_DTYPE)
    w, h = image_size
    rc = lib().a3o_charuco_pose(_p(bi, C.c_uint32), _p(bx, C.c_float), bi.size, _p(cxy, C.c_float), _p(i, C.c_uint32), _p(px, C.c_float),
                                i.size, rec.ctypes.data_as(C.c_void_p), rec.size, None if ci is None else _p(ci, C.c_float),
                                None if di is None else _p(di, C.c_float), w, h, out.ctypes.data_as(C.c_void_p))
    assert rc == 0
    return out[0]
