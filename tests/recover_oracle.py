"""ctypes binding of tests/recover_oracle.c: the CPU restatement of the board-aided marker recovery (a3_set_board_recovery /
a3_recover_markers, include/aruco3_hip.h) that the device kernel k_recover_frames is held to.  TEST INFRASTRUCTURE ONLY -- the tests
and tools/recover_bench.py load it; aruco3_amd never does.

The library is compiled on first use into a temporary directory of its own (tests/oracle_build.py)."""
import ctypes as C

import numpy as np

from tests.oracle_build import build

_lib = None

# a3_marker (include/aruco3_hip.h), as aruco3_amd._lib.MARKER_DTYPE lays it out
MARKER_DTYPE = np.dtype([("frame", "<u4"), ("id", "<u4"), ("code", "<u8"), ("corners", "<u4", (8,)), ("hamming_distance", "u1"),
                         ("rotation", "u1"), ("candidate_index", "<u2")], align=True)
FIELDS = ("frame", "id", "code", "corners", "hamming_distance", "rotation", "candidate_index")
NO_BITS = 255


def lib():
    global _lib
    if _lib is None:
        L = build("recover_oracle")
        u32p, u64p, u8p, f32p, f64p, vp = (C.POINTER(C.c_uint32), C.POINTER(C.c_uint64), C.POINTER(C.c_uint8), C.POINTER(C.c_float),
                                           C.POINTER(C.c_double), C.c_void_p)
        L.a3o_recover_markers.restype = C.c_uint32
        L.a3o_recover_markers.argtypes = [u32p, f32p, C.c_uint32, u64p, u32p, u32p, C.c_uint32, u32p, u64p, u8p, C.c_uint32, C.c_uint32, C.c_float,
                                          C.c_uint32, C.c_uint32, vp]
        L.a3o_recover_expected.restype = C.c_int
        L.a3o_recover_expected.argtypes = [u32p, f32p, C.c_uint32, u32p, u32p, C.c_uint32, C.c_uint32, f64p, u8p]
        _lib = L
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def _arr(a, dtype, shape):
    a = np.ascontiguousarray(np.asarray(a, dtype=dtype).reshape(shape))
    return a if a.size else np.zeros((1,) + tuple(s for s in a.shape[1:]), dtype)   # (never a null pointer)


def _inputs(board, detected_ids, detected_corners, candidate_corners=None, codes4=None, has_codes=None):
    bi = np.ascontiguousarray(board.ids, dtype=np.uint32)
    bx = np.ascontiguousarray(np.asarray(board.corners, dtype=np.float32).reshape(-1, 8))
    di = np.asarray(detected_ids, dtype=np.uint32).reshape(-1)
    nd = di.size
    dx = _arr(detected_corners, np.uint32, (-1, 8))
    di = _arr(di, np.uint32, (-1,))
    if candidate_corners is None:
        return bi, bx, di, dx, nd
    nc = np.asarray(candidate_corners).reshape(-1, 8).shape[0]
    return bi, bx, di, dx, nd, _arr(candidate_corners, np.uint32, (-1, 8)), _arr(codes4, np.uint64, (-1, 4)), _arr(has_codes, np.uint8, (-1,)), nc


def recover_markers(board, code_list, detected_ids, detected_corners, candidate_corners, codes4, has_codes, min_markers, max_distance_px, max_hamming,
                    frame=0):
    """the contract's steps 1-5 of one frame -> MARKER_DTYPE records in candidate order"""
    bi, bx, di, dx, nd, cx, ck, ch, nc = _inputs(board, detected_ids, detected_corners, candidate_corners, codes4, has_codes)
    dict_ = np.ascontiguousarray(code_list, dtype=np.uint64)
    out = np.zeros(max(min(bi.size, nc), 1), MARKER_DTYPE)
    n = lib().a3o_recover_markers(_p(bi, C.c_uint32), _p(bx, C.c_float), bi.size, _p(dict_, C.c_uint64), _p(di, C.c_uint32), _p(dx, C.c_uint32), nd,
                                  _p(cx, C.c_uint32), _p(ck, C.c_uint64), _p(ch, C.c_uint8), nc, int(min_markers), float(np.float32(max_distance_px)),
                                  int(max_hamming), int(frame), out.ctypes.data_as(C.c_void_p))
    return out[:int(n)]


def expected_corners(board, detected_ids, detected_corners, min_markers=1):
    """steps 1-2 -> (whether the frame has a homography, float64 (slots, 4, 2) expected corners, bool (slots,): the slot is missing and
    its expected corners exist)"""
    bi, bx, di, dx, nd = _inputs(board, detected_ids, detected_corners)
    e = np.zeros((bi.size, 4, 2), np.float64)
    ok = np.zeros(bi.size, np.uint8)
    have = lib().a3o_recover_expected(_p(bi, C.c_uint32), _p(bx, C.c_float), bi.size, _p(di, C.c_uint32), _p(dx, C.c_uint32), nd, int(min_markers),
                                      _p(e, C.c_double), _p(ok, C.c_uint8))
    return bool(have), e, ok.astype(bool)


def same_records(a, b) -> bool:
    """field by field (the padding of a record is not part of it)"""
    return len(a) == len(b) and all(np.array_equal(a[f], b[f]) for f in FIELDS)
