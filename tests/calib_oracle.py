"""ctypes binding of tests/calib_oracle.c: the CPU restatement of the camera calibration (a3_calibrate_cameras, include/aruco3_hip.h) that
the device kernel k_calibrate is held to, the f64 forward model the test data is projected with, and the C compiler's view of the
structs.  TEST INFRASTRUCTURE ONLY -- the tests and tools/calib_bench.py load it; aruco3_amd never does.

The library is compiled on first use into a temporary directory of its own (gcc / cc, -ffp-contract=off as the kernels), so the
repository tree is not written to."""
import ctypes as C

import numpy as np

from aruco3_amd import _lib as A
from tests.oracle_build import build

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = build("calib_oracle")
        f32p, f64p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint32)
        L.a3o_calibrate.restype = C.c_int
        L.a3o_calibrate.argtypes = [C.POINTER(A.CalibCamera), C.c_size_t, u32p, C.c_size_t, f32p, f32p, C.POINTER(A.CalibResult),
                                    C.POINTER(A.CalibView)]
        L.a3o_calib_project.restype = None
        L.a3o_calib_project.argtypes = [f64p, f64p, f64p, f64p, C.c_size_t, f64p]
        L.a3o_calib_layout.restype = None
        L.a3o_calib_layout.argtypes = [C.POINTER(C.c_size_t)]
        _lib = L
    return _lib


def calibrate(cams, view_offsets, object_xy, image_xy):
    """a3o_calibrate: the same arguments as Context.calibrate_cameras -> (CalibResult array, CalibView array)"""
    off = np.ascontiguousarray(np.asarray(view_offsets, dtype=np.uint32).reshape(-1))
    obj = np.ascontiguousarray(np.asarray(object_xy, dtype=np.float32).reshape(-1, 2))
    img = np.ascontiguousarray(np.asarray(image_xy, dtype=np.float32).reshape(-1, 2))
    n_views = off.size - 1
    res = (A.CalibResult * len(cams))()
    views = (A.CalibView * max(n_views, 1))()
    rc = lib().a3o_calibrate(cams, len(cams), off.ctypes.data_as(C.POINTER(C.c_uint32)), n_views, obj.ctypes.data_as(C.POINTER(C.c_float)),
                             img.ctypes.data_as(C.POINTER(C.c_float)), res, views)
    assert rc == 0
    return res, views


def project(a, R, t, xy) -> np.ndarray:
    """the contract's forward model in f64: intrinsics a (12), R (3x3), t (3), board points (n, 2) -> pixels (n, 2) float64"""
    a = np.ascontiguousarray(np.asarray(a, np.float64).reshape(12))
    R = np.ascontiguousarray(np.asarray(R, np.float64).reshape(9))
    t = np.ascontiguousarray(np.asarray(t, np.float64).reshape(3))
    xy = np.ascontiguousarray(np.asarray(xy, np.float64).reshape(-1, 2))
    out = np.zeros_like(xy)
    p = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    lib().a3o_calib_project(p(a), p(R), p(t), p(xy), xy.shape[0], p(out))
    return out


def layout():
    """sizes and offsets of a3_calib_camera / _result / _view as gcc lays out include/aruco3_hip.h (a3o_calib_layout's order)"""
    out = (C.c_size_t * 14)()
    lib().a3o_calib_layout(out)
    return list(out)
