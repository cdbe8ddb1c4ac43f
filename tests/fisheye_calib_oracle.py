"""ctypes binding of tests/fisheye_calib_oracle.c: the CPU restatement of the fisheye camera calibration
(a3_calibrate_fisheye_cameras, include/aruco3_hip.h) that the device kernel k_calibrate_fisheye is held to, the f64 forward model the
test data is projected with, the contract's arctangent A64, one point's augmented rows, the start's kept-point rule, and the C
compiler's view of the structs.  TEST INFRASTRUCTURE ONLY -- the tests and tools/calib_bench.py load it; aruco3_amd never does.

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
        L = build("fisheye_calib_oracle")
        f32p, f64p, u32p = C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_uint32)
        L.a3o_calibrate_fisheye.restype = C.c_int
        L.a3o_calibrate_fisheye.argtypes = [C.POINTER(A.CalibCamera), C.c_size_t, u32p, C.c_size_t, f32p, f32p, C.POINTER(A.CalibResult),
                                            C.POINTER(A.CalibView)]
        L.a3o_a64.restype = C.c_double
        L.a3o_a64.argtypes = [C.c_double]
        L.a3o_fisheye_calib_row.restype = None
        L.a3o_fisheye_calib_row.argtypes = [f64p, f64p, f64p, C.c_double, C.c_double, C.c_double, C.c_double, f64p, f64p]
        L.a3o_fisheye_calib_project.restype = None
        L.a3o_fisheye_calib_project.argtypes = [f64p, f64p, f64p, f64p, C.c_size_t, f64p]
        L.a3o_fisheye_calib_start.restype = None
        L.a3o_fisheye_calib_start.argtypes = [f64p, f32p, C.c_size_t, C.POINTER(C.c_int), f32p]
        L.a3o_fisheye_calib_layout.restype = None
        L.a3o_fisheye_calib_layout.argtypes = [C.POINTER(C.c_size_t)]
        _lib = L
    return _lib


def _d(v):
    return v.ctypes.data_as(C.POINTER(C.c_double))


def calibrate(cams, view_offsets, object_xy, image_xy):
    """a3o_calibrate_fisheye: the same arguments as Context.calibrate_fisheye_cameras -> (CalibResult array, CalibView array)"""
    off = np.ascontiguousarray(np.asarray(view_offsets, dtype=np.uint32).reshape(-1))
    obj = np.ascontiguousarray(np.asarray(object_xy, dtype=np.float32).reshape(-1, 2))
    img = np.ascontiguousarray(np.asarray(image_xy, dtype=np.float32).reshape(-1, 2))
    n_views = off.size - 1
    res = (A.CalibResult * len(cams))()
    views = (A.CalibView * max(n_views, 1))()
    rc = lib().a3o_calibrate_fisheye(cams, len(cams), off.ctypes.data_as(C.POINTER(C.c_uint32)), n_views, obj.ctypes.data_as(C.POINTER(C.c_float)),
                                     img.ctypes.data_as(C.POINTER(C.c_float)), res, views)
    assert rc == 0
    return res, views


def a64(t: float) -> float:
    """the contract's arctangent"""
    return float(lib().a3o_a64(float(t)))


def row(a, R, t, X, Y, u=0.0, v=0.0):
    """one point's two augmented rows (15,) each: 14 Jacobian columns, then the residual"""
    a = np.ascontiguousarray(np.asarray(a, np.float64).reshape(8))
    R = np.ascontiguousarray(np.asarray(R, np.float64).reshape(9))
    t = np.ascontiguousarray(np.asarray(t, np.float64).reshape(3))
    au, av = np.zeros(15), np.zeros(15)
    lib().a3o_fisheye_calib_row(_d(a), _d(R), _d(t), float(X), float(Y), float(u), float(v), _d(au), _d(av))
    return au, av


def project(a, R, t, xy) -> np.ndarray:
    """the contract's forward model in f64: intrinsics a (8: fx fy cx cy k1 k2 k3 k4), R (3x3), t (3), board points (n, 2) -> pixels"""
    a = np.ascontiguousarray(np.asarray(a, np.float64).reshape(8))
    R = np.ascontiguousarray(np.asarray(R, np.float64).reshape(9))
    t = np.ascontiguousarray(np.asarray(t, np.float64).reshape(3))
    xy = np.ascontiguousarray(np.asarray(xy, np.float64).reshape(-1, 2))
    out = np.zeros_like(xy)
    lib().a3o_fisheye_calib_project(_d(a), _d(R), _d(t), _d(xy), xy.shape[0], _d(out))
    return out


def start_points(a, image_xy):
    """step 2's rule on image points (n, 2) at the start parameters a (8) -> (kept (n,) bool, normalised points (n, 2) float32)"""
    a = np.ascontiguousarray(np.asarray(a, np.float64).reshape(8))
    img = np.ascontiguousarray(np.asarray(image_xy, np.float32).reshape(-1, 2))
    kept = np.zeros(img.shape[0], np.int32)
    xy = np.zeros_like(img)
    lib().a3o_fisheye_calib_start(_d(a), img.ctypes.data_as(C.POINTER(C.c_float)), img.shape[0], kept.ctypes.data_as(C.POINTER(C.c_int)),
                                  xy.ctypes.data_as(C.POINTER(C.c_float)))
    return kept.astype(bool), xy


def layout():
    """sizes and offsets of a3_calib_camera / _result / _view as gcc lays out include/aruco3_hip.h"""
    out = (C.c_size_t * 14)()
    lib().a3o_fisheye_calib_layout(out)
    return list(out)
