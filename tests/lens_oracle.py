"""ctypes binding of tests/lens_oracle.c: the CPU restatement of the lens undistortion (a3_set_distortion, include/aruco3_hip.h) that
the device kernel k_undistort_corners is held to, and the forward model.  TEST INFRASTRUCTURE ONLY -- the tests and tools/lens_bench.py
load it; aruco3_amd never does.

The library is compiled on first use into a temporary directory of its own (gcc / cc, -ffp-contract=off as the kernels), so the
repository tree is not written to."""
import ctypes as C

import numpy as np

from tests.oracle_build import build

_lib = None

# coefficient sets the tests sweep: (k1, k2, p1, p2, k3, k4, k5, k6)
COEFFS = {
    "barrel": (-0.28, 0.09, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
    "pincushion": (0.12, 0.03, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0),
    "tangential": (0.0, 0.0, 1.5e-3, -8e-4, 0.0, 0.0, 0.0, 0.0),
    "webcam5": (-0.28, 0.09, 1e-3, -5e-4, -0.012, 0.0, 0.0, 0.0),
    "rational8": (2.1, 0.8, 4e-4, -3e-4, 0.02, 2.4, 1.3, 0.11),
}


def lib():
    global _lib
    if _lib is None:
        L = build("lens_oracle")
        f32p = C.POINTER(C.c_float)
        L.a3o_undistort.restype = None
        L.a3o_undistort.argtypes = [f32p, C.c_size_t, f32p, f32p, C.c_uint32, C.c_float, f32p, f32p]
        L.a3o_distort.restype = None
        L.a3o_distort.argtypes = [f32p, C.c_size_t, f32p, f32p, f32p]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _f32(a, shape):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(shape))


def undistort(points, intr, coeffs, iterations=20, max_residual_px=0.1):
    """points (..., 2) pixels, intr (fx, fy, cx, cy), coeffs (k1 k2 p1 p2 k3 k4 k5 k6) -> (out float32 (n, 2), residual float32 (n,))"""
    xy = _f32(points, (-1, 2))
    n = xy.shape[0]
    out = np.zeros((n, 2), np.float32)
    res = np.zeros(n, np.float32)
    lib().a3o_undistort(_p(xy), n, _p(_f32(intr, 4)), _p(_f32(coeffs, 8)), iterations, max_residual_px, _p(out), _p(res))
    return out, res


def distort(points, intr, coeffs):
    """the forward model, f32: ideal pixels (..., 2) -> distorted pixels float32 (n, 2)"""
    xy = _f32(points, (-1, 2))
    out = np.zeros_like(xy)
    lib().a3o_distort(_p(xy), xy.shape[0], _p(_f32(intr, 4)), _p(_f32(coeffs, 8)), _p(out))
    return out
