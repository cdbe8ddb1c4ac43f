"""ctypes binding of tests/fisheye_oracle.c: the CPU restatement of the fisheye lens model (a3_distortion model A3_DIST_FISHEYE,
include/aruco3_hip.h) -- its fixed-arithmetic arctangent, the forward model, the corner undistortion and the frame rectification --
that the device kernels k_undistort_corners and k_rectify are held to.  TEST INFRASTRUCTURE ONLY -- the tests and the tools' checks
load it; aruco3_amd never does.

The library is compiled on first use into a temporary directory of its own (gcc / cc, -ffp-contract=off as the kernels), so the
repository tree is not written to."""
import ctypes as C

import numpy as np

from tests import rectify_oracle
from tests.oracle_build import build

_lib = None

# coefficient sets the tests sweep: (k1, k2, k3, k4), cv::fisheye's D
COEFFS = {
    "equidistant": (0.0, 0.0, 0.0, 0.0),
    "mild": (-0.02, 0.005, -0.003, 0.0005),
    "strong": (0.08, -0.03, 0.01, -0.002),
    "neg": (-0.12, 0.02, -0.004, 0.0003),
}

# the source camera: at K every pixel of the frame has a root (theta_d up to 1.39); at K_WIDE the corners of the frame have none
SRC_SIZE = (333, 251)
K = (150.0, 150.0, 166.0, 125.0)
K_WIDE = (100.0, 100.0, 166.0, 125.0)

# rectify_oracle's views, the zoomed-out one at half its focal length so that the edge of the fisheye field is in view
VIEWS = dict(rectify_oracle.VIEWS)
VIEWS["zoomed_out"] = ((60.0, 60.0, 158.5, 101.0), (317, 203), 0.0)

rot_y = rectify_oracle.rot_y


def lib():
    global _lib
    if _lib is None:
        L = build("fisheye_oracle")
        f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        L.a3o_fisheye_atan.restype = None
        L.a3o_fisheye_atan.argtypes = [f32p, C.c_size_t, f32p]
        L.a3o_fisheye_distort.restype = None
        L.a3o_fisheye_distort.argtypes = [f32p, C.c_size_t, f32p, f32p, f32p]
        L.a3o_fisheye_undistort.restype = None
        L.a3o_fisheye_undistort.argtypes = [f32p, C.c_size_t, f32p, f32p, C.c_uint32, C.c_float, f32p, f32p]
        L.a3o_fisheye_rectify.restype = None
        L.a3o_fisheye_rectify.argtypes = [u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, C.c_uint32, f32p, f32p, f32p, f32p,
                                          C.c_uint8, u8p, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, u8p]
        _lib = L
    return _lib


def _p(a):
    return a.ctypes.data_as(C.POINTER(C.c_float))


def _f32(a, shape):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(shape))


def slots8(coeffs):
    """(k1, k2, k3, k4) -> the 8 slots of a3_distortion: k1 k2 p1 p2 k3 k4 k5 k6"""
    k1, k2, k3, k4 = (float(v) for v in coeffs)
    return (k1, k2, 0.0, 0.0, k3, k4, 0.0, 0.0)


def atan(t):
    """the contract's A, f32, elementwise"""
    a = _f32(t, -1)
    out = np.zeros_like(a)
    lib().a3o_fisheye_atan(_p(a), a.size, _p(out))
    return out


def distort(points, intr, coeffs):
    """the forward model, f32: ideal pixels (..., 2) -> distorted pixels float32 (n, 2); coeffs (k1 k2 k3 k4)"""
    xy = _f32(points, (-1, 2))
    out = np.zeros_like(xy)
    lib().a3o_fisheye_distort(_p(xy), xy.shape[0], _p(_f32(intr, 4)), _p(_f32(coeffs, 4)), _p(out))
    return out


def undistort(points, intr, coeffs, iterations=20, max_residual_px=0.1):
    """points (..., 2) pixels, intr (fx, fy, cx, cy), coeffs (k1 k2 k3 k4) -> (out float32 (n, 2), residual float32 (n,))"""
    xy = _f32(points, (-1, 2))
    n = xy.shape[0]
    out = np.zeros((n, 2), np.float32)
    res = np.zeros(n, np.float32)
    lib().a3o_fisheye_undistort(_p(xy), n, _p(_f32(intr, 4)), _p(_f32(coeffs, 4)), iterations, max_residual_px, _p(out), _p(res))
    return out, res


def rectify_raw(src, sw, sh, bpp, src_row, src_frame, n, K, coeffs, new_K, R, fill, dst, dw, dh, dst_row, dst_frame, inside=None):
    """the C call on flat uint8 buffers with explicit strides (src / dst: 1-d uint8 arrays; dst is written in place);
    coeffs (k1 k2 k3 k4)"""
    k, ks, kd, r = _f32(slots8(coeffs), 8), _f32(K, 4), _f32(new_K, 4), _f32(R, 9)
    u8 = C.POINTER(C.c_uint8)
    lib().a3o_fisheye_rectify(src.ctypes.data_as(u8), sw, sh, bpp, src_row, src_frame, n, _p(ks), _p(k), _p(kd), _p(r), fill,
                              dst.ctypes.data_as(u8), dw, dh, dst_row, dst_frame, inside.ctypes.data_as(u8) if inside is not None else None)


def rectify(frames, K, coeffs, new_K=None, new_size=None, R=None, fill=0, with_inside=False):
    """frames (N, H, W, C) or (H, W) / (H, W, C) uint8, K / new_K (fx, fy, cx, cy), coeffs (k1 k2 k3 k4), R 3 x 3
    -> (N, H', W', C) uint8 (and the (H', W') bool inside mask with with_inside)"""
    a = np.asarray(frames)
    if a.ndim == 2:
        a = a[None, :, :, None]
    elif a.ndim == 3:
        a = a[None] if a.shape[-1] in (1, 3, 4) else a[..., None]
    a = np.ascontiguousarray(a, dtype=np.uint8)
    n, h, w, c = a.shape
    dw, dh = new_size if new_size is not None else (w, h)
    out = np.empty((n, dh, dw, c), np.uint8)
    inside = np.zeros((dh, dw), np.uint8)
    rectify_raw(a.reshape(-1), w, h, c, w * c, h * w * c, n, K, coeffs, new_K if new_K is not None else K, np.eye(3) if R is None else R,
                fill, out.reshape(-1), dw, dh, dw * c, dh * dw * c, inside)
    return (out, inside.astype(bool)) if with_inside else out
