"""ctypes binding of tests/rectify_oracle.c: the CPU restatement of the frame rectification (a3_rectify_frames, include/aruco3_hip.h)
that the device kernel k_rectify is held to.  TEST INFRASTRUCTURE ONLY -- the tests load it; aruco3_amd never does.

The library is compiled on first use into a temporary directory of its own (gcc / cc, -ffp-contract=off as the kernels), so the
repository tree is not written to."""
import ctypes as C

import numpy as np

from tests.oracle_build import build

_lib = None

# the source camera and the five views the tests sweep: (K of the view, (width, height), rotation about y in degrees)
SRC_K = (300.0, 300.0, 166.0, 125.0)
SRC_SIZE = (333, 251)
VIEWS = {
    "same": (SRC_K, (333, 251), 0.0),
    "zoomed_out": ((120.0, 120.0, 158.5, 101.0), (317, 203), 0.0),
    "zoomed_in": ((900.0, 900.0, 20.0, 10.0), (64, 48), 0.0),
    "rot5": (SRC_K, (333, 251), 5.0),
    "rot80": ((100.0, 100.0, 166.0, 125.0), (333, 251), 80.0),
}


def rot_y(deg):
    """rotation about y, float64 3 x 3 (identity for 0)"""
    t = np.radians(deg)
    return np.array([[np.cos(t), 0.0, np.sin(t)], [0.0, 1.0, 0.0], [-np.sin(t), 0.0, np.cos(t)]]) if deg else np.eye(3)


def lib():
    global _lib
    if _lib is None:
        L = build("rectify_oracle")
        f32p, u8p = C.POINTER(C.c_float), C.POINTER(C.c_uint8)
        L.a3o_rectify.restype = None
        L.a3o_rectify.argtypes = [u8p, C.c_uint32, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, C.c_uint32, f32p, f32p, f32p, f32p, C.c_uint8,
                                  u8p, C.c_uint32, C.c_uint32, C.c_size_t, C.c_size_t, u8p]
        _lib = L
    return _lib


def _f(a, n):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float32).reshape(n))


def rectify_raw(src, sw, sh, bpp, src_row, src_frame, n, K, coeffs, new_K, R, fill, dst, dw, dh, dst_row, dst_frame, inside=None):
    """the C call on flat uint8 buffers with explicit strides (src / dst: 1-d uint8 arrays; dst is written in place)"""
    k, ks, kd, r = _f(coeffs if coeffs is not None else np.zeros(8), 8), _f(K, 4), _f(new_K, 4), _f(R, 9)
    u8 = C.POINTER(C.c_uint8)
    fp = C.POINTER(C.c_float)
    lib().a3o_rectify(src.ctypes.data_as(u8), sw, sh, bpp, src_row, src_frame, n, ks.ctypes.data_as(fp), k.ctypes.data_as(fp),
                      kd.ctypes.data_as(fp), r.ctypes.data_as(fp), fill, dst.ctypes.data_as(u8), dw, dh, dst_row, dst_frame,
                      inside.ctypes.data_as(u8) if inside is not None else None)


def rectify(frames, K, coeffs, new_K=None, new_size=None, R=None, fill=0, with_inside=False):
    """frames (N, H, W, C) or (H, W) / (H, W, C) uint8, K / new_K (fx, fy, cx, cy), coeffs (k1 k2 p1 p2 k3 k4 k5 k6) or None, R 3 x 3
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
