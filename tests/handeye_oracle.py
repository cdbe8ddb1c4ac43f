"""ctypes binding of tests/handeye_oracle.c: the CPU restatement of the hand-eye calibration (a3_calibrate_hand_eyes,
include/aruco3_hip.h) that the device kernel k_handeye is held to, and the C compiler's view of the structs.  TEST INFRASTRUCTURE
ONLY -- the tests and tools/handeye_bench.py load it; aruco3_amd never does.

The library is compiled on first use into a temporary directory of its own (gcc / cc, the flags of tests/oracle_build.py), so the
repository tree is not written to."""
import ctypes as C

import numpy as np

from aruco3_amd import _lib as A
from tests.oracle_build import build

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = build("handeye_oracle")
        f32p = C.POINTER(C.c_float)
        L.a3o_calibrate_hand_eyes.restype = C.c_int
        L.a3o_calibrate_hand_eyes.argtypes = [C.POINTER(A.HandEyeProblem), C.c_size_t, C.POINTER(A.HandEyeFrame), C.c_size_t, f32p, f32p,
                                              C.POINTER(A.HandEyeResult), C.POINTER(A.HandEyeFrameResult)]
        L.a3o_handeye_pivots.restype = None
        L.a3o_handeye_pivots.argtypes = [C.POINTER(C.c_double)]
        L.a3o_handeye_layout.restype = None
        L.a3o_handeye_layout.argtypes = [C.POINTER(C.c_size_t)]
        _lib = L
    return _lib


def calibrate_hand_eyes(problems, frames, object_xy, image_xy):
    """a3o_calibrate_hand_eyes: the arguments and the result of Context.calibrate_hand_eyes"""
    obj = np.ascontiguousarray(np.asarray(object_xy, dtype=np.float32).reshape(-1, 2))
    img = np.ascontiguousarray(np.asarray(image_xy, dtype=np.float32).reshape(-1, 2))
    res = (A.HandEyeResult * max(len(problems), 1))()
    fres = (A.HandEyeFrameResult * max(len(frames), 1))()
    rc = lib().a3o_calibrate_hand_eyes(problems, len(problems), frames, len(frames), obj.ctypes.data_as(C.POINTER(C.c_float)),
                                       img.ctypes.data_as(C.POINTER(C.c_float)), res, fres)
    assert rc == 0
    return res, fres


def pivots():
    """(the winning chart's, the translation system's) smallest pivot over the largest diagonal entry, of the last problem whose start ran"""
    out = (C.c_double * 2)()
    lib().a3o_handeye_pivots(out)
    return float(out[0]), float(out[1])


def layout():
    """sizes and offsets of the a3_handeye* structs as gcc lays out include/aruco3_hip.h (a3o_handeye_layout's order)"""
    out = (C.c_size_t * 20)()
    lib().a3o_handeye_layout(out)
    return list(out)
