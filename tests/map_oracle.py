"""ctypes binding of tests/map_oracle.c: the CPU restatement of the marker map solve (a3_build_marker_maps, include/aruco3_hip.h) that
the device kernel k_map is held to, and the C compiler's view of the structs.  TEST INFRASTRUCTURE ONLY -- the tests and
tools/map_bench.py load it; aruco3_amd never does.

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
        L = build("map_oracle")
        L.a3o_build_marker_maps.restype = C.c_int
        L.a3o_build_marker_maps.argtypes = [C.POINTER(A.Map), C.c_size_t, C.POINTER(A.MapMarker), C.c_size_t, C.POINTER(A.MapObservation),
                                            C.c_size_t, C.POINTER(C.c_float), C.POINTER(A.MapResult), C.POINTER(A.MapMarkerResult),
                                            C.POINTER(A.MapFrame), C.c_size_t, C.POINTER(A.MapObservationResult)]
        L.a3o_map_candidates.restype = C.c_int
        L.a3o_map_candidates.argtypes = [C.POINTER(C.c_double), C.c_float, C.POINTER(C.c_float), C.POINTER(C.c_double), C.POINTER(C.c_double)]
        L.a3o_map_layout.restype = None
        L.a3o_map_layout.argtypes = [C.POINTER(C.c_size_t)]
        _lib = L
    return _lib


def build_marker_maps(maps, markers, obs, image_xy):
    """a3o_build_marker_maps: the arguments and the result of Context.build_marker_maps"""
    img = np.ascontiguousarray(np.asarray(image_xy, dtype=np.float32).reshape(-1, 8))
    n_frames = max([int(r.first_frame) + int(r.n_frames) for r in maps], default=0)
    res = (A.MapResult * max(len(maps), 1))()
    mres = (A.MapMarkerResult * max(len(markers), 1))()
    frames = (A.MapFrame * max(n_frames, 1))()
    ores = (A.MapObservationResult * max(len(obs), 1))()
    rc = lib().a3o_build_marker_maps(maps, len(maps), markers, len(markers), obs, len(obs), img.ctypes.data_as(C.POINTER(C.c_float)), res,
                                     mres, frames, n_frames, ores)
    assert rc == 0
    return res, mres, frames, ores


def candidates(a, marker_length, corners):
    """step 1 for one observation: -> (used, [(R, t), (R, t)] marker -> camera, [cost, cost]): the homography's candidate, the mirrored one"""
    a = np.ascontiguousarray(np.asarray(a, np.float64).reshape(12))
    img = np.ascontiguousarray(np.asarray(corners, np.float32).reshape(8))
    P, c = np.zeros(24), np.zeros(2)
    d = lambda v: v.ctypes.data_as(C.POINTER(C.c_double))   # noqa: E731
    used = lib().a3o_map_candidates(d(a), float(marker_length), img.ctypes.data_as(C.POINTER(C.c_float)), d(P), d(c))
    return bool(used), [(P[12 * k:12 * k + 9].reshape(3, 3).copy(), P[12 * k + 9:12 * k + 12].copy()) for k in range(2)], [float(c[0]), float(c[1])]


def layout():
    """sizes and offsets of the a3_map* structs as gcc lays out include/aruco3_hip.h (a3o_map_layout's order)"""
    out = (C.c_size_t * 18)()
    lib().a3o_map_layout(out)
    return list(out)
