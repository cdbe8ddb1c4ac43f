"""ctypes binding of tests/refine_oracle.c: the CPU restatement of sub-pixel corner refinement (a3_refine_config) that the device
kernel is held to bit for bit.  TEST INFRASTRUCTURE ONLY -- the tests and tools/refine_bench.py load it; aruco3_amd never does.

The library is compiled on first use into a temporary directory of its own (gcc / cc, -ffp-contract=off as the kernels), so the
repository tree is not written to."""
import ctypes as C

import numpy as np

from tests.oracle_build import build

_lib = None


class RefineConfig(C.Structure):
    """a3o_refine_config (the layout of include/aruco3_hip.h a3_refine_config); default() = a3_default_refine_config"""
    _fields_ = [("method", C.c_uint32), ("win_half", C.c_uint32), ("relative_win", C.c_float), ("max_iterations", C.c_uint32),
                ("min_shift", C.c_float)]

    @classmethod
    def default(cls):
        return cls(1, 5, 0.4, 30, 0.01)


def lib():
    global _lib
    if _lib is None:
        L = build("refine_oracle")
        u8p, u32p, f32p = C.POINTER(C.c_uint8), C.POINTER(C.c_uint32), C.POINTER(C.c_float)
        L.a3o_quad_cell_px.restype = C.c_float
        L.a3o_quad_cell_px.argtypes = [u32p, C.c_uint32]
        L.a3o_refine_weights.restype = None
        L.a3o_refine_weights.argtypes = [C.c_uint32, f32p]
        L.a3o_refine_corners.restype = C.c_int
        L.a3o_refine_corners.argtypes = [u8p, C.c_uint32, C.c_uint32, C.POINTER(RefineConfig), f32p, f32p, C.c_size_t]
        L.a3o_refine_corners_trace.restype = C.c_int
        L.a3o_refine_corners_trace.argtypes = [u8p, C.c_uint32, C.c_uint32, C.POINTER(RefineConfig), f32p, f32p, C.c_size_t, C.c_int,
                                               C.POINTER(C.c_int32), u32p, C.POINTER(C.c_int32), f32p]
        _lib = L
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def quad_cell_px(corners, cells: int) -> float:
    """shortest side of an integer quad / cells across the marker (the relative window's cell size)"""
    c = np.ascontiguousarray(corners, dtype=np.uint32).reshape(8)
    return float(lib().a3o_quad_cell_px(_p(c, C.c_uint32), cells))


def refine_weights(w: int) -> np.ndarray:
    g = np.zeros(2 * w + 1, dtype=np.float32)
    lib().a3o_refine_weights(w, _p(g, C.c_float))
    return g


def refine_corners(grey: np.ndarray, corners, config: RefineConfig = None, cell_px=None) -> np.ndarray:
    """one grey frame: corners (..., 2) float -> refined float32 (n, 2); cell_px: one value per corner or None"""
    g = np.ascontiguousarray(grey, dtype=np.uint8)
    h, w = g.shape
    xy = np.ascontiguousarray(np.asarray(corners, dtype=np.float32).reshape(-1, 2)).copy()
    cp = None if cell_px is None else np.ascontiguousarray(np.asarray(cell_px, dtype=np.float32).reshape(-1))
    assert cp is None or cp.size == xy.shape[0]
    cfg = config or RefineConfig.default()
    rc = lib().a3o_refine_corners(_p(g, C.c_uint8), w, h, C.byref(cfg), _p(xy, C.c_float), None if cp is None else _p(cp, C.c_float),
                                  xy.shape[0])
    if rc != 0:
        raise ValueError("a3o_refine_corners: bad refinement config")
    return xy


EXITS = ("det0", "nonfinite", "revert", "converged", "cap")   # a3o_refine_corners_trace's `how` (A3O_EXIT_*)
VARIANTS = range(1, 10)   # the deliberately wrong restatements (tests/refine_oracle.c lists them); 0 is the contract


def refine_corners_trace(grey: np.ndarray, corners, config: RefineConfig = None, cell_px=None, variant: int = 0) -> dict:
    """refine_corners with a record per corner: {"xy" float32 (n, 2), "w" int32, "iters" uint32, "exit" int32 (an index into EXITS),
    "excursion" float32 (the largest max(|cx - q0x|, |cy - q0y|) over the estimates kept)}.  variant 0 is the contract."""
    g = np.ascontiguousarray(grey, dtype=np.uint8)
    h, w = g.shape
    xy = np.ascontiguousarray(np.asarray(corners, dtype=np.float32).reshape(-1, 2)).copy()
    n = xy.shape[0]
    cp = None if cell_px is None else np.ascontiguousarray(np.asarray(cell_px, dtype=np.float32).reshape(-1))
    assert cp is None or cp.size == n
    cfg = config or RefineConfig.default()
    win, iters, how, far = np.zeros(n, np.int32), np.zeros(n, np.uint32), np.zeros(n, np.int32), np.zeros(n, np.float32)
    rc = lib().a3o_refine_corners_trace(_p(g, C.c_uint8), w, h, C.byref(cfg), _p(xy, C.c_float), None if cp is None else _p(cp, C.c_float), n,
                                        variant, _p(win, C.c_int32), _p(iters, C.c_uint32), _p(how, C.c_int32), _p(far, C.c_float))
    if rc != 0:
        raise ValueError("a3o_refine_corners_trace: bad refinement config or variant")
    return {"xy": xy, "w": win, "iters": iters, "exit": how, "excursion": far}


def refine_markers(grey: np.ndarray, markers, cells: int, config: RefineConfig = None) -> np.ndarray:
    """the refinement a detection batch applies: every marker's integer corners (a3_marker order), its window from the quad's
    cell size -> float32 (n_markers, 4, 2)"""
    if len(markers) == 0:
        return np.zeros((0, 4, 2), dtype=np.float32)
    quads = np.array([np.asarray(q, dtype=np.uint32).reshape(8) for q in markers], dtype=np.uint32)
    cell = np.repeat(np.array([quad_cell_px(q, cells) for q in quads], dtype=np.float32), 4)
    return refine_corners(grey, quads.reshape(-1, 2).astype(np.float32), config, cell).reshape(-1, 4, 2)
