"""ctypes binding of tests/inverted_edge_oracle.c: edge-fit corner refinement (A3_REFINE_EDGES) restated with a polarity per quad, what a
batch in mode A3_POLARITY_BOTH applies to its flagged markers.  TEST INFRASTRUCTURE ONLY.  Compiled on first use through
tests/oracle_build.build."""
import ctypes as C

import numpy as np

from tests.oracle_build import build
from tests.refine_oracle import RefineConfig, quad_cell_px

_lib = None


def lib():
    global _lib
    if _lib is None:
        L = build("inverted_edge_oracle")
        L.a3i_refine_quads.restype = C.c_int
        L.a3i_refine_quads.argtypes = [C.POINTER(C.c_uint8), C.c_uint32, C.c_uint32, C.POINTER(RefineConfig), C.POINTER(C.c_float),
                                       C.POINTER(C.c_float), C.POINTER(C.c_uint32), C.c_size_t]
        _lib = L
    return _lib


def _p(a, t):
    return a.ctypes.data_as(C.POINTER(t))


def refine_quads(grey: np.ndarray, quads, cfg: RefineConfig, cell_px=None, polarity=None) -> np.ndarray:
    """one grey frame: quads (n, 4, 2) float (a3_marker order) -> refined float32 (n, 4, 2); cell_px: one value per quad or None;
    polarity: one word per quad (bit 0: bright inside) or None (all dark inside)"""
    g = np.ascontiguousarray(grey, dtype=np.uint8)
    h, w = g.shape
    xy = np.ascontiguousarray(np.asarray(quads, dtype=np.float32).reshape(-1, 4, 2)).copy()
    cp = None if cell_px is None else np.ascontiguousarray(np.asarray(cell_px, dtype=np.float32).reshape(-1))
    pol = None if polarity is None else np.ascontiguousarray(np.asarray(polarity, dtype=np.uint32).reshape(-1))
    assert (cp is None or cp.size == xy.shape[0]) and (pol is None or pol.size == xy.shape[0])
    rc = lib().a3i_refine_quads(_p(g, C.c_uint8), w, h, C.byref(cfg), _p(xy, C.c_float), None if cp is None else _p(cp, C.c_float),
                                None if pol is None else _p(pol, C.c_uint32), xy.shape[0])
    if rc != 0:
        raise ValueError("a3i_refine_quads: bad refinement config")
    return xy


def refine_markers(grey: np.ndarray, markers, cells: int, cfg: RefineConfig, flags) -> np.ndarray:
    """what a detection batch in mode A3_POLARITY_BOTH applies with method EDGES: every marker's integer corners (a3_marker order), its
    search range from the quad's cell size, its polarity from its flag word -> float32 (n_markers, 4, 2)"""
    if len(markers) == 0:
        return np.zeros((0, 4, 2), dtype=np.float32)
    quads = np.array([np.asarray(q, dtype=np.uint32).reshape(8) for q in markers], dtype=np.uint32)
    cell = np.array([quad_cell_px(q, cells) for q in quads], dtype=np.float32)
    return refine_quads(grey, quads.reshape(-1, 4, 2).astype(np.float32), cfg, cell, flags)
