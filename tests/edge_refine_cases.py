"""Small hand-made scenes for edge-fit corner refinement (A3_REFINE_EDGES), shared by tests/test_oracle_edge_refine.py (the CPU
restatement) and tests/test_gpu_edge_refine.py (the kernel, bit for bit against it).  A scene is a grey frame of 160 x 120 with dark
convex quads rendered by 16 x 16 supersampling (pixel centres at integer coordinates, as in the contract), the analytic corners, and
start quads.  Nothing here comes from the library under test.  TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

from tests import edge_refine_oracle as ero

W, H = 160, 120
SS = 16


def render(quads, lo=30, hi=220, w=W, h=H) -> np.ndarray:
    """dark (lo) convex quads, corners clockwise in image coordinates (y down), on a bright (hi) ground: the mean of SS x SS point samples
    per pixel, rounded"""
    sub = (np.arange(SS) + 0.5) / SS - 0.5
    xs = (np.arange(w)[:, None] + sub[None, :]).reshape(-1)
    ys = (np.arange(h)[:, None] + sub[None, :]).reshape(-1)
    X, Y = np.meshgrid(xs, ys)
    cover = np.zeros((h, w))
    for q in np.asarray(quads, dtype=np.float64).reshape(-1, 4, 2):
        inside = np.ones(X.shape, bool)
        for e in range(4):
            a, b = q[e], q[(e + 1) & 3]
            inside &= (b[0] - a[0]) * (Y - a[1]) - (b[1] - a[1]) * (X - a[0]) >= 0.0   # (clockwise with y down: the inside is on the right)
        cover += inside.reshape(h, SS, w, SS).mean(axis=(1, 3))
    return np.rint(hi - (hi - lo) * np.clip(cover, 0.0, 1.0)).astype(np.uint8)


def square(cx, cy, half, degrees) -> np.ndarray:
    """(4, 2) float64 corners in a3_marker order (clockwise with y down, corner 0 top-left at 0 degrees)"""
    t = np.deg2rad(degrees)
    R = np.array([[np.cos(t), -np.sin(t)], [np.sin(t), np.cos(t)]])
    return np.array([cx, cy]) + np.array([[-half, -half], [half, -half], [half, half], [-half, half]]) @ R.T


def along(q, corner, px):
    """q with one corner moved px along the side that leaves it"""
    q = np.array(q, dtype=np.float64)
    d = q[(corner + 1) & 3] - q[corner]
    q[corner] += px * d / np.linalg.norm(d)
    return q


SLANTED = square(80.3, 59.6, 35.0, 17.0)
BORDER = np.array([[30.4, 1.0], [101.7, 1.0], [101.7, 70.2], [30.4, 70.2]])   # the top side runs 1 px from the frame border
SMALL = square(80.0, 60.0, 1.4, 0.0)   # sides of 2.8 px


@functools.lru_cache(maxsize=None)
def slanted_frame() -> np.ndarray:
    g = render([SLANTED])
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def border_frame() -> np.ndarray:
    g = render([BORDER])
    g.setflags(write=False)
    return g


def slanted_start() -> np.ndarray:
    """one corner 6 px along its side, the others within 1 px of the analytic corners"""
    off = np.array([[0.0, 0.0], [0.7, -0.6], [-0.9, 0.4], [0.3, 0.8]])
    return (along(SLANTED, 0, 6.0) + off).astype(np.float32)


def far_start() -> np.ndarray:
    """one corner 30 px off"""
    q = SLANTED.copy()
    q[2] += np.array([-21.0, -21.5])
    return q.astype(np.float32)


@functools.lru_cache(maxsize=None)
def scenes():
    """name -> (grey frame, start quads float32 (n, 4, 2), config, cell_px per quad or None): everything the GPU test runs through
    a3_refine_corners, in one list"""
    flat = np.full((H, W), 117, np.uint8)
    faint = render([SLANTED], lo=105, hi=120)   # contrast 15: no station is live
    rounded = np.rint(SLANTED).astype(np.float32)
    two = np.stack([slanted_start(), rounded])
    out = {
        "flat": (flat, rounded[None], ero.config(5, 0.0), None),
        "faint": (faint, rounded[None], ero.config(5, 0.0), None),
        "slanted": (slanted_frame(), two, ero.config(10, 0.0), None),
        "slanted_relative": (slanted_frame(), two, ero.config(10, 0.4), np.array([70.0 / 8.0, 4.0], np.float32)),   # r = 3 and 2
        "far": (slanted_frame(), far_start()[None], ero.config(10, 0.0), None),
        "border": (border_frame(), np.rint(BORDER).astype(np.float32)[None], ero.config(5, 0.0), None),
        "no_pass": (slanted_frame(), two, ero.config(10, 0.0, max_iterations=0), None),
        "one_pass": (slanted_frame(), two, ero.config(10, 0.0, max_iterations=1), None),
        "short_side": (render([SMALL]), SMALL.astype(np.float32)[None], ero.config(5, 0.0), None),
    }
    for v in out.values():
        v[0].setflags(write=False)
    return out
