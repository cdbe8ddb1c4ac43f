"""Frames seen through a lens, rendered on the host: a planar board at a known pose, imaged by a pinhole camera K and then distorted by
OpenCV's rational model.  Every output pixel is mapped back -- distorted pixel -> ideal normalised point (fixed-point inversion in
float64) -> ray -> board plane -> marker cell -- and supersampled S x S.  The true ideal-pinhole corners come from
board_util.project.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from aruco3_amd import synth

W720, H720 = 1280, 720
K720 = (900.0, 900.0, 640.0, 360.0)   # fx, fy, cx, cy
# k1 k2 p1 p2 k3 k4 k5 k6 of a wide webcam lens: corners near the image edge move by up to ~100 px
WEBCAM = (-0.28, 0.09, 1e-3, -5e-4, 0.0, 0.0, 0.0, 0.0)
BLACK, WHITE, PAPER_MARGIN, BACKGROUND = 25.0, 235.0, 12.0, 110.0


def undistort_normalized(xd, yd, k, iterations=40):
    """float64 inverse of the forward model by fixed-point iteration (the renderer's, not the contract's)"""
    k1, k2, p1, p2, k3, k4, k5, k6 = k
    x, y = xd.copy(), yd.copy()
    for _ in range(iterations):
        r2 = x * x + y * y
        icd = (1 + ((k6 * r2 + k5) * r2 + k4) * r2) / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        x, y = (xd - dx) * icd, (yd - dy) * icd
    return x, y


_rays = {}


def _ideal_grid(k, K, width, height, S):
    """ideal normalised (x, y) of every subsample of every pixel, float64 (height, width, S, S) each -- the same for every frame"""
    key = (tuple(k), tuple(K), width, height, S)
    if key not in _rays:
        fx, fy, cx, cy = K
        off = (np.arange(S) + 0.5) / S - 0.5
        yy, xx, sy, sx = np.meshgrid(np.arange(height, dtype=np.float64), np.arange(width, dtype=np.float64), off, off, indexing="ij")
        _rays.clear()
        _rays[key] = undistort_normalized((xx + sx - cx) / fx, (yy + sy - cy) / fy, k)
    return _rays[key]


def render(board, d, R, t, k=WEBCAM, K=K720, width=W720, height=H720, S=3) -> np.ndarray:
    """one grey frame (height, width) uint8 of `board` (a GridBoard) at pose R, t through lens k"""
    Hb = np.column_stack([np.asarray(R, np.float64)[:, 0], np.asarray(R, np.float64)[:, 1], np.asarray(t, np.float64)])
    Hinv = np.linalg.inv(Hb)
    L, step = board.marker_length, board.marker_length + board.marker_separation
    cell_tab = np.stack([synth.marker_cells(int(d.code_list[i]), d.num_bits) for i in board.ids]).astype(np.float64)   # 1 = white
    n = cell_tab.shape[1]
    bx0, bx1 = -PAPER_MARGIN, board.markers_x * step - board.marker_separation + PAPER_MARGIN
    by1, by0 = PAPER_MARGIN, -(board.markers_y * step - board.marker_separation) - PAPER_MARGIN
    gx, gy = _ideal_grid(k, K, width, height, S)
    qz = Hinv[2, 0] * gx + Hinv[2, 1] * gy + Hinv[2, 2]
    X = (Hinv[0, 0] * gx + Hinv[0, 1] * gy + Hinv[0, 2]) / qz
    Y = (Hinv[1, 0] * gx + Hinv[1, 1] * gy + Hinv[1, 2]) / qz
    val = np.full(X.shape, BACKGROUND)
    paper = (X >= bx0) & (X < bx1) & (Y <= by1) & (Y > by0) & (qz > 0)
    val[paper] = WHITE
    col, row = np.floor(X / step), np.floor(-Y / step)
    u, v = X - col * step, -Y - row * step
    inside = paper & (col >= 0) & (col < board.markers_x) & (row >= 0) & (row < board.markers_y) & (u < L) & (v < L)
    slot = np.where(inside, row * board.markers_x + col, 0).astype(np.int64)
    cu = np.clip(np.floor(u / L * n), 0, n - 1).astype(np.int64)
    cv = np.clip(np.floor(v / L * n), 0, n - 1).astype(np.int64)
    val = np.where(inside, np.where(cell_tab[slot, cv, cu] > 0, WHITE, BLACK), val)
    return np.clip(np.rint(val.mean(axis=(2, 3))), 0, 255).astype(np.uint8)
