"""Frames seen through a fisheye lens, rendered on the host: tests/lens_util.py's renderer with the Kannala-Brandt model (cv::fisheye)
in place of the rational one.  Every output pixel is mapped back -- distorted pixel -> theta_d -> theta by Newton's method in float64
(on theta, with numpy's tangent: the renderer's inverse, not the contract's) -> ray -> board plane -> marker cell -- and supersampled
S x S.  The true ideal-pinhole corners come from board_util.project.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from aruco3_amd import synth
from tests.lens_util import BACKGROUND, BLACK, H720, K720, PAPER_MARGIN, W720, WHITE

# k1 k2 k3 k4: at K720 a corner 600 px right of and 330 px below the principal point lies 186 px from where the ideal camera sees it
MILD = (-0.02, 0.005, -0.003, 0.0005)


def undistort_normalized(xd, yd, k, iterations=30):
    """float64 inverse of the fisheye forward model: Newton on theta_d(theta) = |(xd, yd)|, then r = tan(theta)"""
    k1, k2, k3, k4 = k
    rd = np.sqrt(xd * xd + yd * yd)
    th = rd.copy()
    for _ in range(iterations):
        t2 = th * th
        g = th * (1 + (((k4 * t2 + k3) * t2 + k2) * t2 + k1) * t2)
        dg = 1 + (((9 * k4 * t2 + 7 * k3) * t2 + 5 * k2) * t2 + 3 * k1) * t2
        th = th - (g - rd) / dg
    s = np.divide(np.tan(th), rd, out=np.ones_like(rd), where=rd > 0)
    return xd * s, yd * s


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


def render(board, d, R, t, k=MILD, K=K720, width=W720, height=H720, S=3) -> np.ndarray:
    """one grey frame (height, width) uint8 of `board` (a GridBoard) at pose R, t through the fisheye lens k"""
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
