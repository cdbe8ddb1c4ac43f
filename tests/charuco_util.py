"""ChArUco scenes: a CharucoBoard at a known pose K [R | t], drawn by the device renderer (a3_synth_render in paper mode: every black
chessboard square is a one-cell all-black "marker", every board marker its real code) or, for the CPU tests, by a supersampled host
renderer.  The true chessboard corners are the board's corners projected through the same camera.  TEST INFRASTRUCTURE ONLY."""
import math
from typing import List

import numpy as np

from aruco3_amd import synth
from tests import board_util as bu

BLACK, WHITE, BACKGROUND = 25.0, 235.0, 200.0


def config():
    """the detector configuration of ChArUco scenes: discard_too_near with board_util's small factor (a white square's hole border
    would otherwise push out the marker inside it; CharucoBoard's docstring states the bound)"""
    return bu.config()


def square_quads(board) -> np.ndarray:
    """(n, 4, 2) board-frame corners of the black squares (TL, TR, BR, BL with y up)"""
    s = board.square_length
    out = []
    for r in range(board.squares_y):
        for c in range(board.squares_x):
            if (r + c) % 2 == 0:
                out.append([(c * s, -r * s), ((c + 1) * s, -r * s), ((c + 1) * s, -(r + 1) * s), (c * s, -(r + 1) * s)])
    return np.array(out, np.float64)


def project_points(xy, R, t, K=bu.K1080) -> np.ndarray:
    fx, fy, cx, cy = K
    X = np.concatenate([np.asarray(xy, np.float64).reshape(-1, 2), np.zeros((len(xy), 1))], axis=1)
    P = X @ np.asarray(R).T + np.asarray(t)
    return np.stack([fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy], axis=1)


def true_corners(board, R, t, K=bu.K1080) -> np.ndarray:
    """(n_corners, 2) image positions of every chessboard corner"""
    return project_points(board.chessboard_corners, R, t, K)


class Scene:
    """one frame: the board at R, t (its markers, optionally without the board slots in `drop`), plus extra (quad, id) markers"""

    def __init__(self, board, R, t, K=bu.K1080, drop=(), extra=()):
        self.board, self.R, self.t, self.K = board, np.asarray(R), np.asarray(t), K
        q = bu.project(board, R, t, K)
        self.markers = [(q[k], int(board.ids[k])) for k in range(len(board)) if k not in set(drop)] + list(extra)
        self.squares = project_points(square_quads(board).reshape(-1, 2), R, t, K).reshape(-1, 4, 2)


def _record(quad, cells: np.ndarray):
    n = cells.shape[0]
    src = np.array([[0, 0], [n, 0], [n, n], [0, n]], dtype=np.float64)
    H = synth._homography(src, np.asarray(quad, np.float64))
    outer = (H @ np.array([[-1, -1, 1], [n + 1, -1, 1], [n + 1, n + 1, 1], [-1, n + 1, 1]], dtype=np.float64).T).T
    outer = outer[:, :2] / outer[:, 2:3]
    bits = 0
    for r in range(n):
        for c in range(n):
            bits |= int(cells[r, c]) << (r * n + c)
    return (np.linalg.inv(H).astype(np.float32).reshape(9), int(math.floor(outer[:, 0].min())) - 1, int(math.floor(outer[:, 1].min())) - 1,
            int(math.ceil(outer[:, 0].max())) + 2, int(math.ceil(outer[:, 1].max())) + 2, (bits & ((1 << 64) - 1), bits >> 64), n, 0)


def layout(scenes: List[Scene], codes, num_bits: int, width: int, height: int):
    """-> (frames, markers) record arrays of a3_synth_render (flat background, no noise)"""
    frames = np.zeros(len(scenes), dtype=synth.SYNTH_FRAME_DTYPE)
    recs = []
    black = np.zeros((1, 1), np.uint8)
    for fi, sc in enumerate(scenes):
        first = len(recs)
        for quad in sc.squares:
            recs.append(_record(quad, black))
        for quad, mid in sc.markers:
            recs.append(_record(quad, synth.marker_cells(int(codes[mid]), num_bits)))
        frames[fi] = (BACKGROUND, 0.0, 0.0, 0.0, first, len(recs) - first, fi)
    marr = np.zeros(max(len(recs), 1), dtype=synth.SYNTH_MARKER_DTYPE)
    for i, r in enumerate(recs):
        marr[i] = r
    for k in ("x0", "y0"):
        marr[k] = np.clip(marr[k], 0, None)
    marr["x1"] = np.clip(marr["x1"], 0, width)
    marr["y1"] = np.clip(marr["y1"], 0, height)
    return frames, marr[: len(recs)]


def render(scenes: List[Scene], d, width: int = bu.W1080, height: int = bu.H1080, device: int = 0):
    """renders the scenes on the GPU -> CUDA uint8 tensor (N, H, W, 3)"""
    import torch

    from aruco3_amd import _lib

    frames, markers = layout(scenes, d.code_list, d.num_bits, width, height)
    out = torch.empty((len(scenes), height, width, 3), dtype=torch.uint8, device=torch.device("cuda", device))
    _lib.synth_render(device, frames, markers, width, height, True, BLACK, WHITE, 3, out.data_ptr(), width * 3, width * height * 3)
    return out


def host_grey(board, R, t, K, width: int, height: int, ss: int = 4) -> np.ndarray:
    """the board at R, t drawn on the host as an into_luma8-like grey frame (H, W) uint8: black squares and the markers' full squares
    BLACK, white squares WHITE, background BACKGROUND, each pixel the mean of ss x ss samples (pixel centres at integer coordinates)"""
    fx, fy, cx, cy = K
    Hm = np.asarray(R, np.float64)[:, :2] * 1.0
    Hm = np.concatenate([Hm, np.asarray(t, np.float64).reshape(3, 1)], axis=1)   # board (X, Y, 1) -> camera
    Kmat = np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]])
    inv = np.linalg.inv(Kmat @ Hm)
    off = (np.arange(ss) + 0.5) / ss - 0.5
    ys, xs = np.mgrid[0:height, 0:width].astype(np.float64)
    acc = np.zeros((height, width))
    s, ml = board.square_length, board.marker_length
    m = (s - ml) / 2
    for oy in off:
        for ox in off:
            p = np.stack([xs + ox, ys + oy, np.ones_like(xs)], axis=-1) @ inv.T
            X, Y = p[..., 0] / p[..., 2], -(p[..., 1] / p[..., 2])   # Y: distance below the top edge
            c, r = np.floor(X / s), np.floor(Y / s)
            inside = (c >= 0) & (c < board.squares_x) & (r >= 0) & (r < board.squares_y)
            u, v = X - c * s, Y - r * s
            in_marker = (u >= m) & (u < s - m) & (v >= m) & (v < s - m)
            black = ((r + c) % 2 == 0) | in_marker
            acc += np.where(inside, np.where(black, BLACK, WHITE), BACKGROUND)
    return np.clip(np.floor(acc / (ss * ss) + 0.5), 0, 255).astype(np.uint8)


def tilted_poses(board, n: int, seed: int = 7, tilt=(15.0, 50.0), distance: float = 900.0):
    """n board poses tilted tilt[0] .. tilt[1] degrees in random directions, facing the camera"""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        R, t = bu.board_pose_facing(board, float(rng.uniform(*tilt)), float(rng.uniform(0, 360)), float(rng.uniform(-20, 20)), distance,
                                    offset_px=(float(rng.uniform(-120, 120)), float(rng.uniform(-60, 60))))
        out.append((R, t))
    return out
