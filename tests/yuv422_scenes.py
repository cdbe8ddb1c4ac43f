"""The frames of tests/test_gpu_yuv422_pipeline.py: four 320 x 240 views of a GridBoard and four of a CharucoBoard, large enough in the
frame that detection on planes reduced by 2, 3 and 4 and on a rectified view still finds markers.  The GPU test draws them with the
library's renderer (board_util.render / charuco_util.render); `host_luma` draws the same poses on the host, so that
tests/test_yuv422_scenes.py can check with the CPU oracle, on any machine, that no comparison of the GPU test is one of empty lists.
TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

from tests import board_util as bu
from tests import charuco_util as cu
from tests import lens_util as lu

W, H = 320, 240
K = (300.0, 300.0, 160.0, 120.0)
SIZE_MM = 40.0
FACTORS = (2, 3, 4)
# the lens of the rectified runs (mild: k1 k2 p1 p2 k3 k4 k5 k6) -- the frames are drawn WITHOUT it; rectifying them bends the board a
# little, which is all the comparison needs (4:2:2 against L8 on the same bytes)
LENS = (-0.08, 0.01, 0.0005, -0.0005, 0.0, 0.0, 0.0, 0.0)
# per frame: tilt, tilt direction, roll (degrees), distance (mm), offset of the board's centre (px)
POSES = ((0.0, 0.0, 0.0, 150.0, (0.0, 0.0)), (0.0, 0.0, 8.0, 160.0, (10.0, -4.0)), (12.0, 30.0, -5.0, 155.0, (-8.0, 6.0)), (0.0, 0.0, 0.0, 170.0, (-20.0, 8.0)))


def dictionary():
    from aruco3_amd import ARDictionary

    return ARDictionary.new_from_named_dict("ARUCO")


def grid_board():
    from aruco3_amd.board import GridBoard

    return GridBoard(2, 2, SIZE_MM, 10.0, first_id=3)


def charuco_board():
    from aruco3_amd.board import CharucoBoard

    return CharucoBoard(3, 3, 36.0, 26.0, first_id=20)


def poses(board):
    return [bu.board_pose_facing(board, tilt, direction, roll, distance, off, K=K) for tilt, direction, roll, distance, off in POSES]


def oracle_config():
    from oracle import a3oracle

    return a3oracle.Config(7, 0.05, 0.2, bu.MIN_CORNER_SEPARATION_FACTOR, 49, 1)


@functools.lru_cache(maxsize=None)
def host_luma(kind: str) -> np.ndarray:
    """(4, H, W) grey frames of the grid ("grid") or the ChArUco board ("charuco") drawn on the host"""
    if kind == "grid":
        b = grid_board()
        out = np.stack([lu.render(b, dictionary(), R, t, k=(0.0,) * 8, K=K, width=W, height=H) for R, t in poses(b)])
    else:
        b = charuco_board()
        out = np.stack([_host_charuco(b, R, t) for R, t in poses(b)])
    out.setflags(write=False)
    return out


def _host_charuco(board, R, t, ss: int = 3) -> np.ndarray:
    """charuco_util.host_grey with the markers' codes painted in: the white cells of every marker WHITE inside its black square"""
    from aruco3_amd import synth

    d = dictionary()
    cells = {int(i): synth.marker_cells(int(d.code_list[int(i)]), d.num_bits) for i in board.ids}
    fx, fy, cx, cy = K
    Hm = np.concatenate([np.asarray(R, np.float64)[:, :2], np.asarray(t, np.float64).reshape(3, 1)], axis=1)   # board (X, Y, 1) -> camera
    inv = np.linalg.inv(np.array([[fx, 0, cx], [0, fy, cy], [0, 0, 1.0]]) @ Hm)
    ys, xs = np.mgrid[0:H, 0:W].astype(np.float64)
    acc = np.zeros((H, W))
    for oy in (np.arange(ss) + 0.5) / ss - 0.5:
        for ox in (np.arange(ss) + 0.5) / ss - 0.5:
            p = np.stack([xs + ox, ys + oy, np.ones_like(xs)], axis=-1) @ inv.T
            X, Y = p[..., 0] / p[..., 2], p[..., 1] / p[..., 2]
            s = board.square_length
            c, r = np.floor(X / s), np.floor(-Y / s)
            inside = (c >= 0) & (c < board.squares_x) & (r >= 0) & (r < board.squares_y)
            v = np.where(inside, np.where((r + c) % 2 == 0, cu.BLACK, cu.WHITE), cu.BACKGROUND)
            for k, mid in enumerate(board.ids):
                q = board.corners[k]          # TL, TR, BR, BL, y up
                n = cells[int(mid)].shape[0]
                side = float(q[1, 0] - q[0, 0])
                u, w_ = (X - q[0, 0]) / side * n, (q[0, 1] - Y) / side * n
                m = (u >= 0) & (u < n) & (w_ >= 0) & (w_ < n)
                ci, ri = np.clip(np.floor(u), 0, n - 1).astype(int), np.clip(np.floor(w_), 0, n - 1).astype(int)
                v = np.where(m, np.where(cells[int(mid)][ri, ci] != 0, cu.WHITE, cu.BLACK), v)
            acc += v
    return np.clip(np.floor(acc / (ss * ss) + 0.5), 0, 255).astype(np.uint8)


def device_luma(kind: str) -> np.ndarray:
    """(4, H, W) grey frames drawn by the library's renderer (needs the GPU): into_luma8 of its RGB frames"""
    from tests import rectified_cases as rc

    d = dictionary()
    if kind == "grid":
        b = grid_board()
        dev = bu.render([bu.board_scene(b, R, t, K) for R, t in poses(b)], d, W, H)
    else:
        b = charuco_board()
        dev = cu.render([cu.Scene(b, R, t, K=K) for R, t in poses(b)], d, W, H)
    return np.ascontiguousarray(rc.luma(dev.cpu().numpy()))
