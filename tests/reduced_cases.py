"""The cases of tests/test_gpu_reduce_frames.py and tests/test_gpu_reduced_detection.py and their CPU expectations, shared with
tests/test_reduced_detection.py, which checks on the CPU that no expectation is empty.  `reduce` restates the a3_reduce_frames contract
in numpy (luma from tests/rectified_cases.luma); a case is one frame of a grid board rendered on the host (tests/lens_util.py, no lens);
its expectation for a factor is oracle.a3oracle on the numpy-reduced plane, the corner map f x + f // 2, and
tests/refine_oracle.refine_markers on the full-size luma from the mapped corners.  Nothing here comes from the library under test.
TEST INFRASTRUCTURE ONLY."""
import functools

import numpy as np

from tests import board_util as bu
from tests import lens_util as lu
from tests import rectified_cases as rc

SIZE = (963, 725)   # no multiple of 2, 3 or 4
K = (680.0, 680.0, 481.0, 362.0)
FACTORS = (2, 3, 4)
EDGE_BLOCKS = 8     # "near the frame's edge": a mapped corner within 8 f px of it

# per case: (board_pose_facing's tilt, direction, roll (degrees), distance (mm), offset of the board's centre (px)), the factors it is used at
CASES = {
    "frontal": ((0.0, 0.0, 0.0, 200.0, (-20.0, -60.0)), (2, 3, 4)),
    "tilted": ((35.0, 200.0, -20.0, 140.0, (-60.0, 50.0)), (2, 3, 4)),
    # (28 px farther out than first proposed: at (-200, -200) no mapped corner came within 8 f px of the edge at any factor, 34 - 38 px)
    "near_corner": ((0.0, 0.0, 0.0, 180.0, (-228.0, -228.0)), (2, 3, 4)),
    "milder_tilt": ((25.0, 40.0, 10.0, 150.0, (40.0, 20.0)), (2, 3)),   # (at 4 the oracle drops a marker)
}

dictionary, board, oracle_config = rc.dictionary, rc.board, rc.oracle_config


def reduce(frames: np.ndarray, f: int, order: str = "rgb") -> np.ndarray:
    """the contract of a3_reduce_frames: (..., H, W, C) uint8 frames, C = 1, 3 or 4 in channel order `order` -> (..., H // f, W // f)
    uint8, (S + f*f // 2) // (f*f) with S the sum of the luma over each f x f block; trailing rows and columns are not read"""
    g = rc.luma(np.asarray(frames), order).astype(np.uint32)
    H, W = g.shape[-2:]
    h, w = H // f, W // f
    blocks = g[..., : h * f, : w * f].reshape(g.shape[:-2] + (h, f, w, f))
    return ((blocks.sum(axis=(-3, -1)) + (f * f) // 2) // (f * f)).astype(np.uint8)


def map_corners(corners, f: int):
    """step 3 of the contract for a list of (x, y)"""
    return [(f * int(x) + f // 2, f * int(y) + f // 2) for x, y in corners]


def cells() -> int:
    return int(np.ceil(np.sqrt(dictionary().num_bits))) + 2


@functools.lru_cache(maxsize=None)
def frame(name: str) -> np.ndarray:
    """(H, W, 3) RGB, rendered once per process"""
    pose, _ = CASES[name]
    tilt, direction, roll, distance, off = pose
    R, t = bu.board_pose_facing(board(), tilt, direction, roll, distance, off, K=K)
    out = rc.tint(lu.render(board(), dictionary(), R, t, k=(0.0,) * 8, K=K, width=SIZE[0], height=SIZE[1]))
    out.setflags(write=False)
    return out


def names(f: int):
    """the cases used at factor f, in the order of their frames"""
    return [n for n, (_, fs) in CASES.items() if f in fs]


@functools.lru_cache(maxsize=None)
def frames(f: int) -> np.ndarray:
    """(N, H, W, 3) RGB: the frames of every case used at factor f"""
    out = np.stack([frame(n) for n in names(f)])
    out.setflags(write=False)
    return out


def bgra(rgb: np.ndarray) -> np.ndarray:
    return np.ascontiguousarray(np.concatenate([rgb[..., ::-1], np.full(rgb.shape[:-1] + (1,), 200, np.uint8)], axis=-1))


@functools.lru_cache(maxsize=None)
def expectation(f: int, threshold_window: int = None):
    """-> (the reduced planes (N, h, w), per frame the oracle's result on its plane with every marker's "corners" mapped to full size
    (the reduced ones kept as "corners_reduced"), per frame the refined corners float32 (n, 4, 2) on the full-size luma)"""
    from oracle import a3oracle
    from tests import refine_oracle as refo

    d = dictionary()
    cfg = oracle_config()
    if threshold_window is not None:
        cfg.threshold_window = threshold_window
    full = frames(f)
    planes = reduce(full, f)
    planes.setflags(write=False)
    res, refined = [], []
    for k, p in enumerate(planes):
        r = a3oracle.detect(p, d.code_list, d.num_bits, d._tau, cfg, keep_debug=False)
        for m in r["markers"]:
            m["corners_reduced"] = m["corners"]
            m["corners"] = map_corners(m["corners"], f)
        res.append(r)
        refined.append(refo.refine_markers(rc.luma(full[k]), [np.array(m["corners"]).reshape(8) for m in r["markers"]], cells()))
    return planes, res, refined
