"""The cases of tests/test_gpu_rectified_detection.py and their CPU expectations, shared with tests/test_rectified_detection.py, which
checks on the CPU that no expectation is empty.  A case is a camera with a lens, a rectified view of it and a few frames of a grid
board rendered THROUGH the lens on the host (tests/lens_util.py, tests/fisheye_util.py); its expectation is the CPU pipeline
tests/rectify_oracle.py (tests/fisheye_oracle.py for the fisheye model) -> numpy luma -> oracle.a3oracle on the rectified frames.
Nothing here comes from the library under test.  TEST INFRASTRUCTURE ONLY."""
import functools
from dataclasses import dataclass
from typing import Optional, Tuple

import numpy as np

from tests import board_util as bu
from tests import fisheye_oracle as fo
from tests import fisheye_util as fu
from tests import lens_util as lu
from tests import rectify_oracle as ro

SRC_SIZE = (480, 360)
SRC_K = (340.0, 340.0, 240.0, 180.0)
EDGE_PX = 8   # "near the view's edge": a marker corner at most this far from it


@dataclass(frozen=True)
class Case:
    model: str                       # "none", "rational", "fisheye"
    coeffs: Optional[Tuple[float, ...]]   # k1 k2 p1 p2 k3 k4 k5 k6, or cv::fisheye's k1 k2 k3 k4
    view_K: Tuple[float, float, float, float]
    view_size: Tuple[int, int]
    rot_deg: float                   # the view's rotation about y against the camera
    fill: int
    # per frame: tilt, tilt direction, roll (degrees), distance (mm), offset of the board's centre from the VIEW's principal point (px)
    poses: Tuple[Tuple[float, float, float, float, Tuple[float, float]], ...]


CASES = {
    # no lens, a view turned by 4 degrees and smaller than the source
    "none_rotated_smaller": Case("none", None, (300.0, 300.0, 200.0, 150.0), (400, 300), 4.0, 0,
                                 ((0.0, 0.0, 0.0, 200.0, (-20.0, -94.0)), (25.0, 40.0, 10.0, 230.0, (40.0, 20.0)), (0.0, 0.0, 0.0, 200.0, (20.0, 93.0)))),
    # a wide webcam lens, undistorted at the camera's own focal length
    "rational": Case("rational", lu.WEBCAM, SRC_K, SRC_SIZE, 0.0, 0,
                     ((0.0, 0.0, 0.0, 230.0, (-158.0, 0.0)), (30.0, 120.0, -15.0, 250.0, (60.0, -40.0)), (0.0, 0.0, 0.0, 230.0, (30.0, 122.0)))),
    # a fisheye lens, rectified to a slightly longer view
    "fisheye": Case("fisheye", fu.MILD, (360.0, 360.0, 240.0, 180.0), SRC_SIZE, 0.0, 31,
                    ((0.0, 0.0, 0.0, 240.0, (157.0, 0.0)), (20.0, 250.0, 20.0, 260.0, (-50.0, 30.0)), (0.0, 0.0, 0.0, 240.0, (-30.0, -124.0)))),
}


def dictionary():
    from aruco3_amd import ARDictionary

    return ARDictionary.new_from_named_dict("ARUCO")


def board():
    from aruco3_amd.board import GridBoard

    return GridBoard(3, 2, 30.0, 6.0, first_id=10)


def oracle_config():
    """bu.config()'s settings for the oracle detector"""
    from oracle import a3oracle

    return a3oracle.Config(7, 0.05, 0.2, bu.MIN_CORNER_SEPARATION_FACTOR, 49, 1)


def rotation(case: Case) -> np.ndarray:
    return ro.rot_y(case.rot_deg)


def coeffs8(case: Case):
    """the a3_distortion slot order k1 k2 p1 p2 k3 k4 k5 k6"""
    if case.model == "fisheye":
        k1, k2, k3, k4 = case.coeffs
        return (k1, k2, 0.0, 0.0, k3, k4, 0.0, 0.0)
    return tuple(case.coeffs) if case.coeffs is not None else (0.0,) * 8


def tint(grey: np.ndarray) -> np.ndarray:
    """(..., H, W) grey -> (..., H, W, 3) RGB whose three planes differ (a swapped channel order changes the luma)"""
    g = grey.astype(np.float64)
    return np.stack([g, np.clip(0.85 * g + 10.0, 0, 255), np.clip(0.6 * g + 40.0, 0, 255)], axis=-1).round().astype(np.uint8)


def luma(frames: np.ndarray, order: str = "rgb") -> np.ndarray:
    """into_luma8's integers of (..., C) frames: C = 1 the byte, else (2126 R + 7152 G + 722 B) / 10000 truncated, alpha ignored"""
    a = frames.astype(np.uint32)
    if a.shape[-1] == 1:
        return frames[..., 0].copy()
    r, g, b = (a[..., 0], a[..., 1], a[..., 2]) if order == "rgb" else (a[..., 2], a[..., 1], a[..., 0])
    return ((2126 * r + 7152 * g + 722 * b) // 10000).astype(np.uint8)


def oracle_rectify(case: Case, frames: np.ndarray) -> np.ndarray:
    """(N, H, W, C) source frames -> (N, H', W', C) as the contract rectifies them"""
    if case.model == "fisheye":
        return fo.rectify(frames, SRC_K, case.coeffs, case.view_K, case.view_size, rotation(case), case.fill)
    return ro.rectify(frames, SRC_K, case.coeffs, case.view_K, case.view_size, rotation(case), case.fill)


@functools.lru_cache(maxsize=None)
def source_frames(name: str) -> np.ndarray:
    """(N, H, W, 3) RGB frames of the case's camera, and nothing else: rendered once per process"""
    case, d, b = CASES[name], dictionary(), board()
    R_view = rotation(case)
    frames = []
    for tilt, direction, roll, distance, off in case.poses:
        R, t = bu.board_pose_facing(b, tilt, direction, roll, distance, off, K=case.view_K)   # board -> view
        Rc, tc = R_view.T @ R, R_view.T @ t                                                     # board -> camera
        if case.model == "fisheye":
            g = fu.render(b, d, Rc, tc, k=case.coeffs, K=SRC_K, width=SRC_SIZE[0], height=SRC_SIZE[1])
        else:
            g = lu.render(b, d, Rc, tc, k=coeffs8(case), K=SRC_K, width=SRC_SIZE[0], height=SRC_SIZE[1])
        frames.append(g)
    out = tint(np.stack(frames))
    out.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def expectation(name: str):
    """-> (rectified RGB frames (N, H', W', 3), their luma planes (N, H', W'), the oracle detector's result per frame)"""
    from oracle import a3oracle

    case, d = CASES[name], dictionary()
    rect = oracle_rectify(case, source_frames(name))
    grey = luma(rect)
    res = [a3oracle.detect(g, d.code_list, d.num_bits, d._tau, oracle_config(), keep_debug=False) for g in grey]
    rect.setflags(write=False)
    grey.setflags(write=False)
    return rect, grey, res


def intrinsics(case: Case):
    """(the camera with its lens, the view) as aruco3_amd.CameraIntrinsics"""
    from aruco3_amd import CameraIntrinsics, Distortion

    dist = None
    if case.model == "rational":
        dist = Distortion(*case.coeffs)
    elif case.model == "fisheye":
        dist = Distortion.fisheye(*case.coeffs)
    return (CameraIntrinsics(SRC_SIZE[0], SRC_SIZE[1], *SRC_K, distortion=dist), CameraIntrinsics(case.view_size[0], case.view_size[1], *case.view_K))


def rectification(case: Case):
    from aruco3_amd import Rectification

    cam, view = intrinsics(case)
    return Rectification(cam, view, rotation(case), case.fill)
