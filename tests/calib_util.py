"""Calibration problems with a known answer: views of a planar target at random tilted poses, projected in f64 through the contract's
forward model (tests/calib_oracle.c) with known intrinsics and lens, rounded to f32 image points.  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

from aruco3_amd import _lib as A
from aruco3_amd.board import CharucoBoard, GridBoard
from tests import board_util as bu
from tests import calib_oracle as co

W720, H720 = 1280, 720
K720 = (900.0, 905.0, 641.5, 357.25)          # fx, fy, cx, cy
WEBCAM = (-0.28, 0.09, 1e-3, -5e-4, 0.0, 0.0, 0.0, 0.0)
WEBCAM5 = (-0.28, 0.09, 1e-3, -5e-4, -0.012, 0.0, 0.0, 0.0)
RATIONAL = (2.1, 0.8, 4e-4, -3e-4, 0.02, 2.4, 1.3, 0.11)


def target_points(kind: str) -> np.ndarray:
    """board points (n, 2): 'charuco' -- the 24 inner corners of a 5 x 7 ChArUco board, 'grid' -- the 140 marker corners of a 5 x 7
    GridBoard, 'dense' -- 4096 points"""
    if kind == "charuco":
        return CharucoBoard(5, 7, 40.0, 30.0).chessboard_corners.astype(np.float64)
    if kind == "dense":      # A3_CALIB_MAX_POINTS points: a 64 x 64 dot grid
        g = np.mgrid[0:64, 0:64].reshape(2, -1).T.astype(np.float64)
        return np.stack([g[:, 1] * 3.0, -g[:, 0] * 3.0], axis=1)
    return GridBoard(5, 7, 30.0, 6.0).corners.reshape(-1, 2).astype(np.float64)


def random_poses(pts, n, rng, K=K720, size=(W720, H720), coeffs=WEBCAM, tilt=(15.0, 45.0), margin=10.0):
    """n board -> camera poses (R, t) that keep every point of `pts` inside the image (with `margin` px) through K and the lens"""
    a = list(K) + list(coeffs)
    c = pts.mean(axis=0)
    ext = float(np.max(np.linalg.norm(pts - c, axis=1)))
    out = []
    while len(out) < n:
        dist = ext * K[0] / rng.uniform(180.0, 330.0)
        off = (rng.uniform(-0.25, 0.25) * size[0], rng.uniform(-0.25, 0.25) * size[1])
        R, t = bu.board_pose_facing(type("B", (), {"corners": pts.reshape(-1, 1, 2)})(), rng.uniform(*tilt), rng.uniform(0, 360),
                                    rng.uniform(-30, 30), dist, off, K=K)
        uv = co.project(a, R, t, pts)
        if np.all(np.isfinite(uv)) and np.all(uv >= margin) and np.all(uv[:, 0] <= size[0] - 1 - margin) and np.all(uv[:, 1] <= size[1] - 1 - margin):
            out.append((R, t))
    return out


def problem(kind="charuco", n_views=25, seed=0, K=K720, coeffs=WEBCAM, noise=0.0, size=(W720, H720), tilt=(15.0, 45.0)):
    """-> dict(obj (N, 2) f32, img (N, 2) f32, offsets (n_views + 1), poses, truth (12,), size)"""
    rng = np.random.default_rng(seed)
    pts = target_points(kind)
    poses = random_poses(pts, n_views, rng, K, size, coeffs, tilt)
    a = np.array(list(K) + list(coeffs), np.float64)
    obj, img = [], []
    for R, t in poses:
        uv = co.project(a, R, t, pts)
        if noise:
            uv = uv + rng.normal(0.0, noise, uv.shape)
        obj.append(pts.astype(np.float32))
        img.append(uv.astype(np.float32))
    offsets = np.concatenate([[0], np.cumsum([len(o) for o in obj])]).astype(np.uint32)
    return dict(obj=np.concatenate(obj), img=np.concatenate(img), offsets=offsets, poses=poses, truth=a, size=size)


def cameras(specs):
    """specs: list of dict(size, first_view, n_views, flags=0, max_iterations=0, guess=None (12 values)) -> CalibCamera array"""
    cams = (A.CalibCamera * len(specs))()
    for c, s in zip(cams, specs):
        c.image_width, c.image_height = s["size"]
        c.first_view, c.n_views = s["first_view"], s["n_views"]
        c.flags = s.get("flags", 0)
        c.max_iterations = s.get("max_iterations", 0)
        g = s.get("guess")
        if g is not None:
            c.guess = A.Intrinsics(s["size"][0], s["size"][1], *[float(v) for v in g[:4]])
            c.guess_distortion = A.DistortionRec(A.DIST_RATIONAL, 20, *[float(v) for v in g[4:12]], 0.1)
    return cams


def one_camera(p, flags=0, guess=None, max_iterations=0):
    return cameras([dict(size=p["size"], first_view=0, n_views=len(p["offsets"]) - 1, flags=flags, guess=guess, max_iterations=max_iterations)])


def params(res) -> np.ndarray:
    """the 12 solved values of a CalibResult, fx fy cx cy k1 .. k6"""
    return np.array([res.fx, res.fy, res.cx, res.cy] + list(res.dist), np.float64)


def rotation_error_deg(Ra, Rb) -> float:
    c = (np.trace(np.asarray(Ra, np.float64) @ np.asarray(Rb, np.float64).T) - 1.0) / 2.0
    return math.degrees(math.acos(max(-1.0, min(1.0, c))))
