"""What the solver front ends (calibration, rig, handeye, markermap) and pinhole.undistort_points share: the one context their device
calls run on, the packing of points and poses into the library's records, the ChArUco view unpacking and the outlier passes."""
import threading

import numpy as np

from . import _lib

_ctx = None
_lock = threading.Lock()   # one context (one stream, one set of buffers) serves every thread: calls take turns


def call(method: str, *args):
    """Context.<method>(*args) on the shared context, created by the first call"""
    global _ctx
    with _lock:
        if _ctx is None:
            _ctx = _lib.Context(_lib.default_config(), np.zeros(1, np.uint64), 64, 1)
        return getattr(_ctx, method)(*args)


def cat_points(lists) -> np.ndarray:
    """per-view (n, 2) arrays as one; none: an empty (0, 2) float32 array"""
    return np.concatenate(lists) if lists else np.zeros((0, 2), np.float32)


def set_pose(record, pose, prefix: str = "") -> None:
    """(R, t) into a record's <prefix>rotation[9] / <prefix>translation[3]"""
    getattr(record, prefix + "rotation")[:] = [float(v) for v in np.asarray(pose[0], np.float64).reshape(9)]
    getattr(record, prefix + "translation")[:] = [float(v) for v in np.asarray(pose[1], np.float64).reshape(3)]


def get_pose(record, prefix: str = ""):
    """a record's <prefix>rotation / <prefix>translation as (3x3 float64, 3 float64)"""
    return np.array(getattr(record, prefix + "rotation"), np.float64).reshape(3, 3), np.array(getattr(record, prefix + "translation"), np.float64)


def charuco_view(board, view):
    """a Detection (its charuco_ids / charuco_corners) or an (ids, corners) pair of a CharucoBoard, None meaning no corner ->
    (object (n, 2), image (n, 2)) float32"""
    ids, corners = (view.charuco_ids, view.charuco_corners) if hasattr(view, "charuco_ids") else view
    ids = np.zeros(0, np.int64) if ids is None else np.asarray(ids, np.int64).reshape(-1)
    corners = np.zeros((0, 2), np.float32) if corners is None else np.asarray(corners, np.float32).reshape(-1, 2)
    return board.chessboard_corners[ids].astype(np.float32), corners


def outlier_limit(errors) -> float:
    """an error counts as an inlier's below max(1 px, 3 x the median)"""
    return max(1.0, 3.0 * float(np.median(errors)))


def solve_with_outlier_passes(sizes, solve, residuals, passes):
    """solve(keep) -- keep: one bool mask per unit (view, observation, frame) of sizes[j] points -- and then `passes` more times, each
    time without the points whose residual is not below outlier_limit of their unit.  residuals(solution, j, keep[j]): the errors of
    unit j's kept points under the solution, or None when the solve did not use unit j.  With passes, solution.inliers = keep."""
    keep = [np.ones(n, bool) for n in sizes]
    solution = solve(keep)
    for _ in range(int(passes)):
        if not solution.ok:
            break
        for j, k in enumerate(keep):
            e = residuals(solution, j, k)
            if e is not None:
                k[np.nonzero(k)[0][~(e < outlier_limit(e))]] = False
        solution = solve(keep)
    if passes:
        solution.inliers = keep
    return solution
