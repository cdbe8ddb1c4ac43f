"""Camera calibration on the device (a3_calibrate_cameras, a3_calibrate_fisheye_cameras): intrinsics and OpenCV's lens model -- the
rational one or cv::fisheye's -- from views of a planar target.

Not part of the reference: an extension whose algorithm include/aruco3_hip.h fixes to the bit (Zhang's initialisation, then a
Levenberg-Marquardt bundle over intrinsics, lens model and per-view poses, in f64, one workgroup per camera).  The result's
`intrinsics` is a `CameraIntrinsics` whose `distortion` is set, ready for `Detector.detect_batch_with_pose` and the board / ChArUco pose
calls.  Views are lists of correspondences: board points (x, y) in board units on z = 0, image points in pixels.

The fisheye solve (`calibrate_camera_fisheye`, or model="fisheye" on the board helpers) is cv::fisheye::calibrate for planar targets:
fx fy cx cy and D = (k1 k2 k3 k4), a kernel and a bit-exact contract of its own; its result's `intrinsics.distortion` is a fisheye
`Distortion`, ready for `rectify_frames`, `undistort_points` and the pose calls."""
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _lib, _solver
from .pinhole import CameraIntrinsics, Distortion

PARAM_NAMES = ("fx", "fy", "cx", "cy", "k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6")
FISHEYE_PARAM_INDEX = (0, 1, 2, 3, 4, 5, 8, 9)   # where a fisheye solve's fx fy cx cy k1 k2 k3 k4 sit in `params` / `std_devs`


@dataclass
class ViewResult:
    """one view (a3_calib_view): status CALIB_VIEW_USED / _TOO_FEW_POINTS (< 4) / _DEGENERATE; the pose board -> camera"""
    status: int
    points: int
    rms_px: float
    rotation: np.ndarray      # 3x3 float32
    translation: np.ndarray   # 3 float32, board units

    @property
    def used(self) -> bool:
        return self.status == _lib.CALIB_VIEW_USED


@dataclass
class Calibration:
    """one camera (a3_calib_result).  status CALIB_OK, or CALIB_TOO_FEW / _NO_INIT / _NOT_FINITE with zeros elsewhere.  `model` says
    which solve made it; a fisheye result keeps a3_distortion's field order in `params` and `std_devs` (k1 k2 0 0 k3 k4 0 0)."""
    status: int
    intrinsics: Optional[CameraIntrinsics]
    params: np.ndarray        # float64 (12,): fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6
    std_devs: np.ndarray      # float64 (12,), same order; 0 for fixed parameters, +inf where the problem is not observable
    rms_px: float
    iterations: int
    converged: bool
    views_used: int
    points_used: int
    views: List[ViewResult] = field(default_factory=list)
    inliers: Optional[List[np.ndarray]] = None   # with outlier_passes: per view, the points the last solve used (bool)
    model: str = "rational"                      # or "fisheye"

    @property
    def ok(self) -> bool:
        return self.status == _lib.CALIB_OK

    @property
    def distortion_coeffs(self) -> np.ndarray:
        """OpenCV's distCoeffs order: k1 k2 p1 p2 k3 k4 k5 k6; for a fisheye result cv::fisheye's D = (k1 k2 k3 k4)"""
        if self.model == "fisheye":
            return self.params[[4, 5, 8, 9]].copy()
        return self.params[4:].copy()

    @classmethod
    def _from(cls, r, views, model: str = "rational") -> "Calibration":
        p = np.array([r.fx, r.fy, r.cx, r.cy] + list(r.dist), np.float64)
        intr = None
        if r.status == _lib.CALIB_OK:
            d = r.distortion
            intr = CameraIntrinsics(r.intrinsics.image_width, r.intrinsics.image_height, r.intrinsics.focal_x, r.intrinsics.focal_y,
                                    r.intrinsics.principal_x, r.intrinsics.principal_y,
                                    distortion=Distortion(d.k1, d.k2, d.p1, d.p2, d.k3, d.k4, d.k5, d.k6, int(d.iterations), d.max_residual_px,
                                                          model=model))
        vr = [ViewResult(int(v.status), int(v.points), float(v.rms_px), np.array(v.rotation, np.float32).reshape(3, 3),
                         np.array(v.translation, np.float32)) for v in views]
        return cls(int(r.status), intr, p, np.array(r.std_dev, np.float64), float(r.rms_px), int(r.iterations), bool(r.converged),
                   int(r.views_used), int(r.points_used), vr, model=model)


def _flags(pr) -> int:
    return ((_lib.CALIB_FIX_PRINCIPAL_POINT if pr.get("fix_principal_point") else 0) | (_lib.CALIB_ZERO_TANGENT_DIST if pr.get("zero_tangent") else 0) |
            (_lib.CALIB_FIX_K3 if pr.get("fix_k3") else 0) | (_lib.CALIB_RATIONAL_MODEL if pr.get("rational") else 0) |
            (_lib.CALIB_USE_INTRINSIC_GUESS if pr.get("guess") is not None else 0))


def _fisheye_flags(pr) -> int:
    return ((_lib.FISHEYE_FIX_PRINCIPAL_POINT if pr.get("fix_principal_point") else 0) | (_lib.FISHEYE_FIX_K1 if pr.get("fix_k1") else 0) |
            (_lib.FISHEYE_FIX_K2 if pr.get("fix_k2") else 0) | (_lib.FISHEYE_FIX_K3 if pr.get("fix_k3") else 0) |
            (_lib.FISHEYE_FIX_K4 if pr.get("fix_k4") else 0) | (_lib.FISHEYE_USE_INTRINSIC_GUESS if pr.get("guess") is not None else 0))


def _rational_lens(d: Distortion) -> None:
    d.rational_coefficients("a calibration guess")   # (a fisheye lens is refused)


def _fisheye_lens(d: Distortion) -> None:
    if d.model != "fisheye":
        raise ValueError("a fisheye calibration guess takes a fisheye Distortion (Distortion.fisheye) or none, not rational lens coefficients")


def _views(object_points, image_points):
    if len(object_points) != len(image_points):
        raise ValueError("one list of object points per list of image points")
    obj, img = [], []
    for o, i in zip(object_points, image_points):
        o = np.asarray(o, np.float64).reshape(-1, np.asarray(o).shape[-1] if np.asarray(o).size else 2)
        if o.shape[1] == 3:
            if np.any(o[:, 2] != 0):
                raise ValueError("object points must lie on the plane z = 0")
            o = o[:, :2]
        i = np.asarray(i, np.float32).reshape(-1, 2)
        if o.shape[0] != i.shape[0]:
            raise ValueError("a view has different numbers of object and image points")
        obj.append(o.astype(np.float32))
        img.append(i)
    return obj, img


def _calibrate(cams, offsets, obj, img, fisheye: bool = False):
    return _solver.call("calibrate_fisheye_cameras" if fisheye else "calibrate_cameras", cams, offsets, obj, img)


def reproject(params, rotation, translation, object_points, model: str = "rational") -> np.ndarray:
    """board points (n, 2) through the camera `params` (fx fy cx cy k1 .. k6, a Calibration's) at pose (rotation, translation) -> pixels
    (n, 2), float64: the forward model of the calibration (`model`: the rational lens or the fisheye one), evaluated on the host"""
    a = np.asarray(params, np.float64)
    o = np.asarray(object_points, np.float64).reshape(-1, 2)
    P = o @ np.asarray(rotation, np.float64).reshape(3, 3)[:, :2].T + np.asarray(translation, np.float64).reshape(3)
    xd = Distortion(*[float(v) for v in a[4:12]], model=model).distort_normalized(P[:, :2] / P[:, 2:3])
    return xd * a[[0, 1]] + a[[2, 3]]


def _calibrate_cameras(problems, model, flags, check_lens, default_lens) -> List[Calibration]:
    """calibrate_cameras for either lens model: `flags` reads a problem's, `check_lens` refuses a guess's lens of the other model and
    `default_lens` stands in for a guess without one"""
    specs, obj, img = [], [], []
    for pr in problems:
        o, i = _views(pr["object_points"], pr["image_points"])
        specs.append((pr, len(obj), len(o)))
        obj += o
        img += i
    cams = (_lib.CalibCamera * max(len(specs), 1))()
    for c, (pr, first, n) in zip(cams, specs):
        w, h = pr["image_size"]
        c.image_width, c.image_height, c.first_view, c.n_views = int(w), int(h), first, n
        c.flags = flags(pr)
        c.max_iterations = int(pr.get("max_iterations") or 0)
        guess = pr.get("guess")
        if guess is not None:
            if guess.distortion is not None:
                check_lens(guess.distortion)
            c.guess = guess._c()
            c.guess_distortion = (guess.distortion or default_lens())._c()
    offsets = np.concatenate([[0], np.cumsum([len(o) for o in obj])]).astype(np.uint32)
    res, views = _calibrate(cams, offsets, _solver.cat_points(obj), _solver.cat_points(img), model == "fisheye")
    return [Calibration._from(res[k], [views[first + j] for j in range(n)], model) for k, (_, first, n) in enumerate(specs)]


def calibrate_cameras(problems: Sequence[dict]) -> List[Calibration]:
    """Several cameras in one launch.  Each problem is a dict of calibrate_camera's arguments: object_points, image_points,
    image_size and optionally fix_principal_point, zero_tangent, fix_k3, rational, guess (a CameraIntrinsics, its distortion the
    starting lens), max_iterations."""
    return _calibrate_cameras(problems, "rational", _flags, _rational_lens, Distortion)


def calibrate_camera(object_points, image_points, image_size, *, fix_principal_point=False, zero_tangent=False, fix_k3=False, rational=False,
                     guess: Optional[CameraIntrinsics] = None, max_iterations: Optional[int] = None, outlier_passes: int = 0) -> Calibration:
    """cv::calibrateCamera for a planar target: object_points / image_points are per-view arrays ((n, 2) or (n, 3) with z = 0, and (n, 2)
    pixels); image_size (width, height).  Views with fewer than 4 points are kept (status CALIB_VIEW_TOO_FEW_POINTS) so that view
    indices match the caller's frames.

    The solve is plain least squares: a correspondence that is wrong by pixels pulls every parameter.  outlier_passes = k solves k more
    times, each time without the correspondences of a solved view that reproject farther than max(1 px, 3 x that view's median) from the
    previous solution; `Calibration.inliers` then says which points of each view the last solve used."""
    kw = dict(image_size=image_size, fix_principal_point=fix_principal_point, zero_tangent=zero_tangent, fix_k3=fix_k3, rational=rational,
              guess=guess, max_iterations=max_iterations)
    return _solve_with_outlier_passes(calibrate_cameras, object_points, image_points, kw, outlier_passes)


def _solve_with_outlier_passes(solve, object_points, image_points, kw, outlier_passes) -> Calibration:
    """one camera by `solve` (calibrate_cameras or calibrate_cameras_fisheye), then the outlier passes of calibrate_camera: the
    reprojection runs through the forward model of the solve's own lens"""
    obj, img = _views(object_points, image_points)

    def residuals(cal, j, k):
        v = cal.views[j]
        return np.linalg.norm(reproject(cal.params, v.rotation, v.translation, obj[j][k], cal.model) - img[j][k], axis=1) if v.used else None

    return _solver.solve_with_outlier_passes(
        [len(o) for o in obj], lambda keep: solve([dict(object_points=[o[k] for o, k in zip(obj, keep)],
                                                        image_points=[i[k] for i, k in zip(img, keep)], **kw)])[0], residuals, outlier_passes)


def calibrate_cameras_fisheye(problems: Sequence[dict]) -> List[Calibration]:
    """Several fisheye cameras in one launch (a3_calibrate_fisheye_cameras).  Each problem is a dict of calibrate_camera_fisheye's
    arguments: object_points, image_points, image_size and optionally fix_principal_point, fix_k1 .. fix_k4, guess (a CameraIntrinsics
    without a lens or with a fisheye one), max_iterations."""
    return _calibrate_cameras(problems, "fisheye", _fisheye_flags, _fisheye_lens, Distortion.fisheye)


def calibrate_camera_fisheye(object_points, image_points, image_size, *, fix_principal_point=False, fix_k1=False, fix_k2=False, fix_k3=False,
                             fix_k4=False, guess: Optional[CameraIntrinsics] = None, max_iterations: Optional[int] = None,
                             outlier_passes: int = 0) -> Calibration:
    """cv::fisheye::calibrate for a planar target: fx fy cx cy and D = (k1 k2 k3 k4) of the Kannala-Brandt model; arguments as
    calibrate_camera.  A fixed coefficient stays at the guess's value, or at 0 without a guess.  Without a guess the focal lengths
    start at max(width, height) / pi.  k3 and k4 need points far off the axis (60 degrees and more) to be told apart: fix them for a
    lens or a set of views that does not reach there.  outlier_passes as in calibrate_camera, reprojecting through the fisheye model."""
    kw = dict(image_size=image_size, fix_principal_point=fix_principal_point, fix_k1=fix_k1, fix_k2=fix_k2, fix_k3=fix_k3, fix_k4=fix_k4,
              guess=guess, max_iterations=max_iterations)
    return _solve_with_outlier_passes(calibrate_cameras_fisheye, object_points, image_points, kw, outlier_passes)


def _by_model(model: str):
    if model not in ("rational", "fisheye"):
        raise ValueError(f"model: 'rational' or 'fisheye', not {model!r}")
    return calibrate_camera_fisheye if model == "fisheye" else calibrate_camera


def board_correspondences(board, detection):
    """aruco's calibrateCameraAruco per frame: the corners of the detection's board markers (refined when present), in detection order; an
    id seen more than once in the frame is left out in all its instances (the board pose's rule) -> (object (n, 2), image (n, 2))"""
    ids = [m.id for m in detection.markers]
    slot = {int(i): k for k, i in enumerate(board.ids)}
    obj, img = [], []
    for m in detection.markers:
        k = slot.get(int(m.id))
        if k is None or ids.count(m.id) > 1:
            continue
        obj.append(board.corners[k])
        img.append(np.asarray(m.corners_refined if m.corners_refined is not None else m.corners, np.float32))
    if not obj:
        return np.zeros((0, 2), np.float32), np.zeros((0, 2), np.float32)
    return np.concatenate(obj).astype(np.float32), np.concatenate(img).astype(np.float32)


def calibrate_camera_board(board, detections, image_size, *, model: str = "rational", **kw) -> Calibration:
    """calibrateCameraAruco: one view per Detection, from the marker corners of `board` (a Board / GridBoard); keywords as
    calibrate_camera, or as calibrate_camera_fisheye with model="fisheye".  Detected marker corners carry outliers (a corner whose
    refinement fell back to the integer quad corner is a few pixels off; now and then a marker is misread), which pull a plain solve
    by several pixels: pass outlier_passes=2 to solve again without them."""
    pairs = [board_correspondences(board, d) for d in detections]
    return _by_model(model)([o for o, _ in pairs], [i for _, i in pairs], image_size, **kw)


def calibrate_camera_charuco(board, views, image_size, *, model: str = "rational", **kw) -> Calibration:
    """calibrateCameraCharuco: one view per Detection (its charuco_ids / charuco_corners; None when the frame showed no corner) or
    (ids, corners) pair of a CharucoBoard; keywords as calibrate_camera, or as calibrate_camera_fisheye with model="fisheye" """
    pairs = [_solver.charuco_view(board, v) for v in views]
    return _by_model(model)([o for o, _ in pairs], [i for _, i in pairs], image_size, **kw)
