"""Camera rig calibration on the device (a3_calibrate_rigs): where the cameras of a rig sit relative to each other, from what they
saw of one planar target at the same instants -- and, with a calibrated rig, one board pose per instant from all cameras at once.

Not part of the reference: an extension whose algorithm include/aruco3_hip.h fixes to the bit (OpenCV's stereoCalibrate with
CALIB_FIX_INTRINSIC for any number of cameras: per-observation poses, a start over the co-visibility graph, then a Levenberg-Marquardt
bundle over the extrinsics and one board pose per frame, in f64, one workgroup per rig).  Intrinsics are known: calibrate every camera
first (aruco3_amd.calibration).  The rig frame is the first camera's; extrinsics are rig -> camera, frame poses board -> rig."""
from dataclasses import dataclass, field
from typing import List, NamedTuple, Optional, Sequence

import numpy as np

from . import _lib, _solver
from . import calibration as _cal


@dataclass
class RigFrameResult:
    """one instant (a3_rig_frame): status RIG_FRAME_USED / _UNUSED (no usable observation); the pose board -> rig"""
    status: int
    obs_used: int
    points_used: int
    rms_px: float
    rotation: np.ndarray      # 3x3 float64
    translation: np.ndarray   # 3 float64, board units

    @property
    def used(self) -> bool:
        return self.status == _lib.RIG_FRAME_USED


@dataclass
class RigObservationResult:
    """one camera's view of one instant: status RIG_OBS_USED / _TOO_FEW_POINTS (< 4) / _DEGENERATE"""
    camera: int
    frame: int
    status: int
    points: int
    rms_px: float

    @property
    def used(self) -> bool:
        return self.status == _lib.RIG_OBS_USED


@dataclass
class RigCalibration:
    """one rig (a3_rig_result and its camera records).  status RIG_OK, or RIG_NOT_CONNECTED (a camera shares no instant with the rest) /
    RIG_NOT_FINITE with zeros elsewhere."""
    status: int
    cameras: np.ndarray       # float64 (C, 12): the intrinsics the solve was given
    rotations: np.ndarray     # float64 (C, 3, 3), rig -> camera; the first is the identity
    translations: np.ndarray  # float64 (C, 3), board units
    std_devs: np.ndarray      # float64 (C, 6): of (w, t), w the Cayley increment at the solution; 0 for the first camera
    camera_rms_px: np.ndarray
    rms_px: float
    iterations: int
    converged: bool
    frames_used: int
    obs_used: int
    points_used: int
    frames: List[RigFrameResult] = field(default_factory=list)
    observations: List[RigObservationResult] = field(default_factory=list)
    inliers: Optional[List[np.ndarray]] = None   # with outlier_passes: per observation, the points the last solve used (bool)

    @property
    def ok(self) -> bool:
        return self.status == _lib.RIG_OK

    def extrinsics(self, camera: int):
        """(R, t) rig -> camera"""
        return self.rotations[camera], self.translations[camera]

    def camera_pose(self, camera: int, frame: int):
        """(R, t) board -> camera at a USED frame: E_c . T_f"""
        R, t = self.extrinsics(camera)
        f = self.frames[frame]
        return R @ f.rotation, R @ f.translation + t


def camera_params(camera) -> np.ndarray:
    """the 12 values fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6 of a Calibration, a CameraIntrinsics (its distortion, if any) or a sequence"""
    if hasattr(camera, "params"):
        return np.asarray(camera.params, np.float64).reshape(12)
    if hasattr(camera, "focal_x"):
        d = camera.distortion
        lens = d.rational_coefficients("a rig or map solve") if d is not None else [0.0] * 8
        return np.array([camera.focal_x, camera.focal_y, camera.principal_x, camera.principal_y] + lens, np.float64)
    return np.asarray(camera, np.float64).reshape(12)


def _solve(*args):
    return _solver.call("calibrate_rigs", *args)


def calibrate_rigs(problems: Sequence[dict]) -> List[RigCalibration]:
    """Several rigs in one launch.  Each problem is a dict of calibrate_rig's arguments: cameras, observations and optionally guess,
    fix_extrinsics, max_iterations, n_frames."""
    n = len(problems)
    params = [np.stack([camera_params(c) for c in pr["cameras"]]) for pr in problems]
    rigs = (_lib.Rig * max(n, 1))()
    cams = (_lib.RigCamera * max(sum(len(p) for p in params), 1))()
    obs = (_lib.RigObservation * max(sum(len(pr["observations"]) for pr in problems), 1))()
    obj, img, spans = [], [], []
    c0 = f0 = o0 = p0 = 0
    for r, (pr, a) in enumerate(zip(problems, params)):
        o, i = _cal._views([ob[2] for ob in pr["observations"]], [ob[3] for ob in pr["observations"]])
        frames = [int(ob[1]) for ob in pr["observations"]]
        F = int(pr.get("n_frames") or (max(frames) + 1 if frames else 1))
        if not 2 <= len(a) <= _lib.RIG_MAX_CAMERAS:
            raise ValueError(f"a rig has 2 .. {_lib.RIG_MAX_CAMERAS} cameras")
        pairs = [(int(ob[0]), int(ob[1])) for ob in pr["observations"]]
        if any(not (0 <= c < len(a) and 0 <= f < F) for c, f in pairs):
            raise ValueError("an observation names a camera or a frame outside the rig")
        if len(set(pairs)) != len(pairs):
            raise ValueError("two observations of one (camera, frame)")
        guess = pr.get("guess")
        fix = bool(pr.get("fix_extrinsics", False))
        if fix and guess is None:
            raise ValueError("fix_extrinsics needs the extrinsics (guess)")
        flags = (_lib.RIG_USE_EXTRINSIC_GUESS if guess is not None else 0) | (_lib.RIG_FIX_EXTRINSICS if fix else 0)
        rigs[r] = _lib.Rig(c0, len(a), f0, F, o0, len(o), flags, int(pr.get("max_iterations") or 0))
        for c in range(len(a)):
            cams[c0 + c].a[:] = [float(v) for v in a[c]]
            _solver.set_pose(cams[c0 + c], guess[c] if guess is not None else (np.eye(3), np.zeros(3)), "guess_")
        for j, ob in enumerate(pr["observations"]):
            obs[o0 + j] = _lib.RigObservation(c0 + int(ob[0]), f0 + int(ob[1]), p0, len(o[j]))
            p0 += len(o[j])
        obj += o
        img += i
        spans.append((c0, len(a), f0, F, o0, len(o)))
        c0, f0, o0 = c0 + len(a), f0 + F, o0 + len(o)
    res, cres, frames, ores = _solve(rigs, cams, obs, _solver.cat_points(obj), _solver.cat_points(img))
    out = []
    for r, (cc, C_, ff, F, oo, NO) in enumerate(spans):
        cr = [cres[cc + c] for c in range(C_)]
        fr = [RigFrameResult(int(f.status), int(f.obs_used), int(f.points_used), float(f.rms_px), *_solver.get_pose(f))
              for f in (frames[ff + j] for j in range(F))]
        ob = [RigObservationResult(int(obs[oo + j].camera) - cc, int(obs[oo + j].frame) - ff, int(ores[oo + j].status), int(ores[oo + j].points),
                                   float(ores[oo + j].rms_px)) for j in range(NO)]
        out.append(RigCalibration(int(res[r].status), params[r], np.array([list(c.rotation) for c in cr], np.float64).reshape(C_, 3, 3),
                                  np.array([list(c.translation) for c in cr], np.float64), np.array([list(c.std_dev) for c in cr], np.float64),
                                  np.array([c.rms_px for c in cr], np.float64), float(res[r].rms_px), int(res[r].iterations),
                                  bool(res[r].converged), int(res[r].frames_used), int(res[r].obs_used), int(res[r].points_used), fr, ob))
    return out


def calibrate_rig(cameras, observations, *, guess=None, fix_extrinsics=False, max_iterations: Optional[int] = None,
                  n_frames: Optional[int] = None, outlier_passes: int = 0) -> RigCalibration:
    """The extrinsics of one rig.  cameras: per camera a Calibration, a CameraIntrinsics or the 12 values fx .. k6; observations: tuples
    (camera, frame, object_points, image_points) -- what that camera saw of the board at that instant, points as for calibrate_camera;
    cameras need not see the same points, nor every instant.  guess: per camera (R, t) rig -> camera to start from; fix_extrinsics: keep
    them and solve only the board pose of every instant, from all its observations at once.

    outlier_passes = k solves k more times, each time without the correspondences of a used observation that reproject farther than
    max(1 px, 3 x that observation's median) from the previous solution (calibrate_camera's rule); `RigCalibration.inliers` then says
    which points of each observation the last solve used."""
    kw = dict(cameras=cameras, guess=guess, fix_extrinsics=fix_extrinsics, max_iterations=max_iterations, n_frames=n_frames)
    head = [(int(ob[0]), int(ob[1])) for ob in observations]
    obj, img = _cal._views([ob[2] for ob in observations], [ob[3] for ob in observations])
    if n_frames is None:
        kw["n_frames"] = max([f for _, f in head], default=0) + 1

    def residuals(rig, j, k):
        r = rig.observations[j]
        if not r.used:
            return None
        R, t = rig.camera_pose(r.camera, r.frame)
        return np.linalg.norm(_cal.reproject(rig.cameras[r.camera], R, t, obj[j][k]) - img[j][k], axis=1)

    return _solver.solve_with_outlier_passes(
        [len(o) for o in obj], lambda keep: calibrate_rigs([dict(observations=[(c, f, o[k], i[k]) for (c, f), o, i, k in zip(head, obj, img, keep)],
                                                                 **kw)])[0], residuals, outlier_passes)


def _board_observations(board, detections_per_camera):
    n = {len(d) for d in detections_per_camera}
    if len(n) != 1:
        raise ValueError("every camera needs one detection per instant (entry k of every list is the same instant)")
    return [(c, f, *_cal.board_correspondences(board, d)) for c, dets in enumerate(detections_per_camera) for f, d in enumerate(dets)], n.pop()


def calibrate_rig_board(board, detections_per_camera, calibrations, **kw) -> RigCalibration:
    """One list of Detections per camera (entry k of every list is the same instant), from the marker corners of `board` (a Board /
    GridBoard); calibrations: per camera as calibrate_rig's cameras; keywords as calibrate_rig.  Detected corners carry outliers: pass
    outlier_passes=2 as for calibrate_camera_board."""
    obs, n = _board_observations(board, detections_per_camera)
    return calibrate_rig(calibrations, obs, n_frames=n, **kw)


def calibrate_rig_charuco(board, views_per_camera, calibrations, **kw) -> RigCalibration:
    """One list of views per camera (entry k the same instant): Detections (charuco_ids / charuco_corners) or (ids, corners) pairs of a
    CharucoBoard; keywords as calibrate_rig"""
    obs = [(c, f, *_solver.charuco_view(board, v)) for c, views in enumerate(views_per_camera) for f, v in enumerate(views)]
    return calibrate_rig(calibrations, obs, n_frames=len(views_per_camera[0]), **kw)


class Stereo(NamedTuple):
    """cv::stereoCalibrate's outputs: camera 1 -> camera 2 (R, T), the essential and the fundamental matrix, and the rig behind them"""
    rms_px: float
    R: np.ndarray
    T: np.ndarray
    E: np.ndarray
    F: np.ndarray
    rig: RigCalibration


def stereo_calibrate(object_points, image_points1, image_points2, camera1, camera2, **kw) -> Stereo:
    """cv::stereoCalibrate with CALIB_FIX_INTRINSIC for a planar target: per instant the board points and what each of the two
    calibrated cameras saw of them (an instant's lists may differ per camera: pass object_points as a pair of lists then).
    E = [T]x R and F = K2^-T E K1^-1 are computed on the host from the solved (R, T)."""
    o1, o2 = object_points if isinstance(object_points, tuple) else (object_points, object_points)
    obs = [(0, f, o, i) for f, (o, i) in enumerate(zip(o1, image_points1))] + [(1, f, o, i) for f, (o, i) in enumerate(zip(o2, image_points2))]
    rig = calibrate_rig([camera1, camera2], obs, n_frames=len(image_points1), **kw)
    R, T = rig.extrinsics(1)
    Tx = np.array([[0.0, -T[2], T[1]], [T[2], 0.0, -T[0]], [-T[1], T[0], 0.0]])
    E = Tx @ R
    K = [np.array([[a[0], 0.0, a[2]], [0.0, a[1], a[3]], [0.0, 0.0, 1.0]]) for a in rig.cameras]
    Fm = np.linalg.inv(K[1]).T @ E @ np.linalg.inv(K[0])
    if Fm[2, 2] != 0.0:
        Fm = Fm / Fm[2, 2]
    return Stereo(rig.rms_px, R.copy(), T.copy(), E, Fm, rig)


def rig_board_poses(rig: RigCalibration, board, detections_per_camera) -> List[RigFrameResult]:
    """With a calibrated rig: one board pose (board -> rig) per instant from the board markers every camera detected, all cameras in one
    least-squares fit -- the multi-camera counterpart of the Detector's board pose"""
    obs, n = _board_observations(board, detections_per_camera)
    fixed = calibrate_rig(rig.cameras, obs, guess=[rig.extrinsics(c) for c in range(len(rig.cameras))], fix_extrinsics=True, n_frames=n)
    return fixed.frames
