"""Hand-eye calibration on the device (a3_calibrate_hand_eyes): where a calibrated camera sits on a robot's flange (eye-in-hand), or
where a fixed camera sits relative to the robot's base (eye-to-hand), from what the camera saw of one planar target at known robot
poses.

Not part of the reference: an extension whose algorithm include/aruco3_hip.h fixes to the bit (OpenCV's calibrateHandEye /
calibrateRobotWorldHandEye, minimising the reprojection error: per-frame board poses, a closed-form start over the frame pairs, then
a Levenberg-Marquardt solve over the two unknown transforms, in f64, one workgroup per problem).  The library knows one chain, board
-> camera G_f = X . M_f . Y with M_f known per frame; this module maps the two set-ups onto it:

    eye_in_hand   M_f = (gripper -> base)_f^-1   X = gripper -> camera   Y = board -> base
    eye_to_hand   M_f = (gripper -> base)_f      X = base -> camera      Y = board -> gripper

Robot poses are gripper -> base, as a controller reports them and as cv::calibrateHandEye takes them, with translations in the units
of the board's points.  Intrinsics are known: calibrate the camera first (aruco3_amd.calibration)."""
from dataclasses import dataclass, field
from typing import List, Optional, Sequence

import numpy as np

from . import _lib, _solver
from . import calibration as _cal
from .rig import camera_params

SETUPS = ("eye_in_hand", "eye_to_hand")


@dataclass
class HandEyeFrameResult:
    """one frame (a3_handeye_frame_result): status HANDEYE_FRAME_USED / _TOO_FEW_POINTS (< 4) / _DEGENERATE; the frame's own pose
    board -> camera from its points alone, to see which view disagrees with the solved chain"""
    status: int
    points: int
    rms_px: float
    rotation: np.ndarray      # 3x3 float64
    translation: np.ndarray   # 3 float64, board units

    @property
    def used(self) -> bool:
        return self.status == _lib.HANDEYE_FRAME_USED


def _inv(T):
    return T[0].T, -T[0].T @ T[1]


def _mul(A, B):
    return A[0] @ B[0], A[0] @ B[1] + A[1]


@dataclass
class HandEyeCalibration:
    """one problem (a3_handeye_result).  status HANDEYE_OK, or HANDEYE_TOO_FEW_FRAMES (fewer than 3 usable frames) / HANDEYE_NO_MOTION
    (the robot only translated, or turned about one axis only) / HANDEYE_NOT_FINITE with zeros elsewhere."""
    status: int
    setup: str
    camera: np.ndarray        # float64 (12,): the intrinsics the solve was given
    X: tuple                  # (R, t): gripper -> camera (eye_in_hand) / base -> camera (eye_to_hand)
    Y: tuple                  # (R, t): board -> base (eye_in_hand) / board -> gripper (eye_to_hand)
    std_devs: np.ndarray      # float64 (12,): of (w, t) of X, then of Y; w the Cayley increment at the solution
    rms_px: float
    iterations: int
    converged: bool
    frames_used: int
    points_used: int
    pairs_used: int
    frames: List[HandEyeFrameResult] = field(default_factory=list)
    inliers: Optional[List[np.ndarray]] = None   # with outlier_passes: per frame, the points the last solve used (bool)

    @property
    def ok(self) -> bool:
        return self.status == _lib.HANDEYE_OK

    def _need(self, setup, name):
        if self.setup != setup:
            raise ValueError(f"{name}() belongs to an {setup} calibration; this one is {self.setup}")

    def camera_to_gripper(self):
        """(R, t) camera -> gripper of an eye-in-hand calibration: cv::calibrateHandEye's R_cam2gripper, t_cam2gripper"""
        self._need("eye_in_hand", "camera_to_gripper")
        return _inv(self.X)

    def board_to_base(self):
        """(R, t) board -> base of an eye-in-hand calibration: where the fixed board stands in the cell"""
        self._need("eye_in_hand", "board_to_base")
        return self.Y

    def camera_to_base(self):
        """(R, t) camera -> base of an eye-to-hand calibration"""
        self._need("eye_to_hand", "camera_to_base")
        return _inv(self.X)

    def board_to_gripper(self):
        """(R, t) board -> gripper of an eye-to-hand calibration: how the board is held"""
        self._need("eye_to_hand", "board_to_gripper")
        return self.Y

    def camera_pose_in_base(self, robot_pose=None):
        """(R, t) camera -> base: for an eye-in-hand calibration at the robot pose given (gripper -> base), for an eye-to-hand one the
        fixed camera (robot_pose is not needed)"""
        if self.setup == "eye_to_hand":
            return _inv(self.X)
        if robot_pose is None:
            raise ValueError("an eye-in-hand camera moves with the robot: pass the robot pose (gripper -> base)")
        return _mul(_pose(robot_pose), _inv(self.X))

    def board_pose_in_camera(self, robot_pose):
        """(R, t) board -> camera the solved chain predicts at a robot pose (gripper -> base): X . M . Y"""
        return _mul(self.X, _mul(_robot_to_M(_pose(robot_pose), self.setup), self.Y))


def _pose(p):
    """(R, t) from (R, t) or a 4 x 4 matrix"""
    if isinstance(p, np.ndarray) and p.shape == (4, 4):
        return np.asarray(p[:3, :3], np.float64), np.asarray(p[:3, 3], np.float64)
    R, t = p
    return np.asarray(R, np.float64).reshape(3, 3), np.asarray(t, np.float64).reshape(3)


def _guess(guess):
    """-> (X, Y or None) from (X, Y), (X, None) or X alone, each pose an (R, t) or a 4 x 4 matrix"""
    if isinstance(guess, np.ndarray) and guess.shape == (4, 4):
        return _pose(guess), None
    if len(guess) == 2 and isinstance(guess[0], np.ndarray) and guess[0].shape == (3, 3):
        return _pose(guess), None
    X, Y = guess
    return _pose(X), (None if Y is None else _pose(Y))


def _robot_to_M(pose, setup):
    return _inv(pose) if setup == "eye_in_hand" else pose


def _solve(*args):
    return _solver.call("calibrate_hand_eyes", *args)


def calibrate_hand_eyes(problems: Sequence[dict]) -> List[HandEyeCalibration]:
    """Several problems in one launch.  Each problem is a dict of calibrate_hand_eye's arguments: camera, robot_poses, observations and
    optionally setup, guess, fix_mount, max_iterations."""
    n = len(problems)
    if not 1 <= n <= _lib.HANDEYE_MAX_PROBLEMS:
        raise ValueError(f"1 .. {_lib.HANDEYE_MAX_PROBLEMS} problems per call")
    if sum(len(pr["robot_poses"]) for pr in problems) > _lib.HANDEYE_MAX_CALL_FRAMES:
        raise ValueError(f"at most {_lib.HANDEYE_MAX_CALL_FRAMES} frames per call")
    probs = (_lib.HandEyeProblem * n)()
    frames = (_lib.HandEyeFrame * sum(len(pr["robot_poses"]) for pr in problems))()
    obj, img, spans = [], [], []
    f0 = p0 = 0
    for r, pr in enumerate(problems):
        setup = pr.get("setup", "eye_in_hand")
        if setup not in SETUPS:
            raise ValueError(f"setup is one of {SETUPS}")
        a = camera_params(pr["camera"])
        if not np.all(np.isfinite(a)) or not (a[0] > 0 and a[1] > 0):
            raise ValueError("the camera's intrinsics must be finite, with focal lengths > 0")
        poses = [_pose(p) for p in pr["robot_poses"]]
        F = len(poses)
        if len(pr["observations"]) != F:
            raise ValueError("one observation (object_points, image_points) per robot pose")
        if not 1 <= F <= _lib.HANDEYE_MAX_FRAMES:
            raise ValueError(f"a problem has 1 .. {_lib.HANDEYE_MAX_FRAMES} frames")
        if any(not (np.all(np.isfinite(R)) and np.all(np.isfinite(t))) for R, t in poses):
            raise ValueError("a robot pose is not finite")
        o, i = _cal._views([ob[0] for ob in pr["observations"]], [ob[1] for ob in pr["observations"]])
        if any(len(v) > _lib.CALIB_MAX_POINTS for v in o):
            raise ValueError(f"a frame has at most {_lib.CALIB_MAX_POINTS} points")
        guess, fix = pr.get("guess"), bool(pr.get("fix_mount", False))
        if fix and guess is None:
            raise ValueError("fix_mount needs the mount (guess)")
        gx = gy = (np.eye(3), np.zeros(3))
        flags = _lib.HANDEYE_FIX_X if fix else 0
        if guess is not None:
            gx, y = _guess(guess)
            if y is not None:
                gy = y
                flags |= _lib.HANDEYE_USE_GUESS
            elif not fix:
                raise ValueError("a guess of X alone goes with fix_mount; otherwise pass (X, Y)")
            if not all(np.all(np.isfinite(v)) for g in (gx, gy) for v in g):
                raise ValueError("the guess is not finite")
        P = probs[r]
        P.first_frame, P.n_frames, P.flags, P.max_iterations = f0, F, flags, int(pr.get("max_iterations") or 0)
        P.a[:] = [float(v) for v in a]
        _solver.set_pose(P, gx, "guess_x_")
        _solver.set_pose(P, gy, "guess_y_")
        for j, pose in enumerate(poses):
            fr = frames[f0 + j]
            _solver.set_pose(fr, _robot_to_M(pose, setup))
            fr.first_point, fr.n_points = p0, len(o[j])
            p0 += len(o[j])
        obj += o
        img += i
        spans.append((f0, F, setup, a))
        f0 += F
    res, fres = _solve(probs, frames, _solver.cat_points(obj), _solver.cat_points(img))
    out = []
    for r, (ff, F, setup, a) in enumerate(spans):
        q = res[r]
        fr = [HandEyeFrameResult(int(f.status), int(f.points), float(f.rms_px), *_solver.get_pose(f)) for f in (fres[ff + j] for j in range(F))]
        out.append(HandEyeCalibration(int(q.status), setup, a, _solver.get_pose(q, "x_"), _solver.get_pose(q, "y_"), np.array(q.std_dev, np.float64), float(q.rms_px), int(q.iterations), bool(q.converged), int(q.frames_used),
                                      int(q.points_used), int(q.pairs_used), fr))
    return out


def calibrate_hand_eye(camera, robot_poses, observations, *, setup: str = "eye_in_hand", guess=None, fix_mount: bool = False,
                       max_iterations: Optional[int] = None, outlier_passes: int = 0) -> HandEyeCalibration:
    """One camera on, or beside, one robot.  camera: a Calibration, a CameraIntrinsics or the 12 values fx .. k6; robot_poses: per frame
    gripper -> base as (R, t) or a 4 x 4 matrix, translations in the board's units; observations: per frame (object_points,
    image_points), what the camera saw of the board at that pose, points as for calibrate_camera.  At least 3 usable frames, with
    rotations about at least two different axes between them.

    guess: (X, Y) as (R, t) pairs in the library's convention (see the module's table) to start from; with fix_mount the mount X is
    kept -- guess may then be X alone, or (X, None) -- and only Y is solved: a known mount locating a moved board.

    outlier_passes = k solves k more times, each time without the correspondences of a used frame that reproject farther than
    max(1 px, 3 x that frame's median) from the previous solution (calibrate_rig's rule); `HandEyeCalibration.inliers` then says which
    points of each frame the last solve used."""
    kw = dict(camera=camera, robot_poses=robot_poses, setup=setup, guess=guess, fix_mount=fix_mount, max_iterations=max_iterations)
    obj, img = _cal._views([ob[0] for ob in observations], [ob[1] for ob in observations])

    def residuals(he, j, k):
        if not he.frames[j].used:
            return None
        R, t = he.board_pose_in_camera(robot_poses[j])
        return np.linalg.norm(_cal.reproject(he.camera, R, t, obj[j][k]) - img[j][k], axis=1)

    return _solver.solve_with_outlier_passes(
        [len(o) for o in obj], lambda keep: calibrate_hand_eyes([dict(observations=[(o[k], i[k]) for o, i, k in zip(obj, img, keep)], **kw)])[0],
        residuals, outlier_passes)


def calibrate_hand_eye_board(board, detections, robot_poses, calibration, **kw) -> HandEyeCalibration:
    """One Detection per robot pose, from the marker corners of `board` (a Board / GridBoard); calibration: the camera as for
    calibrate_hand_eye; keywords as calibrate_hand_eye.  Detected corners carry outliers: pass outlier_passes=2 as for
    calibrate_rig_board."""
    return calibrate_hand_eye(calibration, robot_poses, [_cal.board_correspondences(board, d) for d in detections], **kw)


def calibrate_hand_eye_charuco(board, views, robot_poses, calibration, **kw) -> HandEyeCalibration:
    """One view per robot pose: Detections (charuco_ids / charuco_corners) or (ids, corners) pairs of a CharucoBoard; keywords as
    calibrate_hand_eye"""
    return calibrate_hand_eye(calibration, robot_poses, [_solver.charuco_view(board, v) for v in views], **kw)
