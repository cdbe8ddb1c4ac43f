"""Host-side mirror of `CameraIntrinsics` (src/pinhole.rs:11-60): a plain parameter record.
The one operation the pose path uses, `unproject` (src/pinhole.rs:88-93), runs inside the pose kernel.

`Distortion` is an extension (the reference assumes an ideal pinhole camera): OpenCV's rational lens model or its fisheye one
(cv::fisheye, Kannala-Brandt), whose inverse runs on the device (include/aruco3_hip.h, a3_set_distortion) before the poses are solved."""
import math
from dataclasses import dataclass
from typing import Optional

import numpy as np


@dataclass
class Distortion:
    """OpenCV's 5- / 8-coefficient lens model (a3_distortion, model A3_DIST_RATIONAL): the coefficients of a calibration as
    cv2.calibrateCamera returns them (k1 k2 p1 p2 k3 [k4 k5 k6]), the iteration count of the undistortion and the largest
    reprojection residual, in pixels, at which an undistorted corner is accepted.
    With model "fisheye" (a3_distortion model A3_DIST_FISHEYE) k1 k2 k3 k4 are cv::fisheye's D -- theta_d = theta (1 + k1 theta^2 +
    k2 theta^4 + k3 theta^6 + k4 theta^8) -- and p1 p2 k5 k6 must be 0: build it with `Distortion.fisheye` / `from_opencv_fisheye`."""
    k1: float = 0.0
    k2: float = 0.0
    p1: float = 0.0
    p2: float = 0.0
    k3: float = 0.0
    k4: float = 0.0
    k5: float = 0.0
    k6: float = 0.0
    iterations: int = 20
    max_residual_px: float = 0.1
    model: str = "rational"

    def __post_init__(self):
        if self.model not in ("rational", "fisheye"):
            raise ValueError(f"Distortion.model: 'rational' or 'fisheye', not {self.model!r}")
        self._check_fisheye()

    def _check_fisheye(self):
        if self.model == "fisheye" and any(float(v) != 0.0 for v in (self.p1, self.p2, self.k5, self.k6)):
            raise ValueError("a fisheye Distortion reads k1 k2 k3 k4 (cv::fisheye's D); p1, p2, k5 and k6 must be 0")

    @classmethod
    def fisheye(cls, k1=0.0, k2=0.0, k3=0.0, k4=0.0, **kw) -> "Distortion":
        """the fisheye model from cv::fisheye's four coefficients"""
        return cls(k1=float(k1), k2=float(k2), k3=float(k3), k4=float(k4), model="fisheye", **kw)

    @classmethod
    def from_opencv_fisheye(cls, D, **kw) -> "Distortion":
        """from cv::fisheye's D (exactly 4 values: k1 k2 k3 k4)"""
        c = [float(v) for v in np.asarray(D, dtype=np.float64).reshape(-1)]
        if len(c) != 4:
            raise ValueError("fisheye distortion coefficients: exactly 4 values (k1 k2 k3 k4)")
        return cls.fisheye(*c, **kw)

    def rational_coefficients(self, what: str):
        """k1 k2 p1 p2 k3 k4 k5 k6 for a consumer that knows the rational model only (`what` names it in the error)"""
        if self.model != "rational":
            raise ValueError(f"{what} takes rational lens coefficients only, not a fisheye Distortion: rectify the frames first "
                             "(rectify_frames), then use the rectified view's plain intrinsics")
        return [self.k1, self.k2, self.p1, self.p2, self.k3, self.k4, self.k5, self.k6]

    @classmethod
    def from_opencv(cls, coeffs, **kw) -> "Distortion":
        """from OpenCV's distCoeffs (4, 5 or 8 values: k1 k2 p1 p2 [k3 [k4 k5 k6]])"""
        c = [float(v) for v in np.asarray(coeffs, dtype=np.float64).reshape(-1)]
        if len(c) not in (4, 5, 8):
            raise ValueError("distortion coefficients: 4, 5 or 8 values (k1 k2 p1 p2 [k3 [k4 k5 k6]])")
        return cls(*(c + [0.0] * (8 - len(c))), **kw)

    def distort_normalized(self, points) -> np.ndarray:
        """the forward model on the host, in the normalised plane: ideal (x, y) (..., 2) -> distorted (xd, yd), float64"""
        p = np.asarray(points, dtype=np.float64)
        x, y = p[..., 0], p[..., 1]
        if self.model == "fisheye":
            self._check_fisheye()
            r = np.sqrt(x * x + y * y)
            th = np.arctan(r)
            t2 = th * th
            thd = th * (1 + (((self.k4 * t2 + self.k3) * t2 + self.k2) * t2 + self.k1) * t2)
            s = np.divide(thd, r, out=np.ones_like(r), where=r > 0)
            return np.stack([x * s, y * s], axis=-1)
        r2 = x * x + y * y
        radial = (1 + ((self.k3 * r2 + self.k2) * r2 + self.k1) * r2) / (1 + ((self.k6 * r2 + self.k5) * r2 + self.k4) * r2)
        xd = x * radial + (2 * self.p1 * x * y + self.p2 * (r2 + 2 * x * x))
        yd = y * radial + (self.p1 * (r2 + 2 * y * y) + 2 * self.p2 * x * y)
        return np.stack([xd, yd], axis=-1)

    def _c(self):
        from . import _lib

        self._check_fisheye()
        model = _lib.DIST_FISHEYE if self.model == "fisheye" else _lib.DIST_RATIONAL
        return _lib.DistortionRec(model, int(self.iterations), self.k1, self.k2, self.p1, self.p2, self.k3, self.k4, self.k5, self.k6,
                                  self.max_residual_px)


@dataclass
class CameraIntrinsics:
    image_width: int
    image_height: int
    focal_x: float
    focal_y: float
    principal_x: Optional[float] = None
    principal_y: Optional[float] = None
    distortion: Optional[Distortion] = None   # (an extension: the lens model the pose calls undistort corners with)

    def __post_init__(self):  # src/pinhole.rs:26-35
        if self.principal_x is None:
            self.principal_x = self.image_width / 2.0
        if self.principal_y is None:
            self.principal_y = self.image_height / 2.0

    @classmethod
    def new(cls, image_width, image_height, focal_x, focal_y, principal_x=None, principal_y=None):
        return cls(image_width, image_height, focal_x, focal_y, principal_x, principal_y)

    @classmethod
    def new_from_fov_horizontal(cls, horizontal_fov_radians, sensor_width_mm, resolution_x, resolution_y):  # src/pinhole.rs:37-60
        aspect = resolution_x / resolution_y
        vfov = horizontal_fov_radians / aspect
        sensor_height_mm = sensor_width_mm / aspect
        fx = (sensor_width_mm * 0.5) / math.tan(horizontal_fov_radians * 0.5)
        fy = (sensor_height_mm * 0.5) / math.tan(vfov * 0.5)
        return cls(resolution_x, resolution_y, fx, fy, resolution_x * 0.5, resolution_y * 0.5)

    def _c(self):
        from . import _lib

        return _lib.Intrinsics(self.image_width, self.image_height, self.focal_x, self.focal_y, self.principal_x, self.principal_y)


def undistort_points(points, intrinsics: CameraIntrinsics):
    """a3_undistort_points: pixel points (..., 2) seen through `intrinsics.distortion` -> (float32 (n, 2) undistorted pixels -- where an
    ideal camera with the same focal lengths and principal point would have seen them --, float32 (n,) residuals in pixels; +inf marks
    a point the model could not invert, returned as it came).  Runs on the device, on the kernel the pose batches use."""
    from . import _solver

    if intrinsics.distortion is None:
        raise ValueError("undistort_points needs CameraIntrinsics.distortion")
    return _solver.call("undistort_points", points, intrinsics._c(), intrinsics.distortion._c())
