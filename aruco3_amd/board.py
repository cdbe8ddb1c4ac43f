"""Planar marker boards and their one-pose-per-frame solve (a3_set_board / a3_get_board_poses / a3_estimate_board_pose).

Not part of the reference: an extension whose contract include/aruco3_hip.h states.  A board is a set of markers of known ids whose
corners lie on the plane z = 0 of the board's frame (x to the right, y up, corner 0 the top-left, as the per-marker IPPE solver's
square).  `Detector(board=...)` hands the board to the device, and `Detector.detect_batch_with_board_pose` returns one `BoardPose`
per frame, solved on the GPU from every board marker of that frame."""
from dataclasses import dataclass
from typing import Sequence, Tuple

import numpy as np

from . import _lib

SQUARE_TOL = 1e-3   # relative, as a3_set_board checks


def check_marker_corners(corners) -> None:
    """raises ValueError unless the four (x, y) corners form a square wound top-left, top-right, bottom-right, bottom-left with y up
    (the test a3_set_board applies)"""
    c = np.asarray(corners, dtype=np.float32).reshape(4, 2).astype(np.float64)
    if not np.all(np.isfinite(c)):
        raise ValueError("a corner is not finite")
    e = np.roll(c, -1, axis=0) - c
    s = float(np.hypot(*e[0]))
    if not s > 0:
        raise ValueError("a marker has no size")
    for k in range(4):
        k1 = (k + 1) % 4
        if abs(float(np.hypot(*e[k])) - s) > SQUARE_TOL * s:
            raise ValueError("a marker's sides differ (its corners must form a square)")
        if abs(float(e[k] @ e[k1])) > SQUARE_TOL * s * s:
            raise ValueError("a marker's corners are not at right angles (they must form a square)")
    if not e[0, 0] * e[1, 1] - e[0, 1] * e[1, 0] < 0:
        raise ValueError("a marker is wound the wrong way (top-left, top-right, bottom-right, bottom-left with y up)")


class Board:
    """`n` markers: ids (unique dictionary indices) and corners (n, 4, 2) in board units (z = 0, x right, y up)."""

    def __init__(self, ids: Sequence[int], corners):
        self.ids = np.asarray(ids, dtype=np.uint32).reshape(-1)
        self.corners = np.asarray(corners, dtype=np.float32).reshape(-1, 4, 2)
        if self.corners.shape[0] != self.ids.size:
            raise ValueError("a board needs four corners per id")
        if not 1 <= self.ids.size <= _lib.BOARD_MAX_MARKERS:
            raise ValueError(f"a board has 1 .. {_lib.BOARD_MAX_MARKERS} markers")
        if np.unique(self.ids).size != self.ids.size:
            raise ValueError("an id appears twice on the board")
        for c in self.corners:
            check_marker_corners(c)

    def __len__(self) -> int:
        return int(self.ids.size)

    def object_points(self, id_: int) -> np.ndarray:
        """the (4, 3) board-frame corners of marker `id_`"""
        k = int(np.nonzero(self.ids == id_)[0][0])
        return np.concatenate([self.corners[k].astype(np.float64), np.zeros((4, 1))], axis=1)


class GridBoard(Board):
    """markers_x x markers_y markers of side marker_length, marker_separation apart; id first_id + row * markers_x + column.
    Origin at the top-left corner of marker (0, 0); columns along +x, rows along -y."""

    def __init__(self, markers_x: int, markers_y: int, marker_length: float, marker_separation: float, first_id: int = 0):
        if markers_x < 1 or markers_y < 1 or not marker_length > 0 or marker_separation < 0:
            raise ValueError("a grid board needs at least one marker, a positive length and a separation >= 0")
        step = marker_length + marker_separation
        ids, corners = [], []
        for r in range(markers_y):
            for c in range(markers_x):
                x0, y0 = c * step, -r * step
                ids.append(first_id + r * markers_x + c)
                corners.append([(x0, y0), (x0 + marker_length, y0), (x0 + marker_length, y0 - marker_length), (x0, y0 - marker_length)])
        self.markers_x, self.markers_y = markers_x, markers_y
        self.marker_length, self.marker_separation = marker_length, marker_separation
        super().__init__(ids, corners)


@dataclass
class BoardPose:
    """One frame's board pose (a3_board_pose): board -> camera.  status BOARD_NONE: no usable board marker in the frame."""
    status: int
    markers_used: int
    markers_rejected: int
    iterations: int
    rms_px: float
    alt_rms_px: float
    rotation: np.ndarray      # 3x3 float32
    translation: np.ndarray   # 3 float32, board units

    @property
    def ok(self) -> bool:
        return self.status == _lib.BOARD_OK

    @classmethod
    def _from(cls, rec) -> "BoardPose":
        return cls(int(rec["status"]), int(rec["markers_used"]), int(rec["markers_rejected"]), int(rec["iterations"]), float(rec["rms_px"]),
                   float(rec["alt_rms_px"]), np.array(rec["rotation"], dtype=np.float32).reshape(3, 3), np.array(rec["translation"], dtype=np.float32))

    def apply_transform_to_points(self, points: Sequence[Tuple[float, float, float]]):
        p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
        return [tuple(map(float, (self.rotation @ v + self.translation).astype(np.float32))) for v in p]

    def apply_inverse_transform_to_points(self, points: Sequence[Tuple[float, float, float]]):
        p = np.asarray(points, dtype=np.float32).reshape(-1, 3)
        return [tuple(map(float, (self.rotation.T @ (v - self.translation)).astype(np.float32))) for v in p]
