"""Planar marker boards and their one-pose-per-frame solve (a3_set_board / a3_get_board_poses / a3_estimate_board_pose).

Not part of the reference: an extension whose contract include/aruco3_hip.h states.  A board is a set of markers of known ids whose
corners lie on the plane z = 0 of the board's frame (x to the right, y up, corner 0 the top-left, as the per-marker IPPE solver's
square).  `Detector(board=...)` hands the board to the device, and `Detector.detect_batch_with_board_pose` returns one `BoardPose`
per frame, solved on the GPU from every board marker of that frame.  A `CharucoBoard` also yields its chessboard corners in every
frame (Detection.charuco_ids / .charuco_corners) and, from `Detector.detect_batch_with_charuco_pose`, one `CharucoPose` per frame."""
from dataclasses import dataclass
from typing import Sequence, Tuple

import math
from typing import Optional

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


class CharucoBoard(Board):
    """A ChArUco board: a squares_x x squares_y chessboard of side square_length with a marker of side marker_length centred in each
    white square.  Origin at the board's top-left outer corner, x right, y up (points of the board have y <= 0), z = 0.  Square (row 0,
    column 0) is black (OpenCV's current, non-legacy pattern); markers sit in the squares with row + column odd, id first_id + k numbered
    row-major from the top-left.  The chessboard corners are the (squares_x - 1)(squares_y - 1) inner corners, id r * (squares_x - 1) + c
    row-major from the top-left; each names the markers of the two white squares that touch it (`adjacent_ids`, 4 per corner, padded
    with CHARUCO_NO_ADJ).

    Detecting the markers of a ChArUco board needs a small DetectorConfig.min_corner_separation_factor: each white square is a hole of
    the black chessboard component, and its border is a quad candidate with a larger perimeter than the marker inside it, whose corners
    lie about m * sqrt(2) px from the marker's (m = (square_length - marker_length) / 2 in pixels).  discard_too_near keeps the larger of
    two quads closer than min_corner_separation_factor * (short image side), so with the default factor (0.1) every marker is dropped:
    the factor must stay below m * sqrt(2) / short side (0.005 with squares of 40 px or more at marker_length / square_length <= 0.75
    in a 1080p frame)."""

    def __init__(self, squares_x: int, squares_y: int, square_length: float, marker_length: float, first_id: int = 0):
        if squares_x < 2 or squares_y < 2:
            raise ValueError("a ChArUco board needs at least 2 squares along each side")
        if not 0 < marker_length < square_length:
            raise ValueError("a ChArUco board needs 0 < marker_length < square_length")
        n_corners = (squares_x - 1) * (squares_y - 1)
        if n_corners > _lib.CHARUCO_MAX_CORNERS:
            raise ValueError(f"a ChArUco board has at most {_lib.CHARUCO_MAX_CORNERS} chessboard corners")
        s, ml = float(square_length), float(marker_length)
        m = (s - ml) / 2
        ids, corners, marker_of = [], [], {}
        for r in range(squares_y):
            for c in range(squares_x):
                if (r + c) % 2 == 1:
                    marker_of[(r, c)] = first_id + len(ids)
                    x0, y0 = c * s + m, -r * s - m
                    ids.append(first_id + len(ids))
                    corners.append([(x0, y0), (x0 + ml, y0), (x0 + ml, y0 - ml), (x0, y0 - ml)])
        self.squares_x, self.squares_y = squares_x, squares_y
        self.square_length, self.marker_length = s, ml
        cxy = np.zeros((n_corners, 2), np.float32)
        adj = np.full((n_corners, 4), _lib.CHARUCO_NO_ADJ, np.uint32)
        for r in range(squares_y - 1):
            for c in range(squares_x - 1):
                k = r * (squares_x - 1) + c
                cxy[k] = ((c + 1) * s, -(r + 1) * s)
                near = [marker_of[q] for q in ((r, c), (r, c + 1), (r + 1, c), (r + 1, c + 1)) if q in marker_of]
                adj[k, :len(near)] = near
        self.chessboard_corners = cxy
        self.adjacent_ids = adj
        super().__init__(ids, corners)

    @property
    def n_corners(self) -> int:
        return int(self.chessboard_corners.shape[0])


@dataclass
class CharucoPose:
    """One frame's ChArUco pose (a3_charuco_pose), board -> camera.  status BOARD_NONE: fewer than 4 corners or no usable start."""
    status: int
    corners_used: int
    iterations: int
    rms_px: float
    alt_rms_px: float
    rotation: np.ndarray      # 3x3 float32
    translation: np.ndarray   # 3 float32, board units

    @property
    def ok(self) -> bool:
        return self.status == _lib.BOARD_OK

    @classmethod
    def _from(cls, rec) -> "CharucoPose":
        return cls(int(rec["status"]), int(rec["corners_used"]), int(rec["iterations"]), float(rec["rms_px"]), float(rec["alt_rms_px"]),
                   np.array(rec["rotation"], dtype=np.float32).reshape(3, 3), np.array(rec["translation"], dtype=np.float32))


@dataclass
class BoardRecovery:
    """Board-aided recovery of markers the decoder rejected (a3_recover_config; not in the reference -- include/aruco3_hip.h states the
    algorithm; OpenCV's refineDetectedMarkers).  Passing one to `Detector(board=..., recovery=...)` makes every detect call look, in each
    frame that shows at least `min_markers` board markers, for the board's other markers among the quads the decoder rejected: a quad
    within `max_distance_px` of where the board's homography puts a marker, whose bits lie within `max_hamming` of that marker's code,
    comes back as a `Marker` with `recovered=True`.  max_hamming None: the default derived from the dictionary's bit count (a random
    code passes with probability below 1e-3); 255: bits are not compared, and quads without a readable code are eligible too."""
    max_distance_px: float = 10.0
    max_hamming: Optional[int] = None
    min_markers: int = 2

    def __post_init__(self):
        d = float(self.max_distance_px)
        if not math.isfinite(d) or not d > 0:
            raise ValueError("BoardRecovery.max_distance_px must be finite and > 0")
        if int(self.min_markers) != self.min_markers or self.min_markers < 1:
            raise ValueError("BoardRecovery.min_markers must be an integer >= 1")
        if self.max_hamming is not None and (int(self.max_hamming) != self.max_hamming or not 0 <= self.max_hamming <= 255):
            raise ValueError("BoardRecovery.max_hamming must be None or an integer in 0..255")

    def _c(self, ctx: "_lib.Context") -> "_lib.RecoverConfig":
        cfg = ctx.default_recover_config()
        cfg.min_markers = int(self.min_markers)
        cfg.max_distance_px = float(self.max_distance_px)
        if self.max_hamming is not None:
            cfg.max_hamming = int(self.max_hamming)
        return cfg


def recover_markers(board: Board, dictionary, detected_ids, detected_corners, candidate_corners, codes4, has_codes,
                    recovery: Optional[BoardRecovery] = None, device: int = 0) -> np.ndarray:
    """stand-alone, one frame (a3_recover_markers): the markers of `board` that `detected_ids` lacks, looked for among caller-given
    rejected quads -- what a refineDetectedMarkers user calls.  detected_corners (n, 4, 2) and candidate_corners (m, 4, 2) are integer
    pixels, codes4 (m, 4) each quad's code read at the four rotations, has_codes (m,) whether it has any.  -> _lib.MARKER_DTYPE records
    in candidate order (candidate_index: the quad's position, rotation: the shift that aligns it with the board)."""
    from .aruco import DetectorConfig

    ctx = _lib.Context(DetectorConfig()._c(), dictionary.code_list, dictionary.num_bits, dictionary._tau, device)
    try:
        ctx.set_board(board.ids, board.corners)
        cfg = (recovery or BoardRecovery())._c(ctx)
        return ctx.recover_markers(detected_ids, detected_corners, candidate_corners, codes4, has_codes, cfg).copy()
    finally:
        ctx.close()
