"""Planar marker boards and their one-pose-per-frame solve (a3_set_board / a3_get_board_poses / a3_estimate_board_pose).

Not part of the reference: an extension whose contract include/aruco3_hip.h states.  A board is a set of markers of known ids whose
corners lie on the plane z = 0 of the board's frame (x to the right, y up, corner 0 the top-left, as the per-marker IPPE solver's
square).  `Detector(board=...)` hands the board to the device, and `Detector.detect_batch_with_board_pose` returns one `BoardPose`
per frame, solved on the GPU from every board marker of that frame.  A `CharucoBoard` also yields its chessboard corners in every
frame (Detection.charuco_ids / .charuco_corners) and, from `Detector.detect_batch_with_charuco_pose`, one `CharucoPose` per frame.

A `Board3D` (a3_set_board3d) is a board whose markers are not coplanar -- a cube with a marker on each face, two grid boards at a right
angle, the markers of a `MarkerMap`: `Detector(board=Board3D...)` returns its pose from `detect_batch_with_board_pose` as a planar
board's, solved on the device from every marker of the frame whichever face it lies on."""
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


def check_marker_corners_3d(corners) -> None:
    """raises ValueError unless the four (x, y, z) corners form a planar square (the test a3_set_board3d applies, in its wording).  The
    order top-left, top-right, bottom-right, bottom-left is as seen from the side the marker is printed on: it defines that side."""
    c = np.asarray(corners, dtype=np.float32).reshape(4, 3).astype(np.float64)
    if not np.all(np.isfinite(c)):
        raise ValueError("a corner is not finite")
    e = np.roll(c, -1, axis=0) - c
    dot = lambda a, b: (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]
    s = math.sqrt(dot(e[0], e[0]))
    if not s > 0:
        raise ValueError("a marker has no size")
    for k in range(4):
        k1 = (k + 1) % 4
        if abs(math.sqrt(dot(e[k], e[k])) - s) > SQUARE_TOL * s:
            raise ValueError("a marker's sides differ (its corners must form a square)")
        if abs(dot(e[k], e[k1])) > SQUARE_TOL * s * s:
            raise ValueError("a marker's corners are not at right angles (they must form a square)")
    g = c[2] - ((c[1] + c[3]) - c[0])
    if math.sqrt(dot(g, g)) > SQUARE_TOL * s:
        raise ValueError("a marker's corners do not lie in one plane (they must form a square)")


class Board3D:
    """`n` markers that need not be coplanar: ids (unique dictionary indices) and corners (n, 4, 3) in board units.  A marker's corners
    are top-left, top-right, bottom-right, bottom-left as seen from the side it is printed on; that order defines the side, and its
    outward normal is (c1 - c0) x (c0 - c3) normalised.  (a3_set_board3d; the ChArUco and recovery settings need a planar board.)"""

    def __init__(self, ids: Sequence[int], corners):
        self.ids = np.asarray(ids, dtype=np.uint32).reshape(-1)
        self.corners = np.asarray(corners, dtype=np.float32).reshape(-1, 4, 3)
        if self.corners.shape[0] != self.ids.size:
            raise ValueError("a board needs four corners per id")
        if not 1 <= self.ids.size <= _lib.BOARD_MAX_MARKERS:
            raise ValueError(f"a board has 1 .. {_lib.BOARD_MAX_MARKERS} markers")
        if np.unique(self.ids).size != self.ids.size:
            raise ValueError("an id appears twice on the board")
        for c in self.corners:
            check_marker_corners_3d(c)

    def __len__(self) -> int:
        return int(self.ids.size)

    def object_points(self, id_: int) -> np.ndarray:
        """the (4, 3) board-frame corners of marker `id_`"""
        k = int(np.nonzero(self.ids == id_)[0][0])
        return self.corners[k].astype(np.float64)

    def normals(self) -> np.ndarray:
        """(n, 3) unit normals out of each marker's printed face"""
        c = self.corners.astype(np.float64)
        n = np.cross(c[:, 1] - c[:, 0], c[:, 0] - c[:, 3])
        return n / np.linalg.norm(n, axis=1, keepdims=True)

    # the cube's faces in id order: (outward normal, the face's "up")
    CUBE_FACES = (((1, 0, 0), (0, 0, 1)), ((-1, 0, 0), (0, 0, 1)), ((0, 1, 0), (0, 0, 1)), ((0, -1, 0), (0, 0, 1)),
                  ((0, 0, 1), (0, 1, 0)), ((0, 0, -1), (0, 1, 0)))

    @classmethod
    def cube(cls, side: float, marker_length: float, first_id: int = 0) -> "Board3D":
        """A cube of edge `side` with its centre at the origin and one marker of side `marker_length` centred on each face: ids
        first_id .. first_id + 5 on the faces +x, -x, +y, -y, +z, -z.  Seen from outside, a marker's up (corner 3 -> corner 0) is +z on
        the four faces +x, -x, +y, -y and +y on the faces +z and -z; its right (corner 0 -> corner 1) is up x normal: +y, -y, -x, +x on
        the first four faces, +x on +z, -x on -z."""
        if not 0 < marker_length <= side:
            raise ValueError("a cube board needs 0 < marker_length <= side")
        h = marker_length / 2.0
        corners = []
        for n, u in cls.CUBE_FACES:
            n, u = np.array(n, np.float64), np.array(u, np.float64)
            r = np.cross(u, n)
            c = n * (side / 2.0)
            corners.append([c - h * r + h * u, c + h * r + h * u, c + h * r - h * u, c - h * r - h * u])
        return cls([first_id + k for k in range(6)], corners)

    @classmethod
    def from_board(cls, board: "Board", R=None, t=None) -> "Board3D":
        """a planar Board / GridBoard lifted into 3-D at the pose (R, t): corner (x, y) -> R (x, y, 0) + t.  R: a rotation (3, 3), None:
        the identity; t: (3,), None: zero"""
        R = np.eye(3) if R is None else np.asarray(R, dtype=np.float64).reshape(3, 3)
        t = np.zeros(3) if t is None else np.asarray(t, dtype=np.float64).reshape(3)
        if not (np.all(np.isfinite(R)) and np.all(np.isfinite(t))):
            raise ValueError("from_board needs a finite R and t")
        if not (np.abs(R @ R.T - np.eye(3)).max() <= 1e-6 and np.linalg.det(R) > 0):
            raise ValueError("from_board needs a rotation matrix R (a reflection would turn the markers' printed sides over)")
        c = board.corners.astype(np.float64).reshape(-1, 2)
        X = np.concatenate([c, np.zeros((c.shape[0], 1))], axis=1) @ R.T + t
        return cls(board.ids, X.reshape(-1, 4, 3))

    @classmethod
    def join(cls, boards: Sequence["Board3D"]) -> "Board3D":
        """several Board3D, given in one common frame, as one board; their ids must be distinct"""
        boards = list(boards)
        if not boards:
            raise ValueError("join needs at least one board")
        return cls(np.concatenate([b.ids for b in boards]), np.concatenate([b.corners for b in boards], axis=0))

    @classmethod
    def from_marker_map(cls, marker_map) -> "Board3D":
        """the markers of a MarkerMap (its ids and their corners_3d) as a board: detect_batch_with_board_pose then returns world -> camera
        of every frame inside the detect call"""
        ids = np.asarray(marker_map.ids).reshape(-1)
        return cls(ids, np.stack([np.asarray(marker_map.corners_3d(int(i)), dtype=np.float64) for i in ids]))


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
