"""Board scenes for the device renderer (a3_synth_render, the record format of aruco3_amd.synth.device_layout): a board's markers
projected through K [R | t] to per-marker image quads, drawn with their real board ids, plus extra markers (foreign ids, duplicates)
placed by hand.  The true corners and pose are kept.  TEST INFRASTRUCTURE ONLY."""
import math
from dataclasses import dataclass, field
from typing import List, Tuple

import numpy as np

from aruco3_amd import synth

W1080, H1080 = 1920, 1080
K1080 = (1400.0, 1400.0, 960.0, 540.0)   # fx, fy, cx, cy
# a grid board's markers are a gap of a few pixels apart: discard_too_near's default minimum corner distance (a tenth of the short
# image side, 108 px at 1080p) would drop most of them
MIN_CORNER_SEPARATION_FACTOR = 0.005


def config():
    """the detector configuration of the board scenes (aruco3_amd._lib.Config): the default with MIN_CORNER_SEPARATION_FACTOR"""
    from aruco3_amd import _lib

    cfg = _lib.default_config()
    cfg.min_corner_separation_factor = MIN_CORNER_SEPARATION_FACTOR
    return cfg


def rot_xyz(ax_deg: float, ay_deg: float, az_deg: float) -> np.ndarray:
    ax, ay, az = (math.radians(v) for v in (ax_deg, ay_deg, az_deg))
    rx = np.array([[1, 0, 0], [0, math.cos(ax), -math.sin(ax)], [0, math.sin(ax), math.cos(ax)]])
    ry = np.array([[math.cos(ay), 0, math.sin(ay)], [0, 1, 0], [-math.sin(ay), 0, math.cos(ay)]])
    rz = np.array([[math.cos(az), -math.sin(az), 0], [math.sin(az), math.cos(az), 0], [0, 0, 1]])
    return rx @ ry @ rz


def board_pose_facing(board, tilt_deg: float, tilt_dir_deg: float, roll_deg: float, distance: float, offset_px=(0.0, 0.0), K=K1080):
    """R, t (board -> camera) of a board whose centre lies `distance` in front of the camera (shifted by offset_px in the image),
    tilted by tilt_deg about an in-plane axis at tilt_dir_deg and rolled by roll_deg.  Frontal (tilt 0): board y up = image up."""
    flip = np.diag([1.0, -1.0, -1.0])   # board z towards the camera, y up -> camera y down
    axis = math.radians(tilt_dir_deg)
    u = np.array([math.cos(axis), math.sin(axis), 0.0])
    a = math.radians(tilt_deg)
    ux = np.array([[0, -u[2], u[1]], [u[2], 0, -u[0]], [-u[1], u[0], 0]])
    tilt = np.eye(3) + math.sin(a) * ux + (1 - math.cos(a)) * (ux @ ux)
    R = flip @ tilt @ rot_xyz(0, 0, roll_deg)
    c = board.corners.reshape(-1, 2).astype(np.float64)
    centre = np.array([(c[:, 0].min() + c[:, 0].max()) / 2, (c[:, 1].min() + c[:, 1].max()) / 2, 0.0])
    fx, fy, cx, cy = K
    target = np.array([offset_px[0] / fx * distance, offset_px[1] / fy * distance, distance])
    t = target - R @ centre
    return R, t


def project(board, R, t, K=K1080) -> np.ndarray:
    """(n, 4, 2) image corners of every board marker (pixel centres at integer coordinates)"""
    fx, fy, cx, cy = K
    X = np.concatenate([board.corners.reshape(-1, 2).astype(np.float64), np.zeros((board.corners.shape[0] * 4, 1))], axis=1)
    P = X @ np.asarray(R).T + np.asarray(t)
    return np.stack([fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy], axis=1).reshape(-1, 4, 2)


@dataclass
class Scene:
    """one frame: markers to draw (quad (4, 2) in TL, TR, BR, BL order, dictionary index) and the truth"""
    quads: List[Tuple[np.ndarray, int]] = field(default_factory=list)
    R: np.ndarray = None
    t: np.ndarray = None


def board_scene(board, R, t, K=K1080, keep=None) -> Scene:
    """the board's markers (all, or the board slots in `keep`) at pose R, t"""
    q = project(board, R, t, K)
    sel = range(len(board)) if keep is None else keep
    return Scene([(q[k], int(board.ids[k])) for k in sel], np.asarray(R), np.asarray(t))


def square_quad(cx: float, cy: float, side: float, angle_deg: float = 0.0) -> np.ndarray:
    a = math.radians(angle_deg)
    sq = np.array([[-0.5, -0.5], [0.5, -0.5], [0.5, 0.5], [-0.5, 0.5]]) * side
    rot = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
    return sq @ rot.T + np.array([cx, cy])


def layout(scenes: List[Scene], codes, num_bits: int, base: float = 200.0):
    """-> (frames, markers) record arrays of a3_synth_render (flat background, no noise)"""
    frames = np.zeros(len(scenes), dtype=synth.SYNTH_FRAME_DTYPE)
    recs = []
    for fi, sc in enumerate(scenes):
        frames[fi] = (base, 0.0, 0.0, 0.0, len(recs), len(sc.quads), fi)
        for quad, mid in sc.quads:
            cells = synth.marker_cells(int(codes[mid]), num_bits)
            n = cells.shape[0]
            src = np.array([[0, 0], [n, 0], [n, n], [0, n]], dtype=np.float64)
            H = synth._homography(src, np.asarray(quad, np.float64))
            outer = (H @ np.array([[-1, -1, 1], [n + 1, -1, 1], [n + 1, n + 1, 1], [-1, n + 1, 1]], dtype=np.float64).T).T
            outer = outer[:, :2] / outer[:, 2:3]
            bits = 0
            for r in range(n):
                for c in range(n):
                    bits |= int(cells[r, c]) << (r * n + c)
            recs.append((np.linalg.inv(H).astype(np.float32).reshape(9), int(math.floor(outer[:, 0].min())) - 1, int(math.floor(outer[:, 1].min())) - 1,
                         int(math.ceil(outer[:, 0].max())) + 2, int(math.ceil(outer[:, 1].max())) + 2, (bits & ((1 << 64) - 1), bits >> 64), n, 0))
    marr = np.zeros(max(len(recs), 1), dtype=synth.SYNTH_MARKER_DTYPE)
    for i, r in enumerate(recs):
        marr[i] = r
    for k in ("x0", "x1"):
        marr[k] = np.clip(marr[k], 0, None)
    for k in ("y0", "y1"):
        marr[k] = np.clip(marr[k], 0, None)
    return frames, marr[: len(recs)]


def render(scenes: List[Scene], d, width: int = W1080, height: int = H1080, device: int = 0):
    """renders the scenes on the GPU -> CUDA uint8 tensor (N, H, W, 3)"""
    import torch

    from aruco3_amd import _lib

    frames, markers = layout(scenes, d.code_list, d.num_bits)
    out = torch.empty((len(scenes), height, width, 3), dtype=torch.uint8, device=torch.device("cuda", device))
    markers["x1"] = np.minimum(markers["x1"], width)
    markers["y1"] = np.minimum(markers["y1"], height)
    _lib.synth_render(device, frames, markers, width, height, True, 25.0, 235.0, 3, out.data_ptr(), width * 3, width * height * 3)
    return out


def rotation_error_deg(Ra, Rb) -> float:
    """angle of Ra^T Rb in degrees (NaN when either is not finite)"""
    if not (np.all(np.isfinite(Ra)) and np.all(np.isfinite(Rb))):
        return float("nan")
    c = (np.trace(np.asarray(Ra, np.float64).T @ np.asarray(Rb, np.float64)) - 1.0) / 2.0
    return math.degrees(math.acos(max(-1.0, min(1.0, c))))
