"""Scenes of 3-D boards (aruco3_amd.board.Board3D) for the renderers: a board's markers projected through K [R | t] to per-marker image
quads, of which those facing the camera are drawn as tests/board_util.py draws a planar board's (its Scene, layout, render, K1080,
config and rotation_error_deg are used by import).  The true corners and pose are kept.  TEST INFRASTRUCTURE ONLY."""
import math
from typing import List

import numpy as np

from aruco3_amd import synth
from tests.board_util import H1080, K1080, W1080, Scene, config, layout, render, rotation_error_deg, square_quad  # noqa: F401

# A marker is drawn when the cosine between its outward normal and the direction from its centre to the camera is at least this.
# Chosen on the CPU: the restated detector (oracle/a3oracle.detect on aruco3_amd.synth's drawing) finds a single face of the cube below
# at every tilt up to 65 degrees (cosine 0.42) from twelve directions each; 0.5 (60 degrees) leaves a margin.  Above the limit the
# detector still misplaces a corner of some strongly sheared rhombi, as the faces of a cube seen corner-on are, so the scenes of this
# file are fixed, and tests/test_oracle_board3d.py::test_cpu_detector_finds_every_drawn_marker checks every one of them.
FACE_COS_LIMIT = 0.5
# the cube of the scenes: markers of 36 units (97 px face-on at 520 units through K1080, cells of 14 px: below the threshold window,
# so a marker is not found twice) on faces of 48; the 6 units around a marker hold its one-cell quiet zone (36 / 7 = 5.1 units), so
# the drawings of two faces never touch
CUBE_SIDE, CUBE_MARKER, CUBE_FIRST_ID, CUBE_DISTANCE = 48.0, 36.0, 10, 520.0
EXTRA = [(150.0, 150.0), (1770.0, 150.0), (150.0, 930.0), (1770.0, 930.0)]   # image spots for markers off the board


def cube():
    from aruco3_amd.board import Board3D

    return Board3D.cube(CUBE_SIDE, CUBE_MARKER, first_id=CUBE_FIRST_ID)


def right_angle_grids(n: int = 3, marker_length: float = 30.0, separation: float = 6.0, first_id: int = 0):
    """two n x n grid boards glued at a right angle like two faces of a box, along the first one's left edge: the first in the plane
    z = 0 facing +z, the second turned about the y axis into the plane x = -separation, facing -x and reaching towards -z"""
    from aruco3_amd.board import Board3D, GridBoard

    a = GridBoard(n, n, marker_length, separation, first_id=first_id)
    b = GridBoard(n, n, marker_length, separation, first_id=first_id + n * n)
    R = np.array([[0.0, 0.0, -1.0], [0.0, 1.0, 0.0], [1.0, 0.0, 0.0]])   # x -> +z, z -> -x: the second board faces -x
    width = n * marker_length + (n - 1) * separation
    return Board3D.join([Board3D.from_board(a), Board3D.from_board(b, R, np.array([-separation, 0.0, -(width + separation)]))])


def view_pose(view_dir, roll_deg: float, distance: float, offset_px=(0.0, 0.0), K=K1080, centre=(0.0, 0.0, 0.0)):
    """R, t (board -> camera) of a camera that looks at the board point `centre` from `distance` along the board-frame direction
    view_dir (from the centre towards the camera), rolled by roll_deg about its axis, the centre shifted by offset_px in the image"""
    d = np.asarray(view_dir, np.float64)
    d = d / np.linalg.norm(d)
    z = -d
    up = np.array([0.0, 0.0, 1.0]) if abs(z[2]) < 0.9 else np.array([0.0, 1.0, 0.0])
    y = -(up - (up @ z) * z)
    y = y / np.linalg.norm(y)
    x = np.cross(y, z)
    a = math.radians(roll_deg)
    roll = np.array([[math.cos(a), -math.sin(a), 0.0], [math.sin(a), math.cos(a), 0.0], [0.0, 0.0, 1.0]])
    R = roll @ np.stack([x, y, z])
    fx, fy, _, _ = K
    target = np.array([offset_px[0] / fx * distance, offset_px[1] / fy * distance, distance])
    return R, target - R @ np.asarray(centre, np.float64)


def project(board, R, t, K=K1080) -> np.ndarray:
    """(n, 4, 2) image corners of every marker of a Board3D (pixel centres at integer coordinates)"""
    fx, fy, cx, cy = K
    P = board.corners.reshape(-1, 3).astype(np.float64) @ np.asarray(R).T + np.asarray(t)
    return np.stack([fx * P[:, 0] / P[:, 2] + cx, fy * P[:, 1] / P[:, 2] + cy], axis=1).reshape(-1, 4, 2)


def facing(board, R, t) -> np.ndarray:
    """(n,) cosine between each marker's outward normal and the direction from its centre to the camera"""
    R, t = np.asarray(R, np.float64), np.asarray(t, np.float64)
    n = board.normals() @ R.T
    c = board.corners.astype(np.float64).mean(axis=1) @ R.T + t
    return -np.sum(n * c, axis=1) / np.linalg.norm(c, axis=1)


def visible(board, R, t, limit: float = FACE_COS_LIMIT) -> List[int]:
    """the board slots that are drawn at pose R, t"""
    return [int(k) for k in np.nonzero(facing(board, R, t) >= limit)[0]]


def board_scene(board, R, t, K=K1080, limit: float = FACE_COS_LIMIT) -> Scene:
    """the markers of a convex Board3D that face the camera at pose R, t"""
    q = project(board, R, t, K)
    return Scene([(q[k], int(board.ids[k])) for k in visible(board, R, t, limit)], np.asarray(R), np.asarray(t))


def _extra(sc: Scene, spot: int, mid: int, side: float = 90.0, angle: float = 0.0) -> Scene:
    sc.quads.append((square_quad(*EXTRA[spot], side, angle), mid))
    return sc


GPU_SCENE_DRAWN = [3, 2, 1, 0, 3, 0]   # cube markers drawn in each of gpu_scenes()


def gpu_scenes(board) -> List[Scene]:
    """0: cube corner-on (3 faces); 1: edge-on (2); 2: one face near-frontal (1, the ambiguous case); 3: nothing; 4: corner-on + a
    foreign id + a second instance of one of its ids; 5: only foreign ids"""
    out = [board_scene(board, *view_pose((1.0, 0.9, 0.95), 10.0, CUBE_DISTANCE)),
           board_scene(board, *view_pose((1.0, -0.85, 0.0), -15.0, CUBE_DISTANCE, (40.0, -20.0))),
           board_scene(board, *view_pose((0.03, 0.02, 1.0), 5.0, CUBE_DISTANCE)),
           Scene()]
    sc = board_scene(board, *view_pose((-0.95, 1.0, -0.9), 0.0, CUBE_DISTANCE))
    out.append(_extra(_extra(sc, 0, 300), 2, sc.quads[1][1], angle=-10.0))
    out.append(_extra(_extra(Scene(), 0, 700), 1, 701))
    return out


def accuracy_scenes(board, n: int = 16, seed: int = 4, min_faces: int = 2) -> List[Scene]:
    """n random cube poses that show at least min_faces faces"""
    rng = np.random.default_rng(seed)
    out = []
    while len(out) < n:
        d = rng.standard_normal(3)
        R, t = view_pose(d, rng.uniform(-30, 30), rng.uniform(480, 560), (rng.uniform(-60, 60), rng.uniform(-30, 30)))
        if len(visible(board, R, t)) >= min_faces:
            out.append(board_scene(board, R, t))
    return out


def render_cpu(scenes: List[Scene], d, width: int = W1080, height: int = H1080) -> np.ndarray:
    """the scenes drawn on the host by aruco3_amd.synth (flat background 200, printed black 25, 3 x 3 supersampling: what render()
    asks of the device) -> uint8 (N, H, W, 3) with the host renderer's fixed channel tint"""
    spec = synth.SynthSpec(width, height, background="flat", paper=True, black=25, white=235, supersample=3)
    out = np.empty((len(scenes), height, width, 3), np.uint8)
    for f, sc in enumerate(scenes):
        gray = np.full((height, width), 200.0, dtype=np.float32)
        for quad, mid in sc.quads:
            synth._draw_marker(gray, synth.marker_cells(int(d.code_list[mid]), d.num_bits), np.asarray(quad, np.float64), spec)
        rgb = np.stack([gray * 1.00, gray * 0.98, gray * 0.94], axis=-1)
        out[f] = np.rint(np.clip(rgb, 0.0, 255.0)).astype(np.uint8)
    return out
