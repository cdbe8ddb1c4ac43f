"""The board pose's CPU restatement (tests/board_oracle.c, the contract of include/aruco3_hip.h a3_set_board) on its own: it recovers
exact poses, reaches the least-squares optimum under noise, keeps the better of its two starts, rejects duplicated ids; and the
Python board types (aruco3_amd.board) lay out and check their markers as a3_set_board does.  No GPU."""
import math

import numpy as np
import pytest

from aruco3_amd.board import Board, GridBoard
from tests import board_oracle as bo
from tests import board_util as bu

K = bu.K1080
W, H = bu.W1080, bu.H1080


def _residuals(board, ids, px, R, t):
    """float64 normalised-plane residuals of the used corners (every id of `ids` on the board, none duplicated)"""
    fx, fy, cx, cy = K
    out = []
    for i, mid in enumerate(ids):
        X = np.concatenate([board.object_points(mid)[:, :2], np.zeros((4, 1))], axis=1)
        P = X @ R.T + t
        z = np.maximum(P[:, 2], 1e-5)
        m = np.stack([(px[i, :, 0] - cx) / fx, (px[i, :, 1] - cy) / fy], axis=1)
        out.append((np.stack([P[:, 0] / z, P[:, 1] / z], axis=1) - m).reshape(-1))
    return np.concatenate(out)


def _scene(tilt=35.0, tilt_dir=20.0, roll=10.0, dist=600.0, board=None):
    board = board or GridBoard(5, 7, 30.0, 6.0)
    R, t = bu.board_pose_facing(board, tilt, tilt_dir, roll, dist)
    return board, R, t, bu.project(board, R, t)


def test_exact_correspondences_recover_the_true_pose():
    for tilt, tilt_dir, roll in [(15.0, 0.0, 0.0), (35.0, 20.0, 10.0), (50.0, 110.0, -30.0)]:
        board, R, t, px = _scene(tilt, tilt_dir, roll)
        rec = bo.board_pose(board, board.ids, px, intrinsics=K)
        assert rec["status"] == 1 and rec["markers_used"] == len(board) and rec["markers_rejected"] == 0
        assert np.abs(rec["rotation"].reshape(3, 3) - R).max() <= 1e-5
        assert np.linalg.norm(rec["translation"] - t) <= 1e-5 * np.linalg.norm(t)
        assert rec["rms_px"] < 1e-2
    # without intrinsics the points are normalised by the image size (x / w, y / h): a pose in that "camera"
    board, R, t, _ = _scene()
    Kwh = (float(W), float(H), 0.0, 0.0)
    px = bu.project(board, R, t, Kwh)
    rec = bo.board_pose(board, board.ids, px, image_size=(W, H))
    assert np.abs(rec["rotation"].reshape(3, 3) - R).max() <= 1e-5
    assert np.linalg.norm(rec["translation"] - t) <= 1e-5 * np.linalg.norm(t)


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_noisy_corners_reach_the_least_squares_optimum(seed):
    from scipy.optimize import least_squares
    from scipy.spatial.transform import Rotation

    board, R, t, px = _scene(25.0 + 10 * seed, 40.0 * seed, 15.0)
    px = px + np.random.default_rng(seed).normal(0.0, 0.5, px.shape)
    px = px.astype(np.float32).astype(np.float64)
    rec = bo.board_pose(board, board.ids, px, intrinsics=K)
    got = _residuals(board, board.ids, px, rec["rotation"].reshape(3, 3).astype(np.float64), rec["translation"].astype(np.float64))

    def f(x):
        return _residuals(board, board.ids, px, Rotation.from_rotvec(x[:3]).as_matrix(), x[3:])

    x0 = np.concatenate([Rotation.from_matrix(R).as_rotvec(), t])
    ref = least_squares(f, x0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15)
    c_got, c_ref = float(got @ got), float(ref.fun @ ref.fun)
    assert abs(c_got - c_ref) <= 1e-4 * c_ref, (c_got, c_ref)
    assert 1 <= rec["iterations"] <= 30


def test_both_starts_are_refined_and_the_lower_cost_is_kept():
    board = GridBoard(2, 2, 40.0, 10.0)
    for tilt in (8.0, 40.0):
        _, R, t, px = _scene(tilt, 30.0, 0.0, 900.0, board)
        px = px + np.random.default_rng(3).normal(0.0, 0.3, px.shape)
        rec, starts = bo.board_pose(board, board.ids, px, intrinsics=K, with_starts=True)
        assert not np.allclose(starts[0], starts[1])   # IPPE's two poses differ
        fin = []
        for s in starts:
            R1, t1, ev, cost, pix = bo.refine_from(board, board.ids, px, s[:9], s[9:], intrinsics=K)
            fin.append((cost, pix, R1, t1, ev))
        keep = 1 if fin[1][0] < fin[0][0] else 0
        assert np.array_equal(rec["rotation"], fin[keep][2].reshape(9))
        assert np.array_equal(rec["translation"], fin[keep][3])
        assert rec["iterations"] == fin[keep][4]
        assert rec["rms_px"] == np.float32(math.sqrt(np.float32(fin[keep][1]) / np.float32(16)))
        assert rec["alt_rms_px"] == np.float32(math.sqrt(np.float32(fin[1 - keep][1]) / np.float32(16)))
        assert bu.rotation_error_deg(rec["rotation"].reshape(3, 3), R) < 2.0


def test_start_marker_is_the_largest_quad_and_its_poses_are_carried_into_the_board_frame():
    """board corners Q S + c: R_b = R_m Q^T, t_b = t_m - R_b c, with the IPPE poses of the largest image quad"""
    a = math.radians(30.0)
    Q = np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
    S = np.array([[-1, 1], [1, 1], [1, -1], [-1, -1]], dtype=np.float64) * 20.0
    board = Board([3, 9], [S @ Q.T + np.array([100.0, 50.0]), S * 0.5 + np.array([-80.0, 0.0])])
    R, t = bu.board_pose_facing(board, 20.0, 0.0, 0.0, 500.0)
    px = bu.project(board, R, t).astype(np.float32)
    rec, starts = bo.board_pose(board, [9, 3], px[::-1], intrinsics=K, with_starts=True)
    fx, fy, cx, cy = K
    pts = np.stack([(px[0, :, 0] - np.float32(cx)) / np.float32(fx), (px[0, :, 1] - np.float32(cy)) / np.float32(fy)], axis=1)
    poses = bo.ippe(pts, 40.0)
    for k in range(2):
        Rm = poses[k, 1:10].reshape(3, 3).astype(np.float64)
        Rb = Rm @ np.block([[Q.T, np.zeros((2, 1))], [np.zeros((1, 2)), np.ones((1, 1))]])
        tb = poses[k, 10:13] - Rb @ np.array([100.0, 50.0, 0.0])
        assert np.allclose(starts[k, :9].reshape(3, 3), Rb, atol=1e-5)
        assert np.allclose(starts[k, 9:], tb, atol=1e-3)
    assert bu.rotation_error_deg(rec["rotation"].reshape(3, 3), R) < 0.5


def test_cayley_update_is_a_rotation_by_twice_the_arctangent():
    from scipy.spatial.transform import Rotation

    R0 = bu.rot_xyz(10.0, -20.0, 30.0)
    for w in ([0.0, 0.0, 0.0], [1e-3, -2e-3, 5e-4], [0.3, 0.1, -0.2], [2.0, -1.0, 0.5]):
        w = np.array(w)
        C = bo.cayley(w, R0).astype(np.float64)
        n = np.linalg.norm(w)
        rv = w / n * 2.0 * math.atan(n) if n > 0 else w
        want = Rotation.from_rotvec(rv).as_matrix() @ R0
        assert np.abs(C - want).max() < 2e-6
        assert np.abs(C @ C.T - np.eye(3)).max() < 2e-6


def test_a_duplicated_id_is_excluded_in_all_its_instances():
    board, R, t, px = _scene()
    ids = list(board.ids) + [int(board.ids[7]), 1000]   # a second instance of slot 7, and an id not on the board
    quads = np.concatenate([px, px[7:8] + 300.0, px[0:1] - 300.0])
    rec = bo.board_pose(board, ids, quads, intrinsics=K)
    assert rec["markers_used"] == len(board) - 1 and rec["markers_rejected"] == 2
    assert np.abs(rec["rotation"].reshape(3, 3) - R).max() <= 1e-5
    keep = [i for i in range(len(board)) if i != 7]
    ref = bo.board_pose(board, board.ids[keep], px[keep], intrinsics=K)
    assert np.allclose(rec["rotation"], ref["rotation"], atol=1e-6)
    none = bo.board_pose(board, [1000, 1001], px[:2], intrinsics=K)
    assert none["status"] == 0 and none["markers_used"] == 0 and not none["rotation"].any() and none["rms_px"] == 0
    only_dups = bo.board_pose(board, [5, 5], px[:2], intrinsics=K)
    assert only_dups["status"] == 0 and only_dups["markers_rejected"] == 2


def test_gridboard_layout_and_winding():
    g = GridBoard(3, 2, 10.0, 2.5, first_id=4)
    assert g.ids.tolist() == [4, 5, 6, 7, 8, 9]
    assert g.corners[0].tolist() == [[0, 0], [10, 0], [10, -10], [0, -10]]
    assert g.corners[2].tolist() == [[25, 0], [35, 0], [35, -10], [25, -10]]       # columns along +x
    assert g.corners[3].tolist() == [[0, -12.5], [10, -12.5], [10, -22.5], [0, -22.5]]   # rows along -y
    for c in g.corners:
        assert bo.check_marker(c) is None
        e0, e1 = c[1] - c[0], c[2] - c[1]
        assert e0[0] * e1[1] - e0[1] * e1[0] < 0   # the IPPE square's winding (y up)


def test_board_validation_errors():
    sq = np.array([[0, 0], [10, 0], [10, -10], [0, -10]], dtype=np.float32)
    cases = {
        "sides differ": np.array([[0, 0], [10, 0], [10, -11], [0, -11]], np.float32),
        "not right angles": np.array([[0, 0], [10, 0], [12, -10], [2, -10]], np.float32),
        "wound the wrong way": sq[::-1].copy(),
        "no size": np.zeros((4, 2), np.float32),
        "not finite": np.array([[0, 0], [np.nan, 0], [10, -10], [0, -10]], np.float32),
    }
    for why, c in cases.items():
        assert bo.check_marker(c) == why
        with pytest.raises(ValueError):
            Board([0], [c])
    rot = sq @ np.array([[0.6, -0.8], [0.8, 0.6]], np.float32).T + 5.0   # any in-plane rotation and position
    assert bo.check_marker(rot) is None
    Board([0, 1], [rot, sq * 3.0])   # mixed sizes
    with pytest.raises(ValueError):
        Board([1, 1], [sq, sq + 20])
    with pytest.raises(ValueError):
        Board(range(1025), [sq] * 1025)
    with pytest.raises(ValueError):
        Board([], [])
