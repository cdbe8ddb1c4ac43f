"""ChArUco boards on the CPU: CharucoBoard's geometry and checks, and the contract's restatement (tests/charuco_oracle.c) on constructed
cases -- exact interpolation through a known homography, the min_markers / duplicate / singular / out-of-frame rules, refinement
accuracy on rendered boards and the pose on noiseless correspondences.  No GPU."""
import math

import numpy as np
import pytest

from aruco3_amd import _lib
from aruco3_amd.board import CharucoBoard
from tests import board_util as bu
from tests import charuco_oracle as co
from tests import charuco_util as cu

NO = _lib.CHARUCO_NO_ADJ


def _homography_image(board, Hm, ids=None):
    """marker ids and their image corners (n, 4, 2) through the 3x3 homography Hm (board units -> pixels), float"""
    c = board.corners.reshape(-1, 2).astype(np.float64)
    p = np.concatenate([c, np.ones((len(c), 1))], axis=1) @ Hm.T
    q = (p[:, :2] / p[:, 2:3]).reshape(-1, 4, 2).astype(np.float32)
    sel = list(range(len(board))) if ids is None else [int(np.nonzero(board.ids == i)[0][0]) for i in ids]
    return board.ids[sel].copy(), q[sel]


def _apply(Hm, xy):
    p = np.concatenate([np.asarray(xy, np.float64), np.ones((len(xy), 1))], axis=1) @ Hm.T
    return p[:, :2] / p[:, 2:3]


HM = np.array([[9.0, 1.2, 300.0], [0.8, -8.5, 200.0], [2e-4, -3e-4, 1.0]])   # board units (y up) -> pixels (y down), with perspective


def test_geometry():
    b = CharucoBoard(5, 7, 40.0, 30.0, first_id=3)
    assert len(b) == 17 and b.n_corners == 24
    assert list(b.ids) == list(range(3, 20))
    # square (0, 1) is the first white square: marker first_id, centred, corner 0 top-left with y up
    assert np.allclose(b.corners[0], [(45, -5), (75, -5), (75, -35), (45, -35)])
    # square (1, 0) holds the third marker (row 0 has squares 1 and 3 white)
    assert np.allclose(b.corners[2], [(5, -45), (35, -45), (35, -75), (5, -75)])
    assert np.all(b.chessboard_corners[:, 1] <= 0) and np.all(b.corners[..., 1] <= 0)
    for r in range(6):
        for c in range(4):
            k = r * 4 + c
            assert tuple(b.chessboard_corners[k]) == ((c + 1) * 40.0, -(r + 1) * 40.0)
            adj = [int(a) for a in b.adjacent_ids[k] if a != NO]
            assert len(adj) == 2 and list(b.adjacent_ids[k][2:]) == [NO, NO]
            # each adjacent marker's square touches the corner: its marker centre is half a square away along both axes
            for a in adj:
                q = b.corners[int(np.nonzero(b.ids == a)[0][0])].astype(np.float64)
                centre = q.mean(axis=0)
                assert np.allclose(np.abs(centre - b.chessboard_corners[k]), 20.0)
    # marker squares are white ((row + column) odd) and the black squares are the rest
    assert len(cu.square_quads(b)) == 35 - 17


@pytest.mark.parametrize("args, msg", [((1, 5, 40, 30), "at least 2"), ((5, 1, 40, 30), "at least 2"), ((5, 5, 40, 40), "marker_length"),
                                       ((5, 5, 40, 0), "marker_length"), ((5, 5, 40, 50), "marker_length"), ((47, 47, 4, 3), "at most 2048")])
def test_validation(args, msg):
    with pytest.raises(ValueError, match=msg):
        CharucoBoard(*args)


def test_large_board():
    b = CharucoBoard(41, 41, 4.0, 3.0)   # 1600 corners, 840 markers
    assert b.n_corners == 1600 and len(b) == 840
    with pytest.raises(ValueError, match="1024 markers"):
        CharucoBoard(46, 46, 4.0, 3.0)   # 2025 corners fit, 1058 markers do not


def test_interpolation_is_exact_through_a_homography():
    b = CharucoBoard(5, 7, 40.0, 30.0)
    ids, px = _homography_image(b, HM)
    rec = co.corners(b, ids, px, config=co.Config.default(refine=0), image_size=(4000, 4000))
    assert list(rec["id"]) == list(range(b.n_corners))
    want = _apply(HM, b.chessboard_corners)
    got = np.stack([rec["x"], rec["y"]], axis=1)
    assert np.abs(got - want).max() < 1e-3
    assert np.array_equal(rec["x"], rec["interp_x"]) and np.all(rec["window"] == 0) and np.all(rec["markers_used"] == 2)


def test_min_markers_rule():
    b = CharucoBoard(5, 7, 40.0, 30.0)
    ids, px = _homography_image(b, HM)
    keep = ids != 6
    hit = {k for k in range(b.n_corners) if 6 in b.adjacent_ids[k]}
    assert len(hit) == 4
    r2 = co.corners(b, ids[keep], px[keep], config=co.Config.default(refine=0), image_size=(4000, 4000))
    assert set(r2["id"]) == set(range(b.n_corners)) - hit
    r1 = co.corners(b, ids[keep], px[keep], config=co.Config.default(refine=0, min_markers=1), image_size=(4000, 4000))
    assert set(r1["id"]) == set(range(b.n_corners))
    assert all(int(r["markers_used"]) == (1 if r["id"] in hit else 2) for r in r1)
    r3 = co.corners(b, ids, px, config=co.Config.default(refine=0, min_markers=3), image_size=(4000, 4000))
    assert r3.size == 0


def test_duplicate_ids_drop_every_instance():
    b = CharucoBoard(5, 7, 40.0, 30.0)
    ids, px = _homography_image(b, HM)
    ids2 = np.concatenate([ids, [6]]).astype(np.uint32)
    px2 = np.concatenate([px, px[6:7] + 500.0])
    hit = {k for k in range(b.n_corners) if 6 in b.adjacent_ids[k]}
    rec = co.corners(b, ids2, px2, config=co.Config.default(refine=0, min_markers=1), image_size=(4000, 4000))
    assert all(int(r["markers_used"]) == (1 if r["id"] in hit else 2) for r in rec)
    # a foreign id (not on the board) changes nothing
    ids3 = np.concatenate([ids, [900]]).astype(np.uint32)
    rec3 = co.corners(b, ids3, np.concatenate([px, px[:1]]), config=co.Config.default(refine=0), image_size=(4000, 4000))
    assert np.array_equal(rec3, co.corners(b, ids, px, config=co.Config.default(refine=0), image_size=(4000, 4000)))


def test_singular_homography_leaves_the_marker_out():
    b = CharucoBoard(5, 7, 40.0, 30.0)
    ids, px = _homography_image(b, HM)
    px = px.copy()
    px[6] = px[6][0]   # all four image corners on one point
    hit = {k for k in range(b.n_corners) if 6 in b.adjacent_ids[k]}
    rec = co.corners(b, ids, px, config=co.Config.default(refine=0, min_markers=1), image_size=(4000, 4000))
    assert {int(r["id"]) for r in rec} == set(range(b.n_corners))
    assert all(int(r["markers_used"]) == (1 if r["id"] in hit else 2) for r in rec)


def test_out_of_frame_corners_are_not_reported():
    b = CharucoBoard(5, 7, 40.0, 30.0)
    ids, px = _homography_image(b, HM)
    want = _apply(HM, b.chessboard_corners)
    W, H = 900, 900
    inside = {k for k in range(b.n_corners) if 0 <= want[k, 0] <= W - 1 and 0 <= want[k, 1] <= H - 1}
    assert 0 < len(inside) < b.n_corners
    rec = co.corners(b, ids, px, config=co.Config.default(refine=0), image_size=(W, H))
    assert {int(r["id"]) for r in rec} == inside


def _scene(seed=3):
    b = CharucoBoard(5, 7, 40.0, 28.0)
    K = (800.0, 800.0, 320.0, 240.0)
    R, t = bu.board_pose_facing(b, 30.0, 40.0 + 25 * seed, 10.0, 650.0, K=K)
    return b, K, R, t


# measured on the first oracle run of these scenes: median 0.048 / 0.070 / 0.051 px, max 0.10 / 0.12 / 0.10 px after refinement
# (interpolation from the integer marker corners: median 0.36 / 0.39 / 0.41 px); the thresholds carry a margin
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_refinement_accuracy_on_rendered_boards(seed):
    b, K, R, t = _scene(seed)
    W, H = 640, 480
    grey = cu.host_grey(b, R, t, K, W, H)
    truth = cu.true_corners(b, R, t, K)
    ids, px = b.ids, np.round(bu.project(b, R, t, K)).astype(np.float32)   # integer marker corners, as an unrefined detection gives
    rec = co.corners(b, ids, px, grey=grey, config=co.Config.default())
    assert rec.size == b.n_corners
    got = np.stack([rec["x"], rec["y"]], axis=1)
    interp = np.stack([rec["interp_x"], rec["interp_y"]], axis=1)
    err = np.hypot(*(got - truth[rec["id"]]).T)
    err0 = np.hypot(*(interp - truth[rec["id"]]).T)
    print(f"seed {seed}: refined median {np.median(err):.4f} max {err.max():.4f} px; interpolated median {np.median(err0):.4f} px")
    assert np.median(err) < 0.1 and err.max() < 0.2
    assert np.median(err) < np.median(err0)
    assert np.all((rec["window"] >= 2) & (rec["window"] <= 5))


@pytest.mark.parametrize("use_intr", [False, True])
def test_pose_on_noiseless_correspondences(use_intr):
    b, K, R, t = _scene(1)
    W, H = 640, 480
    ids, px = b.ids, bu.project(b, R, t, K).astype(np.float32)
    truth = cu.true_corners(b, R, t, K).astype(np.float32)
    rec = np.zeros(b.n_corners, co.CORNER_DTYPE)
    rec["id"] = np.arange(b.n_corners)
    rec["x"], rec["y"] = truth[:, 0], truth[:, 1]
    p = co.pose(b, ids, px, rec, (W, H), intrinsics=K if use_intr else None)
    assert p["status"] == 1 and p["corners_used"] == b.n_corners
    if use_intr:   # (a float32 rotation's angle to the truth reads ~0.02 deg through acos near 1: the threshold is that floor)
        Rg = np.asarray(p["rotation"], np.float64).reshape(3, 3)
        assert bu.rotation_error_deg(Rg, R) < 0.05
        assert np.abs(Rg - R).max() < 1e-6
        assert np.linalg.norm(np.asarray(p["translation"]) - t) < 1e-4 * np.linalg.norm(t)
        assert p["rms_px"] < 1e-2
    else:   # (x / w, y / h is no pinhole camera: a pose, not the truth)
        assert np.isfinite(p["rms_px"]) and p["iterations"] >= 1


def test_pose_needs_four_corners():
    b, K, R, t = _scene(1)
    ids, px = b.ids, bu.project(b, R, t, K).astype(np.float32)
    rec = np.zeros(3, co.CORNER_DTYPE)
    rec["id"] = [0, 1, 2]
    p = co.pose(b, ids, px, rec, (640, 480), intrinsics=K)
    assert p["status"] == 0 and p["corners_used"] == 3 and not np.any(p["rotation"])


def test_window_follows_the_marker_distance():
    b = CharucoBoard(5, 7, 40.0, 30.0)
    ids, px = _homography_image(b, HM)
    rec = co.corners(b, ids, px, config=co.Config.default(refine=0), image_size=(4000, 4000))
    # with refine = 1 the window is min(5, max(2, floor(0.5 d))), d the distance to the nearest corner of a marker used
    grey = np.full((4000, 4000), 128, np.uint8)
    r1 = co.corners(b, ids, px, grey=grey, config=co.Config.default(max_iterations=0))
    assert np.array_equal(r1["interp_x"], rec["x"])
    for r in r1:
        ix, iy = float(r["interp_x"]), float(r["interp_y"])
        d = min(math.hypot(float(c[0]) - ix, float(c[1]) - iy) for a in b.adjacent_ids[r["id"]] if a != NO
                for c in px[int(np.nonzero(ids == a)[0][0])])
        assert int(r["window"]) == min(5, max(2, math.floor(0.5 * d)))
