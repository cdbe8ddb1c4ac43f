"""The 3-D board pose's CPU restatement (tests/board3d_oracle.c, the contract of include/aruco3_hip.h a3_set_board3d) on its own: it
recovers exact poses of a cube and of two grids at a right angle, gives the planar oracle's starts on a flat board, carries a tilted
marker's IPPE pose into the board frame, rejects duplicated ids; aruco3_amd.board.Board3D lays out and checks its markers as
a3_set_board3d does; and the restated detector finds every marker tests/board3d_util.py draws.  No GPU."""
import math

import numpy as np
import pytest

from aruco3_amd.board import Board, Board3D, GridBoard
from tests import board3d_oracle as o3
from tests import board3d_util as b3
from tests import board_oracle as bo
from tests import board_util as bu

K = bu.K1080
W, H = bu.W1080, bu.H1080


def _is_truth(rec, R, t):
    """the planar test's bounds (tests/test_oracle_board.py)"""
    assert np.abs(rec["rotation"].reshape(3, 3) - R).max() <= 1e-5
    assert np.linalg.norm(rec["translation"] - t) <= 1e-5 * np.linalg.norm(t)
    assert rec["rms_px"] < 1e-2


CUBE_VIEWS = [((1.0, 0.9, 0.95), 3), ((1.0, -0.85, 0.0), 2), ((0.2, 0.1, 1.0), 1)]


@pytest.mark.parametrize("use_intr", [True, False])
@pytest.mark.parametrize("view,faces", CUBE_VIEWS)
def test_exact_correspondences_recover_the_cube(view, faces, use_intr):
    cube = b3.cube()
    R, t = b3.view_pose(view, 10.0, 520.0, (30.0, -20.0))
    Kp = K if use_intr else (float(W), float(H), 0.0, 0.0)   # (without intrinsics the points are normalised x / w, y / h: a pose in that "camera")
    vis = b3.visible(cube, R, t)
    assert len(vis) == faces
    px = b3.project(cube, R, t, Kp)[vis]
    rec = o3.board_pose(cube, cube.ids[vis], px, image_size=(W, H), intrinsics=K if use_intr else None)
    assert rec["status"] == 1 and rec["markers_used"] == faces and rec["markers_rejected"] == 0
    _is_truth(rec, R, t)


@pytest.mark.parametrize("use_intr", [True, False])
def test_exact_correspondences_recover_two_grids_at_a_right_angle(use_intr):
    board = b3.right_angle_grids(3)
    R, t = b3.view_pose((-1.0, 0.2, 1.0), -8.0, 600.0, centre=(0.0, -50.0, 0.0))
    assert len(b3.visible(board, R, t)) == 18   # both grids face the camera
    Kp = K if use_intr else (float(W), float(H), 0.0, 0.0)
    rec = o3.board_pose(board, board.ids, b3.project(board, R, t, Kp), image_size=(W, H), intrinsics=K if use_intr else None)
    assert rec["status"] == 1 and rec["markers_used"] == 18
    _is_truth(rec, R, t)


def test_a_flat_board_gives_the_planar_oracles_starts():
    """The slot frame (e_x, e_y, e_z, c) of a marker on the plane z = 0 is the planar slot's (cs, sn, c): the starts agree.  The two
    frames differ by a few f32 roundings of an orthonormal basis (about 1e-7) that pass through three-term sums; 1e-5 leaves ten
    times that, and a wrong axis or sign is an error of order 1."""
    grid = GridBoard(5, 7, 30.0, 6.0)
    lifted = Board3D.from_board(grid)
    rot = lambda a: np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
    sq = np.array([[-1, 1], [1, 1], [1, -1], [-1, -1]], np.float64)
    turned = Board([40, 41, 42], [sq * 32 @ rot(0.3).T, sq * 25 @ rot(2.0).T + [120, 30], sq * 30 @ rot(-0.5).T + [-125, -40]])
    for board, b3d in ((grid, lifted), (turned, Board3D.from_board(turned))):
        for tilt, tilt_dir, roll in [(15.0, 0.0, 0.0), (35.0, 20.0, 10.0), (50.0, 110.0, -30.0)]:
            R, t = bu.board_pose_facing(board, tilt, tilt_dir, roll, 600.0)
            px = bu.project(board, R, t)
            for intr, size in ((K, None), (None, (W, H))):
                want, s2 = bo.board_pose(board, board.ids, px, image_size=size, intrinsics=intr, with_starts=True)
                got, s3 = o3.board_pose(b3d, board.ids, px, image_size=size, intrinsics=intr, with_starts=True)
                assert got["status"] == want["status"] == 1 and got["markers_used"] == want["markers_used"]
                for k in range(2):
                    assert np.abs(s3[k, :9] - s2[k, :9]).max() <= 1e-5, (tilt, k)
                    assert np.linalg.norm(s3[k, 9:] - s2[k, 9:]) <= 1e-5 * np.linalg.norm(s2[k, 9:]), (tilt, k)


def test_slot_frame_is_the_markers_own():
    """e_x along corner 0 -> 1, e_y along corner 3 -> 0, e_z out of the printed face, c the centre, s the side"""
    cube = b3.cube()
    for k, (n, u) in enumerate(Board3D.CUBE_FACES):
        s = o3.slot(cube.corners[k])
        assert np.allclose(s["ez"], n, atol=1e-6) and np.allclose(s["ey"], u, atol=1e-6)
        assert np.allclose(s["ex"], np.cross(u, n), atol=1e-6)
        assert np.allclose(s["c"], np.array(n) * b3.CUBE_SIDE / 2, atol=1e-5) and s["side"] == np.float32(b3.CUBE_MARKER)
    R = bu.rot_xyz(25.0, -40.0, 70.0)
    one = Board3D.from_board(Board([5], [[(-10, 10), (10, 10), (10, -10), (-10, -10)]]), R, [3.0, -4.0, 5.0])
    s = o3.slot(one.corners[0])
    assert np.allclose(np.stack([s["ex"], s["ey"], s["ez"]], axis=1), R, atol=1e-6)
    assert np.allclose(s["c"], [3.0, -4.0, 5.0], atol=1e-5) and abs(s["side"] - 20.0) < 1e-5
    assert np.allclose(one.normals()[0], R[:, 2], atol=1e-6)


@pytest.mark.parametrize("angles,tb", [((25.0, -40.0, 70.0), (30.0, -45.0, 12.0)), ((-100.0, 15.0, 200.0), (-5.0, 60.0, -30.0))])
def test_a_tilted_markers_ippe_pose_is_carried_into_the_board_frame(angles, tb):
    """one marker placed at an arbitrary pose in the board: with exact corners IPPE's first pose is the marker's, and the kept start,
    carried through (e_x, e_y, e_z, c), is the board's true pose before any LM step moves it"""
    Rmb, tmb = bu.rot_xyz(*angles), np.array(tb)
    board = Board3D.from_board(Board([7], [[(-20, 20), (20, 20), (20, -20), (-20, -20)]]), Rmb, tmb)
    # the camera sees the marker's printed face at 30 degrees: the board pose is that view composed with the marker's placement
    Rm, tm = b3.view_pose((0.4, 0.3, 1.0), 15.0, 500.0)
    R, t = Rm @ Rmb.T, tm - Rm @ Rmb.T @ tmb
    px = b3.project(board, R, t)
    assert b3.facing(board, R, t)[0] > 0.8
    rec, starts = o3.board_pose(board, board.ids, px, intrinsics=K, with_starts=True)
    costs = [o3.cost_at(board, board.ids, px, s[:9], s[9:], intrinsics=K)[0] for s in starts]
    keep = 1 if costs[1] < costs[0] else 0
    assert np.abs(starts[keep, :9].reshape(3, 3) - R).max() <= 1e-5
    assert np.linalg.norm(starts[keep, 9:] - t) <= 1e-5 * np.linalg.norm(t)
    assert costs[keep] < 1e-10 and costs[1 - keep] > 100 * costs[keep]
    _is_truth(rec, R, t)
    assert np.abs(rec["rotation"] - starts[keep, :9]).max() <= 1e-5   # LM stays at the start it was handed


def test_both_starts_are_refined_and_the_lower_cost_is_kept():
    cube = b3.cube()
    R, t = b3.view_pose((1.0, -0.85, 0.0), -15.0, 520.0)
    vis = b3.visible(cube, R, t)
    px = b3.project(cube, R, t)[vis] + np.random.default_rng(3).normal(0.0, 0.3, (len(vis), 4, 2))
    rec, starts = o3.board_pose(cube, cube.ids[vis], px, intrinsics=K, with_starts=True)
    fin = [o3.refine_from(cube, cube.ids[vis], px, s[:9], s[9:], intrinsics=K) for s in starts]
    keep = 1 if fin[1][3] < fin[0][3] else 0
    assert np.array_equal(rec["rotation"], fin[keep][0].reshape(9)) and np.array_equal(rec["translation"], fin[keep][1])
    assert rec["iterations"] == fin[keep][2]
    nc = np.float32(4 * len(vis))
    assert rec["rms_px"] == np.float32(math.sqrt(np.float32(fin[keep][4]) / nc))
    assert rec["alt_rms_px"] == np.float32(math.sqrt(np.float32(fin[1 - keep][4]) / nc))
    assert bu.rotation_error_deg(rec["rotation"].reshape(3, 3), R) < 1.0


def test_a_duplicated_id_is_excluded_in_all_its_instances():
    cube = b3.cube()
    R, t = b3.view_pose((1.0, 0.9, 0.95), 10.0, 520.0)
    vis = b3.visible(cube, R, t)
    px = b3.project(cube, R, t)[vis]
    ids = list(cube.ids[vis])
    wrong = bu.square_quad(300.0, 300.0, 90.0)[None]
    rec = o3.board_pose(cube, ids + [ids[1], 999], np.concatenate([px, wrong, wrong + 400.0]), intrinsics=K)
    assert (rec["status"], rec["markers_used"], rec["markers_rejected"]) == (1, 2, 2)
    _is_truth(rec, R, t)   # (the misplaced second instance took no part)
    alone = o3.board_pose(cube, [ids[0], ids[2]], px[[0, 2]], intrinsics=K)
    assert np.array_equal(rec["rotation"], alone["rotation"]) and np.array_equal(rec["translation"], alone["translation"])


def test_a_frame_without_board_markers_has_no_pose():
    cube = b3.cube()
    for ids, px in (([], np.zeros((0, 4, 2))), ([300, 301], np.stack([bu.square_quad(300, 300, 90), bu.square_quad(900, 500, 90)]))):
        rec = o3.board_pose(cube, ids, px, intrinsics=K)
        assert rec.tobytes() == bytes(rec.nbytes)   # A3_BOARD_NONE, zeros
    sq = bu.square_quad(300, 300, 90)
    rec = o3.board_pose(cube, [10, 10], np.stack([sq, sq + 200]), intrinsics=K)   # only a duplicated id
    assert (rec["status"], rec["markers_used"], rec["markers_rejected"]) == (0, 0, 2) and not rec["rotation"].any()


# ---- the Python surface ----
def test_cube_faces_point_outwards():
    cube = Board3D.cube(80.0, 60.0, first_id=4)
    assert list(cube.ids) == [4, 5, 6, 7, 8, 9] and cube.corners.shape == (6, 4, 3)
    axes = np.array([n for n, _ in Board3D.CUBE_FACES], np.float64)
    assert np.allclose(cube.normals(), axes, atol=1e-12)
    for k in range(6):
        c = cube.corners[k].astype(np.float64)
        assert np.allclose(c.mean(axis=0), 40.0 * axes[k]) and np.allclose(c @ axes[k], 40.0)   # centred on its face
        assert np.allclose(c[0] - c[3], 60.0 * np.array(Board3D.CUBE_FACES[k][1]))              # up, as the docstring states it
        assert np.allclose(o3.slot(c)["ez"], axes[k], atol=1e-6)
        assert np.array_equal(cube.object_points(4 + k), c)
    for bad in ((80.0, 0.0), (80.0, 81.0), (80.0, float("nan"))):
        with pytest.raises(ValueError):
            Board3D.cube(*bad)


def test_from_board_join_and_from_marker_map():
    grid = GridBoard(3, 2, 30.0, 6.0, first_id=20)
    flat = Board3D.from_board(grid)
    assert np.array_equal(flat.ids, grid.ids) and np.array_equal(flat.corners[..., :2], grid.corners) and not flat.corners[..., 2].any()
    R, t = bu.rot_xyz(90.0, 0.0, 0.0), np.array([0.0, 10.0, -5.0])
    up = Board3D.from_board(GridBoard(3, 2, 30.0, 6.0, first_id=30), R, t)
    assert np.allclose(up.object_points(30), grid.object_points(20) @ R.T + t, atol=1e-5)
    both = Board3D.join([flat, up])
    assert len(both) == 12 and list(both.ids) == list(range(20, 26)) + list(range(30, 36))
    assert np.array_equal(both.corners[6:], up.corners)
    with pytest.raises(ValueError, match="an id appears twice"):
        Board3D.join([flat, Board3D.from_board(grid, R, t)])
    with pytest.raises(ValueError):
        Board3D.join([])
    with pytest.raises(ValueError, match="rotation matrix"):
        Board3D.from_board(grid, np.diag([1.0, 1.0, -1.0]))
    with pytest.raises(ValueError, match="rotation matrix"):
        Board3D.from_board(grid, 2.0 * np.eye(3))

    class Map:   # what Board3D reads of an aruco3_amd.markermap.MarkerMap
        ids = np.array([7, 3, 11], np.int64)
        corners = np.stack([b3.cube().corners[k].astype(np.float64) + 100.0 * k for k in (0, 2, 4)])

        def corners_3d(self, marker_id):
            return self.corners[int(np.nonzero(self.ids == marker_id)[0][0])]

    m = Map()
    board = Board3D.from_marker_map(m)
    assert list(board.ids) == [7, 3, 11]
    for i in m.ids:
        assert np.array_equal(board.object_points(int(i)), m.corners_3d(int(i)))


def test_from_marker_map_takes_a_real_marker_map():
    from aruco3_amd.markermap import MarkerMap

    c = np.stack([b3.cube().corners[k].astype(np.float64) for k in range(6)])
    z = np.zeros
    mm = MarkerMap(status=1, ids=np.arange(6, dtype=np.int64), marker_length=36.0, rotations=z((6, 3, 3)), translations=z((6, 3)), corners=c,
                   std_devs=z((6, 6)), marker_status=z(6, np.int64), marker_rms_px=z(6))
    board = Board3D.from_marker_map(mm)
    assert np.array_equal(board.corners, c.astype(np.float32)) and list(board.ids) == list(range(6))


SQ = np.array([[0, 0, 0], [10, 0, 0], [10, -10, 0], [0, -10, 0]], np.float64)


@pytest.mark.parametrize("corners,message", [
    (SQ + [[np.nan, 0, 0], [0, 0, 0], [0, 0, 0], [0, 0, 0]], "a corner is not finite"),
    (SQ * 0.0, "a marker has no size"),
    (SQ * [1.0, 1.2, 1.0], "a marker's sides differ"),
    ([[0, 0, 0], [10, 0, 0], [16, -8, 0], [6, -8, 0]], "not at right angles"),
    (SQ + [[0, 0, 0], [0, 0, 0], [0, 0, 0.2], [0, 0, 0]], "do not lie in one plane"),
])
def test_every_refusal_raises_value_error_in_the_librarys_wording(corners, message):
    from pathlib import Path

    with pytest.raises(ValueError, match=message) as e:
        Board3D([1], [corners])
    header = (Path(__file__).resolve().parent.parent / "aruco3_amd" / "csrc" / "a3_board3d_check.h").read_text()
    assert f'"a3_set_board3d: {e.value}"' in header


def test_board_shape_refusals():
    with pytest.raises(ValueError, match="four corners per id"):
        Board3D([1, 2], [SQ])
    with pytest.raises(ValueError, match="an id appears twice"):
        Board3D([1, 1], [SQ, SQ + 20.0])
    with pytest.raises(ValueError, match="1 .. 1024 markers"):
        Board3D([], np.zeros((0, 4, 3)))
    with pytest.raises(ValueError, match="1 .. 1024 markers"):
        Board3D(list(range(1025)), [SQ] * 1025)
    Board3D([1], [SQ[::-1]])   # the other winding is the other printed side: a valid marker
    Board3D([1], [SQ * [100.0, 100.1, 1.0]])   # sides 1000 and 1001: at the tolerance, exactly


def test_detector_refuses_recovery_on_a_board3d():
    from aruco3_amd.aruco import Detector
    from aruco3_amd.board import BoardRecovery

    with pytest.raises(ValueError, match="planar board"):
        Detector(board=b3.cube(), recovery=BoardRecovery())
    det = Detector(board=b3.cube())
    with pytest.raises(ValueError, match="CharucoBoard"):
        det.detect_batch_with_charuco_pose(np.zeros((1, 8, 8, 3), np.uint8))


def test_the_entry_point_is_declared_everywhere():
    import re
    from pathlib import Path

    from aruco3_amd import _lib

    root = Path(__file__).resolve().parent.parent
    header = re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", (root / "include" / "aruco3_hip.h").read_text(), flags=re.S))
    assert "int a3_set_board3d(a3_ctx *ctx, const uint32_t *ids, const float *corners_xyz, size_t n);" in header
    assert re.search(r"#define\s+A3_ABI_VERSION\s+5\b", header)   # additive: the ABI version stays
    assert "a3_set_board3d" in _lib.SYMBOLS and hasattr(_lib.load(), "a3_set_board3d")
    assert re.search(r"pub\s+fn\s+a3_set_board3d\s*\(", (root / "integration" / "aruco3_hip.rs").read_text())
    launch = (root / "aruco3_amd" / "csrc" / "a3_launch.h").read_text()
    assert "hipError_t launch_board3d_pose(hipStream_t st, const BoardPoseLaunch& b);" in launch
    make = (root / "aruco3_amd" / "csrc" / "Makefile").read_text()
    assert "k_board3d.hip" in make and "a3_board3d_check.h" in make and "a3_board3d.h" in make
    import aruco3_amd

    assert aruco3_amd.Board3D is Board3D


def test_without_a_device_the_first_call_fails_and_nothing_falls_back():
    torch = pytest.importorskip("torch")
    if torch.cuda.is_available():
        pytest.skip("a GPU is present")
    from aruco3_amd import _lib
    from aruco3_amd.aruco import Detector

    det = Detector(board=b3.cube())   # (no context yet: the board reaches the library with the first call)
    with pytest.raises(_lib.A3Error) as e:
        det.detect_batch_with_board_pose(np.zeros((1, 8, 8, 3), np.uint8))
    assert e.value.code == _lib.ERR_NO_DEVICE


def test_cpu_detector_finds_every_drawn_marker():
    """every marker tests/board3d_util.py draws in the scenes of tests/test_gpu_board3d.py is found, once, by the CPU restatement of
    the detector on the host renderer's drawing: the GPU tests may hold markers_used to the number of markers drawn"""
    from aruco3_amd import ARDictionary
    from oracle import a3oracle

    d = ARDictionary.new_from_named_dict("ARUCO")
    codes = np.asarray(d.code_list, np.uint64)
    cfg = a3oracle.Config.default()
    cfg.min_corner_separation_factor = bu.MIN_CORNER_SEPARATION_FACTOR
    cube = b3.cube()
    scenes = b3.gpu_scenes(cube)
    assert [sum(1 for _, mid in sc.quads if mid in cube.ids and sc.R is not None) for sc in scenes] == [3, 2, 1, 0, 4, 0]
    assert [len(b3.visible(cube, sc.R, sc.t)) if sc.R is not None else 0 for sc in scenes] == b3.GPU_SCENE_DRAWN
    scenes = scenes + b3.accuracy_scenes(cube)
    assert all(len(sc.quads) >= 2 for sc in scenes[6:])
    imgs = b3.render_cpu(scenes, d)
    for f, sc in enumerate(scenes):
        res = a3oracle.detect(imgs[f], codes, d.num_bits, d._tau, cfg, keep_debug=False)
        assert sorted(m["id"] for m in res["markers"]) == sorted(mid for _, mid in sc.quads), f
