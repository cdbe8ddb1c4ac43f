"""3-D boards on the MI355X (k_board3d_pose; a3_set_board3d, served by a3_get_board_poses / a3_estimate_board_pose): equal to the CPU
restatement (tests/board3d_oracle.c) from the same markers and corners, in a batch, stand-alone and past the lanes' register cache;
a flat board through the 3-D path; a 3-D board changes no other result; switching between the two kinds of board; the scheduling
paths; the Detector surface; and the board pose beats single-marker poses on rendered cubes."""
import numpy as np
import pytest

from tests import board3d_oracle as o3
from tests import board3d_util as b3
from tests import board_util as bu
from tests.util import marker_tuples

pytestmark = pytest.mark.gpu

W, H = bu.W1080, bu.H1080
K = bu.K1080


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


def _dict():
    from aruco3_amd import ARDictionary

    return ARDictionary.new_from_named_dict("ARUCO")


def _intr():
    from aruco3_amd import _lib

    return _lib.Intrinsics(W, H, *K)


def _grid():
    from aruco3_amd.board import GridBoard

    return GridBoard(5, 7, 30.0, 6.0, first_id=10)


def _ctx(d, board3d=None, refine=False, planar=None):
    from aruco3_amd import _lib

    ctx = _lib.Context(bu.config(), d.code_list, d.num_bits, d._tau)
    if refine:
        ctx.set_corner_refinement(_lib.default_refine_config())
    if planar is not None:
        ctx.set_board(planar.ids, planar.corners)
    if board3d is not None:
        ctx.set_board3d(board3d.ids, board3d.corners)
    return ctx


def _same(got, want, where):
    """the tolerances of tests/test_gpu_board_pose.py::_check"""
    assert (got["status"], got["markers_used"], got["markers_rejected"]) == (want["status"], want["markers_used"], want["markers_rejected"]), where
    if not want["status"]:
        assert not got["rotation"].any() and got["rms_px"] == 0
        return
    assert np.abs(got["rotation"] - want["rotation"]).max() <= 1e-4, (where, got, want)
    assert np.linalg.norm(got["translation"] - want["translation"]) <= 1e-4 * np.linalg.norm(want["translation"]), (where, got, want)
    assert abs(got["rms_px"] - want["rms_px"]) <= 1e-3 * max(float(want["rms_px"]), 1e-3), (where, got, want)


def _check(board, markers, per, recs, refined=None, intr=None):
    """every frame's record against the oracle from the same markers and corners"""
    assert len(recs) == len(per)
    pos = 0
    for f in range(len(per)):
        cnt = int(per[f])
        mk = markers[pos: pos + cnt]
        px = refined[pos: pos + cnt] if refined is not None else mk["corners"].reshape(-1, 4, 2).astype(np.float32)
        _same(recs[f], o3.board_pose(board, mk["id"], px, image_size=(W, H), intrinsics=intr), f)
        pos += cnt


def _run_pose(ctx, dev, n, intr=None, size=b3.CUBE_MARKER):
    from aruco3_amd import _lib

    return ctx.detect_batch_pose(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, n, size, intr)


@pytest.fixture(scope="module")
def scene():
    torch = _torch()
    d = _dict()
    cube = b3.cube()
    scenes = b3.gpu_scenes(cube)
    dev = bu.render(scenes, d)
    torch.cuda.synchronize()
    return d, cube, scenes, dev


@pytest.fixture(scope="module")
def flat_scene():
    from tests.test_gpu_board_pose import _scenes

    torch = _torch()
    d = _dict()
    grid = _grid()
    scenes = [_scenes(grid)[k] for k in (0, 1, 3, 5)]
    dev = bu.render(scenes, d)
    torch.cuda.synchronize()
    return d, grid, scenes, dev


@pytest.mark.parametrize("use_intr", [False, True])
@pytest.mark.parametrize("refine", [False, True])
def test_batch_board_poses_equal_oracle(scene, use_intr, refine):
    d, cube, scenes, dev = scene
    ctx = _ctx(d, cube, refine)
    intr = _intr() if use_intr else None
    m, p, _ = _run_pose(ctx, dev, len(scenes), intr)
    recs = ctx.board_poses()
    assert [int(r["status"]) for r in recs] == [1, 1, 1, 0, 1, 0]
    # every drawn marker is found (tests/test_oracle_board3d.py checks the scenes on the CPU); scene 4 shows one of its three twice
    assert [int(r["markers_used"]) for r in recs] == [3, 2, 1, 0, 2, 0]
    assert [int(r["markers_rejected"]) for r in recs] == [0, 0, 0, 0, 2, 0]
    _check(cube, m, p, recs, ctx.refined_corners() if refine else None, intr)
    if use_intr:
        assert all(r["alt_rms_px"] >= r["rms_px"] for r in recs)   # fx == fy: the pixel cost orders the starts as the normalised cost does


def test_standalone_equals_in_batch(scene):
    from aruco3_amd import _lib

    d, cube, scenes, dev = scene
    ctx = _ctx(d, cube)
    intr = _intr()
    m, p, _ = _run_pose(ctx, dev, len(scenes), intr)
    recs = ctx.board_poses()
    pos = 0
    for f in range(len(scenes)):
        mk = m[pos: pos + int(p[f])]
        pos += int(p[f])
        one = ctx.estimate_board_pose(mk["id"], mk["corners"].reshape(-1, 4, 2).astype(np.float32), intrinsics=intr)
        assert one.tobytes() == recs[f].tobytes(), f
    ctx.set_board3d(None)
    with pytest.raises(_lib.A3Error) as e:
        ctx.estimate_board_pose(m["id"][:1], m["corners"][:1].reshape(-1, 4, 2), intrinsics=intr)
    assert e.value.code == _lib.ERR_INVALID


def test_many_corners_run_the_reread_loop():
    """two 9 x 9 grids at a right angle: 648 corners, past the 256 the lanes keep in registers"""
    _torch()
    d = _dict()
    board = b3.right_angle_grids(9)
    assert len(board) == 162
    R, t = b3.view_pose((-1.0, 0.25, 0.9), 12.0, 1400.0, centre=(0.0, -160.0, 0.0))
    assert len(b3.visible(board, R, t, 0.3)) == 162
    ctx = _ctx(d, board)
    for intr, Kp in ((_intr(), K), (None, (float(W), float(H), 0.0, 0.0))):
        px = b3.project(board, R, t, Kp).astype(np.float32)
        order = np.random.default_rng(5).permutation(162)   # (batch order is not slot order)
        got = ctx.estimate_board_pose(board.ids[order], px[order], image_size=(W, H), intrinsics=intr)
        _same(got, o3.board_pose(board, board.ids[order], px[order], image_size=(W, H), intrinsics=intr), intr is not None)
        assert got["markers_used"] == 162
        assert np.abs(got["rotation"].reshape(3, 3) - R).max() <= 1e-4
        assert np.linalg.norm(got["translation"] - t) <= 1e-4 * np.linalg.norm(t)


def test_flat_board_through_the_3d_path(flat_scene):
    from aruco3_amd.board import Board3D

    d, grid, scenes, dev = flat_scene
    lifted = Board3D.from_board(grid)
    intr = _intr()
    for refine in (False, True):
        c3, c2 = _ctx(d, lifted, refine), _ctx(d, planar=grid, refine=refine)
        m3, p3, q3 = _run_pose(c3, dev, len(scenes), intr, 30.0)
        m2, p2, q2 = _run_pose(c2, dev, len(scenes), intr, 30.0)
        assert marker_tuples(m3) == marker_tuples(m2) and p3.tolist() == p2.tolist() and q3.tobytes() == q2.tobytes()   # (a record's 4 padding bytes are not data)
        recs = c3.board_poses()
        assert [int(r["markers_used"]) for r in recs] == [int(r["markers_used"]) for r in c2.board_poses()]
        _check(lifted, m3, p3, recs, c3.refined_corners() if refine else None, intr)


def test_board3d_changes_nothing_else(scene):
    from aruco3_amd import _lib

    d, cube, scenes, dev = scene
    for refine in (False, True):
        plain, with_board = _ctx(d, None, refine), _ctx(d, cube, refine)
        m0, p0, q0 = _run_pose(plain, dev, len(scenes), _intr())
        m1, p1, q1 = _run_pose(with_board, dev, len(scenes), _intr())
        assert marker_tuples(m0) == marker_tuples(m1) and p0.tolist() == p1.tolist()
        assert q0.tobytes() == q1.tobytes()
        if refine:
            assert plain.refined_corners().tobytes() == with_board.refined_corners().tobytes()
        with pytest.raises(_lib.A3Error) as e:   # no board: no board poses
            plain.board_poses()
        assert e.value.code == _lib.ERR_INVALID
        with_board.detect_batch(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, len(scenes))
        with pytest.raises(_lib.A3Error) as e:   # not a pose batch
            with_board.board_poses()
        assert e.value.code == _lib.ERR_INVALID


def test_switching_boards(scene, flat_scene):
    from aruco3_amd import _lib
    from aruco3_amd.board import CharucoBoard

    d, cube, scenes, dev = scene
    _, grid, flat, flat_dev = flat_scene
    intr = _intr()

    def poses(ctx, frames, n, size):
        _run_pose(ctx, frames, n, intr, size)
        return ctx.board_poses().tobytes()

    want2, want3 = poses(_ctx(d, planar=grid), flat_dev, len(flat), 30.0), poses(_ctx(d, cube), dev, len(scenes), b3.CUBE_MARKER)
    ctx = _ctx(d, cube)
    ctx.set_board(grid.ids, grid.corners)
    assert poses(ctx, flat_dev, len(flat), 30.0) == want2
    ctx.set_board3d(cube.ids, cube.corners)
    assert poses(ctx, dev, len(scenes), b3.CUBE_MARKER) == want3
    ctx.set_board(grid.ids, grid.corners)   # (and back, with both kinds of tables uploaded before)
    assert poses(ctx, flat_dev, len(flat), 30.0) == want2
    # the settings that need a plane
    ctx.set_board3d(cube.ids, cube.corners)
    cb = CharucoBoard(4, 4, 40.0, 30.0)
    for call, msg in ((lambda: ctx.set_charuco(cb.chessboard_corners, cb.adjacent_ids), "a3_set_charuco: the board is a 3-D board"),
                      (lambda: ctx.set_board_recovery(ctx.default_recover_config()), "a3_set_board_recovery: the board is a 3-D board")):
        with pytest.raises(_lib.A3Error, match=msg) as e:
            call()
        assert e.value.code == _lib.ERR_INVALID
    ctx.set_board_recovery(None)   # (switching it off is always allowed)
    ctx.set_charuco(None)
    # a 3-D board switches recovery off
    ctx.set_board(grid.ids, grid.corners)
    ctx.set_board_recovery(ctx.default_recover_config())
    ctx.set_board3d(cube.ids, cube.corners)
    assert poses(ctx, dev, len(scenes), b3.CUBE_MARKER) == want3
    with pytest.raises(_lib.A3Error) as e:
        ctx.recovered_counts(len(scenes))
    assert e.value.code == _lib.ERR_INVALID
    # not while a batch is in flight
    ctx.submit_pose(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, len(scenes), b3.CUBE_MARKER, intr)
    with pytest.raises(_lib.A3Error, match="a3_set_board3d: a submitted batch has not been collected") as e:
        ctx.set_board3d(cube.ids, cube.corners)
    assert e.value.code == _lib.ERR_INVALID
    ctx.collect_pose()
    assert ctx.board_poses().tobytes() == want3
    # clearing
    ctx.set_board3d(None)
    with pytest.raises(_lib.A3Error) as e:
        ctx.estimate_board_pose([10], bu.square_quad(500, 500, 90)[None], intrinsics=intr)
    assert e.value.code == _lib.ERR_INVALID
    _run_pose(ctx, dev, len(scenes), intr)
    with pytest.raises(_lib.A3Error):
        ctx.board_poses()


def test_set_board3d_errors(scene):
    from aruco3_amd import _lib

    d, cube, _, _ = scene
    ctx = _ctx(d)
    sq = np.array([[0, 0, 0], [10, 0, 0], [10, -10, 0], [0, -10, 0]], np.float32)
    for ids, corners, msg in [([0], [sq * [1, 1.2, 1]], "sides differ"), ([0], [sq + [[0, 0, 0], [0, 0, 0], [0, 0, 0.2], [0, 0, 0]]], "one plane"),
                              ([0, 0], [sq, sq + 20], "appears twice"), ([len(d.code_list)], [sq], "not in the dictionary"),
                              (list(range(1025)), [sq] * 1025, "more than A3_BOARD_MAX_MARKERS")]:
        with pytest.raises(_lib.A3Error, match=msg) as e:
            ctx.set_board3d(ids, corners)
        assert e.value.code == _lib.ERR_INVALID


def _expected(d, cube, dev, n, intr):
    ctx = _ctx(d, cube)
    m, p, _ = _run_pose(ctx, dev, n, intr)
    return marker_tuples(m), p.tolist(), ctx.board_poses().tobytes()


@pytest.mark.parametrize("gates", [False, True])
def test_four_context_rotation_gives_the_same_board_poses(scene, gates):
    from aruco3_amd import _lib

    d, cube, scenes, dev = scene
    intr = _intr()
    ctxs = [_ctx(d, cube) for _ in range(4)]
    want = [_expected(d, cube, dev[f: f + 1], 1, intr) for f in range(len(scenes))]
    got = [None] * len(scenes)
    inflight = {}
    for f in range(len(scenes) + 4):
        k = f % 4
        if k in inflight:
            g = inflight.pop(k)
            m, p, _ = ctxs[k].collect_pose()
            got[g] = (marker_tuples(m), p.tolist(), ctxs[k].board_poses().tobytes())
        if f < len(scenes):
            if gates:
                for j in range(k + 1, 4):
                    ctxs[k].order_after(ctxs[j])
            ctxs[k].submit_pose(dev[f].data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, 1, b3.CUBE_MARKER, intr)
            inflight[k] = f
    assert got == want


def test_detector_surface(scene):
    from aruco3_amd.aruco import BatchQueue, Detector, DetectorConfig
    from aruco3_amd.pinhole import CameraIntrinsics

    d, cube, scenes, dev = scene
    det = Detector(DetectorConfig(min_corner_separation_factor=bu.MIN_CORNER_SEPARATION_FACTOR), d, board=cube)
    ci = CameraIntrinsics(W, H, *K)
    R, t = scenes[0].R, scenes[0].t

    def close(bp):
        assert bp.ok and bp.markers_used == 3
        assert bu.rotation_error_deg(bp.rotation, R) < 1.0
        c = bp.apply_transform_to_points([(0.0, 0.0, 0.0)])[0]
        assert np.linalg.norm(np.array(c) - t) < 0.02 * np.linalg.norm(t)

    out = det.detect_batch_with_board_pose(dev, ci, marker_size_mm=b3.CUBE_MARKER)
    assert len(out) == len(scenes) and [bp.ok for _, bp in out] == [True, True, True, False, True, False]
    close(out[0][1])
    q = BatchQueue(det, depth=2)
    try:
        q.submit_with_board_pose(dev[:2], ci, marker_size_mm=b3.CUBE_MARKER)
        q.submit_with_board_pose(dev[2:], ci, marker_size_mm=b3.CUBE_MARKER)
        got = q.collect_with_board_pose() + q.collect_with_board_pose()
    finally:
        q.close()
    close(got[0][1])
    for (da, a), (db, b) in zip(out, got):
        assert [mk.id for mk in da.markers] == [mk.id for mk in db.markers]
        assert (a.status, a.markers_used, a.iterations, a.rms_px) == (b.status, b.markers_used, b.iterations, b.rms_px)
        assert np.array_equal(a.rotation, b.rotation) and np.array_equal(a.translation, b.translation)


def test_accuracy_against_the_renderers_truth():
    """16 random cube poses at 1080p showing two or three faces, known K: median errors of the board pose against those of the best
    single-marker IPPE pose of each frame (carried into the board frame through the marker's own).  The ordering is asserted on the
    detector's own corners.  With sub-pixel refinement on, the medians are printed and not compared: the comparator picks the better
    of a frame's two or three markers knowing the truth, which a least-squares fit of both is not expected to beat once the corners'
    errors are small and alike, and in 5 of these 16 frames the refinement moves one corner of a steep face by 4 to 5 px, which spoils
    that marker and the fit but not the other marker.  Measured on an MI355X: detector corners, board 0.649 deg / 0.0019 against
    1.023 deg / 0.0038; refined corners, board 0.154 deg / 0.0017 against 0.124 deg / 0.0022, the board pose within 0.03 deg of the
    float64 least-squares optimum of the same corners in every frame."""
    torch = _torch()
    d = _dict()
    cube = b3.cube()
    scenes = b3.accuracy_scenes(cube)
    dev = bu.render(scenes, d)
    torch.cuda.synchronize()
    intr = _intr()
    c = cube.corners.astype(np.float64)
    ex, ey = c[:, 1] - c[:, 0], c[:, 0] - c[:, 3]
    ex, ey = ex / np.linalg.norm(ex, axis=1, keepdims=True), ey / np.linalg.norm(ey, axis=1, keepdims=True)
    frame = np.stack([ex, ey, np.cross(ex, ey)], axis=2)   # (slot, 3, 3): marker -> board
    centre = c.mean(axis=1)
    for refine in (False, True):
        ctx = _ctx(d, cube, refine)
        m, p, poses = _run_pose(ctx, dev, len(scenes), intr)
        recs = ctx.board_poses()
        rb, tb, rs, ts = [], [], [], []
        pos = 0
        for f, sc in enumerate(scenes):
            assert recs[f]["status"] == 1 and recs[f]["markers_used"] >= 2
            rb.append(bu.rotation_error_deg(recs[f]["rotation"].reshape(3, 3), sc.R))
            tb.append(np.linalg.norm(recs[f]["translation"] - sc.t) / np.linalg.norm(sc.t))
            best_r, best_t = 1e9, 1e9
            for i in range(pos, pos + int(p[f])):
                if m[i]["id"] not in cube.ids or not np.all(np.isfinite(poses[i, 0])):
                    continue
                slot = int(np.nonzero(cube.ids == m[i]["id"])[0][0])
                Rb = poses[i, 0, 1:10].reshape(3, 3).astype(np.float64) @ frame[slot].T
                best_r = min(best_r, bu.rotation_error_deg(Rb, sc.R))
                best_t = min(best_t, np.linalg.norm(poses[i, 0, 10:13] - Rb @ centre[slot] - sc.t) / np.linalg.norm(sc.t))
            pos += int(p[f])
            rs.append(best_r)
            ts.append(best_t)
        res = (np.median(rb), np.median(tb), np.median(rs), np.median(ts))
        print(f"refine={refine}: board rot {res[0]:.3f} deg, trans {res[1]:.4f}; best single marker rot {res[2]:.3f} deg, trans {res[3]:.4f}")
        if not refine:
            assert res[0] < res[2] and res[1] < res[3]
