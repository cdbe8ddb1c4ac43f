"""Detection on reduced frames on the MI355X (a3_set_reduction; k_reduce_frames ahead of the threshold kernel, k_scale_markers behind
the marker list): markers and mapped corners against the oracle detector on the numpy-reduced plane (tests/reduced_cases.py), the same
call against the two-call form, and everything behind the marker list -- refined corners, poses, the board pose, ChArUco corners --
against the oracles from the mapped corners on the FULL-SIZE frames.  tests/test_reduced_detection.py checks on the CPU that none of
the expectations used here is empty."""
import ctypes as C

import numpy as np
import pytest

from tests import board_oracle as bo
from tests import board_util as bu
from tests import reduced_cases as rd
from tests.util import marker_tuples, markers_of_hip, markers_of_oracle

pytestmark = pytest.mark.gpu

W, H = rd.SIZE
SIZE_MM = 30.0


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


def _rec(f):
    from aruco3_amd import _lib

    return _lib.ReductionRec(f)


def _ctx(f=None, window=None):
    from aruco3_amd import _lib

    _torch()
    assert hasattr(_lib.load(), "a3_set_reduction"), "the library has no a3_set_reduction"
    d = rd.dictionary()
    cfg = bu.config()
    if window is not None:
        cfg.threshold_window = window
    ctx = _lib.Context(cfg, d.code_list, d.num_bits, d._tau)
    if f is not None:
        ctx.set_reduction(_rec(f))
    return ctx


def _layouts(f):
    """the factor's frames as (name, call arguments, keepalive): RGB8 and BGRA8 on the device, RGB8 on the host"""
    from aruco3_amd import _lib

    torch = _torch()
    rgb = rd.frames(f).copy()
    n = len(rgb)
    dev = torch.from_numpy(rgb).cuda()
    dev4 = torch.from_numpy(rd.bgra(rgb)).cuda()
    torch.cuda.synchronize()
    return [("rgb8_device", (dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, n), dev),
            ("bgra8_device", (dev4.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_BGRA8, W, H, W * 4, W * H * 4, n), dev4),
            ("rgb8_host", (rgb.ctypes.data, _lib.MEM_HOST, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, n), rgb)]


def _same_as_expectation(m, per, res, what):
    """ids, codes, mapped corners, hamming distances, rotations, candidate indices, order and per-frame counts"""
    assert [int(v) for v in per] == [len(r["markers"]) for r in res], what
    pos = 0
    for k, r in enumerate(res):
        mk = m[pos: pos + int(per[k])]
        assert markers_of_hip(mk) == markers_of_oracle(r), (what, k)
        assert [int(v) for v in mk["candidate_index"]] == [x["candidate_index"] for x in r["markers"]], (what, k)
        assert all(int(v) == k for v in mk["frame"])
        pos += int(per[k])
    assert pos == len(m)


def _bit_equal(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, (what, bad[:4].tolist())


# ---- 1. the markers, and the two-call form ----

@pytest.mark.parametrize("f", rd.FACTORS)
def test_markers_equal_the_oracle_on_the_reduced_plane(f):
    _, res, _ = rd.expectation(f)
    ctx = _ctx(f)
    for name, args, keep in _layouts(f):
        m, per = ctx.detect_batch(*args)
        _same_as_expectation(m, per, res, (f, name))
    ctx.close()


@pytest.mark.parametrize("f", rd.FACTORS)
def test_one_call_equals_reduce_then_detect_then_map(f):
    """the same call against a3_reduce_frames to a packed plane, a plain detector on it as A3_FMT_L8, and the corner map in numpy --
    and with taps on a3_download_grey returns that plane byte for byte"""
    from aruco3_amd import _lib

    torch = _torch()
    planes, _, _ = rd.expectation(f)
    n, h, w = planes.shape
    for name, args, keep in _layouts(f)[:2]:
        one = _ctx(f)
        one.set_debug_taps(True)
        m1, per1 = one.detect_batch(*args)
        for k in range(n):
            assert np.array_equal(one.download_grey(k, w, h), planes[k]), (f, name, k)
            assert one.candidates(k).shape[0] >= int(per1[k])   # (the taps report the reduced view)
        two = _ctx()
        plane = torch.empty((n, h, w), dtype=torch.uint8, device="cuda")
        torch.cuda.synchronize()
        two.reduce_frames(*args[:8], f, plane.data_ptr(), _lib.MEM_DEVICE, w, w * h)
        assert np.array_equal(plane.cpu().numpy(), planes)
        m2, per2 = two.detect_batch(plane.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_L8, w, h, w, w * h, n)
        m2 = m2.copy()
        m2["corners"] = f * m2["corners"] + f // 2
        assert marker_tuples(m1) == marker_tuples(m2) and np.array_equal(per1, per2) and len(m1) >= 3 * n, (f, name)
        one.close()
        two.close()


# ---- 2. behind the marker list: the full-size frames ----

def _want_poses(oracle, refined, intr):
    out = []
    for q in np.asarray(refined, np.float32):
        if intr is not None:
            pts = np.stack([(q[:, 0] - np.float32(intr.principal_x)) / np.float32(intr.focal_x),
                            (q[:, 1] - np.float32(intr.principal_y)) / np.float32(intr.focal_y)], axis=1)
        else:
            pts = np.stack([q[:, 0] / np.float32(W), q[:, 1] / np.float32(H)], axis=1)   # the FULL size
        p1, p2 = oracle.solve_with_normalized_points(pts.astype(np.float32).reshape(8), SIZE_MM)
        out.append(np.array([np.concatenate([[e], np.asarray(r).reshape(9), t]) for e, r, t in (p1, p2)], np.float32))
    return np.array(out, np.float32)


def _check_board(board, m, per, recs, px, intr):
    """tests/test_gpu_board_pose.py's comparison, with the full image size"""
    pos = 0
    for k in range(len(per)):
        cnt = int(per[k])
        want = bo.board_pose(board, m["id"][pos: pos + cnt], px[pos: pos + cnt], image_size=(W, H), intrinsics=intr)
        got = recs[k]
        pos += cnt
        assert (got["status"], got["markers_used"], got["markers_rejected"]) == (want["status"], want["markers_used"], want["markers_rejected"]), k
        assert want["status"] == 1 and want["markers_used"] >= 3
        assert np.abs(got["rotation"] - want["rotation"]).max() <= 1e-4, (k, got, want)
        assert np.linalg.norm(got["translation"] - want["translation"]) <= 1e-4 * np.linalg.norm(want["translation"]), (k, got, want)
        assert abs(got["rms_px"] - want["rms_px"]) <= 1e-3 * max(float(want["rms_px"]), 1e-3), (k, got, want)


@pytest.mark.parametrize("with_intrinsics", [True, False])
@pytest.mark.parametrize("f", rd.FACTORS)
def test_refined_corners_poses_and_board_pose(oracle, f, with_intrinsics):
    """with CornerRefinement's defaults: refined corners bit-equal to the oracle's refinement of the MAPPED corners on the full-size
    luma; marker poses bit-equal to the oracle's IPPE of them (tests/test_gpu_corner_refine.py's comparison; without intrinsics
    normalised by the full W x H); the board pose within tests/test_gpu_board_pose.py's tolerances.  Then without refinement: the poses
    from the mapped integer corners (tests/test_gpu_round3.py's tolerances)."""
    from aruco3_amd import _lib

    _, res, refined = rd.expectation(f)
    want_ref = np.concatenate(refined)
    intr = _lib.Intrinsics(W, H, *rd.K) if with_intrinsics else None
    board = rd.board()
    ctx = _ctx(f)
    ctx.set_board(board.ids, board.corners)
    ctx.set_corner_refinement(_lib.default_refine_config())
    for name, args, keep in _layouts(f):
        m, per, poses = ctx.detect_batch_pose(*args, SIZE_MM, intr)
        _same_as_expectation(m, per, res, (f, name))
        got_ref = ctx.refined_corners()
        _bit_equal(got_ref, want_ref, (f, name, "refined"))
        _bit_equal(poses, _want_poses(oracle, want_ref, intr), (f, name, "poses"))
        _check_board(board, m, per, ctx.board_poses(), got_ref, intr)
    ctx.set_corner_refinement(None)
    name, args, keep = _layouts(f)[0]
    m, per, poses = ctx.detect_batch_pose(*args, SIZE_MM, intr)
    _same_as_expectation(m, per, res, (f, "unrefined"))
    for i, rec in enumerate(m):
        c = rec["corners"]
        ref = (oracle.solve_with_intrinsics(c, SIZE_MM, *rd.K) if with_intrinsics else oracle.solve_with_undistorted_points(c, SIZE_MM, (W, H)))
        for (e, r, t), q in zip(ref, poses[i]):
            assert abs(float(q[0]) - e) <= 1e-4 and np.abs(q[1:10].reshape(3, 3) - np.asarray(r).reshape(3, 3)).max() <= 1e-4, (f, i)
    _check_board(board, m, per, ctx.board_poses(), m["corners"].reshape(-1, 4, 2).astype(np.float32), intr)
    ctx.close()


@pytest.mark.parametrize("f", [2, 3])
def test_charuco_corners_equal_the_stand_alone_call(f):
    """a ChArUco board rendered on the device at the cases' size: the batch's chessboard corners equal a3_interpolate_charuco given the
    same mapped markers and the full-size frames"""
    from aruco3_amd import _lib
    from aruco3_amd.board import CharucoBoard
    from tests import charuco_util as cu

    torch = _torch()
    b = CharucoBoard(4, 3, 40.0, 28.0, first_id=5)
    scenes = []
    # (frontal views: a ChArUco marker has a 6 mm white rim inside its square, 18 - 20 px here and 6 at factor 3, which a tilt eats up)
    for distance, off in ((200.0, (0.0, 0.0)), (180.0, (-45.0, 35.0))):
        R, t = bu.board_pose_facing(b, 0.0, 0.0, 0.0, distance, off, K=rd.K)
        scenes.append(cu.Scene(b, R, t, K=rd.K))
    dev = cu.render(scenes, rd.dictionary(), W, H)
    torch.cuda.synchronize()
    ctx = _ctx(f)
    ctx.set_board(b.ids, b.corners)
    ctx.set_charuco(b.chessboard_corners, b.adjacent_ids, None)
    m, per = ctx.detect_batch(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, len(scenes))
    recs = ctx.charuco_corners()
    assert len(m) >= 3 * len(scenes) and len(recs) >= 4, (len(m), len(recs))
    assert np.all(m["corners"] % f == f // 2)   # (mapped corners)
    alone = _ctx()   # (no reduction: the stand-alone call never looks at the setting anyway)
    alone.set_board(b.ids, b.corners)
    alone.set_charuco(b.chessboard_corners, b.adjacent_ids, None)
    pos = 0
    for k in range(len(scenes)):
        cnt = int(per[k])
        px = m["corners"][pos: pos + cnt].reshape(-1, 4, 2).astype(np.float32)
        for c in (ctx, alone):
            got = c.interpolate_charuco(dev[k].data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, m["id"][pos: pos + cnt], px)
            want = recs[recs["frame"] == k].copy()
            want["frame"] = 0
            assert got.dtype == want.dtype and got.shape == want.shape and len(got) >= 2, (f, k)
            for field in got.dtype.names:
                assert np.ascontiguousarray(got[field]).tobytes() == np.ascontiguousarray(want[field]).tobytes(), (f, k, field)
        pos += cnt
    ctx.close()
    alone.close()


@pytest.mark.parametrize("f", [2, 4])
def test_threshold_window_16_samples_the_reduced_grey_plane(f):
    """the separable threshold path: the decode stage samples the reduced grey plane, the refinement still the caller's frames"""
    from aruco3_amd import _lib

    _, res, refined = rd.expectation(f, 16)
    assert all(len(r["markers"]) >= 3 for r in res)
    ctx = _ctx(f, window=16)
    ctx.set_corner_refinement(_lib.default_refine_config())
    for name, args, keep in _layouts(f):
        m, per = ctx.detect_batch(*args)
        _same_as_expectation(m, per, res, (f, name))
        _bit_equal(ctx.refined_corners(), np.concatenate(refined), (f, name))
    ctx.close()


# ---- 3. in flight, and the Python surface ----

@pytest.mark.parametrize("f", [2, 3])
def test_batch_queue_equals_the_synchronous_call(f):
    """two contexts in rotation, one batch each"""
    from aruco3_amd import Detector, DetectorConfig, Reduction
    from aruco3_amd.aruco import BatchQueue, CornerRefinement

    torch = _torch()
    _, res, refined = rd.expectation(f)
    det = Detector(DetectorConfig(min_corner_separation_factor=bu.MIN_CORNER_SEPARATION_FACTOR), rd.dictionary(), refinement=CornerRefinement(),
                   reduction=Reduction(f))
    rgb = rd.frames(f).copy()
    batches = [torch.from_numpy(rgb[:2]).cuda(), rgb[2:]]   # one on the device, one on the host
    torch.cuda.synchronize()
    want = [det.detect_batch(b) for b in batches]
    flat = [d for w in want for d in w]
    assert [[(m.id, m.code, tuple(m.corners), m.hamming_distance) for m in d.markers] for d in flat] == \
        [[(x["id"], x["code"], tuple(x["corners"]), x["hamming_distance"]) for x in r["markers"]] for r in res]
    for d, ref in zip(flat, refined):
        _bit_equal(np.array([m.corners_refined for m in d.markers], np.float32), ref, f)
    q = BatchQueue(det, depth=2)
    for b in batches:
        q.submit(b)
    got = [q.collect(), q.collect()]
    q.close()
    assert got == want
    # populate=True returns the reduced grey plane
    planes, _, _ = rd.expectation(f)
    tapped = det.detect_batch(rgb[:1], populate=True)
    assert np.array_equal(tapped[0].grey, planes[0]) and tapped[0].markers == want[0][0].markers


def test_set_get_unset_and_refusals():
    from aruco3_amd import _lib

    torch = _torch()
    f = 3
    _, res, _ = rd.expectation(f)
    name, args, keep = _layouts(f)[0]
    ctx = _ctx()
    assert ctx.reduction() is None
    fresh_m, fresh_per = ctx.detect_batch(*args)
    ctx.set_reduction(_rec(f))
    assert bytes(ctx.reduction()) == bytes(_rec(f))
    m, per = ctx.detect_batch(*args)
    _same_as_expectation(m, per, res, "set")
    # the setter during a submitted batch is refused, and the batch keeps its setting
    ctx.submit(*args)
    for r in (None, _rec(2)):
        with pytest.raises(_lib.A3Error) as e:
            ctx.set_reduction(r)
        assert e.value.code == _lib.ERR_INVALID and "a3_set_reduction: a submitted batch has not been collected" in str(e.value)
    assert ctx.reduction().factor == f
    m, per = ctx.collect()
    _same_as_expectation(m, per, res, "submitted")
    # bad records
    for bad in (0, 1, 5):
        with pytest.raises(_lib.A3Error) as e:
            ctx.set_reduction(_rec(bad))
        assert e.value.code == _lib.ERR_INVALID and "a3_set_reduction: factor must be 2, 3 or 4" in str(e.value)
    r = _rec(2)
    r.reserved[1] = 1
    with pytest.raises(_lib.A3Error) as e:
        ctx.set_reduction(r)
    assert "a3_reduction.reserved must be 0" in str(e.value) and ctx.reduction().factor == f   # (a refused record is not kept)
    # together with a rectification: refused either way round
    rect = _lib.default_rectify(_lib.Intrinsics(W, H, *rd.K))
    with pytest.raises(_lib.A3Error) as e:
        ctx.set_rectification(rect)
    assert e.value.code == _lib.ERR_INVALID and "a3_set_rectification: a reduction is set" in str(e.value) and ctx.rectification() is None
    # frames smaller than one block
    with pytest.raises(_lib.A3Error) as e:
        ctx.detect_batch(args[0], args[1], args[2], 2, 9, 6, 54, 1)
    assert e.value.code == _lib.ERR_INVALID and "at least one block" in str(e.value)
    # NULL: off again -- what a context that never had the setting returns
    ctx.set_reduction(None)
    assert ctx.reduction() is None
    raw, on = _lib.ReductionRec(9), C.c_int(7)
    assert _lib.load().a3_get_reduction(ctx.handle, C.byref(raw), C.byref(on)) == 0 and on.value == 0 and bytes(raw) == bytes(16)
    m2, per2 = ctx.detect_batch(*args)
    never = _ctx()
    m3, per3 = never.detect_batch(*args)
    assert marker_tuples(m2) == marker_tuples(m3) == marker_tuples(fresh_m) and np.array_equal(per2, per3) and np.array_equal(per2, fresh_per)
    assert len(m2) >= 3 and marker_tuples(m2) != marker_tuples(m)
    ctx.set_rectification(rect)
    with pytest.raises(_lib.A3Error) as e:
        ctx.set_reduction(_rec(2))
    assert e.value.code == _lib.ERR_INVALID and "a3_set_reduction: a rectification is set" in str(e.value) and ctx.reduction() is None
    ctx.close()
    never.close()
