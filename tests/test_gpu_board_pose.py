"""Board pose on the MI355X (k_board_pose; a3_set_board / a3_get_board_poses / a3_estimate_board_pose): equal to the CPU restatement
(tests/board_oracle.c) from the same markers and corners, in every input form and through every scheduling path; the stand-alone call
equals the in-batch result; a board changes no other result; and the board pose beats single-marker poses on rendered boards."""
import math

import numpy as np
import pytest

from tests import board_oracle as bo
from tests import board_util as bu
from tests.util import marker_tuples

pytestmark = pytest.mark.gpu

W, H = bu.W1080, bu.H1080
K = bu.K1080
EXTRA = [(150.0, 150.0), (1770.0, 150.0), (150.0, 930.0), (1770.0, 930.0)]   # image spots for markers off the board


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


def _board():
    from aruco3_amd.board import GridBoard

    return GridBoard(5, 7, 30.0, 6.0, first_id=10)


def _extra(sc, spot, mid, side=90.0, angle=0.0):
    sc.quads.append((bu.square_quad(*EXTRA[spot], side, angle), mid))
    return sc


def _scenes(board):
    """0: whole board; 1: some board markers + foreign ids; 2: nothing; 3: one board marker + a foreign id; 4: whole board + a second
    instance of one of its ids; 5: near-frontal (ambiguous); 6: only foreign ids"""
    out = []
    R, t = bu.board_pose_facing(board, 35.0, 20.0, 10.0, 520.0)
    out.append(bu.board_scene(board, R, t))
    R, t = bu.board_pose_facing(board, 25.0, 100.0, -15.0, 520.0, (40.0, -20.0))
    out.append(_extra(_extra(bu.board_scene(board, R, t, keep=[0, 3, 7, 12, 18, 19, 25, 33]), 0, 300), 3, 901, angle=20.0))
    out.append(bu.Scene())
    R, t = bu.board_pose_facing(board, 20.0, 45.0, 5.0, 520.0)
    out.append(_extra(bu.board_scene(board, R, t, keep=[16]), 1, 500))
    R, t = bu.board_pose_facing(board, 45.0, -30.0, 0.0, 520.0)
    out.append(_extra(bu.board_scene(board, R, t), 2, int(board.ids[12]), angle=-10.0))
    R, t = bu.board_pose_facing(board, 2.0, 0.0, 0.0, 520.0)
    out.append(bu.board_scene(board, R, t))
    out.append(_extra(_extra(bu.Scene(), 0, 700), 1, 701))
    return out


def _ctx(d, board=None, refine=False):
    from aruco3_amd import _lib

    ctx = _lib.Context(bu.config(), d.code_list, d.num_bits, d._tau)
    if refine:
        ctx.set_corner_refinement(_lib.default_refine_config())
    if board is not None:
        ctx.set_board(board.ids, board.corners)
    return ctx


def _check(board, markers, per, recs, refined=None, intr=None, frames=None):
    """every frame's record against the oracle from the same markers and corners"""
    assert len(recs) == len(per)
    pos = 0
    for f in range(len(per)):
        cnt = int(per[f])
        mk = markers[pos: pos + cnt]
        px = refined[pos: pos + cnt] if refined is not None else mk["corners"].reshape(-1, 4, 2).astype(np.float32)
        want = bo.board_pose(board, mk["id"], px, image_size=(W, H), intrinsics=intr)
        got = recs[f]
        pos += cnt
        if frames is not None and f not in frames:
            continue
        assert (got["status"], got["markers_used"], got["markers_rejected"]) == (want["status"], want["markers_used"], want["markers_rejected"]), f
        if not want["status"]:
            assert not got["rotation"].any() and got["rms_px"] == 0
            continue
        assert np.abs(got["rotation"] - want["rotation"]).max() <= 1e-4, (f, got, want)
        assert np.linalg.norm(got["translation"] - want["translation"]) <= 1e-4 * np.linalg.norm(want["translation"]), (f, got, want)
        assert abs(got["rms_px"] - want["rms_px"]) <= 1e-3 * max(float(want["rms_px"]), 1e-3), (f, got, want)


@pytest.fixture(scope="module")
def scene():
    torch = _torch()
    d = _dict()
    board = _board()
    scenes = _scenes(board)
    dev = bu.render(scenes, d)
    torch.cuda.synchronize()
    return d, board, scenes, dev


def _run_pose(ctx, dev, n, intr=None, size=30.0):
    from aruco3_amd import _lib

    return ctx.detect_batch_pose(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, n, size, intr)


@pytest.mark.parametrize("use_intr", [False, True])
@pytest.mark.parametrize("refine", [False, True])
def test_batch_board_poses_equal_oracle(scene, use_intr, refine):
    d, board, scenes, dev = scene
    ctx = _ctx(d, board, refine)
    intr = _intr() if use_intr else None
    m, p, _ = _run_pose(ctx, dev, len(scenes), intr)
    recs = ctx.board_poses()
    assert [int(r["status"]) for r in recs] == [1, 1, 0, 1, 1, 1, 0]
    assert recs[0]["markers_used"] == 35 and recs[4]["markers_used"] >= 30 and recs[4]["markers_rejected"] == 2
    assert recs[1]["markers_used"] == 8 and recs[3]["markers_used"] == 1 and recs[6]["markers_rejected"] == 0
    _check(board, m, p, recs, ctx.refined_corners() if refine else None, intr)
    if use_intr:
        # fx == fy: the pixel cost orders the starts as the normalised cost does
        assert all(r["alt_rms_px"] >= r["rms_px"] for r in recs)
        # the near-frontal board is ambiguous: both starts end close (errors only).  (Without intrinsics the x / w, y / h
        # normalisation is no pinhole camera for these frames, and the residuals are tens of pixels whichever start wins.)
        assert abs(recs[5]["alt_rms_px"] - recs[5]["rms_px"]) <= 0.5 * recs[5]["rms_px"] + 0.05


@pytest.mark.parametrize("form", ["L8", "RGBA8", "BGRA8", "host_strided"])
def test_formats_and_layouts(scene, form):
    from aruco3_amd import _lib

    torch = _torch()
    d, board, scenes, dev = scene
    n = len(scenes)
    ctx = _ctx(d, board, refine=True)
    intr = _intr()
    if form == "host_strided":
        host = np.zeros((n, H, W * 3 + 48), np.uint8)
        host[:, :, : W * 3] = dev.cpu().numpy().reshape(n, H, W * 3)
        args = (host.ctypes.data, _lib.MEM_HOST, _lib.FMT_RGB8, W, H, W * 3 + 48, H * (W * 3 + 48))
    elif form == "L8":
        g = dev[..., 0].contiguous()
        args = (g.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_L8, W, H, W, W * H)
    else:
        a = torch.cat([dev, torch.full_like(dev[..., :1], 255)], dim=-1)
        if form == "BGRA8":
            a = a[..., [2, 1, 0, 3]]
        a = a.contiguous()
        args = (a.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGBA8 if form == "RGBA8" else _lib.FMT_BGRA8, W, H, W * 4, W * H * 4)
    torch.cuda.synchronize()
    m, p, _ = ctx.detect_batch_pose(*args, n, 30.0, intr)
    _check(board, m, p, ctx.board_poses(), ctx.refined_corners(), intr)


def test_mixed_marker_sizes():
    from aruco3_amd.board import Board

    torch = _torch()
    d = _dict()
    sq = np.array([[-1, 1], [1, 1], [1, -1], [-1, -1]], np.float64)
    rot = lambda a: np.array([[math.cos(a), -math.sin(a)], [math.sin(a), math.cos(a)]])
    board = Board([40, 41, 42, 43, 44], [sq * 32 @ rot(0.3).T + [0, 0], sq * 25 + [120, 30], sq * 30 @ rot(-0.5).T + [-125, -40],
                                          sq * 35 + [20, -140], sq * 27.5 + [-100, 120]])
    R, t = bu.board_pose_facing(board, 30.0, 60.0, 0.0, 650.0)
    dev = bu.render([bu.board_scene(board, R, t)], d)
    torch.cuda.synchronize()
    ctx = _ctx(d, board)
    intr = _intr()
    m, p, _ = _run_pose(ctx, dev, 1, intr)
    recs = ctx.board_poses()
    assert recs[0]["markers_used"] >= 4   # (all five, unless the detector reads one of them twice: then that one is rejected)
    _check(board, m, p, recs, None, intr)
    assert bu.rotation_error_deg(recs[0]["rotation"].reshape(3, 3), R) < 1.0


def test_standalone_equals_in_batch(scene):
    d, board, scenes, dev = scene
    ctx = _ctx(d, board)
    intr = _intr()
    m, p, _ = _run_pose(ctx, dev, len(scenes), intr)
    recs = ctx.board_poses()
    pos = 0
    for f in range(len(scenes)):
        mk = m[pos: pos + int(p[f])]
        pos += int(p[f])
        one = ctx.estimate_board_pose(mk["id"], mk["corners"].reshape(-1, 4, 2).astype(np.float32), intrinsics=intr)
        assert one.tobytes() == recs[f].tobytes(), f
    ctx.set_board(None)
    from aruco3_amd import _lib

    with pytest.raises(_lib.A3Error):
        ctx.estimate_board_pose(m["id"][:1], m["corners"][:1].reshape(-1, 4, 2), intrinsics=intr)


def test_board_changes_nothing_else(scene):
    from aruco3_amd import _lib

    d, board, scenes, dev = scene
    for refine in (False, True):
        plain, with_board = _ctx(d, None, refine), _ctx(d, board, refine)
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


def test_set_board_errors(scene):
    from aruco3_amd import _lib

    d, board, _, _ = scene
    ctx = _ctx(d)
    sq = np.array([[0, 0], [10, 0], [10, -10], [0, -10]], np.float32)
    for ids, corners in [([0], [sq[::-1]]), ([0], [np.array([[0, 0], [10, 0], [10, -12], [0, -12]], np.float32)]), ([0, 0], [sq, sq + 20]),
                         ([len(d.code_list)], [sq]), (list(range(1025)), [sq] * 1025)]:
        with pytest.raises(_lib.A3Error) as e:
            ctx.set_board(ids, corners)
        assert e.value.code == _lib.ERR_INVALID


def _expected(ctx_factory, board, dev, n, intr):
    ctx = ctx_factory()
    m, p, _ = _run_pose(ctx, dev, n, intr)
    return marker_tuples(m), p.tolist(), ctx.board_poses().tobytes()


@pytest.mark.parametrize("gates", [False, True])
def test_four_context_rotation_gives_the_same_board_poses(scene, gates):
    d, board, scenes, dev = scene
    intr = _intr()
    ctxs = [_ctx(d, board) for _ in range(4)]
    want = [_expected(lambda: _ctx(d, board), board, dev[f: f + 1], 1, intr) for f in range(len(scenes))]
    from aruco3_amd import _lib

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
            ctxs[k].submit_pose(dev[f].data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, 1, 30.0, intr)
            inflight[k] = f
    assert got == want


def test_shared_stream_deferred_decode(scene):
    from aruco3_amd import _lib

    torch = _torch()
    d, board, scenes, dev = scene
    intr = _intr()
    want = [_expected(lambda: _ctx(d, board), board, dev[f: f + 2], 2, intr) for f in (0, 3)]
    s = torch.cuda.Stream()
    a, b = _ctx(d, board), _ctx(d, board)
    a.set_stream(s.cuda_stream)
    b.set_stream(s.cuda_stream)
    a.submit_pose(dev[0].data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, 2, 30.0, intr)
    b.submit_pose(dev[3].data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, 2, 30.0, intr)
    got = []
    for c in (a, b):
        m, p, _ = c.collect_pose()
        got.append((marker_tuples(m), p.tolist(), c.board_poses().tobytes()))
    assert got == want


def test_synchronous_rerun_and_a_long_marker_list(scene):
    """a noise frame in a batch shaped like the clean one before it forces a synchronous re-run; a batch after an empty one has more
    markers than the read-back guess -- the board poses are those of a3_detect_batch_pose either way"""
    from aruco3_amd import _lib, synth

    torch = _torch()
    d, board, scenes, dev = scene
    intr = _intr()
    want = _expected(lambda: _ctx(d, board), board, dev, len(scenes), intr)
    ctx = _ctx(d, board)
    _run_pose(ctx, dev[2:3], 1, intr)   # no markers: the next read-back guess is short
    ctx.submit_pose(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, len(scenes), 30.0, intr)
    m, p, _ = ctx.collect_pose()
    assert len(m) > 64 and (marker_tuples(m), p.tolist(), ctx.board_poses().tobytes()) == want

    mixed = dev[:2].clone()
    mixed[1] = torch.from_numpy(synth.noise_frame(W, H, 11)).cuda()
    torch.cuda.synchronize()
    want2 = _expected(lambda: _ctx(d, board), board, mixed, 2, intr)
    for use_submit in (False, True):
        ctx = _ctx(d, board)
        _run_pose(ctx, dev[:2], 2, intr)
        if use_submit:
            ctx.submit_pose(mixed.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, 2, 30.0, intr)
            m, p, _ = ctx.collect_pose()
        else:
            m, p, _ = _run_pose(ctx, mixed, 2, intr)
        assert ctx.stats()["reruns"] >= 1
        assert (marker_tuples(m), p.tolist(), ctx.board_poses().tobytes()) == want2


def test_detector_surface(scene):
    from aruco3_amd.aruco import Detector, DetectorConfig
    from aruco3_amd.pinhole import CameraIntrinsics

    d, board, scenes, dev = scene
    det = Detector(DetectorConfig(min_corner_separation_factor=bu.MIN_CORNER_SEPARATION_FACTOR), d, board=board)
    ci = CameraIntrinsics(W, H, *K)
    out = det.detect_batch_with_board_pose(dev, ci)
    assert len(out) == len(scenes)
    assert [bp.ok for _, bp in out] == [True, True, False, True, True, True, False]
    R, t = scenes[0].R, scenes[0].t
    bp = out[0][1]
    assert bu.rotation_error_deg(bp.rotation, R) < 1.0
    c = bp.apply_transform_to_points([(0.0, 0.0, 0.0)])[0]
    assert np.linalg.norm(np.array(c) - t) < 0.02 * np.linalg.norm(t)


def test_accuracy_against_the_renderers_truth():
    """5 x 7 grid board at 1080p tilted 15 .. 50 degrees, known K: median errors of the board pose against those of the best
    single-marker IPPE pose of each frame"""
    torch = _torch()
    d = _dict()
    board = _board()
    rng = np.random.default_rng(7)
    scenes = []
    for k in range(16):
        R, t = bu.board_pose_facing(board, 15.0 + 35.0 * k / 15, rng.uniform(0, 360), rng.uniform(-30, 30), rng.uniform(480, 560),
                                    (rng.uniform(-60, 60), rng.uniform(-30, 30)))
        scenes.append(bu.board_scene(board, R, t))
    dev = bu.render(scenes, d)
    torch.cuda.synchronize()
    intr = _intr()
    res = {}
    for refine in (False, True):
        ctx = _ctx(d, board, refine)
        m, p, poses = _run_pose(ctx, dev, len(scenes), intr)
        recs = ctx.board_poses()
        rb, tb, rs, ts = [], [], [], []
        pos = 0
        for f, sc in enumerate(scenes):
            assert recs[f]["markers_used"] >= 20
            rb.append(bu.rotation_error_deg(recs[f]["rotation"].reshape(3, 3), sc.R))
            tb.append(np.linalg.norm(recs[f]["translation"] - sc.t) / np.linalg.norm(sc.t))
            best_r, best_t = 1e9, 1e9
            for i in range(pos, pos + int(p[f])):
                if m[i]["id"] not in board.ids:
                    continue
                slot = int(np.nonzero(board.ids == m[i]["id"])[0][0])
                c = board.corners[slot].mean(axis=0)
                Rm = poses[i, 0, 1:10].reshape(3, 3)
                if not np.all(np.isfinite(poses[i, 0])):   # (IPPE has no pose for some near-degenerate quads)
                    continue
                best_r = min(best_r, bu.rotation_error_deg(Rm, sc.R))
                tm = poses[i, 0, 10:13] - Rm @ np.array([c[0], c[1], 0.0])
                best_t = min(best_t, np.linalg.norm(tm - sc.t) / np.linalg.norm(sc.t))
            pos += int(p[f])
            rs.append(best_r)
            ts.append(best_t)
        res[refine] = (np.median(rb), np.median(tb), np.median(rs), np.median(ts))
        print(f"refine={refine}: board rot {res[refine][0]:.3f} deg, trans {res[refine][1]:.4f}; best single marker rot {res[refine][2]:.3f} deg, "
              f"trans {res[refine][3]:.4f}")
        assert res[refine][0] < res[refine][2] and res[refine][1] < res[refine][3]
    assert res[False][0] < 0.3 and res[True][0] < 0.15   # (measured over 256 such frames: 0.15 and 0.07 degrees)
