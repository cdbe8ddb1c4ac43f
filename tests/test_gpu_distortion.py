"""Lens distortion on the MI355X (k_undistort_corners; a3_set_distortion / a3_get_undistorted_corners / a3_undistort_points): bit-equal
to the CPU restatement (tests/lens_oracle.c) from the same corners, in every frame form and through every scheduling path; poses and
board poses solved from the undistorted corners as their oracles solve them; distortion off changes nothing; and on frames rendered
through a real lens model the undistorted corners and the board pose land where the ideal camera puts them."""
import numpy as np
import pytest

from tests import board_oracle as bo
from tests import board_util as bu
from tests import lens_oracle as lo
from tests.util import marker_tuples

pytestmark = pytest.mark.gpu

W, H = bu.W1080, bu.H1080
K = bu.K1080
COEF = lo.COEFFS["webcam5"]


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


def _dict(name="ARUCO"):
    from aruco3_amd import ARDictionary

    return ARDictionary.new_from_named_dict(name)


def _intr(w=W, h=H, k=K):
    from aruco3_amd import _lib

    return _lib.Intrinsics(w, h, *k)


def _dist(coeffs=COEF, iterations=20, max_residual_px=0.1):
    from aruco3_amd import _lib

    return _lib.DistortionRec(_lib.DIST_RATIONAL, iterations, *coeffs, max_residual_px)


def _ctx(d, dist=True, refine=False, board=None, cfg=None):
    from aruco3_amd import _lib

    ctx = _lib.Context(cfg or _lib.default_config(), d.code_list, d.num_bits, d._tau)
    if refine:
        ctx.set_corner_refinement(_lib.default_refine_config())
    if board is not None:
        ctx.set_board(board.ids, board.corners)
    if dist:
        ctx.set_distortion(_dist())
    return ctx


def _k4(intr):
    return (intr.focal_x, intr.focal_y, intr.principal_x, intr.principal_y)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _check_undist(ctx, markers, intr, refined=None, coeffs=COEF):
    """the batch's undistorted corners and residuals against the oracle from the same input corners -> (corners, residuals)"""
    xy, res = ctx.undistorted_corners()
    src = refined if refined is not None else markers["corners"].reshape(-1, 4, 2).astype(np.float32)
    assert xy.shape == (len(markers), 4, 2) and res.shape == (len(markers), 4)
    want_xy, want_res = lo.undistort(src, _k4(intr), coeffs)
    assert np.array_equal(_bits(xy).reshape(-1), _bits(want_xy).reshape(-1))
    assert np.array_equal(_bits(res).reshape(-1), _bits(want_res).reshape(-1))
    return xy, res


def _check_poses(oracle, poses, und, intr, size, every=1):
    """per-marker poses against the reference solver fed the undistorted corners, normalised in float32"""
    f = np.float32
    for i in range(0, len(und), every):
        q = und[i]
        pts = np.stack([(q[:, 0] - f(intr.principal_x)) / f(intr.focal_x), (q[:, 1] - f(intr.principal_y)) / f(intr.focal_y)], axis=1)
        p1, p2 = oracle.solve_with_normalized_points(pts.astype(np.float32).reshape(8), size)
        want = np.array([np.concatenate([[e], r.reshape(9), t]) for e, r, t in (p1, p2)], np.float32)
        got = np.asarray(poses[i], np.float32).reshape(2, 13)
        assert np.allclose(got, want, rtol=1e-4, atol=1e-4, equal_nan=True), (i, got, want)


# ---- stand-alone ----

def test_standalone_equals_oracle_bit_for_bit():
    """about 10^5 points over a 1080p field and beyond it, every coefficient set, failures of a strong lens included"""
    from aruco3_amd import _lib

    _torch()
    ctx = _ctx(_dict(), dist=False)
    rng = np.random.default_rng(3)
    intr = _intr()
    total = fails = 0
    cases = [(c, _intr()) for c in lo.COEFFS.values()] + [((-0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0), _intr(k=(500.0, 500.0, 960.0, 540.0)))]
    for coeffs, intr in cases:
        pts = np.stack([rng.uniform(-200, W + 200, 18000), rng.uniform(-200, H + 200, 18000)], axis=1).astype(np.float32)
        pts[:4] = [[0, 0], [W - 1, H - 1], [intr.principal_x, intr.principal_y], [W / 2 + 0.25, 3.5]]
        for it, mr in ((20, 0.1), (5, 0.01)):
            got, res = ctx.undistort_points(pts, intr, _dist(coeffs, it, mr))
            want, wres = lo.undistort(pts, _k4(intr), coeffs, it, mr)
            assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(res), _bits(wres)), coeffs
            bad = ~np.isfinite(res)
            assert np.array_equal(got[bad], pts[bad])   # a failed point comes back as it went in
            total += len(pts)
            fails += int(bad.sum())
    assert total >= 10 ** 5 and fails > 1000
    # all-zero coefficients: (x0 * fx + cx, y0 * fy + cy) exactly
    pts = np.stack([rng.uniform(0, W, 4096), rng.uniform(0, H, 4096)], axis=1).astype(np.float32)
    got, res = ctx.undistort_points(pts, intr, _dist((0.0,) * 8))
    f = np.float32
    x0 = (pts[:, 0] - f(intr.principal_x)) / f(intr.focal_x)
    y0 = (pts[:, 1] - f(intr.principal_y)) / f(intr.focal_y)
    assert np.array_equal(_bits(got[:, 0]), _bits(x0 * f(intr.focal_x) + f(intr.principal_x)))
    assert np.array_equal(_bits(got[:, 1]), _bits(y0 * f(intr.focal_y) + f(intr.principal_y)))
    assert not res.any()
    for bad in (_lib.DistortionRec(_lib.DIST_NONE, 20), _dist(iterations=0), _dist(iterations=101), _dist((float("nan"),) + COEF[1:]),
                _dist(max_residual_px=-1.0), _lib.DistortionRec(7, 20)):
        with pytest.raises(_lib.A3Error) as e:
            ctx.undistort_points(pts[:4], intr, bad)
        assert e.value.code == _lib.ERR_INVALID


# ---- in a batch ----

@pytest.mark.parametrize("refine", [False, True])
def test_config2_full_batch_equal_oracle(oracle, refine):
    """BASELINE config 2: one 256-frame 1080p batch rendered on the device; every marker's undistorted corners bit-equal to the oracle,
    the poses of every 4th marker against the reference solver on them"""
    from aruco3_amd import _lib, synth

    torch = _torch()
    spec, name = synth.config_spec(2)
    d = _dict(name)
    seeds = [synth.frame_seed(2, i) for i in range(256)]
    dev, _ = synth.render_frames_device(spec, d.code_list, d.num_bits, seeds)
    torch.cuda.synchronize()
    w, h = spec.width, spec.height
    intr = _intr(w, h)
    ctx = _ctx(d, refine=refine)
    m, p, poses = ctx.detect_batch_pose(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, 256, 100.0, intr,
                                        out_cap=256 * 64)
    assert len(m) >= 256 * 3
    und, res = _check_undist(ctx, m, intr, ctx.refined_corners() if refine else None)
    assert np.isfinite(res).mean() > 0.99
    _check_poses(oracle, poses, und, intr, 100.0, every=4)


def _layouts(frames):
    """(name, fmt, host buffer, byte offset, row_stride, frame_stride) of the frames in every pixel format, packed and padded"""
    from aruco3_amd import _lib

    n, h, w, _ = frames.shape
    a = np.full(frames.shape[:3] + (1,), 255, np.uint8)
    f32 = frames.astype(np.uint32)
    luma = ((2126 * f32[..., 0] + 7152 * f32[..., 1] + 722 * f32[..., 2]) // 10000).astype(np.uint8)[..., None]
    out = []
    for name, fmt, px in (("rgb", _lib.FMT_RGB8, frames), ("rgba", _lib.FMT_RGBA8, np.concatenate([frames, a], 3)),
                          ("bgra", _lib.FMT_BGRA8, np.concatenate([frames[..., ::-1], a], 3)), ("l8", _lib.FMT_L8, luma)):
        bpp = px.shape[3]
        for pad_row, pad_frame, off in ((0, 0, 0), (24, 1000, 13)):
            rs = w * bpp + pad_row
            fs = rs * h + pad_frame
            buf = np.zeros(off + fs * n + 64, np.uint8)
            view = np.lib.stride_tricks.as_strided(buf[off:], shape=(n, h, w * bpp), strides=(fs, rs, 1))
            view[...] = px.reshape(n, h, w * bpp)
            out.append((name, fmt, buf, off, rs, fs))
    return out


def test_formats_layouts_and_memory(oracle):
    from aruco3_amd import _lib, synth

    torch = _torch()
    frames, _ = synth.config_frames(1, 2)
    d = _dict("ARUCO_DEFAULT")
    n, h, w, _ = frames.shape
    intr = _intr(w, h, (1.1 * w, 1.1 * w, w / 2 - 7.5, h / 2 + 4.0))
    base = None
    for refine in (False, True):
        for name, fmt, buf, off, rs, fs in _layouts(frames):
            for memory in (_lib.MEM_HOST, _lib.MEM_DEVICE):
                ctx = _ctx(d, refine=refine)
                if memory == _lib.MEM_HOST:
                    ptr, keep = buf.ctypes.data + off, buf
                else:
                    keep = torch.from_numpy(buf).cuda()
                    torch.cuda.synchronize()
                    ptr = keep.data_ptr() + off
                m, p, poses = ctx.detect_batch_pose(ptr, memory, fmt, w, h, rs, fs, n, 100.0, intr)
                und, res = _check_undist(ctx, m, intr, ctx.refined_corners() if refine else None)
                key = (refine,)
                if base is None or base[0] != key:
                    base = (key, marker_tuples(m), und.tobytes(), poses.tobytes())
                    assert len(m) >= 8
                    _check_poses(oracle, poses, und, intr, 100.0)
                assert (marker_tuples(m), und.tobytes(), poses.tobytes()) == base[1:], (name, off, memory, refine)
                del keep


# ---- board pose ----

def _board():
    from aruco3_amd.board import GridBoard

    return GridBoard(5, 7, 30.0, 6.0, first_id=10)


@pytest.fixture(scope="module")
def scene():
    torch = _torch()
    d = _dict()
    board = _board()
    scenes = []
    for tilt, direction, roll, off in ((35.0, 20.0, 10.0, (0.0, 0.0)), (25.0, 100.0, -15.0, (300.0, -150.0)), (45.0, -30.0, 0.0, (-320.0, 160.0))):
        R, t = bu.board_pose_facing(board, tilt, direction, roll, 520.0, off)
        scenes.append(bu.board_scene(board, R, t))
    dev = bu.render(scenes, d)
    torch.cuda.synchronize()
    return d, board, scenes, dev


def _run(ctx, dev, n, intr, size=30.0):
    from aruco3_amd import _lib

    return ctx.detect_batch_pose(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, n, size, intr)


def _check_board(board, markers, per, recs, und, intr):
    pos = 0
    for f in range(len(per)):
        cnt = int(per[f])
        mk = markers[pos: pos + cnt]
        want = bo.board_pose(board, mk["id"], und[pos: pos + cnt], image_size=(W, H), intrinsics=intr)
        got = recs[f]
        pos += cnt
        assert (got["status"], got["markers_used"], got["markers_rejected"]) == (want["status"], want["markers_used"], want["markers_rejected"]), f
        assert np.abs(got["rotation"] - want["rotation"]).max() <= 1e-4, (f, got, want)
        assert np.linalg.norm(got["translation"] - want["translation"]) <= 1e-4 * np.linalg.norm(want["translation"]), (f, got, want)
        assert abs(got["rms_px"] - want["rms_px"]) <= 1e-3 * max(float(want["rms_px"]), 1e-3), (f, got, want)


@pytest.mark.parametrize("refine", [False, True])
def test_board_and_marker_poses_from_undistorted_corners(oracle, scene, refine):
    d, board, scenes, dev = scene
    intr = _intr()
    ctx = _ctx(d, refine=refine, board=board, cfg=bu.config())
    m, p, poses = _run(ctx, dev, len(scenes), intr)
    und, _ = _check_undist(ctx, m, intr, ctx.refined_corners() if refine else None)
    recs = ctx.board_poses()
    assert all(r["status"] == 1 and r["markers_used"] >= 30 for r in recs)
    _check_board(board, m, p, recs, und, intr)
    _check_poses(oracle, poses, und, intr, 30.0, every=3)
    # the stand-alone board pose applies the context's distortion with intrinsics: equal to the batch's
    pos = 0
    for f in range(len(scenes)):
        mk = m[pos: pos + int(p[f])]
        src = ctx.refined_corners()[pos: pos + int(p[f])] if refine else mk["corners"].reshape(-1, 4, 2).astype(np.float32)
        pos += int(p[f])
        assert ctx.estimate_board_pose(mk["id"], src, intrinsics=intr).tobytes() == recs[f].tobytes(), f


# ---- scheduling paths ----

def _result(ctx, m, p, poses, with_board=True):
    xy, res = ctx.undistorted_corners()
    return marker_tuples(m), p.tolist(), poses.tobytes(), xy.tobytes(), res.tobytes(), ctx.board_poses().tobytes() if with_board else None


def _single(d, board, dev, n, intr):
    ctx = _ctx(d, board=board, cfg=bu.config())
    m, p, poses = _run(ctx, dev, n, intr)
    return _result(ctx, m, p, poses)


@pytest.mark.parametrize("gates", [False, True])
def test_four_context_rotation(scene, gates):
    from aruco3_amd import _lib

    d, board, scenes, dev = scene
    intr = _intr()
    order = [0, 1, 2, 1, 0, 2, 2, 0]
    want = {f: _single(d, board, dev[f: f + 1], 1, intr) for f in range(len(scenes))}
    ctxs = [_ctx(d, board=board, cfg=bu.config()) for _ in range(4)]
    got = [None] * len(order)
    inflight = {}
    for j in range(len(order) + 4):
        k = j % 4
        if k in inflight:
            g = inflight.pop(k)
            got[g] = _result(ctxs[k], *ctxs[k].collect_pose())
        if j < len(order):
            if gates:
                for o in range(k + 1, 4):
                    ctxs[k].order_after(ctxs[o])
            f = order[j]
            ctxs[k].submit_pose(dev[f].data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, 1, 30.0, intr)
            inflight[k] = j
    assert got == [want[f] for f in order]


def test_shared_stream_deferred_decode(scene):
    from aruco3_amd import _lib

    torch = _torch()
    d, board, scenes, dev = scene
    intr = _intr()
    want = [_single(d, board, dev[f: f + 2], 2, intr) for f in (0, 1)]
    s = torch.cuda.Stream()
    a, b = _ctx(d, board=board, cfg=bu.config()), _ctx(d, board=board, cfg=bu.config())
    a.set_stream(s.cuda_stream)
    b.set_stream(s.cuda_stream)
    for _ in range(2):
        a.submit_pose(dev[0].data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, 2, 30.0, intr)
        b.submit_pose(dev[1].data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, 2, 30.0, intr)
        assert [_result(c, *c.collect_pose()) for c in (a, b)] == want


def test_synchronous_rerun_and_a_long_marker_list(scene):
    from aruco3_amd import _lib, synth

    torch = _torch()
    d, board, scenes, dev = scene
    intr = _intr()
    blank = torch.full_like(dev[:1], 200)
    want = _single(d, board, dev, len(scenes), intr)
    ctx = _ctx(d, board=board, cfg=bu.config())
    _run(ctx, blank, 1, intr)   # no markers: the next read-back guess (64) is short of the ~105 markers
    ctx.submit_pose(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, len(scenes), 30.0, intr)
    r = _result(ctx, *ctx.collect_pose())
    assert len(r[0]) > 64 and r == want

    mixed = dev[:2].clone()
    mixed[1] = torch.from_numpy(synth.noise_frame(W, H, 11)).cuda()
    torch.cuda.synchronize()
    want2 = _single(d, board, mixed, 2, intr)
    for use_submit in (False, True):
        ctx = _ctx(d, board=board, cfg=bu.config())
        _run(ctx, dev[:2], 2, intr)
        if use_submit:
            ctx.submit_pose(mixed.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, 2, 30.0, intr)
            r = _result(ctx, *ctx.collect_pose())
        else:
            r = _result(ctx, *_run(ctx, mixed, 2, intr))
        assert ctx.stats()["reruns"] >= 1
        assert r == want2


def test_setter_between_submit_and_collect(scene):
    from aruco3_amd import _lib

    d, board, scenes, dev = scene
    intr = _intr()
    want = _single(d, board, dev, len(scenes), intr)
    ctx = _ctx(d, board=board, cfg=bu.config())
    ctx.submit_pose(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, len(scenes), 30.0, intr)
    ctx.set_distortion(None)   # applies to the next batch: this one keeps its distortion
    assert _result(ctx, *ctx.collect_pose()) == want
    _run(ctx, dev, len(scenes), intr)
    with pytest.raises(_lib.A3Error) as e:
        ctx.undistorted_corners()
    assert e.value.code == _lib.ERR_INVALID
    ctx.submit_pose(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, len(scenes), 30.0, intr)
    ctx.set_distortion(_dist())   # ... and the other way round
    ctx.collect_pose()
    with pytest.raises(_lib.A3Error):
        ctx.undistorted_corners()
    assert _result(ctx, *_run(ctx, dev, len(scenes), intr)) == want


# ---- off means off ----

def test_off_changes_nothing(scene):
    from aruco3_amd import _lib

    d, board, scenes, dev = scene
    intr = _intr()
    for refine in (False, True):
        never = _ctx(d, dist=False, refine=refine, board=board, cfg=bu.config())
        cleared = _ctx(d, dist=True, refine=refine, board=board, cfg=bu.config())
        _run(cleared, dev, len(scenes), intr)
        cleared.set_distortion(None)
        outs = []
        for c in (never, cleared):
            m, p, poses = _run(c, dev, len(scenes), intr)
            outs.append((marker_tuples(m), p.tolist(), poses.tobytes(), c.board_poses().tobytes(),
                         c.refined_corners().tobytes() if refine else None))
            with pytest.raises(_lib.A3Error) as e:
                c.undistorted_corners()
            assert e.value.code == _lib.ERR_INVALID
        assert outs[0] == outs[1]
        cleared.set_distortion(_lib.DistortionRec(_lib.DIST_NONE, 0))   # model NONE clears as well
        assert (lambda r: (marker_tuples(r[0]), r[1].tolist(), r[2].tobytes()))(_run(cleared, dev, len(scenes), intr)) == outs[0][:3]
    ctx = _ctx(d, board=board, cfg=bu.config())
    with pytest.raises(_lib.A3Error) as e:   # the coefficients are in focal units: a pose batch needs intrinsics
        _run(ctx, dev, len(scenes), None)
    assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.A3Error) as e:
        ctx.submit_pose(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, len(scenes), 30.0, None)
    assert e.value.code == _lib.ERR_INVALID
    m, p = ctx.detect_batch(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, len(scenes))   # detection only
    assert marker_tuples(m) == outs[0][0]
    with pytest.raises(_lib.A3Error) as e:
        ctx.undistorted_corners()
    assert e.value.code == _lib.ERR_INVALID
    for bad in (_dist(iterations=0), _dist((float("inf"),) + COEF[1:]), _lib.DistortionRec(2, 20)):
        with pytest.raises(_lib.A3Error) as e:
            ctx.set_distortion(bad)
        assert e.value.code == _lib.ERR_INVALID


# ---- Python surface ----

def test_detector_surface(scene):
    from aruco3_amd import undistort_points
    from aruco3_amd.aruco import Detector, DetectorConfig
    from aruco3_amd.pinhole import CameraIntrinsics, Distortion

    d, board, scenes, dev = scene
    dist = Distortion(*COEF)
    ci = CameraIntrinsics(W, H, *K, distortion=dist)
    det = Detector(DetectorConfig(min_corner_separation_factor=bu.MIN_CORNER_SEPARATION_FACTOR), d, board=board)
    out = det.detect_batch_with_pose(dev, 30.0, ci)
    mk = [m for det_, _ in out for m in det_.markers]
    assert len(mk) >= 90 and all(m.corners_undistorted is not None and len(m.undistort_residual_px) == 4 for m in mk)
    und, res = undistort_points(np.array([m.corners for m in mk], np.float32), ci)
    assert np.array_equal(_bits(und).reshape(-1), _bits(np.array([m.corners_undistorted for m in mk], np.float32)).reshape(-1))
    assert np.array_equal(_bits(res), _bits(np.array([m.undistort_residual_px for m in mk], np.float32)).reshape(-1))
    bp = det.detect_batch_with_board_pose(dev, ci, 30.0)
    assert all(b.ok for _, b in bp) and bp[0][0].markers[0].corners_undistorted is not None
    plain = det.detect_batch_with_pose(dev, 30.0, CameraIntrinsics(W, H, *K))
    assert all(m.corners_undistorted is None and m.undistort_residual_px is None for det_, _ in plain for m in det_.markers)
    assert [[m.corners for m in x.markers] for x, _ in plain] == [[m.corners for m in x.markers] for x, _ in out]


# ---- accuracy through a lens ----

def test_accuracy_through_a_lens():
    """5 x 7 grid board at 1280 x 720 rendered on the host through k1 -0.28, k2 0.09, p1 1e-3, p2 -5e-4: the undistorted refined
    corners against the ideal pinhole projections, and the board pose's rotation error with and without the distortion set"""
    from aruco3_amd import _lib
    from tests import lens_util as lu

    torch = _torch()
    d = _dict()
    board = _board()
    rng = np.random.default_rng(11)
    scenes, frames = [], []
    for off in ((-300.0, -90.0), (290.0, 90.0), (-280.0, 100.0), (300.0, -90.0)):   # (the board reaches into the image corners)
        R, t = bu.board_pose_facing(board, rng.uniform(20, 40), rng.uniform(0, 360), rng.uniform(-20, 20), rng.uniform(480, 520), off, K=lu.K720)
        scenes.append((R, t))
        frames.append(lu.render(board, d, R, t))
    frames = np.stack(frames)[..., None]
    n, h, w = frames.shape[:3]
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    torch.cuda.synchronize()
    intr = _intr(w, h, lu.K720)
    res = {}
    for with_dist in (False, True):
        ctx = _ctx(d, dist=False, refine=True, board=board, cfg=bu.config())
        if with_dist:
            ctx.set_distortion(_dist(lu.WEBCAM))
        m, p, _ = ctx.detect_batch_pose(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_L8, w, h, w, w * h, n, 30.0, intr)
        recs = ctx.board_poses()
        corners = ctx.undistorted_corners()[0] if with_dist else ctx.refined_corners()
        errs, rot = [], []
        pos = 0
        for f, (R, t) in enumerate(scenes):
            truth = bu.project(board, R, t, lu.K720)
            for i in range(pos, pos + int(p[f])):
                slot = np.nonzero(board.ids == m[i]["id"])[0]
                if slot.size:
                    errs.append(np.linalg.norm(corners[i] - truth[slot[0]], axis=1))
            pos += int(p[f])
            assert recs[f]["status"] == 1 and recs[f]["markers_used"] >= 15, (f, recs[f])
            rot.append(bu.rotation_error_deg(recs[f]["rotation"].reshape(3, 3), R))
        errs = np.concatenate(errs)
        res[with_dist] = (float(np.median(errs)), float(np.percentile(errs, 95)), float(np.median(rot)), float(np.max(rot)))
        print(f"distortion={with_dist}: corner error median {res[with_dist][0]:.3f} px, p95 {res[with_dist][1]:.3f} px; "
              f"board rotation error median {res[with_dist][2]:.3f} deg, max {res[with_dist][3]:.3f} deg")
    # measured on the MI355X: 13.0 px / 5.85 deg without (max 7.7 deg), 0.31 px / 0.124 deg with (max 0.64 deg)
    assert res[False][0] > 5.0                              # the lens moves the corners by tens of pixels
    assert res[True][0] < 0.5
    assert res[True][2] < 0.05 * res[False][2] and res[True][3] < 1.0
