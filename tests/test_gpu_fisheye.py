"""The fisheye lens model (a3_distortion model A3_DIST_FISHEYE) on the MI355X: a3_undistort_points and the pose batches' undistorted
corners bit-equal to the CPU restatement (tests/fisheye_oracle.c), the per-marker, board and ChArUco poses solved from them as their
oracles solve them, a3_rectify_frames byte-equal to a3o_fisheye_rectify in every format, view, size and frame count, the chain into
the detector, the argument errors, the Python surface, and the accuracy on frames rendered through a fisheye lens."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from tests import board_oracle as bo
from tests import board_util as bu
from tests import fisheye_oracle as fo
from tests.util import markers_of_hip, markers_of_oracle

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SW, SH = fo.SRC_SIZE
W, H = bu.W1080, bu.H1080
FILL = 77
MILD = fo.COEFFS["mild"]


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


def _dict(name="ARUCO"):
    from aruco3_amd import ARDictionary

    return ARDictionary.new_from_named_dict(name)


def _dist(coeffs=MILD, iterations=20, max_residual_px=0.1):
    from aruco3_amd import _lib

    return _lib.DistortionRec(_lib.DIST_FISHEYE, iterations, *fo.slots8(coeffs), max_residual_px)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _k4(intr):
    return (intr.focal_x, intr.focal_y, intr.principal_x, intr.principal_y)


@pytest.fixture(scope="module")
def ctx():
    from aruco3_amd import _lib

    _torch()
    c = _lib.Context(_lib.default_config(), np.zeros(1, np.uint64), 64, 1)
    yield c
    c.close()


# ---- a3_undistort_points ----

def _field():
    """every pixel of the 333 x 251 frame, a ring of points up to 40 px outside it, and the principal point itself"""
    ys, xs = np.mgrid[0:SH, 0:SW]
    grid = np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1).astype(np.float32)
    t = np.linspace(0.0, 2 * np.pi, 720, endpoint=False)
    ring = np.concatenate([np.stack([166.0 + (210.0 + m) * np.cos(t) * 1.0, 125.0 + (210.0 + m) * np.sin(t)], axis=1) for m in (0.25, 17.5, 40.0)])
    return np.concatenate([np.array([[fo.K[2], fo.K[3]]], np.float32), grid, ring.astype(np.float32)])


@pytest.mark.parametrize("name", list(fo.COEFFS))
def test_undistort_points_equal_oracle_bit_for_bit(ctx, name):
    """every iteration count at both cameras: at K every pixel of the frame inverts, at K_WIDE the frame's corners have no root"""
    from aruco3_amd import _lib

    pts = _field()
    k = fo.COEFFS[name]
    for K in (fo.K, fo.K_WIDE):
        intr = _lib.Intrinsics(SW, SH, *K)
        for it in (1, 5, 20, 100):
            got, res = ctx.undistort_points(pts, intr, _dist(k, it))
            want, wres = fo.undistort(pts, K, k, it)
            assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(res), _bits(wres)), (name, K, it)
            bad = ~np.isfinite(res)
            assert np.array_equal(got[bad], pts[bad])
            if it == 20:
                inside = slice(0, 1 + SW * SH)
                if K == fo.K_WIDE:
                    assert 0.05 < bad[inside].mean() < 0.5, (name, float(bad[inside].mean()))
                elif name != "neg":
                    assert not bad[inside].any(), name
        # the principal point: rd = 0, the scale is 1, the residual 0
        assert got[0].tolist() == [K[2], K[3]] and res[0] == 0.0


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257])
def test_undistort_points_block_edges(ctx, n):
    from aruco3_amd import _lib

    pts = _field()[1000: 1000 + 97 * n: 97]
    assert len(pts) == n
    got, res = ctx.undistort_points(pts, _lib.Intrinsics(SW, SH, *fo.K), _dist(fo.COEFFS["strong"]))
    want, wres = fo.undistort(pts, fo.K, fo.COEFFS["strong"])
    assert np.array_equal(_bits(got), _bits(want)) and np.array_equal(_bits(res), _bits(wres))


# ---- pose batches ----

def _board():
    from aruco3_amd.board import GridBoard

    return GridBoard(5, 7, 30.0, 6.0, first_id=10)


@pytest.fixture(scope="module")
def scene():
    torch = _torch()
    d = _dict()
    board = _board()
    scenes = []
    for tilt, direction, roll, off in ((35.0, 20.0, 10.0, (0.0, 0.0)), (25.0, 100.0, -15.0, (300.0, -150.0))):
        R, t = bu.board_pose_facing(board, tilt, direction, roll, 520.0, off)
        scenes.append(bu.board_scene(board, R, t))
    dev = bu.render(scenes, d)
    torch.cuda.synchronize()
    return d, board, scenes, dev


def _pose_ctx(d, refine, board):
    from aruco3_amd import _lib

    c = _lib.Context(bu.config(), d.code_list, d.num_bits, d._tau)
    if refine:
        c.set_corner_refinement(_lib.default_refine_config())
    c.set_board(board.ids, board.corners)
    c.set_distortion(_dist())
    return c


def _check_undist(c, markers, intr, refined=None, coeffs=MILD):
    xy, res = c.undistorted_corners()
    src = refined if refined is not None else markers["corners"].reshape(-1, 4, 2).astype(np.float32)
    assert xy.shape == (len(markers), 4, 2) and res.shape == (len(markers), 4)
    want_xy, want_res = fo.undistort(src, _k4(intr), coeffs)
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
    from aruco3_amd import _lib

    d, board, scenes, dev = scene
    intr = _lib.Intrinsics(W, H, *bu.K1080)
    c = _pose_ctx(d, refine, board)
    m, p, poses = c.detect_batch_pose(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, len(scenes), 30.0, intr)
    refined = c.refined_corners() if refine else None
    und, res = _check_undist(c, m, intr, refined)
    assert len(m) >= 60 and np.isfinite(res).all()
    src = refined if refine else m["corners"].reshape(-1, 4, 2).astype(np.float32)
    assert np.linalg.norm(und - src, axis=2).max() > 20.0   # (the lens really moves these corners)
    recs = c.board_poses()
    assert all(r["status"] == 1 and r["markers_used"] >= 30 for r in recs)
    _check_board(board, m, p, recs, und, intr)
    _check_poses(oracle, poses, und, intr, 30.0, every=3)
    # the stand-alone board pose applies the context's distortion with intrinsics: equal to the batch's
    pos = 0
    for f in range(len(scenes)):
        assert c.estimate_board_pose(m["id"][pos: pos + int(p[f])], src[pos: pos + int(p[f])], intrinsics=intr).tobytes() == recs[f].tobytes(), f
        pos += int(p[f])
    c.close()


def test_charuco_pose_from_undistorted_corners():
    """one ChArUco batch with the fisheye lens set: the pose of every frame against the ChArUco oracle fed the markers' and the
    chessboard corners' positions undistorted by the fisheye oracle (a corner that does not invert keeps its position)"""
    from aruco3_amd import _lib
    from aruco3_amd.board import CharucoBoard
    from tests import charuco_oracle as co
    from tests import charuco_util as cu

    torch = _torch()
    d = _dict("ARUCO_DEFAULT")
    b = CharucoBoard(5, 7, 40.0, 28.0, first_id=5)
    scenes = [cu.Scene(b, R, t) for R, t in cu.tilted_poses(b, 2, seed=11, tilt=(15.0, 35.0), distance=800.0)]
    dev = cu.render(scenes, d)
    torch.cuda.synchronize()
    K = (1400.0, 1400.0, 960.0, 540.0)
    c = _lib.Context(cu.config(), d.code_list, d.num_bits, d._tau)
    c.set_corner_refinement(_lib.default_refine_config())
    c.set_board(b.ids, b.corners)
    c.set_charuco(b.chessboard_corners, b.adjacent_ids, None)
    c.set_distortion(_dist())
    intr = _lib.Intrinsics(W, H, *K)
    m, per, _ = c.detect_batch_pose(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, len(scenes), 28.0, intr)
    recs, poses = c.charuco_corners(), c.charuco_poses()
    und, _ = _check_undist(c, m, intr, c.refined_corners())
    pos = solved = 0
    for f in range(len(scenes)):
        cnt = int(per[f])
        r = recs[recs["frame"] == f].copy()
        assert len(r) >= 6
        xy, _ = fo.undistort(np.stack([r["x"], r["y"]], axis=1), K, MILD)
        r["x"], r["y"] = xy[:, 0], xy[:, 1]
        want = co.pose(b, m["id"][pos: pos + cnt], und[pos: pos + cnt], r, (W, H), K, None)
        got = poses[f]
        pos += cnt
        assert got["status"] == want["status"] and got["corners_used"] == want["corners_used"] == len(r)
        if got["status"]:
            solved += 1
            assert np.abs(got["rotation"] - want["rotation"]).max() < 1e-4
            assert np.linalg.norm(got["translation"] - want["translation"]) <= 1e-4 * np.linalg.norm(want["translation"])
            assert abs(float(got["rms_px"]) - float(want["rms_px"])) < 1e-3
    assert solved >= 1
    c.close()


# ---- a3_rectify_frames ----

def _fmts():
    from aruco3_amd import _lib

    return {"L8": (_lib.FMT_L8, 1), "RGB8": (_lib.FMT_RGB8, 3), "RGBA8": (_lib.FMT_RGBA8, 4), "BGRA8": (_lib.FMT_BGRA8, 4)}


def _rec(src_size, K, coeffs, new_size, new_K, R=None, fill=FILL):
    from aruco3_amd import _lib

    r = _lib.RectifyRec()
    r.src = _lib.Intrinsics(src_size[0], src_size[1], *K)
    r.distortion = _dist(coeffs)
    r.dst = _lib.Intrinsics(new_size[0], new_size[1], *new_K)
    r.rotation = (C.c_float * 9)(*[float(v) for v in (np.eye(3) if R is None else np.asarray(R)).reshape(9)])
    r.fill = fill
    return r


def _noise(n, h, w, c, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, c), dtype=np.uint8)


def _run(ctx, frames, fmt, rec):
    """dense frames (N, H, W, C), device to device -> (output (N, H', W', C), info)"""
    from aruco3_amd import _lib

    torch = _torch()
    n, h, w, c = frames.shape
    dw, dh = int(rec.dst.image_width), int(rec.dst.image_height)
    src = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    dst = torch.full((n, dh, dw, c), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    info = ctx.rectify_frames(src.data_ptr(), _lib.MEM_DEVICE, fmt, w * c, h * w * c, n, rec, dst.data_ptr(), _lib.MEM_DEVICE, dw * c, dh * dw * c)
    return dst.cpu().numpy(), info


def _fisheye_path(info, dw, dh):
    tiles = ((dw + 255) // 256) * ((dh + 3) // 4)
    assert info.tiles == tiles and list(info.path_tiles) == [0, tiles, 0, 0]


@pytest.mark.parametrize("fmt", ["L8", "RGB8", "RGBA8", "BGRA8"])
def test_rectify_equals_oracle_byte_for_byte(ctx, fmt):
    """every coefficient set x every view, one call each, on one frame of noise: the edge of the fisheye field in the zoomed-out view,
    rays with Wz <= 0 in the 80 degree one"""
    f, c = _fmts()[fmt]
    frames = _noise(1, SH, SW, c, 3)
    for name, coeffs in fo.COEFFS.items():
        for view, (new_K, size, deg) in fo.VIEWS.items():
            R = fo.rot_y(deg)
            got, info = _run(ctx, frames, f, _rec((SW, SH), fo.K, coeffs, size, new_K, R))
            want, inside = fo.rectify(frames, fo.K, coeffs, new_K, size, R, FILL, with_inside=True)
            assert np.array_equal(got, want), (name, view, int((got != want).sum()))
            assert inside.any() and (view not in ("zoomed_out", "rot80") or not inside.all()), (name, view)
            _fisheye_path(info, *size)


def test_rectify_row_and_tile_edges(ctx):
    """output widths around the lane run (4 pixels), the 64-pixel and the 256-pixel wave segment, heights around the 4-row workgroup"""
    f, c = _fmts()["RGB8"]
    coeffs = fo.COEFFS["strong"]
    frames = _noise(2, SH, SW, c, 7)
    for dw in (1, 3, 5, 63, 64, 65, 255, 256, 257):
        for dh in (1, 4, 5):
            new_K = (120.0, 120.0, dw * 0.5, dh * 0.5)
            got, info = _run(ctx, frames, f, _rec((SW, SH), fo.K, coeffs, (dw, dh), new_K))
            assert np.array_equal(got, fo.rectify(frames, fo.K, coeffs, new_K, (dw, dh), None, FILL)), (dw, dh)
            _fisheye_path(info, dw, dh)


@pytest.mark.parametrize("n", [1, 15, 16, 17, 33])
def test_rectify_frame_counts(ctx, n):
    """different noise in every frame: a slip in the frame chunks (16 frames each) or in a frame stride shows"""
    f, c = _fmts()["RGB8"]
    frames = _noise(n, 83, 141, c, 100 + n)
    K = (70.0, 70.0, 70.0, 41.0)
    got, _ = _run(ctx, frames, f, _rec((141, 83), K, fo.COEFFS["neg"], (141, 83), K))
    want = fo.rectify(frames, K, fo.COEFFS["neg"], K, (141, 83), None, FILL)
    for k in range(n):
        assert np.array_equal(got[k], want[k]), k


def test_rectify_strides_and_padding(ctx):
    """the source 5 bytes into its buffer with row stride = row bytes + 7, the output with row stride = row bytes + 3 and a gap between
    frames: rows that are not dword-aligned, and not one padding byte written"""
    from aruco3_amd import _lib

    torch = _torch()
    f, c = _fmts()["RGB8"]
    n, h, w = 3, 59, 131
    frames = _noise(n, h, w, c, 17)
    K, new_K, (dw, dh) = (60.0, 60.0, 65.0, 29.0), (90.0, 90.0, 131.0, 10.0), (262, 21)
    rec = _rec((w, h), K, MILD, (dw, dh), new_K)
    lead, srow, drow, gap = 5, w * c + 7, dw * c + 3, 13
    sframe, dframe = srow * h + gap, drow * dh + gap
    src = np.zeros(lead + sframe * n, np.uint8)
    view = np.lib.stride_tricks.as_strided(src[lead:], shape=(n, h, w * c), strides=(sframe, srow, 1))
    view[...] = frames.reshape(n, h, w * c)
    src_t = torch.from_numpy(src).cuda()
    dst_t = torch.full((dframe * n,), 0xA5, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.rectify_frames(src_t.data_ptr() + lead, _lib.MEM_DEVICE, f, srow, sframe, n, rec, dst_t.data_ptr(), _lib.MEM_DEVICE, drow, dframe)
    dst = dst_t.cpu().numpy()
    want = fo.rectify(frames, K, MILD, new_K, (dw, dh), None, FILL)
    written = np.zeros(dst.size, bool)
    for k in range(n):
        for y in range(dh):
            o = k * dframe + y * drow
            assert np.array_equal(dst[o: o + dw * c], want[k, y].reshape(-1)), (k, y)
            written[o: o + dw * c] = True
    assert np.all(dst[~written] == 0xA5)


def test_chain_into_the_detector():
    """the config-1 fixture rectified on the device through the fisheye lens and handed, device-resident, straight to a3_detect_batch:
    the markers of the oracle detector on the oracle-rectified frame (K and the view chosen so that the oracle finds all four)"""
    from aruco3_amd import _lib
    from oracle import a3oracle

    torch = _torch()
    w, h = 640, 480
    raw = np.fromfile(ROOT / "tests" / "fixtures" / "inputs" / "c1_640x480_aruco.raw", np.uint8).reshape(1, h, w, 3)
    d = _dict("ARUCO_DEFAULT")
    K, new_K = (700.0, 700.0, 320.0, 240.0), (630.0, 630.0, 320.0, 240.0)
    det = _lib.Context(_lib.default_config(), d.code_list, d.num_bits, d._tau)
    src = torch.from_numpy(raw).cuda()
    dst = torch.empty((1, h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    det.rectify_frames(src.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w * 3, w * h * 3, 1, _rec((w, h), K, MILD, (w, h), new_K, fill=0),
                       dst.data_ptr(), _lib.MEM_DEVICE, w * 3, w * h * 3)
    m, per = det.detect_batch(dst.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, 1)
    want_frame = fo.rectify(raw, K, MILD, new_K, fill=0)[0]
    ref = a3oracle.detect(want_frame, d.code_list, d.num_bits, d._tau, keep_debug=False)
    assert len(ref["markers"]) == 4 and int(per[0]) == 4
    assert markers_of_hip(m) == markers_of_oracle(ref)
    assert np.array_equal(dst.cpu().numpy()[0], want_frame)
    det.close()


# ---- argument errors: all refused on the host ----

def test_argument_errors(ctx):
    from aruco3_amd import _lib

    torch = _torch()
    w, h, c = 32, 16, 3
    src = torch.zeros((1, h, w, c), dtype=torch.uint8, device="cuda")
    dst = torch.zeros((1, h, w, c), dtype=torch.uint8, device="cuda")
    K = (40.0, 40.0, 16.0, 8.0)
    intr = _lib.Intrinsics(w, h, *K)
    pts = np.array([[3.0, 4.0], [20.0, 9.0]], np.float32)

    def entry_points(d):
        rec = _rec((w, h), K, MILD, (w, h), K)
        rec.distortion = d
        return (lambda: ctx.set_distortion(d), lambda: ctx.undistort_points(pts, intr, d),
                lambda: ctx.rectify_frames(src.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w * c, h * w * c, 1, rec, dst.data_ptr(), _lib.MEM_DEVICE,
                                           w * c, h * w * c))

    for call in entry_points(_dist()):   # (the arguments every case below departs from are accepted)
        call()
    ctx.set_distortion(None)
    bad = []
    for field in ("p1", "p2", "k5", "k6"):
        d = _dist()
        setattr(d, field, 1e-3)
        bad.append(d)
    d = _dist()
    d.k4 = float("nan")
    bad.append(d)
    for model in (2, 4):
        d = _dist()
        d.model = model
        bad.append(d)
    for d in bad:
        for call in entry_points(d):
            with pytest.raises(_lib.A3Error) as e:
                call()
            assert e.value.code == _lib.ERR_INVALID


# ---- Python surface ----

def test_python_surface(scene):
    """rectify_frames: numpy in / numpy out and CUDA tensor in / CUDA tensor out, the same bytes.  undistort_points: numpy only -- it
    and a3_undistort_points below it take host pointers, with the rational model as well, and the fisheye model changes no
    signature.  Detector.detect_batch_with_pose fills corners_undistorted."""
    import aruco3_amd
    from aruco3_amd import CameraIntrinsics, Distortion, undistort_points
    from aruco3_amd.aruco import Detector, DetectorConfig

    torch = _torch()
    frames = _noise(2, 59, 131, 3, 29)
    K = (60.0, 60.0, 65.0, 29.0)
    ci = CameraIntrinsics(131, 59, *K, distortion=Distortion.fisheye(*MILD))
    a = aruco3_amd.rectify_frames(frames, ci, fill=FILL)
    assert isinstance(a, np.ndarray) and np.array_equal(a, fo.rectify(frames, K, MILD, K, (131, 59), None, FILL))
    t = aruco3_amd.rectify_frames(torch.from_numpy(frames).cuda(), ci, fill=FILL)
    assert isinstance(t, torch.Tensor) and t.is_cuda and np.array_equal(t.cpu().numpy(), a)
    pts = _field()[::41]
    und, res = undistort_points(pts, ci)
    want, wres = fo.undistort(pts, K, MILD)
    assert np.array_equal(_bits(und), _bits(want)) and np.array_equal(_bits(res), _bits(wres))

    d, board, scenes, dev = scene
    ci = CameraIntrinsics(W, H, *bu.K1080, distortion=Distortion.from_opencv_fisheye(MILD))
    det = Detector(DetectorConfig(min_corner_separation_factor=bu.MIN_CORNER_SEPARATION_FACTOR), d, board=board)
    out = det.detect_batch_with_pose(dev, 30.0, ci)
    mk = [m for det_, _ in out for m in det_.markers]
    assert len(mk) >= 60 and all(m.corners_undistorted is not None and len(m.undistort_residual_px) == 4 for m in mk)
    und, res = fo.undistort(np.array([m.corners for m in mk], np.float32), bu.K1080, MILD)
    assert np.array_equal(_bits(und).reshape(-1), _bits(np.array([m.corners_undistorted for m in mk], np.float32)).reshape(-1))
    assert np.array_equal(_bits(res), _bits(np.array([m.undistort_residual_px for m in mk], np.float32)).reshape(-1))
    bp = det.detect_batch_with_board_pose(dev, ci, 30.0)
    assert all(b.ok for _, b in bp) and bp[0][0].markers[0].corners_undistorted is not None


# ---- accuracy through a lens ----

def test_accuracy_through_a_fisheye_lens():
    """test_gpu_distortion.py's test_accuracy_through_a_lens with the fisheye renderer (tests/fisheye_util.py): the 5 x 7 grid board at
    1280 x 720 through the `mild` lens at K720 -- the undistorted refined corners against the ideal pinhole projections, and the board
    pose's rotation error with and without the distortion set.  The bounds are that test's own."""
    from aruco3_amd import _lib
    from tests import fisheye_util as fu

    torch = _torch()
    d = _dict()
    board = _board()
    rng = np.random.default_rng(11)
    scenes, frames = [], []
    for off in ((-300.0, -90.0), (290.0, 90.0), (-280.0, 100.0), (300.0, -90.0)):   # (the board reaches into the image corners)
        R, t = bu.board_pose_facing(board, rng.uniform(20, 40), rng.uniform(0, 360), rng.uniform(-20, 20), rng.uniform(480, 520), off, K=fu.K720)
        scenes.append((R, t))
        frames.append(fu.render(board, d, R, t))
    frames = np.stack(frames)[..., None]
    n, h, w = frames.shape[:3]
    dev = torch.from_numpy(np.ascontiguousarray(frames)).cuda()
    torch.cuda.synchronize()
    intr = _lib.Intrinsics(w, h, *fu.K720)
    res = {}
    for with_dist in (False, True):
        c = _lib.Context(bu.config(), d.code_list, d.num_bits, d._tau)
        c.set_corner_refinement(_lib.default_refine_config())
        c.set_board(board.ids, board.corners)
        if with_dist:
            c.set_distortion(_dist(fu.MILD))
        m, p, _ = c.detect_batch_pose(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_L8, w, h, w, w * h, n, 30.0, intr)
        recs = c.board_poses()
        corners = c.undistorted_corners()[0] if with_dist else c.refined_corners()
        errs, rot = [], []
        pos = 0
        for f, (R, t) in enumerate(scenes):
            truth = bu.project(board, R, t, fu.K720)
            for i in range(pos, pos + int(p[f])):
                slot = np.nonzero(board.ids == m[i]["id"])[0]
                if slot.size:
                    errs.append(np.linalg.norm(corners[i] - truth[slot[0]], axis=1))
            pos += int(p[f])
            assert recs[f]["status"] == 1 and recs[f]["markers_used"] >= 15, (f, recs[f])
            rot.append(bu.rotation_error_deg(recs[f]["rotation"].reshape(3, 3), R))
        errs = np.concatenate(errs)
        res[with_dist] = (float(np.median(errs)), float(np.percentile(errs, 95)), float(np.max(errs)), float(np.median(rot)), float(np.max(rot)))
        print(f"fisheye distortion={with_dist}: corner error median {res[with_dist][0]:.3f} px, p95 {res[with_dist][1]:.3f} px, "
              f"max {res[with_dist][2]:.3f} px; board rotation error median {res[with_dist][3]:.3f} deg, max {res[with_dist][4]:.3f} deg")
        c.close()
    # the same scenes through the CPU restatements of the chain: 16.1 px / 6.93 deg without (max 9.2 deg), 0.31 px / 0.125 deg with
    # (max 0.56 deg)
    assert res[False][0] > 5.0                              # the lens moves the corners by tens of pixels
    assert res[True][0] < 0.5
    assert res[True][3] < 0.05 * res[False][3] and res[True][4] < 1.0
