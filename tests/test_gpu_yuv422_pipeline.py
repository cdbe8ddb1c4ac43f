"""The luma rule end to end: every call that takes frames returns, for a packed 4:2:2 buffer (YUYV, UYVY), bit for bit what it returns for
the L8 plane of those luma bytes -- markers against the CPU oracle, and the pose call, refinement, board pose, ChArUco corners and pose,
board recovery, a lens on the pose call, detection on reduced and on rectified frames, reduce_frames, rectify_frames and a BatchQueue
against the library's own L8 run, every returned array compared byte for byte.  Four 320 x 240 frames of a GridBoard and four of a
CharucoBoard (tests/yuv422_scenes.py; tests/test_yuv422_scenes.py shows on the CPU that none of the lists compared here is empty), drawn
by the library's renderer, interleaved with noise chroma; from host and from device memory, and once more as planar NV12 / I420 buffers.
GPU only."""
import dataclasses
import struct

import numpy as np
import pytest

from tests import board_util as bu
from tests import reduced_cases as rd
from tests import rectify_oracle as ro
from tests import yuv422_scenes as sc
from tests import yuv422_util as yu

pytestmark = pytest.mark.gpu


# ---- bit-for-bit comparison of whatever a call returns ----------------------------------------------------------------------------
def _same(a, b, where="result"):
    """lists, tuples, dataclasses, numpy arrays (dtype, shape and bytes), floats (their bits), everything else by =="""
    assert type(a) is type(b), (where, type(a), type(b))
    if isinstance(a, (list, tuple)):
        assert len(a) == len(b), (where, len(a), len(b))
        for i, (x, y) in enumerate(zip(a, b)):
            _same(x, y, f"{where}[{i}]")
    elif dataclasses.is_dataclass(a):
        for f in dataclasses.fields(a):
            _same(getattr(a, f.name), getattr(b, f.name), f"{where}.{f.name}")
    elif isinstance(a, np.ndarray):
        assert a.dtype == b.dtype and a.shape == b.shape, (where, a.dtype, b.dtype, a.shape, b.shape)
        assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), (where, a, b)
    elif isinstance(a, float):
        assert struct.pack("<d", a) == struct.pack("<d", b), (where, a, b)
    else:
        assert a == b, (where, a, b)


def _n_markers(result):
    """markers in a list of Detections or of (Detection, something) pairs"""
    return sum(len((r[0] if isinstance(r, tuple) else r).markers) for r in result)


# ---- the frames ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def luma():
    import torch

    assert torch.cuda.is_available(), "needs the MI355X"
    out = {kind: sc.device_luma(kind) for kind in ("grid", "charuco")}
    for g in out.values():
        g.setflags(write=False)
    return out


def _inputs(luma_frames):
    """(name, frames, pixel_format) for both formats, from host and from device memory, as drawn and with the chroma complemented"""
    import torch

    out = []
    for fmt in yu.FORMATS:
        px = yu.interleave(luma_frames, fmt, seed=7)
        out.append((f"{fmt} host", px, yu.PIXEL_FORMAT[fmt]))
        out.append((f"{fmt} device", torch.from_numpy(px).cuda(), yu.PIXEL_FORMAT[fmt]))
        out.append((f"{fmt} device, chroma complemented", torch.from_numpy(yu.complement_chroma(px, fmt)).cuda(), yu.PIXEL_FORMAT[fmt]))
    torch.cuda.synchronize()
    return out


def _config():
    from aruco3_amd import DetectorConfig

    return DetectorConfig(min_corner_separation_factor=bu.MIN_CORNER_SEPARATION_FACTOR)


def _detector(**kw):
    from aruco3_amd import Detector

    return Detector(_config(), sc.dictionary(), **kw)


def _camera(lens=False):
    from aruco3_amd import CameraIntrinsics, Distortion

    return CameraIntrinsics(sc.W, sc.H, *sc.K, distortion=Distortion(*sc.LENS) if lens else None)


def _check(call, luma_frames, least_markers=1):
    """call(frames, pixel_format) on the L8 plane, then on every 4:2:2 input: the same, to the bit -> the L8 result"""
    want = call(np.ascontiguousarray(luma_frames), None)
    if least_markers:
        assert _n_markers(want) >= least_markers, "the L8 run found nothing: the comparison would prove nothing"
    for name, frames, pf in _inputs(luma_frames):
        _same(call(frames, pf), want, name)
    return want


# ---- 1. markers against the oracle, the debug taps ---------------------------------------------------------------------------------
def test_detect_batch_equals_the_oracle(oracle, luma):
    d = sc.dictionary()
    det = _detector()
    g = luma["grid"]
    refs = [oracle.detect(np.ascontiguousarray(f), d.code_list, d.num_bits, d._tau, sc.oracle_config()) for f in g]
    assert all(len(r["markers"]) >= 3 for r in refs), [len(r["markers"]) for r in refs]
    for name, frames, pf in _inputs(g):
        got = det.detect_batch(frames, populate=True, pixel_format=pf)
        for f, (dt, r) in enumerate(zip(got, refs)):
            assert [(m.id, m.code, tuple(m.corners), m.hamming_distance) for m in dt.markers] == \
                [(x["id"], x["code"], tuple(map(tuple, x["corners"])), x["hamming_distance"]) for x in r["markers"]], (name, f)
            assert np.array_equal(dt.grey, g[f]), (name, f)                                 # Detection.grey is the luma plane
            assert dt.candidates == [list(map(tuple, q)) for q in r["candidates"].tolist()], (name, f)
    _check(lambda x, pf: det.detect_batch(x, pixel_format=pf), g, 12)
    _check(lambda x, pf: [det.detect(x[0], pixel_format=pf)], g, 3)
    raw = det.detect_batch_raw(np.ascontiguousarray(g))
    for name, frames, pf in _inputs(g):
        m, per = det.detect_batch_raw(frames, pixel_format=pf)
        assert m.tobytes() == raw[0].tobytes() and np.array_equal(per, raw[1]), name


# ---- 2. everything behind the marker list ----------------------------------------------------------------------------------------------
def test_poses_refinement_board_recovery_and_lens(luma):
    from aruco3_amd import BoardRecovery
    from aruco3_amd.aruco import CornerRefinement

    g, board = luma["grid"], sc.grid_board()
    plain, refining = _detector(), _detector(refinement=CornerRefinement())
    _check(lambda x, pf: plain.detect_batch_with_pose(x, sc.SIZE_MM, _camera(), pixel_format=pf), g, 12)
    _check(lambda x, pf: plain.detect_batch_with_pose(x, sc.SIZE_MM, None, pixel_format=pf), g, 12)
    want = _check(lambda x, pf: refining.detect_batch_with_pose(x, sc.SIZE_MM, _camera(), pixel_format=pf), g, 12)
    assert all(m.corners_refined is not None for d, _ in want for m in d.markers)
    want = _check(lambda x, pf: plain.detect_batch_with_pose(x, sc.SIZE_MM, _camera(lens=True), pixel_format=pf), g, 12)   # a lens on the pose call
    assert all(m.corners_undistorted is not None for d, _ in want for m in d.markers)
    on_board = _detector(board=board, refinement=CornerRefinement())
    want = _check(lambda x, pf: on_board.detect_batch_with_board_pose(x, _camera(), sc.SIZE_MM, pixel_format=pf), g, 12)
    assert all(p.status == 1 and p.markers_used >= 3 for _, p in want)
    recovering = _detector(board=board, recovery=BoardRecovery(max_hamming=255))
    _check(lambda x, pf: recovering.detect_batch(x, pixel_format=pf), g, 12)
    # the stand-alone refinement of caller corners
    starts = np.array([m.corners for m in want[0][0].markers], np.float32) + np.float32(0.4)
    alone = _check(lambda x, pf: [refining.refine_corners(x[0], starts, pixel_format=pf)], g, 0)
    assert alone[0].shape == (len(starts) * 4, 2) and np.isfinite(alone[0]).all() and not np.array_equal(alone[0], starts.reshape(-1, 2))


def test_charuco_corners_and_pose(luma):
    from aruco3_amd.aruco import CornerRefinement

    g, board = luma["charuco"], sc.charuco_board()
    det = _detector(board=board, refinement=CornerRefinement())
    want = _check(lambda x, pf: det.detect_batch_with_charuco_pose(x, _camera(), sc.SIZE_MM, pixel_format=pf), g, 8)
    assert sum(len(d.charuco_ids) for d, _ in want) >= 8 and sum(1 for _, p in want if p.status == 1) >= 2
    want = _check(lambda x, pf: det.detect_batch(x, pixel_format=pf), g, 8)
    # the stand-alone interpolation from caller markers
    d0 = want[0]
    ids = np.array([m.id for m in d0.markers], np.uint32)
    corners = np.array([m.corners for m in d0.markers], np.float32)
    alone = _check(lambda x, pf: list(det.interpolate_charuco(x[0], ids, corners, pixel_format=pf)), g, 0)
    assert len(alone[0]) >= 1


# ---- 3. reduced and rectified frames -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("f", sc.FACTORS)
def test_detection_on_reduced_frames(luma, f):
    import aruco3_amd
    from aruco3_amd import Reduction
    from aruco3_amd.aruco import CornerRefinement

    g = luma["grid"]
    det = _detector(reduction=Reduction(f), refinement=CornerRefinement())
    _check(lambda x, pf: det.detect_batch_with_pose(x, sc.SIZE_MM, _camera(), pixel_format=pf), g, 6)
    want = _check(lambda x, pf: det.detect_batch(x, populate=True, pixel_format=pf), g, 6)
    planes = rd.reduce(g[..., None], f)
    assert all(np.array_equal(d.grey, p) for d, p in zip(want, planes))
    # reduce_frames: the numpy restatement of the contract on the luma plane, and the library's own L8 run
    assert np.array_equal(aruco3_amd.reduce_frames(np.ascontiguousarray(g), f), planes)
    for name, frames, pf in _inputs(g):
        out = aruco3_amd.reduce_frames(frames, f, pixel_format=pf)
        out = out.cpu().numpy() if hasattr(out, "cpu") else out
        assert out.dtype == np.uint8 and np.array_equal(out, planes), (name, f)
    # an odd block-column count (W = 318 for f = 3 anyway; a width that is no multiple of the lane's run for the others)
    part = np.ascontiguousarray(g[:, :37, :70])
    for fmt in yu.FORMATS:
        out = aruco3_amd.reduce_frames(yu.interleave(part, fmt, 3), f, pixel_format=yu.PIXEL_FORMAT[fmt])
        assert np.array_equal(out, rd.reduce(part[..., None], f)), (fmt, f)


def test_detection_on_rectified_frames(luma):
    import aruco3_amd
    from aruco3_amd import Rectification

    g = luma["grid"]
    cam = _camera(lens=True)
    det = _detector(rectification=Rectification(cam))
    want = _check(lambda x, pf: det.detect_batch(x, populate=True, pixel_format=pf), g, 8)
    _check(lambda x, pf: det.detect_batch_with_pose(x, sc.SIZE_MM, _camera(), pixel_format=pf), g, 8)
    # rectify_frames: one byte per pixel out -- the CPU oracle on the luma plane, the library's own L8 run, and the plane detected on
    plane = ro.rectify(g[..., None], sc.K, sc.LENS, sc.K, (sc.W, sc.H), None, 0)
    assert np.array_equal(aruco3_amd.rectify_frames(np.ascontiguousarray(g), cam), plane)
    assert all(np.array_equal(d.grey, p[..., 0]) for d, p in zip(want, plane))
    for name, frames, pf in _inputs(g):
        out = aruco3_amd.rectify_frames(frames, cam, pixel_format=pf)
        out = out.cpu().numpy() if hasattr(out, "cpu") else out
        assert out.shape == (4, sc.H, sc.W, 1) and out.dtype == np.uint8 and np.array_equal(out, plane), name
    # another view size and a fill: the destination is a plane of its own width
    from aruco3_amd import CameraIntrinsics

    view = CameraIntrinsics(201, 150, 190.0, 190.0, 100.0, 75.0)
    plane = ro.rectify(g[..., None], sc.K, sc.LENS, (190.0, 190.0, 100.0, 75.0), (201, 150), ro.rot_y(3.0), 77)
    for name, frames, pf in _inputs(g)[:2]:
        out = aruco3_amd.rectify_frames(frames, cam, view, ro.rot_y(3.0), 77, pixel_format=pf)
        out = out.cpu().numpy() if hasattr(out, "cpu") else out
        assert np.array_equal(out, plane), name


# ---- 4. in flight, and planar buffers ----------------------------------------------------------------------------------------------------
def test_batch_queue_with_two_batches_in_flight(luma):
    from aruco3_amd.aruco import BatchQueue, CornerRefinement

    g = luma["grid"]
    det = _detector(refinement=CornerRefinement())

    def queued(x, pf):
        q = BatchQueue(det, depth=2)
        q.submit(x[:2], pixel_format=pf)
        q.submit(x[2:], pixel_format=pf)
        assert len(q) == 2
        out = q.collect() + q.collect()
        q.close()
        return out

    want = _check(queued, g, 12)
    _same(want, det.detect_batch(np.ascontiguousarray(g)), "queue against the synchronous call")


@pytest.mark.parametrize("layout", ["nv12", "i420"])
def test_planar_buffers_read_in_place(luma, layout):
    import torch

    g = luma["grid"]
    det = _detector()
    want = det.detect_batch(np.ascontiguousarray(g), populate=True)
    assert _n_markers(want) >= 12
    buf = yu.planar(g, seed=len(layout))
    for name, frames in (("host", buf), ("device", torch.from_numpy(buf).cuda())):
        got = det.detect_batch(frames, populate=True, pixel_format=layout)
        _same(got, want, f"{layout} {name}")
        assert all(np.array_equal(d.grey, f) for d, f in zip(got, g))
    _same(det.detect_batch_with_pose(buf, sc.SIZE_MM, _camera(), pixel_format=layout), det.detect_batch_with_pose(np.ascontiguousarray(g), sc.SIZE_MM, _camera()), layout)
