"""Rectification inside the detect calls on the MI355X (a3_set_rectification; k_rectify's grey form): the grey plane byte for byte
against the CPU restatement of the contract (tests/rectify_oracle.c / tests/fisheye_oracle.c, then numpy luma), the markers against
the oracle detector on the oracle-rectified frames, and everything behind the markers against the two-call form (a3_rectify_frames,
then the same call without the setting), which the contract says it equals to the bit.  tests/test_rectified_detection.py checks on
the CPU that none of the expectations used here is empty."""
import ctypes as C
import functools
import re
from pathlib import Path

import numpy as np
import pytest

from tests import board_util as bu
from tests import fisheye_oracle as fo
from tests import lens_oracle as lo
from tests import rectified_cases as rc
from tests import rectify_oracle as ro
from tests.util import marker_tuples, markers_of_hip, markers_of_oracle

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SW, SH = ro.SRC_SIZE   # 333 x 251, the fisheye tests' field
FILL = 77


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


def _kernel_constant(name):
    """a constexpr int of k_rectify.hip"""
    text = (ROOT / "aruco3_amd" / "csrc" / "k_rectify.hip").read_text()
    return int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))


K_CHUNK, K_TILE_H = _kernel_constant("kChunk"), _kernel_constant("kTileH")
N_GREY = K_CHUNK + 1   # more frames than one frame chunk: the grid's z axis is 2


def _fmts():
    from aruco3_amd import _lib

    return {"L8": (_lib.FMT_L8, 1, "rgb"), "RGB8": (_lib.FMT_RGB8, 3, "rgb"), "RGBA8": (_lib.FMT_RGBA8, 4, "rgb"), "BGRA8": (_lib.FMT_BGRA8, 4, "bgr")}


# the lenses of the grey-plane test: (model, source K, coefficients in the oracle's order, rotation)
LENSES = {
    "none_rotated": ("none", ro.SRC_K, None, ro.rot_y(5.0)),
    "rational": ("rational", ro.SRC_K, lo.COEFFS["webcam5"], None),
    "fisheye": ("fisheye", fo.K, fo.COEFFS["mild"], None),
}
# destination sizes against the kernel's store rules: a width that is a multiple of 256 (and a height above one tile), widths = 1, 2, 3
# mod 4 (rows that are not dword-aligned, a last lane that stores byte by byte), one below 4, a destination of one row
VIEWS = [(256, K_TILE_H + 1), (257, 3), (130, 2), (67, 1), (3, 7)]
# a wide view of the 333 x 251 source, whose rim sees nothing: 30 - 37 % of it sees the source through the pinhole lenses at a focal
# length of 50 px, 69 % through the fisheye lens at 20 px (at 50 px that lens still fills the view)
FILL_VIEWS = {lens: ((131, 59), (f, f, 65.0, 29.0)) for lens, f in (("none_rotated", 50.0), ("rational", 50.0), ("fisheye", 20.0))}


def _rec(src_size, K, model, coeffs, new_size, new_K, R=None, fill=FILL):
    from aruco3_amd import _lib

    r = _lib.RectifyRec()
    r.src = _lib.Intrinsics(src_size[0], src_size[1], *K)
    if model == "rational":
        r.distortion = _lib.DistortionRec(_lib.DIST_RATIONAL, 20, *coeffs, 0.1)
    elif model == "fisheye":
        k1, k2, k3, k4 = coeffs
        r.distortion = _lib.DistortionRec(_lib.DIST_FISHEYE, 20, k1, k2, 0.0, 0.0, k3, k4, 0.0, 0.0, 0.1)
    r.dst = _lib.Intrinsics(new_size[0], new_size[1], *new_K)
    r.rotation = (C.c_float * 9)(*[float(v) for v in (np.eye(3) if R is None else np.asarray(R)).reshape(9)])
    r.fill = fill
    return r


def _oracle(model, frames, K, coeffs, new_K, new_size, R, fill=FILL, with_inside=False):
    f = fo.rectify if model == "fisheye" else ro.rectify
    return f(frames, K, coeffs, new_K, new_size, R, fill, with_inside=with_inside)


@functools.lru_cache(maxsize=None)
def _noise(n, h, w, c, seed):
    a = np.random.default_rng(seed).integers(0, 256, (n, h, w, c), dtype=np.uint8)
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _want_grey_inputs(lens, c, view):
    """the oracle-rectified noise frames of one lens, channel count and view, shared by the formats and memory kinds that use them"""
    model, K, coeffs, R = LENSES[lens]
    size, new_K = view
    out, inside = _oracle(model, _noise(N_GREY, SH, SW, c, 3 + c), K, coeffs, new_K, size, R, with_inside=True)
    out.setflags(write=False)
    return out, inside


def _strided(frames, lead=5, row_pad=7, frame_gap=13):
    """the frames `lead` bytes (odd) into a buffer with padded rows and frames -> (buffer, lead, row stride, frame stride)"""
    n, h, w, c = frames.shape
    row = w * c + row_pad
    frame = row * h + frame_gap
    buf = np.full(lead + frame * n, 0x5A, np.uint8)
    for k in range(n):
        v = buf[lead + k * frame: lead + k * frame + row * h].reshape(h, row)
        v[:, : w * c] = frames[k].reshape(h, w * c)
    return buf, lead, row, frame


class _Source:
    """frames laid out by _strided, on the host or on the device"""

    def __init__(self, frames, on_device, **kw):
        from aruco3_amd import _lib

        buf, self.lead, self.row, self.frame = _strided(frames, **kw)
        if on_device:
            torch = _torch()
            self.keep = torch.from_numpy(buf).cuda()
            torch.cuda.synchronize()
            self.ptr, self.mem = self.keep.data_ptr() + self.lead, _lib.MEM_DEVICE
        else:
            self.keep = buf
            self.ptr, self.mem = buf.ctypes.data + self.lead, _lib.MEM_HOST
        self.n, self.h, self.w = frames.shape[:3]

    def args(self, fmt):
        return (self.ptr, self.mem, fmt, self.w, self.h, self.row, self.frame, self.n)


def _ctx(cfg=None):
    from aruco3_amd import _lib

    _torch()
    d = rc.dictionary()
    return _lib.Context(cfg or bu.config(), d.code_list, d.num_bits, d._tau)


def _has_setter():
    from aruco3_amd import _lib

    assert hasattr(_lib.load(), "a3_set_rectification"), "the library has no a3_set_rectification"


# ---- 1. the grey plane, every pixel ----

@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("lens", list(LENSES))
@pytest.mark.parametrize("fmt", ["L8", "RGB8", "RGBA8", "BGRA8"])
def test_grey_plane_equals_luma_of_the_oracle(fmt, lens, mem):
    """a3_download_grey of a tapped batch = luma of the oracle's rectified frame, byte for byte: noise frames (R and B differ, so a
    swapped order shows) of 333 x 251 with padded row and frame strides 5 bytes into their buffer, K_CHUNK + 1 of them, into views at
    the kernel's store rules and into one whose rim sees nothing"""
    _has_setter()
    f, c, order = _fmts()[fmt]
    model, K, coeffs, R = LENSES[lens]
    ctx = _ctx()
    ctx.set_debug_taps(True)
    src = _Source(_noise(N_GREY, SH, SW, c, 3 + c), mem == "device")
    views = [((dw, dh), (300.0, 300.0, dw * 0.5, dh * 0.5)) for dw, dh in VIEWS] + [FILL_VIEWS[lens]]
    for view in views:
        (dw, dh), new_K = view
        ctx.set_rectification(_rec((SW, SH), K, model, coeffs, (dw, dh), new_K, R))
        ctx.detect_batch(*src.args(f), out_cap=4096)
        rect, inside = _want_grey_inputs(lens, c, view)
        want = rc.luma(rect, order)
        for k in range(N_GREY):
            got = ctx.download_grey(k, dw, dh)
            assert np.array_equal(got, want[k]), (fmt, lens, mem, view, k, int((got != want[k]).sum()))
        if view is FILL_VIEWS[lens]:
            assert inside.any() and not inside.all()   # the view partly sees nothing
            assert np.all(want[:, ~inside] == FILL)
    ctx.close()


@pytest.mark.parametrize("fmt", ["L8", "BGRA8"])
def test_grey_plane_of_a_one_column_source(fmt):
    """the pair load has no neighbour to fetch"""
    _has_setter()
    f, c, order = _fmts()[fmt]
    sw, sh = 1, 7
    K = (8.0, 8.0, 0.0, 3.0)
    frames = _noise(3, sh, sw, c, 13)
    ctx = _ctx()
    ctx.set_debug_taps(True)
    for new_K, size in (((32.0, 32.0, 16.0, 12.0), (33, 25)), ((8.0, 8.0, 2.0, 1.0), (5, 3))):
        ctx.set_rectification(_rec((sw, sh), K, "rational", lo.COEFFS["tangential"], size, new_K))
        src = _Source(frames, True, lead=3, row_pad=2, frame_gap=1)
        ctx.detect_batch(*src.args(f))
        rect, inside = ro.rectify(frames, K, lo.COEFFS["tangential"], new_K, size, None, FILL, with_inside=True)
        assert inside.any()
        want = rc.luma(rect, order)
        for k in range(3):
            assert np.array_equal(ctx.download_grey(k, *size), want[k]), (fmt, size, k)
    ctx.close()


# ---- 2. the markers ----

def _case_ctx(name, **kw):
    ctx = _ctx(**kw)
    ctx.set_rectification(rc.rectification(rc.CASES[name])._c())
    return ctx


@pytest.mark.parametrize("mem", ["host", "device"])
@pytest.mark.parametrize("name", list(rc.CASES))
def test_markers_equal_the_oracle_on_oracle_rectified_frames(name, mem):
    """ids, corners, codes, hamming distance, rotation, order and per-frame counts"""
    from aruco3_amd import _lib

    _has_setter()
    frames = rc.source_frames(name)
    _, _, res = rc.expectation(name)
    ctx = _case_ctx(name)
    src = _Source(frames, mem == "device")
    m, per = ctx.detect_batch(*src.args(_lib.FMT_RGB8))
    assert [int(v) for v in per] == [len(r["markers"]) for r in res]
    pos = 0
    for f, r in enumerate(res):
        assert markers_of_hip(m[pos: pos + int(per[f])]) == markers_of_oracle(r), (name, f)
        assert all(int(v) == f for v in m[pos: pos + int(per[f])]["frame"])
        pos += int(per[f])
    assert pos == len(m)
    ctx.close()


# ---- 3. everything behind the markers: the one-call form against the two-call form ----

def _same_records(a, b, what):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    assert a.dtype == b.dtype and a.shape == b.shape, (what, a.shape, b.shape)
    if a.dtype.names:
        for field in a.dtype.names:   # (field by field: padding bytes of a record are not data)
            assert np.ascontiguousarray(a[field]).tobytes() == np.ascontiguousarray(b[field]).tobytes(), (what, field)
    else:
        assert a.tobytes() == b.tobytes(), what


def _everything(ctx, args, intr, board, charuco):
    """a pose batch with refinement and the board set -> every result the batch has"""
    from aruco3_amd import _lib

    ctx.set_corner_refinement(_lib.default_refine_config())
    ctx.set_board(board.ids, board.corners)
    if charuco:
        ctx.set_charuco(board.chessboard_corners, board.adjacent_ids, None)
    m, per, poses = ctx.detect_batch_pose(*args, 30.0, intr)
    out = {"markers": m, "per": per, "poses": poses, "refined": ctx.refined_corners(), "board": ctx.board_poses()}
    if charuco:
        out["charuco"] = ctx.charuco_corners()
        out["charuco_pose"] = ctx.charuco_poses()
    return out


def _two_calls(case, frames_dev, intr, board, charuco):
    from aruco3_amd import _lib

    torch = _torch()
    n, h, w, c = frames_dev.shape
    dw, dh = case.view_size
    ctx = _ctx()
    flat = torch.empty((n, dh, dw, c), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.rectify_frames(frames_dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w * c, h * w * c, n, rc.rectification(case)._c(), flat.data_ptr(),
                       _lib.MEM_DEVICE, dw * c, dh * dw * c)
    out = _everything(ctx, (flat.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, dw, dh, dw * c, dh * dw * c, n), intr, board, charuco)
    ctx.close()
    return out


def _one_call(case, frames_dev, intr, board, charuco):
    from aruco3_amd import _lib

    n, h, w, c = frames_dev.shape
    ctx = _ctx()
    ctx.set_rectification(rc.rectification(case)._c())
    out = _everything(ctx, (frames_dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * c, h * w * c, n), intr, board, charuco)
    ctx.close()
    return out


@pytest.mark.parametrize("with_intrinsics", [True, False])
@pytest.mark.parametrize("name", list(rc.CASES))
def test_grid_board_results_equal_the_two_call_form(name, with_intrinsics):
    """refined corners, marker poses and the board pose of a GridBoard; without intrinsics the poses normalise by the VIEW's size"""
    from aruco3_amd import _lib

    _has_setter()
    torch = _torch()
    case = rc.CASES[name]
    dev = torch.from_numpy(rc.source_frames(name).copy()).cuda()
    torch.cuda.synchronize()
    intr = _lib.Intrinsics(case.view_size[0], case.view_size[1], *case.view_K) if with_intrinsics else None
    one, two = _one_call(case, dev, intr, rc.board(), False), _two_calls(case, dev, intr, rc.board(), False)
    assert len(one["markers"]) >= 3 * len(dev) and all(int(s) == 1 for s in one["board"]["status"])
    assert marker_tuples(one["markers"]) == marker_tuples(two["markers"])
    for key in ("per", "poses", "refined", "board"):
        _same_records(one[key], two[key], key)


@pytest.mark.parametrize("name", ["rational", "fisheye"])
def test_charuco_results_equal_the_two_call_form(name):
    """ChArUco corners and the ChArUco pose: a small chessboard rendered on the device and taken as the frames of the case's camera"""
    from aruco3_amd import _lib
    from aruco3_amd.board import CharucoBoard
    from tests import charuco_util as cu

    _has_setter()
    torch = _torch()
    case = rc.CASES[name]
    b = CharucoBoard(4, 3, 40.0, 28.0, first_id=5)
    scenes = []
    for tilt, direction, roll, off in ((0.0, 0.0, 0.0, (0.0, 0.0)), (25.0, 70.0, 10.0, (30.0, -20.0)), (15.0, 200.0, -12.0, (-60.0, 25.0))):
        R, t = bu.board_pose_facing(b, tilt, direction, roll, 300.0, off, K=rc.SRC_K)
        scenes.append(cu.Scene(b, R, t, K=rc.SRC_K))
    dev = cu.render(scenes, rc.dictionary(), rc.SRC_SIZE[0], rc.SRC_SIZE[1])
    torch.cuda.synchronize()
    intr = _lib.Intrinsics(case.view_size[0], case.view_size[1], *case.view_K)
    one, two = _one_call(case, dev, intr, b, True), _two_calls(case, dev, intr, b, True)
    # (not an empty comparison: 3 markers per frame on average, chessboard corners, and a frame whose ChArUco pose was solved)
    found = (len(one["markers"]), len(one["charuco"]), [int(s) for s in one["charuco_pose"]["status"]])
    assert found[0] >= 3 * len(dev) and found[1] >= 6 and 1 in found[2], found
    assert marker_tuples(one["markers"]) == marker_tuples(two["markers"])
    for key in ("per", "poses", "refined", "board", "charuco", "charuco_pose"):
        _same_records(one[key], two[key], key)


def test_python_detector_equals_rectify_frames_then_detect():
    """Detector(rectification=...) against aruco3_amd.rectify_frames + a plain Detector, on a CUDA tensor and on a numpy array"""
    import aruco3_amd
    from aruco3_amd import Detector, DetectorConfig
    from aruco3_amd.aruco import CornerRefinement

    _has_setter()
    torch = _torch()
    case = rc.CASES["rational"]
    cam, view = rc.intrinsics(case)
    frames = rc.source_frames("rational").copy()
    cfg = DetectorConfig(min_corner_separation_factor=bu.MIN_CORNER_SEPARATION_FACTOR)
    kw = dict(config=cfg, dictionary=rc.dictionary(), refinement=CornerRefinement(), board=rc.board())
    one, plain = Detector(rectification=rc.rectification(case), **kw), Detector(**kw)
    for images in (torch.from_numpy(frames).cuda(), frames):
        flat = aruco3_amd.rectify_frames(images, cam, view, rc.rotation(case), case.fill)
        got, want = one.detect_batch_with_pose(images, 30.0, view), plain.detect_batch_with_pose(flat, 30.0, view)
        assert len(got) == len(want) == len(frames)
        for (gd, gp), (wd, wp) in zip(got, want):
            assert gd.markers == wd.markers and len(gd.markers) >= 3
            assert all(a.error == b.error and np.array_equal(a.rotation, b.rotation) and np.array_equal(a.translation, b.translation)
                       for g, w in zip(gp, wp) for a, b in zip(g, w))
        gb, wb = one.detect_batch_with_board_pose(images, view, 30.0), plain.detect_batch_with_board_pose(flat, view, 30.0)
        assert all(g[0].markers == w[0].markers and g[1].ok and np.array_equal(g[1].rotation, w[1].rotation)
                   and np.array_equal(g[1].translation, w[1].translation) for g, w in zip(gb, wb))
    tapped = one.detect_batch(frames, populate=True)   # the debug taps report the view
    _, grey, _ = rc.expectation("rational")
    assert all(np.array_equal(d.grey, grey[k]) for k, d in enumerate(tapped))


# ---- 4. in flight ----

def _batches(name):
    """8 small batches with different contents: two frames of the case each, one of them shifted by a few columns"""
    frames = rc.source_frames(name)
    return [np.ascontiguousarray(np.stack([frames[k % 3], np.roll(frames[(k + 1) % 3], 3 * k - 9, axis=1)])) for k in range(8)]


@pytest.mark.parametrize("resident", ["device", "host"])
@pytest.mark.parametrize("gates", [False, True])
@pytest.mark.parametrize("name", ["fisheye", "none_rotated_smaller"])   # a view of the source's size, and a smaller one
def test_batch_queue_equals_the_synchronous_results(name, gates, resident):
    """... and with gates the library does hold chains: a batch's plan is asked for with the VIEW's size, which is the batch's"""
    from aruco3_amd import Detector, DetectorConfig
    from aruco3_amd.aruco import BatchQueue

    _has_setter()
    torch = _torch()
    case = rc.CASES[name]
    det = Detector(DetectorConfig(min_corner_separation_factor=bu.MIN_CORNER_SEPARATION_FACTOR), rc.dictionary(), rectification=rc.rectification(case))
    batches = _batches(name)
    if resident == "device":
        batches = [torch.from_numpy(b).cuda() for b in batches]
        torch.cuda.synchronize()
    want = [det.detect_batch(b) for b in batches]
    assert all(sum(len(d.markers) for d in w) >= 3 for w in want) and len({repr(w) for w in want}) > 1
    q = BatchQueue(det, depth=4, gates=gates)
    got, seen = [], []
    for rounds in range(2):   # a second pass: every context of the rotation is re-used, its plan and pools in place
        pending = 0
        for b in batches:
            if q.full:
                got.append(q.collect())
                seen.append(q.last_stepping)
                pending -= 1
            q.submit(b)
            pending += 1
        while pending:
            got.append(q.collect())
            seen.append(q.last_stepping)
            pending -= 1
    q.close()
    assert got == want + want
    if gates:   # (no quiet fall-back to the ungated path)
        assert "held_released_by_last" in seen and "burst_last" in seen, seen
    else:
        assert set(seen) == {"whole"}, seen


def test_gated_submit_after_a_plain_batch_of_the_sources_size():
    """two contexts whose device plan comes from a plain batch of the SOURCE's size get a rectification with a smaller view: the gated
    submit that follows is planned by the view's size -- not held while that shape has no plan, held once it has one -- and every
    batch equals the oracle"""
    from aruco3_amd import _lib

    _has_setter()
    torch = _torch()
    name = "none_rotated_smaller"
    case = rc.CASES[name]
    assert case.view_size != rc.SRC_SIZE
    _, _, res = rc.expectation(name)
    frames = rc.source_frames(name)
    src = _Source(frames, True, lead=0, row_pad=0, frame_gap=0)
    a, b = _ctx(), _ctx()
    plain = torch.zeros_like(src.keep)
    torch.cuda.synchronize()
    w, h = rc.SRC_SIZE
    for c in (a, b):   # a plain batch of the source's size and frame count: the context's plan is now valid for that shape
        m, _ = c.detect_batch(plain.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, len(frames))
        assert len(m) == 0
        c.set_rectification(rc.rectification(case)._c())

    def same_as_oracle(m, per):
        assert [int(v) for v in per] == [len(r["markers"]) for r in res]
        pos = 0
        for f, r in enumerate(res):
            assert markers_of_hip(m[pos: pos + int(per[f])]) == markers_of_oracle(r), f
            pos += int(per[f])

    steppings = []
    for rounds in range(3):
        a.order_after(b)
        a.submit(*src.args(_lib.FMT_RGB8))        # gated: a burst member
        between = a.stats()["stepping"]
        b.submit(*src.args(_lib.FMT_RGB8))        # no gates: the burst's last member
        same_as_oracle(*a.collect())
        steppings.append((between, a.stats()["stepping"]))
        same_as_oracle(*b.collect())
        steppings[-1] += (b.stats()["stepping"],)
    assert steppings[0] == ("whole", "whole", "whole"), steppings   # the view's shape had no plan yet: nothing to hold
    assert steppings[-1] == ("held", "held_released_by_last", "burst_last"), steppings
    a.close()
    b.close()


# ---- 5. setting and unsetting ----

def test_set_get_and_unset():
    from aruco3_amd import _lib

    _has_setter()
    torch = _torch()
    name = "none_rotated_smaller"
    case = rc.CASES[name]
    rect, grey, res = rc.expectation(name)
    ctx = _ctx()
    assert ctx.rectification() is None
    r = rc.rectification(case)._c()
    ctx.set_rectification(r)
    assert bytes(ctx.rectification()) == bytes(r)
    src = _Source(rc.source_frames(name), True)
    m, per = ctx.detect_batch(*src.args(_lib.FMT_RGB8))
    assert [int(v) for v in per] == [len(x["markers"]) for x in res]
    ctx.set_rectification(None)
    assert ctx.rectification() is None
    raw = _lib.RectifyRec()
    on = C.c_int(7)
    assert _lib.load().a3_get_rectification(ctx.handle, C.byref(raw), C.byref(on)) == 0 and on.value == 0 and bytes(raw) == bytes(len(bytes(raw)))
    # plain frames of the destination size: what a context that never had the setting returns
    dw, dh = case.view_size
    plain = torch.from_numpy(rect.copy()).cuda()
    torch.cuda.synchronize()
    args = (plain.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, dw, dh, dw * 3, dw * dh * 3, len(rect))
    m2, per2 = ctx.detect_batch(*args)
    fresh = _ctx()
    m3, per3 = fresh.detect_batch(*args)
    assert marker_tuples(m2) == marker_tuples(m3) and np.array_equal(per2, per3) and marker_tuples(m2) == marker_tuples(m)
    fresh.close()
    ctx.close()


# ---- 6. refusals ----

def _refused(fn, needle=None):
    from aruco3_amd import _lib

    with pytest.raises(_lib.A3Error) as e:
        fn()
    assert e.value.code == _lib.ERR_INVALID
    if needle is not None:
        assert needle in str(e.value), str(e.value)


def test_detect_refuses_a_size_that_is_not_the_sources():
    from aruco3_amd import _lib

    _has_setter()
    torch = _torch()
    ctx = _case_ctx("rational")
    w, h = rc.SRC_SIZE
    frames = torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    D = _lib.MEM_DEVICE
    for ww, hh in ((w - 1, h), (w, h - 1), (h, w), (0, h)):
        _refused(lambda: ctx.detect_batch(frames.data_ptr(), D, _lib.FMT_RGB8, ww, hh, ww * 3, ww * hh * 3, 1), "a3_set_rectification")
        _refused(lambda: ctx.submit(frames.data_ptr(), D, _lib.FMT_RGB8, ww, hh, ww * 3, ww * hh * 3, 1))
        _refused(lambda: ctx.detect_batch_pose(frames.data_ptr(), D, _lib.FMT_RGB8, ww, hh, ww * 3, ww * hh * 3, 1, 30.0, None))
    m, per = ctx.detect_batch(frames.data_ptr(), D, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, 1)   # (and the source's size goes through)
    assert len(m) == 0 and int(per[0]) == 0
    ctx.close()


def test_setter_refuses_what_rectify_frames_refuses_about_an_a3_rectify():
    """every refusal of tests/test_gpu_rectify.py's test_argument_errors that concerns the a3_rectify, with a3_last_error naming the setter"""
    _has_setter()
    ctx = _ctx()
    w, h = 32, 16
    K = (40.0, 40.0, 16.0, 8.0)

    def good():
        return _rec((w, h), K, "rational", lo.COEFFS["webcam5"], (w, h), K)

    def refused(rec):
        _refused(lambda: ctx.set_rectification(rec), "a3_set_rectification")
        assert ctx.rectification() is None   # (a refused record is not kept)

    for which in ("src", "dst"):
        for field, value in (("image_width", 0), ("image_height", 0), ("image_width", 65536), ("image_height", 65536)):
            rec = good()
            setattr(getattr(rec, which), field, value)
            refused(rec)
        rec = good()
        getattr(rec, which).image_width = getattr(rec, which).image_height = 32768   # 2^30 pixels
        refused(rec)
        for field in ("focal_x", "focal_y", "principal_x", "principal_y"):
            for value in (float("nan"), float("inf")):
                rec = good()
                setattr(getattr(rec, which), field, value)
                refused(rec)
        for field in ("focal_x", "focal_y"):
            for value in (0.0, -40.0):
                rec = good()
                setattr(getattr(rec, which), field, value)
                refused(rec)
    for model in (2, 4):   # (2 stays unassigned)
        rec = good()
        rec.distortion.model = model
        refused(rec)
    for k in range(3):
        rec = good()
        rec.reserved[k] = 1
        refused(rec)
    for field in ("k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6"):
        rec = good()
        setattr(rec.distortion, field, float("nan"))
        refused(rec)
    for field in ("p1", "p2", "k5", "k6"):   # the fisheye model reads k1 k2 k3 k4
        rec = _rec((w, h), K, "fisheye", fo.COEFFS["mild"], (w, h), K)
        setattr(rec.distortion, field, 1e-3)
        refused(rec)
    for k in range(9):
        rec = good()
        rec.rotation[k] = float("inf")
        refused(rec)
    ctx.set_rectification(good())   # (the record every case above departs from is accepted)
    assert ctx.rectification() is not None
    ctx.close()


def test_setter_refused_while_a_batch_is_submitted():
    from aruco3_amd import _lib

    _has_setter()
    torch = _torch()
    ctx = _case_ctx("rational")
    r = rc.rectification(rc.CASES["rational"])._c()
    w, h = rc.SRC_SIZE
    frames = torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.submit(frames.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, 1)
    _refused(lambda: ctx.set_rectification(None), "a3_set_rectification")
    _refused(lambda: ctx.set_rectification(r), "a3_set_rectification")
    assert bytes(ctx.rectification()) == bytes(r)
    m, _ = ctx.collect()
    assert len(m) == 0
    ctx.set_rectification(None)   # (and once the batch is collected the setter goes through)
    ctx.close()
