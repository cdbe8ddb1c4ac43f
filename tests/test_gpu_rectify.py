"""Frame rectification on the MI355X (k_rectify; a3_rectify_frames): byte-equal to the CPU restatement (tests/rectify_oracle.c) for
every format, lens and view, at the edges of rows, tiles and frame chunks, through strided buffers whose padding stays untouched,
from and to host and device memory, and chained into the detector without leaving the card."""
import ctypes as C
from pathlib import Path

import numpy as np
import pytest

from tests import lens_oracle as lo
from tests import rectify_oracle as ro
from tests.util import marker_tuples, markers_of_hip, markers_of_oracle

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
SW, SH = ro.SRC_SIZE
FILL = 77


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


@pytest.fixture(scope="module")
def ctx():
    from aruco3_amd import _lib

    _torch()
    c = _lib.Context(_lib.default_config(), np.zeros(1, np.uint64), 64, 1)
    yield c
    c.close()


def _fmts():
    from aruco3_amd import _lib

    return {"L8": (_lib.FMT_L8, 1), "RGB8": (_lib.FMT_RGB8, 3), "RGBA8": (_lib.FMT_RGBA8, 4), "BGRA8": (_lib.FMT_BGRA8, 4)}


def _rec(src_size, K, coeffs, new_size, new_K, R=None, fill=FILL):
    from aruco3_amd import _lib

    r = _lib.RectifyRec()
    r.src = _lib.Intrinsics(src_size[0], src_size[1], *K)
    if coeffs is not None:
        r.distortion = _lib.DistortionRec(_lib.DIST_RATIONAL, 20, *coeffs, 0.1)
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


def _want(frames, K, coeffs, new_size, new_K, R=None, fill=FILL):
    return ro.rectify(frames, K, coeffs, new_K, new_size, R, fill)


def _one_path(info):
    assert info.tiles > 0 and info.path_tiles[0] == info.tiles and list(info.path_tiles)[1:] == [0, 0, 0]   # one launch path ships


# ---- parity ----

@pytest.mark.parametrize("fmt", ["L8", "RGB8", "RGBA8", "BGRA8"])
def test_equals_oracle_byte_for_byte(ctx, fmt):
    """every coefficient set x every view, one call each: 19-25 % of the pixels inside in the zoomed-out view, rays with Wz <= 0 in
    the 80 degree one"""
    f, c = _fmts()[fmt]
    frames = _noise(1, SH, SW, c, 3)
    for name, coeffs in lo.COEFFS.items():
        for view, (new_K, size, deg) in ro.VIEWS.items():
            R = ro.rot_y(deg)
            got, info = _run(ctx, frames, f, _rec((SW, SH), ro.SRC_K, coeffs, size, new_K, R))
            want = _want(frames, ro.SRC_K, coeffs, size, new_K, R)
            assert np.array_equal(got, want), (name, view, int((got != want).sum()))
            _one_path(info)


def test_no_lens_and_identity(ctx):
    """model A3_DIST_NONE takes the coefficients as 0; with fx = fy = 256 and an integer principal point the output is the input"""
    from aruco3_amd import _lib

    for fmt, (f, c) in _fmts().items():
        frames = _noise(2, 61, 97, c, 5)
        K = (256.0, 256.0, 40.0, 23.0)
        got, _ = _run(ctx, frames, f, _rec((97, 61), K, None, (97, 61), K))
        assert np.array_equal(got, frames), fmt
        rec = _rec((97, 61), K, lo.COEFFS["barrel"], (97, 61), K)
        rec.distortion.model = _lib.DIST_NONE   # (coefficients present but not read)
        got, _ = _run(ctx, frames, f, rec)
        assert np.array_equal(got, frames), fmt


# ---- edges of rows, tiles and sources ----

def test_row_and_tile_edges(ctx):
    """output widths around the lane run (4 pixels), the 64-pixel and the 256-pixel wave segment, heights around the 4-row workgroup"""
    coeffs = lo.COEFFS["webcam5"]
    for fmt in ("L8", "RGB8", "RGBA8"):
        f, c = _fmts()[fmt]
        frames = _noise(2, SH, SW, c, 7)
        for dw in (1, 2, 3, 5, 63, 64, 65, 255, 256, 257, 317, 515):
            for dh in (1, 4, 5, 17):
                new_K = (300.0, 300.0, dw * 0.5, dh * 0.5)
                got, _ = _run(ctx, frames, f, _rec((SW, SH), ro.SRC_K, coeffs, (dw, dh), new_K))
                assert np.array_equal(got, _want(frames, ro.SRC_K, coeffs, (dw, dh), new_K)), (fmt, dw, dh)


@pytest.mark.parametrize("size", [(1, 1), (1, 7), (2, 5), (7, 1), (2, 2)])
def test_tiny_sources(ctx, size):
    """a one-pixel, one-column, two-column and one-row source: the pair load has no neighbour to fetch"""
    sw, sh = size
    K = (8.0, 8.0, (sw - 1) * 0.5, (sh - 1) * 0.5)
    for fmt in ("L8", "RGB8", "RGBA8"):
        f, c = _fmts()[fmt]
        frames = _noise(3, sh, sw, c, 13)
        for new_K, new_size in ((K, (sw, sh)), ((32.0, 32.0, 16.0, 12.0), (33, 25)), ((8.0, 8.0, 2.0, 1.0), (5, 3))):
            got, _ = _run(ctx, frames, f, _rec(size, K, lo.COEFFS["tangential"], new_size, new_K))
            want, inside = ro.rectify(frames, K, lo.COEFFS["tangential"], new_K, new_size, None, FILL, with_inside=True)
            assert np.array_equal(got, want), (fmt, size, new_size)
        assert inside.any()


# ---- strides, padding, frames ----

def _strided_call(ctx, fmt, frames, rec, src_mem, dst_mem, src_lead=5, src_pad=7, dst_pad=3, frame_gap=13):
    """the frames laid out `src_lead` bytes into a buffer with padded rows and frames; the output into a padded buffer pre-filled with
    0xA5 -> (output frames, whether every padding byte is still 0xA5)"""
    from aruco3_amd import _lib

    torch = _torch()
    n, h, w, c = frames.shape
    dw, dh = int(rec.dst.image_width), int(rec.dst.image_height)
    srow, drow = w * c + src_pad, dw * c + dst_pad
    sframe, dframe = srow * h + frame_gap, drow * dh + frame_gap
    src = np.zeros(src_lead + sframe * n, np.uint8)
    for k in range(n):
        for y in range(h):
            o = src_lead + k * sframe + y * srow
            src[o: o + w * c] = frames[k, y].reshape(-1)
    dst = np.full(dframe * n, 0xA5, np.uint8)
    if src_mem == _lib.MEM_DEVICE:
        src_t = torch.from_numpy(src).cuda()
        sp = src_t.data_ptr() + src_lead
    else:
        sp = src.ctypes.data + src_lead
    if dst_mem == _lib.MEM_DEVICE:
        dst_t = torch.from_numpy(dst).cuda()
        dp = dst_t.data_ptr()
    else:
        dp = dst.ctypes.data
    torch.cuda.synchronize()
    ctx.rectify_frames(sp, src_mem, fmt, srow, sframe, n, rec, dp, dst_mem, drow, dframe)
    if dst_mem == _lib.MEM_DEVICE:
        dst = dst_t.cpu().numpy()
    out = np.empty((n, dh, dw, c), np.uint8)
    written = np.zeros(dst.size, bool)
    for k in range(n):
        for y in range(dh):
            o = k * dframe + y * drow
            out[k, y] = dst[o: o + dw * c].reshape(dw, c)
            written[o: o + dw * c] = True
    return out, bool(np.all(dst[~written] == 0xA5))


@pytest.mark.parametrize("fmt", ["L8", "RGB8", "RGBA8"])
def test_strides_and_padding(ctx, fmt):
    """the source 5 bytes into its buffer with row stride = row bytes + 7, the output with row stride = row bytes + 3 and a gap
    between frames: rows that are not dword-aligned, and not one padding byte written"""
    from aruco3_amd import _lib

    f, c = _fmts()[fmt]
    frames = _noise(3, 59, 131, c, 17)
    K = (120.0, 120.0, 65.0, 29.0)
    for new_size, new_K in (((131, 59), K), ((262, 21), (200.0, 200.0, 131.0, 10.0))):
        rec = _rec((131, 59), K, lo.COEFFS["barrel"], new_size, new_K)
        got, clean = _strided_call(ctx, f, frames, rec, _lib.MEM_DEVICE, _lib.MEM_DEVICE)
        assert np.array_equal(got, _want(frames, K, lo.COEFFS["barrel"], new_size, new_K)) and clean
        got, clean = _strided_call(ctx, f, frames, rec, _lib.MEM_DEVICE, _lib.MEM_DEVICE, src_lead=0, src_pad=1, dst_pad=4 - (new_size[0] * c) % 4)
        assert np.array_equal(got, _want(frames, K, lo.COEFFS["barrel"], new_size, new_K)) and clean   # (dword-aligned output rows)


@pytest.mark.parametrize("n", [1, 5, 37])
def test_frame_counts(ctx, n):
    """different noise in every frame: a slip in the frame chunks (16 frames each) or in a frame stride shows"""
    f, c = _fmts()["RGB8"]
    frames = _noise(n, 83, 141, c, 100 + n)
    K = (130.0, 130.0, 70.0, 41.0)
    got, _ = _run(ctx, frames, f, _rec((141, 83), K, lo.COEFFS["rational8"], (141, 83), K))
    want = _want(frames, K, lo.COEFFS["rational8"], (141, 83), K)
    for k in range(n):
        assert np.array_equal(got[k], want[k]), k


def test_memory_kinds(ctx):
    """host / device x host / device, strided on both sides"""
    from aruco3_amd import _lib

    f, c = _fmts()["RGB8"]
    frames = _noise(3, 59, 131, c, 19)
    K = (120.0, 120.0, 65.0, 29.0)
    rec = _rec((131, 59), K, lo.COEFFS["webcam5"], (140, 50), (110.0, 110.0, 70.0, 25.0))
    want = _want(frames, K, lo.COEFFS["webcam5"], (140, 50), (110.0, 110.0, 70.0, 25.0))
    for src_mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
        for dst_mem in (_lib.MEM_HOST, _lib.MEM_DEVICE):
            got, clean = _strided_call(ctx, f, frames, rec, src_mem, dst_mem)
            assert np.array_equal(got, want) and clean, (src_mem, dst_mem)
            got, clean = _strided_call(ctx, f, frames, rec, src_mem, dst_mem, src_lead=0, src_pad=0, dst_pad=0, frame_gap=0)
            assert np.array_equal(got, want) and clean, (src_mem, dst_mem)


def test_deterministic(ctx):
    f, c = _fmts()["RGBA8"]
    frames = _noise(4, SH, SW, c, 23)
    new_K, size, deg = ro.VIEWS["rot5"]
    rec = _rec((SW, SH), ro.SRC_K, lo.COEFFS["webcam5"], size, new_K, ro.rot_y(deg))
    a, _ = _run(ctx, frames, f, rec)
    b, _ = _run(ctx, frames, f, rec)
    assert np.array_equal(a, b)


# ---- Python surface and the chain into the detector ----

def test_python_surface():
    """a CUDA tensor in gives a CUDA tensor out, a numpy array a numpy array, the same bytes; new_intrinsics defaults to the camera
    without its lens"""
    import aruco3_amd
    from aruco3_amd import CameraIntrinsics, Distortion

    torch = _torch()
    frames = _noise(2, 59, 131, 3, 29)
    K = (120.0, 120.0, 65.0, 29.0)
    coeffs = lo.COEFFS["webcam5"]
    ci = CameraIntrinsics(131, 59, *K, distortion=Distortion(*coeffs))
    a = aruco3_amd.rectify_frames(frames, ci, fill=FILL)
    assert isinstance(a, np.ndarray) and np.array_equal(a, _want(frames, K, coeffs, (131, 59), K))
    t = aruco3_amd.rectify_frames(torch.from_numpy(frames).cuda(), ci, fill=FILL)
    assert isinstance(t, torch.Tensor) and t.is_cuda and np.array_equal(t.cpu().numpy(), a)
    new = CameraIntrinsics(140, 50, 110.0, 110.0, 70.0, 25.0)
    R = ro.rot_y(5.0)
    b = aruco3_amd.rectify_frames(frames[0, :, :, 0], ci, new, rotation=R, fill=3)   # (one grey frame, H x W)
    assert b.shape == (1, 50, 140, 1) and np.array_equal(b, ro.rectify(frames[0, :, :, 0], K, coeffs, (110.0, 110.0, 70.0, 25.0), (140, 50), R, 3))
    plain = aruco3_amd.rectify_frames(frames, CameraIntrinsics(131, 59, *K))   # no lens at all
    assert np.array_equal(plain, _want(frames, K, None, (131, 59), K, fill=0))


def test_chain_into_the_detector():
    """the config-1 fixture rectified on the device through the barrel lens and handed, device-resident, straight to a3_detect_batch:
    the markers of the oracle detector on the oracle-rectified frame"""
    from aruco3_amd import ARDictionary, _lib
    from oracle import a3oracle

    torch = _torch()
    w, h = 640, 480
    raw = np.fromfile(ROOT / "tests" / "fixtures" / "inputs" / "c1_640x480_aruco.raw", np.uint8).reshape(1, h, w, 3)
    d = ARDictionary.new_from_named_dict("ARUCO_DEFAULT")
    K, new_K = (700.0, 700.0, 320.0, 240.0), (560.0, 560.0, 320.0, 240.0)
    det = _lib.Context(_lib.default_config(), d.code_list, d.num_bits, d._tau)
    src = torch.from_numpy(raw).cuda()
    dst = torch.empty((1, h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    det.rectify_frames(src.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w * 3, w * h * 3, 1, _rec((w, h), K, lo.COEFFS["barrel"], (w, h), new_K, fill=0),
                       dst.data_ptr(), _lib.MEM_DEVICE, w * 3, w * h * 3)
    m, per = det.detect_batch(dst.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, 1)
    want_frame = ro.rectify(raw, K, lo.COEFFS["barrel"], new_K, fill=0)[0]
    ref = a3oracle.detect(want_frame, d.code_list, d.num_bits, d._tau, keep_debug=False)
    assert len(ref["markers"]) == 4 and int(per[0]) == 4
    assert markers_of_hip(m) == markers_of_oracle(ref)
    assert np.array_equal(dst.cpu().numpy()[0], want_frame)
    det.close()


# ---- argument errors: all refused on the host, nothing is launched ----

def test_argument_errors(ctx):
    from aruco3_amd import _lib

    torch = _torch()
    f, c = _fmts()["RGB8"]
    w, h = 32, 16
    src = torch.zeros((1, h, w, c), dtype=torch.uint8, device="cuda")
    dst = torch.zeros((1, h, w, c), dtype=torch.uint8, device="cuda")
    K = (40.0, 40.0, 16.0, 8.0)
    D = _lib.MEM_DEVICE

    def good():
        return _rec((w, h), K, lo.COEFFS["webcam5"], (w, h), K)

    def call(rec=None, sp=None, dp=None, fmt=f, srow=w * c, sframe=h * w * c, n=1, smem=D, dmem=D, drow=w * c, dframe=h * w * c):
        return ctx.rectify_frames(src.data_ptr() if sp is None else sp, smem, fmt, srow, sframe, n, rec if rec is not None else good(),
                                  dst.data_ptr() if dp is None else dp, dmem, drow, dframe)

    def refused(**kw):
        with pytest.raises(_lib.A3Error) as e:
            call(**kw)
        assert e.value.code == _lib.ERR_INVALID, kw

    call()   # (the arguments every case below departs from are accepted)
    refused(sp=0)
    refused(dp=0)
    with pytest.raises(_lib.A3Error) as e:   # a null a3_rectify
        _lib.check(_lib.load().a3_rectify_frames(ctx.handle, C.c_void_p(src.data_ptr()), D, f, w * c, h * w * c, 1, None, C.c_void_p(dst.data_ptr()), D,
                                                 w * c, h * w * c, None), ctx.handle)
    assert e.value.code == _lib.ERR_INVALID
    refused(n=0)
    refused(n=65536)
    for which in ("src", "dst"):
        for field, value in (("image_width", 0), ("image_height", 0), ("image_width", 65536), ("image_height", 65536)):
            rec = good()
            setattr(getattr(rec, which), field, value)
            refused(rec=rec, srow=1 << 20, sframe=1 << 40, drow=1 << 20, dframe=1 << 40)
        rec = good()
        getattr(rec, which).image_width = getattr(rec, which).image_height = 32768   # 2^30 pixels
        refused(rec=rec, srow=1 << 20, sframe=1 << 40, drow=1 << 20, dframe=1 << 40)
        for field in ("focal_x", "focal_y", "principal_x", "principal_y"):
            for value in (float("nan"), float("inf")):
                rec = good()
                setattr(getattr(rec, which), field, value)
                refused(rec=rec)
        for field in ("focal_x", "focal_y"):
            for value in (0.0, -40.0):
                rec = good()
                setattr(getattr(rec, which), field, value)
                refused(rec=rec)
    refused(srow=w * c - 1)
    refused(drow=w * c - 1)
    refused(srow=w * c + 4)                    # (the frame stride no longer holds h rows)
    refused(sframe=h * w * c - 1)
    refused(dframe=h * w * c - 1)
    refused(fmt=4)
    refused(fmt=-1)
    refused(smem=2)
    refused(dmem=2)
    rec = good()
    rec.distortion.model = 2
    refused(rec=rec)
    for k in range(3):
        rec = good()
        rec.reserved[k] = 1
        refused(rec=rec)
    for field in ("k1", "k2", "p1", "p2", "k3", "k4", "k5", "k6"):
        rec = good()
        setattr(rec.distortion, field, float("nan"))
        refused(rec=rec)
    for k in range(9):
        rec = good()
        rec.rotation[k] = float("inf")
        refused(rec=rec)


def test_not_while_a_batch_is_submitted():
    from aruco3_amd import ARDictionary, _lib

    torch = _torch()
    d = ARDictionary.new_from_named_dict("ARUCO")
    det = _lib.Context(_lib.default_config(), d.code_list, d.num_bits, d._tau)
    w, h = 64, 48
    frames = torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda")
    out = torch.zeros((1, h, w, 3), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    K = (60.0, 60.0, 32.0, 24.0)
    rec = _rec((w, h), K, None, (w, h), K)
    args = (frames.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w * 3, w * h * 3, 1, rec, out.data_ptr(), _lib.MEM_DEVICE, w * 3, w * h * 3)
    det.submit(frames.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, 1)
    with pytest.raises(_lib.A3Error) as e:
        det.rectify_frames(*args)
    assert e.value.code == _lib.ERR_INVALID
    m, _ = det.collect()
    assert len(marker_tuples(m)) == 0
    det.rectify_frames(*args)   # (and once the batch is collected the call goes through)
    det.close()
