"""Every launch path of the threshold stage against tests/threshold_util.py's numpy reference, bit for bit, through detect_batch:
radii 1..7 (the register-resident kernel: every ring size, column strips, row strips in both directions, frames lower than the
window, every pixel format, aligned and unaligned layouts, the parked rows' flush), 8..31 (the ring kernel, its flush too), 32..128 (separable),
above 128 (brute force) -- on contents that sit on the comparison's boundary.  The batches come from threshold_util's table, which
tests/test_threshold_reference.py holds against the CPU oracle and shows to discriminate.  GPU only."""
import numpy as np
import pytest

from tests import threshold_util as tu

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def hip():
    from aruco3_amd import _lib

    _lib.load()
    return _lib


def _context(dicts, radius):
    from aruco3_amd.aruco import Detector, DetectorConfig

    det = Detector(DetectorConfig(threshold_window=radius), dicts.new_from_named_dict("ARUCO"))
    return det, det._context()


def _fmt(hip, name):
    return {"RGB8": hip.FMT_RGB8, "RGBA8": hip.FMT_RGBA8, "BGRA8": hip.FMT_BGRA8, "L8": hip.FMT_L8}[name]


def _oracle_luma(oracle, px, fmt):
    return oracle.to_luma8(px[..., 0] if fmt == "L8" else (px[..., [2, 1, 0, 3]] if fmt == "BGRA8" else px))


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} px differ, first (y, x) {bad[:5].tolist()}"


def _compare(hip, ctx, case, names, want, taps, want_grey=None):
    """the last batch's planes against the reference; without taps a kernel that writes no grey plane (radii 1..31) must refuse to
    hand one out"""
    for f, name in enumerate(names):
        what = f"{case.id} {name} frame {f} taps {taps}"
        _same(ctx.download_grey(f, case.w, case.h, thresholded=True), want[f], what)
        if taps or case.radius > 31:
            if want_grey is not None:
                _same(ctx.download_grey(f, case.w, case.h), want_grey[f], what + " grey")
    if not taps and case.radius <= 31:
        with pytest.raises(hip.A3Error):
            ctx.download_grey(0, case.w, case.h)


def _check_case(hip, ctx, oracle, case, tapped=True):
    """one batch from packed host memory, with debug taps (grey plane against into_luma8) and without"""
    names, px, grey = case.frames()
    n, h, w, c = px.shape
    want = tu.reference(grey, case.radius)[0]
    want_grey = [_oracle_luma(oracle, px[f], case.fmt) for f in range(n)]
    for taps in ((True, False) if tapped else (False,)):
        ctx.set_debug_taps(taps)
        ctx.detect_batch(px.ctypes.data, hip.MEM_HOST, _fmt(hip, case.fmt), w, h, w * c, h * w * c, n)
        _compare(hip, ctx, case, names, want, taps, want_grey)


# ---- a. radii 1..7: shapes x formats x contents ----------------------------------------------------------------------------
@pytest.mark.parametrize("radius", tu.K1_RADII)
def test_k1_shapes_formats_contents(hip, dicts, oracle, radius):
    """k_grey_threshold7<FMT, FAST, R> for every R: heights 1 .. 2R+2, 33 and 100 (six strips of 17 rows, down and up; the FAST loop
    overruns each into clamped rows), widths 1 .. 1985 (one, two and three column strips, W % 16 == 0 and not), RGB8 everywhere and all
    four formats at widths 1008 and 1009; noise, ramp, all255, all0, knife(0), knife(253), impulses, stripes as one batch per shape."""
    det, ctx = _context(dicts, radius)
    for case in tu.k1_cases(radius):
        _check_case(hip, ctx, oracle, case)


# ---- b. radii 1..7: layouts ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", tu.K1_RADII)
def test_k1_layouts(hip, dicts, oracle, radius):
    """100 x 1008 and 100 x 1009 packed (FAST where W % 16 == 0), with rows padded by 32 bytes (aligned: still FAST), with rows padded by 20
    bytes behind a base pointer offset by 3 (per-pixel loads) and with a frame stride that is no multiple of 16; from host memory and
    from a device tensor, whose alignment is the one the kernel sees."""
    import torch

    det, ctx = _context(dicts, radius)
    for case in tu.layout_cases(radius):
        names, px, grey = case.frames()
        n, h, w, c = px.shape
        want = tu.reference(grey, radius)[0]
        want_grey = [_oracle_luma(oracle, px[f], case.fmt) for f in range(n)]
        for layout, (row_pad, frame_pad, off) in tu.LAYOUTS.items():
            row_stride = w * c + row_pad
            frame_stride = row_stride * h + frame_pad
            raw = np.zeros(n * frame_stride + off + 16, np.uint8)
            start = (-raw.ctypes.data) % 16 + off          # the first pixel sits `off` bytes behind a 16-byte boundary
            for f in range(n):
                rows = raw[start + f * frame_stride: start + f * frame_stride + h * row_stride].reshape(h, row_stride)
                rows[:, : w * c] = px[f].reshape(h, w * c)
            dev = torch.from_numpy(raw[start - off:]).cuda()
            assert dev.data_ptr() % 16 == 0
            for mem, ptr in ((hip.MEM_HOST, raw.ctypes.data + start), (hip.MEM_DEVICE, dev.data_ptr() + off)):
                for taps in (True, False):
                    ctx.set_debug_taps(taps)
                    ctx.detect_batch(ptr, mem, _fmt(hip, case.fmt), w, h, row_stride, frame_stride, n)
                    case_l = tu.Case(f"{case.path}[{layout},{'device' if mem == hip.MEM_DEVICE else 'host'}]", radius, h, w, case.fmt, {})
                    _compare(hip, ctx, case_l, names, want, taps, want_grey)


# ---- c. radii 1..7: the parked rows' flush ---------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", ["2048x16x300", "1024x16x260"])
@pytest.mark.parametrize("radius", tu.K1_RADII)
def test_k1_parked_rows_flush(hip, dicts, oracle, radius, shape):
    """strips taller than the 128 rows a wave parks in LDS: 2048 frames of 16 x 300 (one strip: two bursts and a remainder) and 1024 of
    16 x 260 (two strips of 130 rows, the second walking upwards: a burst and a remainder of 2); every frame is compared"""
    det, ctx = _context(dicts, radius)
    case = tu.flush_cases(radius)[0 if shape == "2048x16x300" else 1]
    assert shape == f"{len(case.contents)}x{case.w}x{case.h}"
    _check_case(hip, ctx, oracle, case)


# ---- d. radii 8..31 on the comparison's boundary ---------------------------------------------------------------------------
@pytest.mark.parametrize("radius", tu.RING_RADII)
def test_ring_kernel_boundary_contents(hip, dicts, oracle, radius):
    """k_grey_threshold_ring with one (8, 15) and two (16, 19, 27, 31) apron lanes -- 19: the first radius with 19 rows of ring in LDS and
    a longer register part, 27: RGB8 with vector loads back at R | R + 1 and one wave per SIMD --: knife(0), knife(253), all255, all0,
    stripes on 40 x 1009 (per-pixel loads) and 129 x 1040 (vector loads, two column strips)"""
    det, ctx = _context(dicts, radius)
    for case in tu.ring_cases(radius):
        _check_case(hip, ctx, oracle, case)


@pytest.mark.parametrize("radius,shape", [(8, "2048x16x300"), (8, "1024x16x260"), (31, "1024x16x200"), (31, "512x16x260")])
def test_ring_parked_rows_flush(hip, dicts, oracle, radius, shape):
    """k_grey_threshold_ring with strips taller than the rows a wave parks in LDS (84 at radius 8, 60 at 31): one strip per frame, and
    two strips of 130 rows of which the second walks upwards (tests/test_threshold_plan.py holds the strips against the planner);
    every frame is compared"""
    det, ctx = _context(dicts, radius)
    case = {f"{len(c.contents)}x{c.w}x{c.h}": c for c in tu.ring_flush_cases(radius)}[shape]
    _check_case(hip, ctx, oracle, case)


# ---- e. the separable and the brute-force path -----------------------------------------------------------------------------
@pytest.mark.parametrize("radius", tu.SEPARABLE_RADII)
def test_separable_path(hip, dicts, oracle, radius):
    """k_grey_generic + k_hsum_generic + k_vsum_threshold_generic: byte and dword loads, two workgroups per row with the apron across
    column 1024, two row strips with H no multiple of 8, row sums of exactly 65535 (all255 at radius 128, W >= 257), tiny frames"""
    det, ctx = _context(dicts, radius)
    for case in tu.separable_cases(radius):
        _check_case(hip, ctx, oracle, case)


@pytest.mark.parametrize("radius", tu.BRUTE_RADII)
def test_brute_force_path(hip, dicts, oracle, radius):
    """k_grey_generic + k_threshold_generic up to the largest radius a3_create accepts (every expression with the radius in the kernel
    compares it plainly or adds it in 64 bits); small frames, the work per pixel being the clipped window's area"""
    det, ctx = _context(dicts, radius)
    for case in tu.brute_cases(radius):
        _check_case(hip, ctx, oracle, case)


# ---- f. refusal --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("radius", [2**31, 2**32 - 1])
def test_radius_beyond_int32_is_refused(hip, dicts, radius):
    """the kernels take the radius as a signed int: a3_create refuses what would turn negative, before anything is launched"""
    from aruco3_amd.aruco import Detector, DetectorConfig

    with pytest.raises(hip.A3Error) as e:
        Detector(DetectorConfig(threshold_window=radius), dicts.new_from_named_dict("ARUCO"))._context()
    assert e.value.code == hip.ERR_INVALID
    assert "threshold_window" in str(e.value)
