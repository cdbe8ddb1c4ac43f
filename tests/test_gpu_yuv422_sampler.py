"""The decode stage's frame sampler on packed 4:2:2 frames (bpp 2 in sample_issue, the luma bytes o and o + 2 in pair_from, the byte loads
of grey_tap) against the oracle on the luma plane, patch byte for patch byte: `debug_sample_frames` keeps a tapped batch on the caller's
frames, quads are injected (tests/sampler_util.quad_set).  Layouts as in tests/test_gpu_yuv422_threshold.py, a row stride of 2^24 and
more (64-bit offsets), frames of a few bytes (`tiny`), and every run a second time with the chroma bytes complemented.  GPU only."""
import functools

import numpy as np
import pytest

from tests import sampler_util as su
from tests import yuv422_util as yu
from tests.test_gpu_decode_sampler import _assert_patches, _check_injected, _device_zeros
from tests.util import markers_of_hip, markers_of_oracle

pytestmark = pytest.mark.gpu

W, H = 64, 40
# (offset of the first byte from a 4-byte aligned address, row pad): the 12-byte reads start at the base rounded down (`mis`); an odd pad
# gives the two rows of a sample different shifts; 16-byte aligned base and stride is the threshold stage's FAST layout
LAYOUTS = {"aligned": (0, 0), "base+1": (1, 0), "base+2": (2, 0), "base+3": (3, 0), "rows+5": (0, 5), "base+3,rows+1": (3, 1)}
BIG_STRIDES = ((1 << 24) - 4, 1 << 24, (1 << 24) + 3)   # the last stride with 32-bit offsets, the first with 64, an odd one
TINY = [   # (w, h, quads): 2 x 2 is 4 bytes of luma in 8 (`tiny`: no wide read), 8 x 1 has no bottom tap, 2 x 3 is 12 bytes
    (2, 2, [[(0, 0), (1, 0), (1, 1), (0, 1)], [(0, 0), (21, 0), (21, 21), (0, 21)]]),
    (8, 1, [[(0, 0), (7, 0), (7, 10), (0, 10)], [(2, 0), (6, 0), (6, 20), (2, 20)]]),
    (2, 3, [[(0, 0), (1, 0), (1, 2), (0, 2)], [(0, 0), (21, 0), (21, 22), (0, 22)]]),
]


@pytest.fixture(scope="module")
def sampler_ctx(dicts):
    from aruco3_amd.aruco import Detector, DetectorConfig

    det = Detector(DetectorConfig.default(), dicts.new_from_named_dict(su.DICTIONARY))
    ctx = det._context()
    ctx.debug_sample_frames(True)
    yield ctx
    ctx.debug_sample_frames(False)
    ctx.set_debug_taps(False)
    del det


@functools.lru_cache(maxsize=None)
def _luma(w, h):
    g = su.noise_frames(11, 1, h, w, "L8")[..., 0]
    g.setflags(write=False)
    return g


_REFS = {}


def _reference(oracle, dicts, w, h, quads):
    """the oracle on the luma plane with these quads: once per frame, shared by both formats and every layout, never written to"""
    key = (w, h, quads.tobytes())
    if key not in _REFS:
        d = dicts.new_from_named_dict(su.DICTIONARY)
        _REFS[key] = oracle.detect(_luma(w, h)[0], d.code_list, d.num_bits, d._tau, quads=quads)
    return _REFS[key]


def _both_chromas(fmt, w, h):
    px = yu.interleave(_luma(w, h), fmt, seed=w * h)
    return (("drawn", px), ("complemented", yu.complement_chroma(px, fmt)))


@pytest.mark.parametrize("fmt", yu.FORMATS)
def test_layouts(sampler_ctx, oracle, dicts, fmt):
    import torch

    from aruco3_amd import _lib

    quads = su.quad_set(W, H)
    ref = _reference(oracle, dicts, W, H, quads)
    assert ref["homography_ok"].all() and len(ref["candidates"]) == len(quads)
    reached = np.zeros(3, np.int64)
    for layout, (lead, pad) in LAYOUTS.items():
        reached += su.sample_modes(oracle, quads, W, H, 2, 2 * W + pad)
        for chroma, frame in _both_chromas(fmt, W, H):
            buf, rs, fs = su.lay(frame, lead, pad, 0, seed=lead * 16 + pad)
            keep = torch.from_numpy(buf).cuda()
            assert keep.data_ptr() % 16 == 0
            _check_injected(sampler_ctx, (keep.data_ptr() + lead, _lib.MEM_DEVICE, yu.fmt_value(_lib, fmt), W, H, rs, fs, 1), quads, ref,
                            f"{fmt} {layout} chroma {chroma}")
            del keep
    assert (reached > 0).all(), dict(zip(su.MODE_NAMES, reached.tolist()))   # OUTSIDE, TAIL and WIDE are each reached
    # from host memory (staged with two bytes per pixel)
    frame = np.ascontiguousarray(_both_chromas(fmt, W, H)[0][1])
    _check_injected(sampler_ctx, (frame.ctypes.data, _lib.MEM_HOST, yu.fmt_value(_lib, fmt), W, H, 2 * W, 2 * W * H, 1), quads, ref, f"{fmt} host")


@pytest.mark.parametrize("fmt", yu.FORMATS)
def test_last_of_three_frames_with_a_gap(sampler_ctx, oracle, dicts, fmt):
    """candidates the contour stage finds itself (the injection hook reaches frame 0 only): three frames 7 bytes apart, so each starts at
    another misalignment; the patches and codes of every frame, the last included"""
    import torch

    from aruco3_amd import _lib

    n, w, h = 3, 96, 80
    d = dicts.new_from_named_dict(su.DICTIONARY)
    luma = su.quad_frames(5, n, h, w, "L8")[..., 0]
    ctx = sampler_ctx
    ctx.set_debug_taps(True)
    px = yu.interleave(luma, fmt, seed=5)
    total = 0
    for chroma, frames in (("drawn", px), ("complemented", yu.complement_chroma(px, fmt))):
        buf, rs, fs = su.lay(frames, 1, 3, 7)
        keep = torch.from_numpy(buf).cuda()
        m, per = ctx.detect_batch(keep.data_ptr() + 1, _lib.MEM_DEVICE, yu.fmt_value(_lib, fmt), w, h, rs, fs, n)
        pos = 0
        for f in range(n):
            what = f"{fmt} chroma {chroma} frame {f}"
            ref = oracle.detect(luma[f], d.code_list, d.num_bits, d._tau)
            assert ctx.candidates(f).tolist() == ref["candidates"].tolist(), what
            patches, ok, codes, dec = ctx.homographies(f, with_patches=True)
            _assert_patches(patches, ref, what)
            assert ok.tolist() == ref["homography_ok"].tolist(), what
            assert dec.tolist() == ref["decode_ok"].tolist() and codes.tolist() == ref["codes"].tolist(), what
            assert markers_of_hip(m[pos: pos + int(per[f])]) == markers_of_oracle(ref), what
            pos += int(per[f])
            total += len(patches)
        del keep
    assert total >= 2 * n   # (the frames show quads: something was sampled in every one)
    ctx.set_debug_taps(False)


@pytest.mark.parametrize("case", TINY, ids=lambda c: f"{c[0]}x{c[1]}")
@pytest.mark.parametrize("fmt", yu.FORMATS)
def test_tiny_frames(sampler_ctx, oracle, dicts, fmt, case):
    import torch

    from aruco3_amd import _lib

    w, h, quads = case
    quads = np.asarray(quads, dtype=np.uint32)
    ref = _reference(oracle, dicts, w, h, quads)
    assert ref["homography_ok"].all()
    modes = su.sample_modes(oracle, quads, w, h, 2, 2 * w)
    assert modes[su.WIDE] == 0 and modes[su.OUTSIDE] > 0 and (modes[su.TAIL] > 0) == (h > 1)   # a few bytes: byte loads only
    assert ref["homographies"].any() == (h > 1)
    for lead in (0, 1):
        for chroma, frame in _both_chromas(fmt, w, h):
            buf, rs, fs = su.lay(frame, lead, 0, 0)
            keep = torch.from_numpy(buf).cuda()
            _check_injected(sampler_ctx, (keep.data_ptr() + lead, _lib.MEM_DEVICE, yu.fmt_value(_lib, fmt), w, h, rs, fs, 1), quads, ref,
                            f"{fmt} {w} x {h} lead {lead} chroma {chroma}")
            del keep


def test_row_strides_around_2_pow_24(sampler_ctx, oracle, dicts):
    """row stride 2^24 - 4: the last layout with 32-bit offsets; 2^24 and 2^24 + 3: 64-bit offsets.  64 x 24 pixels: the 0.4 GiB of
    tests/test_gpu_decode_sampler.py's case, one zero-filled buffer for both formats and every stride"""
    import torch

    from aruco3_amd import _lib

    w, h, lead = 64, 24, 1
    quads = su.quad_set(w, h)
    ref = _reference(oracle, dicts, w, h, quads)
    buf = _device_zeros(su.frame_bytes(w, h, 2, max(BIG_STRIDES)) + lead + 16)
    try:
        for fmt in yu.FORMATS:
            for chroma, frame in _both_chromas(fmt, w, h):
                src = torch.from_numpy(np.ascontiguousarray(frame[0].reshape(h, w * 2))).cuda()
                for rs in BIG_STRIDES:
                    assert su.offsets_are_64_bit(w, h, 2, rs) == (rs >= 1 << 24)
                    rows = torch.as_strided(buf, (h, w * 2), (rs, 1), lead)
                    rows.copy_(src)
                    _check_injected(sampler_ctx, (buf.data_ptr() + lead, _lib.MEM_DEVICE, yu.fmt_value(_lib, fmt), w, h, rs, 0, 1), quads, ref,
                                    f"{fmt} row stride {rs} chroma {chroma}")
                    rows.zero_()
    finally:
        del buf
        torch.cuda.empty_cache()
