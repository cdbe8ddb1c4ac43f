"""The decode stage's frame sampler -- what every shipped detection runs on the caller's pixel format, strides and alignment -- against
the oracle, patch byte for patch byte.  Debug taps alone switch the decode stage to the packed grey plane; `debug_sample_frames` keeps a
tapped batch on the caller's frames, so the patches compared here are those of sample_issue / sample_finish / pair_from / luma_px on every
format, base misalignment and row stride, on frames beyond frame 0, on frames smaller than one wide read, and with both offset widths.
The cases and the sampler cases they reach are tests/sampler_util.py's (counted in tests/test_sampler_cases.py).  GPU only."""
import functools

import numpy as np
import pytest

from tests import sampler_util as su
from tests.util import marker_tuples, markers_of_hip, markers_of_oracle

pytestmark = pytest.mark.gpu


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


def _fmt(name):
    from aruco3_amd import _lib

    return {"L8": _lib.FMT_L8, "RGB8": _lib.FMT_RGB8, "RGBA8": _lib.FMT_RGBA8, "BGRA8": _lib.FMT_BGRA8}[name]


@functools.lru_cache(maxsize=None)
def _frame(fmt, w, h):
    f = su.noise_frames(7, 1, h, w, fmt)
    f.setflags(write=False)
    return f


_REFS = {}


def _reference(oracle, dicts, fmt, w, h, quads):
    """the oracle on the packed frame with these quads: computed once per frame, shared by every layout of it, never written to"""
    key = (fmt, w, h, quads.tobytes())
    if key not in _REFS:
        d = dicts.new_from_named_dict(su.DICTIONARY)
        _REFS[key] = oracle.detect(su.for_oracle(_frame(fmt, w, h)[0], fmt), d.code_list, d.num_bits, d._tau, quads=quads)
    return _REFS[key]


def _assert_patches(patches, ref, what):
    if not np.array_equal(patches, ref["homographies"]):
        bad = [(k, int((patches[k] != ref["homographies"][k]).sum())) for k in range(len(patches)) if not np.array_equal(patches[k], ref["homographies"][k])]
        k = bad[0][0]
        y, x = np.argwhere(patches[k] != ref["homographies"][k])[0]
        raise AssertionError(f"{what}: patches differ, (candidate, pixels) {bad}; first at candidate {k} ({x}, {y}): "
                             f"HIP {patches[k][y, x]} oracle {ref['homographies'][k][y, x]}")


def _check_injected(ctx, args, quads, ref, what):
    """frame 0 with `quads` injected: the tapped batch (sampling the frames: the hook) equals the oracle in every decode-stage output, the
    batch without taps equals the tapped one in all it keeps"""
    got = {}
    for taps in (True, False):
        ctx.set_debug_taps(taps)
        # the injection hook is one-shot, disarmed at the first enqueue, and the first batch of a shape runs twice: the frame goes through
        # once as it is first
        ctx.detect_batch(*args)
        ctx.debug_inject_candidates(quads)
        m, per = ctx.detect_batch(*args)
        cand = ctx.candidates(0)
        patches, ok, codes, dec = ctx.homographies(0, with_patches=taps)
        got[taps] = (marker_tuples(m), per.tolist(), cand.tolist(), ok.tolist(), codes.tolist(), dec.tolist())
        if taps:
            assert cand.tolist() == ref["candidates"].tolist(), what
            _assert_patches(patches, ref, what)
            assert ok.tolist() == ref["homography_ok"].tolist(), what
            assert dec.tolist() == ref["decode_ok"].tolist() and codes.tolist() == ref["codes"].tolist(), what
            assert markers_of_hip(m) == markers_of_oracle(ref), what
    assert got[True] == got[False], what + ": taps on and off differ"


# ------------------------------------------------------------------------------------------------------------------
# a: formats x alignment x stride
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fmt,host", [(f, False) for f in su.A_FORMATS] + [("RGB8", True), ("L8", True)])
def test_formats_alignments_strides(sampler_ctx, oracle, dicts, fmt, host):
    """one 61 x 47 noise frame at base offsets 0..3 (the 12-byte reads start at the base rounded down: `mis`) with row pads 0, 1, 2, 3, 13
    (row_stride % 4 != 0: the two rows of a sample need different shifts), every quad of quad_set"""
    import torch

    from aruco3_amd import _lib

    w, h = su.A_SIZE
    frame, quads = _frame(fmt, w, h), su.quad_set(w, h)
    ref = _reference(oracle, dicts, fmt, w, h, quads)
    assert ref["homography_ok"].all() and len(ref["candidates"]) == len(quads)
    for lead in su.A_LEADS:
        for pad in su.A_PADS:
            buf, rs, fs = su.lay(frame, lead, pad, 0, seed=lead * 16 + pad)
            if host:
                keep, ptr, mem = buf, buf.ctypes.data + lead, _lib.MEM_HOST
            else:
                keep = torch.from_numpy(buf).cuda()
                ptr, mem = keep.data_ptr() + lead, _lib.MEM_DEVICE
                assert keep.data_ptr() % 4 == 0
            _check_injected(sampler_ctx, (ptr, mem, _fmt(fmt), w, h, rs, fs, 1), quads, ref,
                            f"{fmt} {'host' if host else 'device'} lead {lead} row pad {pad}")
            del keep


# ------------------------------------------------------------------------------------------------------------------
# b: frames beyond 0 (found candidates), both instantiations of k_decode
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", su.FOUND_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
@pytest.mark.parametrize("fmt", su.FOUND_FORMATS)
def test_every_frame_of_a_batch(sampler_ctx, oracle, dicts, fmt, case):
    """the frame gap is odd, so every frame of the batch starts at another misalignment; patches and codes of every frame"""
    import torch

    from aruco3_amd import _lib

    n, w, h, lead, pad, gap = case
    d = dicts.new_from_named_dict(su.DICTIONARY)
    frames = su.quad_frames(5, n, h, w, fmt)
    buf, rs, fs = su.lay(frames, lead, pad, gap)
    keep = torch.from_numpy(buf).cuda()
    args = (keep.data_ptr() + lead, _lib.MEM_DEVICE, _fmt(fmt), w, h, rs, fs, n)
    ctx = sampler_ctx
    ctx.set_debug_taps(True)
    m1, per1 = ctx.detect_batch(*args, out_cap=64 * n)
    tapped, pos, total = [], 0, 0
    for f in range(n):
        what = f"{fmt} {n} x {w} x {h}, frame {f}"
        ref = oracle.detect(su.for_oracle(frames[f], fmt), d.code_list, d.num_bits, d._tau)
        assert ctx.candidates(f).tolist() == ref["candidates"].tolist(), what
        patches, ok, codes, dec = ctx.homographies(f, with_patches=True)
        _assert_patches(patches, ref, what)
        assert ok.tolist() == ref["homography_ok"].tolist(), what
        assert dec.tolist() == ref["decode_ok"].tolist() and codes.tolist() == ref["codes"].tolist(), what
        assert markers_of_hip(m1[pos: pos + int(per1[f])]) == markers_of_oracle(ref), what
        pos += int(per1[f])
        total += len(patches)
        tapped.append((ok.tolist(), codes.tolist(), dec.tolist()))
    assert pos == len(m1) and total >= n - n // 10
    ctx.set_debug_taps(False)
    m0, per0 = ctx.detect_batch(*args, out_cap=64 * n)
    assert marker_tuples(m0) == marker_tuples(m1) and per0.tolist() == per1.tolist()
    for f in range(n):
        _, ok, codes, dec = ctx.homographies(f, with_patches=False)
        assert (ok.tolist(), codes.tolist(), dec.tolist()) == tapped[f], f"{fmt} {n} x {w} x {h}, frame {f}: taps on and off differ"
    del keep


# ------------------------------------------------------------------------------------------------------------------
# c: tiny frames
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", su.TINY_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_tiny_frames(sampler_ctx, oracle, dicts, case):
    """frames below 16 bytes read a stand-in base and take byte loads only (`tiny`), 16 bytes hold exactly one wide offset, a single row or
    column holds no sample at all"""
    import torch

    from aruco3_amd import _lib

    fmt, w, h, quads, modes = case
    quads = np.asarray(quads, dtype=np.uint32)
    frame = _frame(fmt, w, h)
    ref = _reference(oracle, dicts, fmt, w, h, quads)
    assert ref["homography_ok"].all() and ref["homographies"].any() == (modes != (su.OUTSIDE,))
    for lead in (0, 1):
        buf, rs, fs = su.lay(frame, lead, 0, 0)
        keep = torch.from_numpy(buf).cuda()
        _check_injected(sampler_ctx, (keep.data_ptr() + lead, _lib.MEM_DEVICE, _fmt(fmt), w, h, rs, fs, 1), quads, ref,
                        f"{fmt} {w} x {h} lead {lead}")
        del keep


# ------------------------------------------------------------------------------------------------------------------
# d: offset widths
# ------------------------------------------------------------------------------------------------------------------
def _device_zeros(nbytes):
    import torch

    try:
        return torch.zeros(nbytes, dtype=torch.uint8, device="cuda")
    except (torch.cuda.OutOfMemoryError, RuntimeError) as e:
        if "out of memory" not in str(e).lower():
            raise
        pytest.skip(f"{nbytes} bytes of device memory cannot be allocated: {e}")


def _check_strided_cases(ctx, oracle, dicts, cases, lead):
    """every case's rows written through a strided view into ONE zero-filled device buffer (and zeroed again afterwards)"""
    import torch

    from aruco3_amd import _lib

    nbytes = max(su.frame_bytes(w, h, su.BPP[fmt], rs) for fmt, w, h, rs in cases) + lead + 16
    buf = _device_zeros(nbytes)
    try:
        for fmt, w, h, rs in cases:
            bpp = su.BPP[fmt]
            quads = su.quad_set(w, h)
            ref = _reference(oracle, dicts, fmt, w, h, quads)
            rows = torch.as_strided(buf, (h, w * bpp), (rs, 1), lead)
            rows.copy_(torch.from_numpy(_frame(fmt, w, h)[0].reshape(h, w * bpp).copy()).cuda())
            wide = su.offsets_are_64_bit(w, h, bpp, rs)
            _check_injected(ctx, (buf.data_ptr() + lead, _lib.MEM_DEVICE, _fmt(fmt), w, h, rs, 0, 1), quads, ref,
                            f"{fmt} {w} x {h} row stride {rs} ({64 if wide else 32}-bit offsets)")
            rows.zero_()
    finally:
        del buf
        torch.cuda.empty_cache()


def test_row_strides_around_2_pow_24(sampler_ctx, oracle, dicts):
    """row stride 2^24 - 4: the last layout with 32-bit offsets (24-bit multiplies); 2^24, 2^24 + 1, 2^24 + 3: 64-bit offsets, the latter
    two with another shift in every row.  0.4 GiB."""
    _check_strided_cases(sampler_ctx, oracle, dicts, su.D_STRIDE_CASES, lead=1)


def test_frames_around_4_gib(sampler_ctx, oracle, dicts):
    """row stride 2^23: 512 rows end below 2^32 (32-bit offsets up to 2^32 - 2^23), 513 rows make frame_bytes 2^32 + 64 (64-bit offsets by the
    frame's size, not by the stride).  4.3 GiB."""
    _check_strided_cases(sampler_ctx, oracle, dicts, su.D_HEIGHT_CASES, lead=2)
