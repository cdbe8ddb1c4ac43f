"""The cases of tests/sampler_util.py, checked where no GPU is needed: every group tests/test_gpu_decode_sampler.py runs reaches the
sampler cases it claims (counted per sample with the f32 operations of the warp), the oracle reads a strided or offset buffer as it
reads the packed copy, and it handles the tiny frames."""
import numpy as np
import pytest

from tests import sampler_util as su


def _dictionary(dicts):
    return dicts.new_from_named_dict(su.DICTIONARY)


def _detect(oracle, dicts, img, quads=None):
    d = _dictionary(dicts)
    return oracle.detect(img, d.code_list, d.num_bits, d._tau, quads=quads)


@pytest.mark.parametrize("w,h", [su.A_SIZE, (64, 24), (64, 512), (64, 513)])
def test_quad_set_survives_discard_too_near(oracle, dicts, w, h):
    """the quads are what is sampled: none is dropped for standing too near another, all have a projection"""
    quads = su.quad_set(w, h)
    r = _detect(oracle, dicts, su.for_oracle(su.noise_frames(3, 1, h, w, "L8")[0], "L8"), quads)
    assert r["candidates"].tolist() == quads.tolist() and r["homography_ok"].all()
    assert int(quads[..., 0].max()) == w + 20 and int(quads[..., 1].max()) == h + 20 and int(quads.min()) == 0
    assert {(0, 0), (w - 1, 0), (w - 1, h - 1), (0, h - 1)} <= {tuple(p) for p in quads.reshape(-1, 2).tolist()}


@pytest.mark.parametrize("fmt", su.A_FORMATS)
def test_group_a_reaches_every_case(oracle, fmt):
    w, h = su.A_SIZE
    for pad in su.A_PADS:
        counts = su.sample_modes(oracle, su.quad_set(w, h), w, h, su.BPP[fmt], w * su.BPP[fmt] + pad)
        assert (counts > 0).all() and counts.sum() == 15 * su.S * su.S, (fmt, pad, counts)
        assert not su.offsets_are_64_bit(w, h, su.BPP[fmt], w * su.BPP[fmt] + pad)


@pytest.mark.parametrize("case", su.FOUND_CASES, ids=lambda c: f"{c[0]}x{c[1]}x{c[2]}")
@pytest.mark.parametrize("fmt", su.FOUND_FORMATS)
def test_group_b_frames_hold_candidates_that_decode(oracle, dicts, fmt, case):
    """the contour stage finds a quad in (nearly) every frame, its taps are wide reads, and most patches pass the border test: their four
    codes are a second witness of what was sampled, in the run without taps as well"""
    n, w, h, lead, pad, gap = case
    frames = su.quad_frames(5, n, h, w, fmt)
    counts = np.zeros(3, dtype=np.int64)
    with_cand = decoded = 0
    for f in range(n):
        r = _detect(oracle, dicts, su.for_oracle(frames[f], fmt))
        with_cand += len(r["candidates"]) > 0 and bool(r["homography_ok"].all())
        decoded += int(r["decode_ok"].sum()) > 0
        counts += su.sample_modes(oracle, r["candidates"], w, h, su.BPP[fmt], w * su.BPP[fmt] + pad)
    assert counts[su.WIDE] > 0 and with_cand >= n - n // 10 and decoded >= n // 2, (counts, with_cand, decoded)
    # the frames' first bytes fall on every misalignment
    assert {(lead + f * (h * (w * su.BPP[fmt] + pad) + gap)) % 4 for f in range(n)} == {0, 1, 2, 3}


@pytest.mark.parametrize("case", su.TINY_CASES, ids=lambda c: f"{c[0]}-{c[1]}x{c[2]}")
def test_group_c_tiny_frames(oracle, dicts, case):
    fmt, w, h, quads, modes = case
    quads = np.asarray(quads, dtype=np.uint32)
    frame = su.noise_frames(3, 1, h, w, fmt)[0]
    r = _detect(oracle, dicts, su.for_oracle(frame, fmt), quads)
    assert r["candidates"].tolist() == quads.tolist() and r["homography_ok"].all()
    counts = su.sample_modes(oracle, quads, w, h, su.BPP[fmt], w * su.BPP[fmt])
    assert [m for m in range(3) if counts[m] > 0] == list(modes), counts
    assert r["homographies"].any() == (su.TAIL in modes or su.WIDE in modes)      # nothing inside: all zero


def test_group_d_reaches_every_case_in_both_offset_widths(oracle):
    wide64 = []
    for fmt, w, h, rs in su.D_STRIDE_CASES + su.D_HEIGHT_CASES:
        counts = su.sample_modes(oracle, su.quad_set(w, h), w, h, su.BPP[fmt], rs)
        assert (counts > 0).all(), (fmt, w, h, rs, counts)
        wide64.append(su.offsets_are_64_bit(w, h, su.BPP[fmt], rs))
    assert wide64 == [False, True, True, True] * 2 + [False, True]
    # the last 32-bit layouts lie right at the edge: one more row stride, or one more row, and the offsets need 64 bits
    assert su.frame_bytes(64, 512, 1, 1 << 23) == (1 << 32) - (1 << 23) + 64 and su.frame_bytes(64, 513, 1, 1 << 23) == (1 << 32) + 64


@pytest.mark.parametrize("fmt", su.A_FORMATS)
def test_oracle_reads_a_laid_out_frame_as_the_packed_copy(oracle, dicts, fmt):
    w, h = su.A_SIZE
    frames = su.noise_frames(11, 2, h, w, fmt)
    quads = su.quad_set(w, h)
    want = [_detect(oracle, dicts, su.for_oracle(np.ascontiguousarray(frames[f]), fmt), quads) for f in range(2)]
    for lead, pad, gap in ((0, 0, 0), (1, 0, 0), (2, 1, 13), (3, 13, 7), (0, 3, 1)):
        buf, rs, fs = su.lay(frames, lead, pad, gap)
        view = su.laid(buf, lead, rs, fs, 2, h, w, su.BPP[fmt])
        for f in range(2):
            img = view[f, :, :, 0] if fmt == "L8" else view[f]
            if fmt != "BGRA8":      # (BGRA8 goes through a channel swap, i.e. a copy; the others are read where they lie)
                assert oracle._u8_rows(img) is img and (pad == 0 or not img.flags["C_CONTIGUOUS"])
            got = _detect(oracle, dicts, su.for_oracle(view[f], fmt), quads)
            assert np.array_equal(got["grey"], want[f]["grey"]) and np.array_equal(got["homographies"], want[f]["homographies"])
            assert got["codes"].tolist() == want[f]["codes"].tolist() and got["markers"] == want[f]["markers"]
