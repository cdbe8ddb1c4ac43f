"""The middle of k_decode -- the Otsu level, the binarisation `> level`, the two-pass f32 triangle resize, `round > 127` -- on the designed
patches of tests/decode_tail_util.py, against the oracle.  tests/test_decode_tail_cases.py has shown on the CPU that the oracle delivers
every designed patch exactly, and counted what the cases reach: thresholds of bit-equal f64 variance in different quarters of 0..255
and in different runs of four, thresholds a few ulps apart, cells of the resize at 126..129 on either side of the cut, shapes from
S = 1 to S = 200 (56 KB of dynamic LDS with a 10-cell dictionary) on both sides of the copy branch.

Every mosaic runs in four arrangements: alone (one frame: at most 64 frames launch k_decode<256, 256>, one threshold per lane, a wave per
quarter) and as frame 0 of a 65-frame batch whose other frames are one flat grey (more than 64 frames launch k_decode<256, 64>, four
thresholds per lane), each with debug taps on and off.  The frame count is the only evidence of the form there is, and it is what
a3_api.hip decides the form by (`few`).  Everything compared is integers and bits: no tolerance anywhere.  GPU only."""
import numpy as np
import pytest

from tests import damage_util as du
from tests import decode_tail_util as tu
from tests.util import marker_tuples, markers_of_hip, markers_of_oracle

pytestmark = pytest.mark.gpu

FORMS = (("k_decode<256, 256>", 1), ("k_decode<256, 64>", 65))


def _where(shape, index, chunk, k):
    c = chunk[k]
    return (f"shape (S, n) = {shape}, mosaic {index}, candidate {k}, tags {sorted(c.tags)}, model's level {c.level}, tied thresholds {list(c.tied)}, "
            f"model's outcome {c.outcome}")


def _assert_patches(patches, ref, shape, index, chunk, what):
    want = ref["homographies"]
    assert patches.shape == want.shape, what
    for k in range(len(want)):
        if not np.array_equal(patches[k], want[k]):
            y, x = np.argwhere(patches[k] != want[k])[0]
            raise AssertionError(f"{what}: patch differs, {int((patches[k] != want[k]).sum())} samples, first at ({x}, {y}): HIP {patches[k][y, x]} "
                                 f"oracle {want[k][y, x]}; {_where(shape, index, chunk, k)}")


def _assert_decoded(ok, dec, codes, ref, shape, index, chunk, what):
    assert ok.tolist() == ref["homography_ok"].tolist(), what
    for k in range(len(chunk)):
        got = (int(dec[k]), tuple(int(v) for v in codes[k]))
        want = (int(ref["decode_ok"][k]), tuple(int(v) for v in ref["codes"][k]))
        if got != want:
            n = shape[1]
            cell = ""
            if got[0] and want[0]:      # the first cell of the unrotated code that differs, row-major over the interior
                idx = (n - 2) ** 2 - (got[1][0] ^ want[1][0]).bit_length()
                cell = f", first differing cell (x, y) = ({1 + idx % (n - 2)}, {1 + idx // (n - 2)})"
            raise AssertionError(f"{what}: decode_ok, codes: HIP {got} oracle {want}{cell}; {_where(shape, index, chunk, k)}")
    assert len(dec) == len(chunk), what


@pytest.mark.parametrize("shape", tu.SHAPES, ids=tu.shape_id)
def test_designed_patches_in_both_forms(oracle, shape):
    """candidates, patches (byte-equal to the oracle's, and so to the design), homography_ok, decode_ok, the four codes and the markers
    with taps on; the marker list and the per-frame counts without taps (the product path); the two forms against one another.
    S = 200 with n = 10 and with n = 6 must launch (the largest dynamic LDS the accepted range asks for) and agree."""
    import torch

    from aruco3_amd import _lib
    from aruco3_amd.aruco import Detector

    S, n = shape
    det = Detector(tu.detector_config(S), du.dictionary(tu.DICT_OF_N[n]))
    ctx = det._context()
    ctx.debug_sample_frames(True)
    made = tu.mosaics(shape)
    H, W = made[0][0].shape
    frames = torch.full((FORMS[1][1], H, W), tu.BACKGROUND, dtype=torch.uint8, device="cuda")
    cap = 4096
    compared = {"mosaics": 0, "candidates": 0, "decode_ok": 0, "markers": 0}
    try:
        for index, (img, quads, chunk) in enumerate(made):
            ref = tu.reference(oracle, shape, index)
            frames[0].copy_(torch.from_numpy(img.copy()))
            torch.cuda.synchronize()
            runs = {}
            for form, count in FORMS:
                args = (frames.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_L8, W, H, W, H * W, count)
                for taps in (True, False):
                    what = f"{form} ({count} frame(s)), taps {'on' if taps else 'off'}, shape {shape}, mosaic {index}"
                    ctx.set_debug_taps(taps)
                    # the injection hook is one-shot, disarmed at the first enqueue, and the first batch of a shape runs twice: the batch
                    # goes through once as it is first
                    ctx.detect_batch(*args, out_cap=cap)
                    ctx.debug_inject_candidates(quads)
                    m, per = ctx.detect_batch(*args, out_cap=cap)
                    assert len(per) == count and not per[1:].any(), what          # the flat frames hold nothing
                    if taps:
                        assert ctx.candidates(0).tolist() == ref["candidates"].tolist() == quads.tolist(), what
                        patches, ok, codes, dec = ctx.homographies(0, with_patches=True)
                        _assert_patches(patches, ref, shape, index, chunk, what)
                        _assert_decoded(ok, dec, codes, ref, shape, index, chunk, what)
                    else:
                        _, ok, codes, dec = ctx.homographies(0, with_patches=False)
                    assert markers_of_hip(m) == markers_of_oracle(ref), what
                    assert [int(r["candidate_index"]) for r in m] == [mk["candidate_index"] for mk in ref["markers"]], what
                    assert per.tolist()[0] == len(ref["markers"]), what
                    runs[(form, taps)] = (marker_tuples(m), int(per[0]), ok.tolist(), codes.tolist(), dec.tolist())
            first = runs[(FORMS[0][0], True)]
            for key, run in runs.items():
                assert run == first, f"shape {shape}, mosaic {index}: {key} differs from {(FORMS[0][0], True)}"
            compared = {"mosaics": index + 1, "candidates": compared["candidates"] + len(first[4]), "decode_ok": compared["decode_ok"] + sum(first[4]),
                        "markers": compared["markers"] + first[1]}
        print(f"{shape}: {compared}, each in {len(FORMS)} forms with taps on and off")
        assert compared["candidates"] == len(tu.cases(shape))
    finally:
        ctx.debug_sample_frames(False)
        ctx.set_debug_taps(False)
        del det, frames
