"""a3_debug_kernel_time: the probe that re-runs one kernel of the last batch -- k_dart_count, k_dart_assign, k_local_contract,
k_decode warm and on cold frames -- through launches it builds itself, beside the product path's.  Only bench.py and
tools/kernel_probe.py call it, with the (kernel, dbg) pairs below, in the tool's order: decode first (it only reads what the batch
left behind), the contract before the assign variants, the whole k_dart_assign (5, which relinks) last.  Every pair returns a
finite, non-negative time; the batch that follows overwrites what the probe left in the contour graph and finds exactly the
markers of the batch before; a kernel index the probe does not know and a context without a batch are refused.  GPU only."""
import math

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

DECODE, DECODE_COLD, LOCAL_CONTRACT, DART_COUNT, DART_ASSIGN = 3, 4, 2, 0, 1
PAIRS = ([(DECODE, m) for m in (0, -1, -2, -3, -4, -5)]        # tools/kernel_probe.py
         + [(DECODE_COLD, -5), (DECODE_COLD, -2)]              # bench.py's roofline_warp
         + [(LOCAL_CONTRACT, m) for m in (-1, 1, 2, 4, 6, 8, 11)]
         + [(DART_COUNT, 0)]
         + [(DART_ASSIGN, m) for m in (1, 2, 3, 4, 5)])


def _detector(dicts):
    from aruco3_amd.aruco import Detector, DetectorConfig

    return Detector(DetectorConfig(), dicts.new_from_named_dict("ARUCO_DEFAULT"))


@pytest.fixture(scope="module")
def scene():
    """four 640 x 480 frames of four markers each, on the device, and their truth: a batch of one chunk"""
    import torch

    from aruco3_amd import synth

    frames, truth = synth.config_frames(1, 4)
    return torch.from_numpy(frames).to("cuda:0"), truth


def test_probe_times_every_pair_and_leaves_the_next_batch_alone(dicts, scene):
    dev, truth = scene
    det = _detector(dicts)
    markers, per = det.detect_batch_raw(dev)
    assert per.tolist() == [len(t) for t in truth]
    ctx = det._context()
    assert ctx.stats()["chunks"] == 1
    for kernel, dbg in PAIRS:
        ms = ctx.debug_kernel_time(kernel, dbg, reps=1)
        print(f"kernel {kernel} dbg {dbg:3d}: {ms * 1e3:8.1f} us")
        assert math.isfinite(ms) and ms >= 0.0, (kernel, dbg, ms)
    again, per_again = det.detect_batch_raw(dev)
    assert np.array_equal(per_again, per)
    assert np.array_equal(again, markers)


def test_probe_refuses_an_unknown_kernel(dicts, scene):
    from aruco3_amd import _lib

    det = _detector(dicts)
    det.detect_batch_raw(scene[0])
    with pytest.raises(_lib.A3Error) as e:
        det._context().debug_kernel_time(5, 0, reps=1)
    assert e.value.code == _lib.ERR_INVALID


def test_probe_refuses_a_context_without_a_batch(dicts):
    from aruco3_amd import _lib

    with pytest.raises(_lib.A3Error) as e:
        _detector(dicts)._context().debug_kernel_time(DECODE, 0, reps=1)
    assert e.value.code == _lib.ERR_INVALID
