"""Every combination of what a batch stages behind its markers (csrc/a3_readback.h): refinement x lens distortion x pose batch or plain
detect x ChArUco, on six rendered 1080p frames of the 5 x 7 board -- some 80 markers and more ChArUco records, both beyond a fresh
context's guess of 64, so the first batch of a context fetches the marker list again and re-reads the records, and the second does not.
Each output must be bit-identical between the two, and bit-identical to the same output of the smallest configuration that produces
it; the getter of a feature that is off refuses with A3_ERR_INVALID; and the all-on batch gives the same through submit / collect on
two contexts sharing a stream, where the read-back is enqueued on the decode stream."""
import itertools

import numpy as np
import pytest

from tests import charuco_util as cu
from tests.test_gpu_charuco import H, INTR, LENS, W, _board, _ctx, _dict, _frames, _torch

pytestmark = pytest.mark.gpu

N_FRAMES = 6
OUTPUTS = ("markers", "per_frame", "poses", "refined", "undist", "undist_res", "board_poses", "charuco", "charuco_poses")
CONFIGS = list(itertools.product((False, True), repeat=4))   # (refine, lens, pose, charuco)


def _context(refine, lens, pose, charuco):
    """a fresh context; the board is set whenever ChArUco or a pose batch is on"""
    from aruco3_amd import _lib

    if pose or charuco:
        ctx = _ctx(_dict(), _board(), refine=refine, charuco=charuco)
    else:
        d = _dict()
        ctx = _lib.Context(cu.config(), d.code_list, d.num_bits, d._tau)
        if refine:
            ctx.set_corner_refinement(_lib.default_refine_config())
    if lens:
        dist = _lib.default_distortion()
        dist.k1, dist.k2 = LENS[0], LENS[1]
        ctx.set_distortion(dist)
    return ctx


def _args(dev):
    from aruco3_amd import _lib

    return (dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, N_FRAMES)


def _getters(ctx):
    return {"refined": ctx.refined_corners, "undist": lambda: ctx.undistorted_corners()[0], "undist_res": lambda: ctx.undistorted_corners()[1],
            "board_poses": ctx.board_poses, "charuco": ctx.charuco_corners, "charuco_poses": ctx.charuco_poses}


def _outputs(ctx, head):
    """every output of the last collected batch as bytes (of the markers: the fields, without the record's 4 padding bytes, which are
    not data); None where the getter refuses, which it must do with A3_ERR_INVALID"""
    from aruco3_amd import _lib

    out = dict(zip(OUTPUTS, head + (None,) * (3 - len(head))))
    out["markers"] = out["markers"].astype(_packed_marker())
    for name, get in _getters(ctx).items():
        try:
            out[name] = get()
        except _lib.A3Error as e:
            assert e.code == _lib.ERR_INVALID, (name, e)
            out[name] = None
    return {k: None if v is None else np.ascontiguousarray(v).view(np.uint8).copy() for k, v in out.items()}


def _packed_marker():
    from aruco3_amd import _lib

    return np.dtype([(name, _lib.MARKER_DTYPE.fields[name][0]) for name in _lib.MARKER_DTYPE.names])


def _run(ctx, dev, pose):
    from aruco3_amd import _lib

    if pose:
        return _outputs(ctx, ctx.detect_batch_pose(*_args(dev), 28.0, _lib.Intrinsics(W, H, *INTR)))
    return _outputs(ctx, ctx.detect_batch(*_args(dev)))


def _same(a, b, what):
    for name in OUTPUTS:
        assert (a[name] is None) == (b[name] is None), (what, name)
        if a[name] is not None:
            assert a[name].shape == b[name].shape and np.array_equal(a[name], b[name]), (what, name)


_RESULTS = {}


def _results():
    """config -> the outputs of the first two batches of a fresh context (short guesses, then guesses that fit), computed once"""
    if not _RESULTS:
        dev, _, _ = _frames(N_FRAMES)
        for cfg in CONFIGS:
            ctx = _context(*cfg)
            _RESULTS[cfg] = (_run(ctx, dev, cfg[2]), _run(ctx, dev, cfg[2]))
    return _RESULTS


def test_both_guesses_are_short_on_a_fresh_context():
    from aruco3_amd import _lib

    all_on = _results()[(True, True, True, True)][0]
    assert len(all_on["markers"]) // _packed_marker().itemsize > 64   # (beyond the guess: the marker list is fetched again)
    assert len(all_on["charuco"]) // _lib.CHARUCO_CORNER_DTYPE.itemsize > 64   # (the rest of the records is re-read)
    assert len(all_on["board_poses"]) // _lib.BOARD_POSE_DTYPE.itemsize == N_FRAMES
    assert len(all_on["charuco_poses"]) // _lib.CHARUCO_POSE_DTYPE.itemsize == N_FRAMES


_IDS = ["".join(n if on else "-" for n, on in zip("RLPC", c)) for c in CONFIGS]


@pytest.mark.parametrize("cfg", CONFIGS, ids=_IDS)
def test_short_guess_equals_a_guess_that_fits(cfg):
    first, second = _results()[cfg]
    _same(first, second, cfg)


@pytest.mark.parametrize("cfg", CONFIGS, ids=_IDS)
def test_outputs_present_and_equal_to_the_smallest_configuration(cfg):
    refine, lens, pose, charuco = cfg
    res = {c: r[1] for c, r in _results().items()}
    got = res[cfg]
    # what is there and what refuses
    present = {"markers": True, "per_frame": True, "poses": pose, "refined": refine, "undist": lens and pose, "undist_res": lens and pose,
               "board_poses": pose, "charuco": charuco, "charuco_poses": charuco and pose}
    assert {k: v is not None for k, v in got.items()} == present
    # the smallest configuration that produces each output; one that depends on refinement or distortion agrees on those
    smallest = {"markers": (False, False, False, False), "per_frame": (False, False, False, False), "refined": (True, False, False, False),
                "poses": (refine, lens, True, False), "undist": (refine, True, True, False), "undist_res": (refine, True, True, False),
                "board_poses": (refine, lens, True, False), "charuco": (refine, lens, False, True), "charuco_poses": (refine, lens, True, True)}
    for name in OUTPUTS:
        if got[name] is not None:
            want = res[smallest[name]][name]
            assert want is not None and got[name].shape == want.shape and np.array_equal(got[name], want), (name, smallest[name])


def test_all_on_through_submit_collect_on_a_shared_stream():
    """two contexts on one stream: the first batch's decode stage and read-back are deferred to the decode stream, behind the second's
    contour stage"""
    from aruco3_amd import _lib

    torch = _torch()
    dev, _, _ = _frames(N_FRAMES)
    cfg = (True, True, True, True)
    want = _results()[cfg][1]
    intr = _lib.Intrinsics(W, H, *INTR)
    s = torch.cuda.Stream()
    ca, cb = _context(*cfg), _context(*cfg)
    for c in (ca, cb, ca, cb):   # (each context's first batches of this shape)
        c.detect_batch_pose(*_args(dev), 28.0, intr)
    ca.set_stream(s.cuda_stream)
    cb.set_stream(s.cuda_stream)
    ca.submit_pose(*_args(dev), 28.0, intr)
    cb.submit_pose(*_args(dev), 28.0, intr)
    got_a = _outputs(ca, ca.collect_pose())
    got_b = _outputs(cb, cb.collect_pose())
    assert ca.stats()["stepping"] == "decode_deferred"
    _same(got_a, want, "deferred read-back")
    _same(got_b, want, "behind a deferred read-back")
