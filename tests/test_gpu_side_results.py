"""The fixed-size side results of a batch (the table in csrc/a3_readback.h: poses, refined corners, undistorted corners and residuals,
board poses, ChArUco poses, recovered counts) where the other tests of the read-back do not reach, through the public binding only.
Trivial batches -- no frames, or frames of width 0 -- on a context with every feature set: each getter of a kind the call turns on
returns the right number of records (one zero record per frame, or no record per marker), each getter of a kind that is off refuses
with A3_ERR_INVALID.  And recovery among the combinations: frame 1 of tests/recover_scene.py's ChArUco drawing (the one frame that
recovers a marker), repeated until the batch holds more than 64 markers, so that a fresh context's first batch fetches the marker
list again and its second does not: every output of the two is bit-identical, the recovered counts included, and markers, per-frame
counts and recovered counts are those of a context with recovery alone."""
import numpy as np
import pytest

from tests import recover_scene as rs

pytestmark = pytest.mark.gpu

W, H = rs.W, rs.H
INTR = (600.0, 600.0, 320.0, 240.0)
SIZE = 112.0   # the ChArUco drawing's marker side, in board units


def _context(everything=True):
    """a fresh context with the ChArUco board and recovery; `everything`: also ChArUco, refinement and lens distortion"""
    import torch

    from aruco3_amd import _lib

    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    board = rs.charuco_board()
    ctx = _lib.Context(rs.detector_config()._c(), rs.DICT.code_list, rs.DICT.num_bits, rs.DICT._tau)
    ctx.set_board(board.ids, board.corners)
    cfg = ctx.default_recover_config()
    cfg.min_markers, cfg.max_distance_px = 2, 10.0
    ctx.set_board_recovery(cfg)
    if everything:
        ctx.set_charuco(board.chessboard_corners, board.adjacent_ids)
        ctx.set_corner_refinement(_lib.default_refine_config())
        d = _lib.default_distortion()
        d.k1 = -0.05
        ctx.set_distortion(d)
    return ctx


def _args(frames):
    from aruco3_amd import _lib

    n, h, w = frames.shape
    return (frames.ctypes.data, _lib.MEM_HOST, _lib.FMT_L8, w, h, w, h * w, n)


def _getters(ctx, n_frames):
    return {"refined": ctx.refined_corners, "undist": lambda: ctx.undistorted_corners()[0], "undist_res": lambda: ctx.undistorted_corners()[1],
            "board_poses": ctx.board_poses, "charuco": ctx.charuco_corners, "charuco_poses": ctx.charuco_poses,
            "recovered": lambda: ctx.recovered_counts(n_frames)}


def _outputs(ctx, head, n_frames):
    """every output of the last collected batch (of the markers: the fields, without the record's padding bytes, which are not data);
    None where the getter refuses, which it must do with A3_ERR_INVALID"""
    from aruco3_amd import _lib

    out = dict(zip(("markers", "per_frame", "poses"), head + (None,) * (3 - len(head))))
    out["markers"] = out["markers"].astype(np.dtype([(name, _lib.MARKER_DTYPE.fields[name][0]) for name in _lib.MARKER_DTYPE.names]))
    for name, get in _getters(ctx, n_frames).items():
        try:
            out[name] = get()
        except _lib.A3Error as e:
            assert e.code == _lib.ERR_INVALID, (name, e)
            out[name] = None
    return out


PER_MARKER, PER_FRAME = ("refined", "undist", "undist_res", "charuco"), ("board_poses", "charuco_poses", "recovered")
ON_PLAIN = {"refined", "charuco", "recovered"}
ON_POSE = ON_PLAIN | {"undist", "undist_res", "board_poses", "charuco_poses"}


@pytest.mark.parametrize("n_frames, width", [(0, W), (3, 0)], ids=["no_frames", "width_0"])
def test_trivial_batches(n_frames, width):
    from aruco3_amd import _lib

    ctx = _context()
    px = np.zeros(16, np.uint8)   # (never read: there is no pixel)
    args = (px.ctypes.data, _lib.MEM_HOST, _lib.FMT_L8, width, H, width, width * H, n_frames)
    intr = _lib.Intrinsics(W, H, *INTR)

    def submit_collect():
        ctx.submit(*args)
        return ctx.collect()

    def submit_collect_pose():
        ctx.submit_pose(*args, SIZE, intr)
        return ctx.collect_pose()

    calls = [("detect", lambda: ctx.detect_batch(*args), ON_PLAIN), ("pose", lambda: ctx.detect_batch_pose(*args, SIZE, intr), ON_POSE),
             ("submit", submit_collect, ON_PLAIN), ("submit_pose", submit_collect_pose, ON_POSE), ("detect again", lambda: ctx.detect_batch(*args), ON_PLAIN)]
    for what, call, on in calls:
        out = _outputs(ctx, call(), n_frames)
        assert len(out["markers"]) == 0 and out["per_frame"].tolist() == [0] * n_frames, what
        if out["poses"] is not None:
            assert len(out["poses"]) == 0, what
        for name in PER_MARKER + PER_FRAME:
            assert (out[name] is not None) == (name in on), (what, name)
            if name in on:
                assert len(out[name]) == (n_frames if name in PER_FRAME else 0), (what, name)
                assert not np.ascontiguousarray(out[name]).view(np.uint8).any(), (what, name)   # zero records
    ctx.close()


def test_recovery_among_all_features_short_guess_and_guess_that_fits():
    from aruco3_amd import _lib

    frame = rs.charuco_frames()[1:2]
    alone = _context(everything=False)
    one, _ = alone.detect_batch(*_args(frame))
    rec_one = int(alone.recovered_counts(1)[0])
    assert rec_one >= 1 and 0 < len(one) <= 64
    n = 64 // len(one) + 1   # just enough frames for more than 64 markers: beyond a fresh context's guess
    frames = np.ascontiguousarray(np.repeat(frame, n, axis=0))
    intr = _lib.Intrinsics(W, H, *INTR)
    ctx = _context()
    first = _outputs(ctx, ctx.detect_batch_pose(*_args(frames), SIZE, intr), n)    # the marker list is fetched again
    second = _outputs(ctx, ctx.detect_batch_pose(*_args(frames), SIZE, intr), n)   # the guess fits
    assert len(first["markers"]) == n * len(one) > 64
    assert first["recovered"].tolist() == [rec_one] * n
    for name in first:
        a, b = first[name], second[name]
        assert a is not None and b is not None and a.shape == b.shape and a.tobytes() == b.tobytes(), name
    for name in PER_MARKER[:3] + ("poses",):
        assert len(first[name]) == len(first["markers"]), name
    for name in PER_FRAME:
        assert len(first[name]) == n, name
    want = _outputs(alone, alone.detect_batch(*_args(frames)), n)
    for name in ("markers", "per_frame", "recovered"):
        assert want[name].shape == first[name].shape and want[name].tobytes() == first[name].tobytes(), name
    ctx.close(); alone.close()
