"""Board-aided marker recovery on the MI355X (k_recover_frames / k_recover_merge; a3_set_board_recovery / a3_recover_markers): the
stand-alone call equal to the CPU restatement (tests/recover_oracle.c) on every designed list of tests/recover_cases.py and on one list
beyond the sizes LDS holds; the merged list of a batch -- out, per_frame_count, the recovered counts -- equal to what the contract
makes of the CPU oracle's detection of the same frames, through every call and scheduling path; what follows the list (board pose,
refinement, undistortion, ChArUco) follows the merged one; and a cleared setting changes nothing.  All equalities are exact."""
import math

import numpy as np
import pytest

from tests import recover_cases, recover_oracle
from tests import recover_scene as rs
from tests.util import marker_tuples

pytestmark = pytest.mark.gpu

CASES = recover_cases.designed()
W, H = rs.W, rs.H


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


def _ctx(dictionary=rs.DICT, board=None, charuco=False):
    from aruco3_amd import _lib

    _torch()
    ctx = _lib.Context(rs.detector_config()._c(), dictionary.code_list, dictionary.num_bits, dictionary._tau)
    if board is not None:
        ctx.set_board(board.ids, board.corners)
        if charuco:
            ctx.set_charuco(board.chessboard_corners, board.adjacent_ids)
    return ctx


def _cfg(ctx, min_markers=2, max_distance_px=10.0, max_hamming=None):
    cfg = ctx.default_recover_config()
    cfg.min_markers, cfg.max_distance_px = min_markers, max_distance_px
    if max_hamming is not None:
        cfg.max_hamming = max_hamming
    return cfg


def _args(frames):
    from aruco3_amd import _lib

    assert frames.flags["C_CONTIGUOUS"] and frames.dtype == np.uint8 and frames.ndim == 3
    n, h, w = frames.shape
    return (frames.ctypes.data, _lib.MEM_HOST, _lib.FMT_L8, w, h, w, h * w, n)


def _standalone(case):
    ctx = _ctx(case.dictionary, case.board)
    got = ctx.recover_markers(case.detected_ids, case.detected_corners, case.candidates, case.codes4, case.has_codes,
                              _cfg(ctx, case.min_markers, case.max_distance_px, case.max_hamming))
    ctx.close()
    return got


# ---- the stand-alone call ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_designed_case_equals_oracle(case):
    got, want = _standalone(case), case.oracle()
    assert recover_oracle.same_records(got, want), (marker_tuples(got), marker_tuples(want))
    assert [(int(m["id"]), int(m["candidate_index"]), int(m["rotation"]), int(m["hamming_distance"])) for m in got] == case.expect


def test_board_of_1024_markers_and_2048_candidates_equals_oracle():
    case = recover_cases.big_case()
    assert len(case.board) == 1024 and len(case.candidates) == 2048
    got, want = _standalone(case), case.oracle()
    assert len(want) > 100
    assert recover_oracle.same_records(got, want)


def test_default_config_is_derived_from_the_bit_count():
    from aruco3_amd import ARDictionary

    for name in ARDictionary.get_dictionary_names():
        d = ARDictionary.new_from_named_dict(name)
        ctx = _ctx(d)
        cfg = ctx.default_recover_config()
        bits = d.num_bits
        exact = max([h for h in range(bits + 1) if sum(math.comb(bits, k) for k in range(h + 1)) * 1000 < 2 ** bits], default=0)
        assert (cfg.mode, cfg.min_markers, cfg.max_distance_px, cfg.max_hamming, bytes(cfg.reserved)) == (1, 2, 10.0, exact, b"\0\0\0"), name
        assert exact == recover_cases.DEFAULT_HAMMING[bits]
        ctx.close()


def test_setter_refusals_and_standalone_errors():
    from aruco3_amd import _lib

    bare = _ctx()
    with pytest.raises(_lib.A3Error, match="no board"):
        bare.set_board_recovery(_cfg(bare))
    bare.set_board_recovery(None)   # clearing needs no board
    assert bare.board_recovery() is None
    case = CASES[0]
    with pytest.raises(_lib.A3Error, match="no board"):
        bare.recover_markers(case.detected_ids, case.detected_corners, case.candidates, case.codes4, case.has_codes, _cfg(bare))
    ctx = _ctx(board=rs.board())
    for bad in (dict(max_distance_px=0.0), dict(max_distance_px=-2.0), dict(max_distance_px=float("nan")), dict(max_distance_px=float("inf")),
                dict(min_markers=0)):
        with pytest.raises(_lib.A3Error) as e:
            ctx.set_board_recovery(_cfg(ctx, **{"min_markers": 2, "max_distance_px": 10.0, **bad}))
        assert e.value.code == _lib.ERR_INVALID
    cfg = _cfg(ctx)
    cfg.reserved[1] = 1
    with pytest.raises(_lib.A3Error, match="reserved"):
        ctx.set_board_recovery(cfg)
    cfg = _cfg(ctx)
    cfg.mode = 2
    with pytest.raises(_lib.A3Error, match="mode"):
        ctx.set_board_recovery(cfg)
    assert ctx.board_recovery() is None   # a refused setting leaves none
    good = _cfg(ctx, 3, 7.5, 2)
    ctx.set_board_recovery(good)
    back = ctx.board_recovery()
    assert (back.mode, back.min_markers, back.max_distance_px, back.max_hamming) == (1, 3, 7.5, 2)
    # refused while a batch is in flight; the batch keeps the setting it was submitted with
    frames = rs.frames()
    ctx.set_board_recovery(_cfg(ctx))
    ctx.submit(*_args(frames))
    with pytest.raises(_lib.A3Error, match="not been collected"):
        ctx.set_board_recovery(None)
    with pytest.raises(_lib.A3Error, match="not been collected"):
        ctx.recover_markers(case.detected_ids, case.detected_corners, case.candidates, case.codes4, case.has_codes, _cfg(ctx))
    _, per = ctx.collect()
    assert ctx.recovered_counts(3).tolist() == [0, 1, 0] and per.tolist() == [6, 5, 1]
    with pytest.raises(_lib.A3Error) as e:
        ctx.recovered_counts(2)
    assert e.value.code == _lib.ERR_CAPACITY
    ctx.set_board(None)   # clearing the board clears the recovery
    assert ctx.board_recovery() is None
    ctx.close(); bare.close()


# ---- batches -------------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def scene(oracle):
    """the three frames, and the contract's merged list from the oracle's detection, under the derived default and without bits"""
    _torch()
    board, frames = rs.board(), rs.frames()
    want = {mh: rs.expected(oracle, frames, board, 2, 10.0, mh) for mh in (recover_cases.MAX_HAMMING, recover_cases.NO_BITS)}
    assert want[recover_cases.MAX_HAMMING][2] == [0, 1, 0] and want[recover_cases.NO_BITS][2] == [0, 2, 0]   # what the frames were drawn for
    return board, frames, want


def _agree(ctx, markers, per, want, what):
    merged, per_want, rec_want = want
    assert marker_tuples(markers) == merged, what
    assert per.tolist() == per_want, what
    assert ctx.recovered_counts(len(per_want)).tolist() == rec_want, what


@pytest.mark.parametrize("max_hamming", [recover_cases.MAX_HAMMING, recover_cases.NO_BITS])
def test_batch_calls_deliver_the_merged_list(scene, max_hamming):
    board, frames, want = scene
    ctx = _ctx(board=board)
    ctx.set_board_recovery(_cfg(ctx, max_hamming=max_hamming))
    args = _args(frames)
    _agree(ctx, *ctx.detect_batch(*args), want[max_hamming], "detect_batch")
    ctx.submit(*args)
    _agree(ctx, *ctx.collect(), want[max_hamming], "submit / collect")
    m, per, poses = ctx.detect_batch_pose(*args, 40.0, None)
    _agree(ctx, m, per, want[max_hamming], "detect_batch_pose")
    assert len(poses) == len(m) and np.all(np.isfinite(poses))
    ctx.submit_pose(*args, 40.0, None)
    m, per, _ = ctx.collect_pose()
    _agree(ctx, m, per, want[max_hamming], "pose submit / collect")
    ctx.set_debug_taps(True)   # the taps still describe the frame's candidates: a recovered marker's candidate_index points into them
    m, per = ctx.detect_batch(*args)
    _agree(ctx, m, per, want[max_hamming], "detect_batch with taps")
    tail = m[int(per[0]) + int(per[1]) - 1]
    assert ctx.candidates(1)[int(tail["candidate_index"])].reshape(-1).tolist() == np.roll(tail["corners"].reshape(4, 2), int(tail["rotation"]), axis=0).reshape(-1).tolist()
    # out_cap one short of the merged total
    from aruco3_amd import _lib

    total = sum(want[max_hamming][1])
    with pytest.raises(_lib.A3Error) as e:
        ctx.detect_batch(*args, out_cap=total - 1)
    assert e.value.code == _lib.ERR_CAPACITY
    m, per = ctx.detect_batch(*args, out_cap=total)
    ctx.set_debug_taps(False)
    _agree(ctx, m, per, want[max_hamming], "out_cap == total")
    ctx.close()


def test_batch_queue_of_two_contexts_and_marker_flags(scene):
    from aruco3_amd.aruco import BatchQueue, Detector
    from aruco3_amd.board import BoardRecovery

    board, frames, want = scene
    merged, per, rec = want[recover_cases.MAX_HAMMING]
    det = Detector(rs.detector_config(), rs.DICT, board=board, recovery=BoardRecovery())

    def check(dets, what):
        pos = 0
        for f, d in enumerate(dets):
            assert [(f, m.id, m.code, tuple(v for xy in m.corners for v in xy), m.hamming_distance) for m in d.markers] == \
                [t[:5] for t in merged[pos: pos + per[f]]], what
            assert [m.recovered for m in d.markers] == [False] * (per[f] - rec[f]) + [True] * rec[f], what
            pos += per[f]

    q = BatchQueue(det, depth=2)
    for _ in range(3):   # every context twice: a second batch of a context finds the setting in place
        q.submit(frames[..., None])
        q.submit(frames[..., None])
        check(q.collect(), "queue, first context")
        check(q.collect(), "queue, second context")
    q.close()
    check(det.detect_batch(frames[..., None]), "Detector.detect_batch")
    check([d for d, _ in det.detect_batch_with_pose(frames[..., None], 40.0)], "Detector.detect_batch_with_pose")
    plain = Detector(rs.detector_config(), rs.DICT, board=board)
    assert [len(d.markers) for d in plain.detect_batch(frames[..., None])] == [p - r for p, r in zip(per, rec)]
    assert not any(m.recovered for d in plain.detect_batch(frames[..., None]) for m in d.markers)


def test_later_stages_take_the_merged_list(scene):
    """the board pose uses the recovered markers, and refinement and undistortion cover them"""
    from aruco3_amd import _lib

    board, frames, want = scene
    merged, per, rec = want[recover_cases.MAX_HAMMING]
    intr = _lib.Intrinsics(W, H, 600.0, 600.0, 320.0, 240.0)
    args = _args(frames)
    plain = _ctx(board=board)
    plain.detect_batch_pose(*args, 147.0, intr)
    before = plain.board_poses()
    ctx = _ctx(board=board)
    ctx.set_board_recovery(_cfg(ctx))
    m, p, _ = ctx.detect_batch_pose(*args, 147.0, intr)
    _agree(ctx, m, p, want[recover_cases.MAX_HAMMING], "pose batch with intrinsics")
    after = ctx.board_poses()
    assert [int(a["markers_used"]) - int(b["markers_used"]) for a, b in zip(after, before)] == rec
    assert [int(a["status"]) for a in after] == [1, 1, 1]
    # refinement and lens distortion on: the same list, one set of float corners per marker of it, recovered ones included
    ctx.set_corner_refinement(_lib.default_refine_config())
    d = _lib.default_distortion()
    d.k1 = -0.05
    ctx.set_distortion(d)
    m, p, poses = ctx.detect_batch_pose(*args, 147.0, intr)
    _agree(ctx, m, p, want[recover_cases.MAX_HAMMING], "pose batch with refinement and distortion")
    refined = ctx.refined_corners()
    und, res = ctx.undistorted_corners()
    total = sum(per)
    assert len(refined) == len(und) == len(res) == len(poses) == total
    k = per[0] + per[1] - 1   # frame 1's recovered marker
    assert rec[1] == 1 and np.all(np.isfinite(refined[k])) and np.all(np.isfinite(und[k]))
    assert [int(a["markers_used"]) for a in ctx.board_poses()] == [int(a["markers_used"]) for a in after]
    ctx.close(); plain.close()


def test_charuco_board(oracle):
    _torch()
    board, frames = rs.charuco_board(), rs.charuco_frames()
    want = rs.expected(oracle, frames, board, 2, 10.0, recover_cases.MAX_HAMMING)
    assert want[2] == [0, 1, 0]
    ctx = _ctx(board=board, charuco=True)
    ctx.set_board_recovery(_cfg(ctx))
    _agree(ctx, *ctx.detect_batch(*_args(frames)), want, "ChArUco, detect_batch")
    ctx.charuco_corners()   # (the corner stage ran on the merged list)
    m, per, _ = ctx.detect_batch_pose(*_args(frames), 112.0, None)
    _agree(ctx, m, per, want, "ChArUco, pose batch")
    assert len(ctx.charuco_poses()) == 3
    ctx.close()


def test_batch_in_two_chunks(scene):
    board, frames, want = scene
    ctx = _ctx(board=board)
    ctx.set_board_recovery(_cfg(ctx))
    args = _args(frames)
    ctx.detect_batch(*args)
    assert ctx.stats()["chunks"] == 1
    darts = ctx.stats()["darts"]
    small = _ctx(board=board)
    small.set_board_recovery(_cfg(small))
    small.set_pool_limits(max_darts=int(darts * 0.6), max_points=0)
    m, per = small.detect_batch(*args)
    assert small.stats()["chunks"] == 2
    _agree(small, m, per, want[recover_cases.MAX_HAMMING], "two chunks")
    ctx.close(); small.close()


def test_cleared_setting_changes_nothing(scene):
    from aruco3_amd import _lib

    board, frames, _ = scene
    args = _args(frames)
    never = _ctx(board=board)
    ctx = _ctx(board=board)
    ctx.set_board_recovery(_cfg(ctx))
    ctx.detect_batch(*args)
    ctx.set_board_recovery(None)
    for call in (lambda c: c.detect_batch(*args), lambda c: c.detect_batch_pose(*args, 40.0, None)):
        a, b = call(never), call(ctx)
        assert marker_tuples(a[0]) == marker_tuples(b[0]) and a[1].tolist() == b[1].tolist()
        assert all(np.array_equal(x, y) for x, y in zip(a[2:], b[2:]))
        assert never.board_poses().tobytes() == ctx.board_poses().tobytes() if len(a) == 3 else True
        with pytest.raises(_lib.A3Error, match="without board recovery"):
            ctx.recovered_counts(3)
    ctx.close(); never.close()
