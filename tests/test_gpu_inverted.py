"""Inverted markers on the MI355X (a3_set_marker_polarity, A3_POLARITY_BOTH): k_decode's inverted instantiations, k_marker_flags, the
flag words through every path the per-marker results take, and the edge fit's sign -- against the numpy rule of tests/inverted_util.py
on the oracle's candidates and patches, and against tests/inverted_edge_oracle.c.  All equalities are exact.  GPU only."""
import numpy as np
import pytest

from tests import damage_util as du
from tests import inverted_util as iu
from tests.util import marker_tuples, markers_of_hip, markers_of_oracle

pytestmark = pytest.mark.gpu

FOUND = "ARUCO"               # family b: found quads
INJECTED = ("ARUCO", "ARUCO_MIP_36H12")


def _args(frames):
    """frames [n, h, w] (L8) in host memory -> the arguments of detect_batch / submit"""
    from aruco3_amd import _lib

    assert frames.flags["C_CONTIGUOUS"] and frames.dtype == np.uint8 and frames.ndim == 3
    n, h, w = frames.shape
    return (frames.ctypes.data, _lib.MEM_HOST, _lib.FMT_L8, w, h, w, h * w, n)


def _yuyv_args(frames):
    """the same luma as packed YUYV (chroma 128) -> (arguments, the array they point into)"""
    from aruco3_amd import _lib

    n, h, w = frames.shape
    packed = np.full((n, h, w, 2), 128, np.uint8)
    packed[..., 0] = frames
    packed = np.ascontiguousarray(packed)
    return (packed.ctypes.data, _lib.MEM_HOST, _lib.FMT_YUYV8, w, h, 2 * w, 2 * h * w, n), packed


def _detector(name, filt=True, both=True, config=None, **kw):
    from aruco3_amd.aruco import Detector

    d = du.dictionary(name)
    det = Detector(config or iu.detector_config(filt, d.num_bits), d, inverted_markers=both, **kw)
    return det, det._context()


def _split(markers, per):
    out, pos = [], 0
    for c in per.tolist():
        out.append(markers[pos: pos + c])
        pos += c
    assert pos == len(markers)
    return out


def _found_frames(n):
    """the first n family-b frames of FOUND: even ones complemented, odd ones mixed"""
    nb = du.table(FOUND)[0]
    grey, which = du.found_frames(FOUND)
    out = [iu.complemented(grey[f]) if f % 2 == 0 else iu.mixed(grey[f], len(which[f]), nb, 100 + f)[0] for f in range(n)]
    return np.ascontiguousarray(np.stack(out))


_expected_cache = {}


def _expected(oracle, frames, filt=True, both=True):
    """-> per frame (marker tuples, candidate indices, flags) by the numpy rule on the oracle's candidates and patches"""
    key = (hash(frames.tobytes()), frames.shape, filt, both)
    if key not in _expected_cache:
        nb, _, codes = du.table(FOUND)
        tau = du.tau_of(FOUND)
        cfg = iu.oracle_config(oracle, filt, nb)
        _expected_cache[key] = [iu.expect_frame(oracle, oracle.detect(fr, codes, nb, tau, config=cfg), codes, nb, tau, filt, both)[:3] for fr in frames]
    return _expected_cache[key]


def _check_found(markers, per, flags, want, what):
    assert len(flags) == len(markers) == int(per.sum()), what
    pos = 0
    for f, (ms, c) in enumerate(zip(_split(markers, per), per.tolist())):
        em, ei, ef = want[f]
        assert markers_of_hip(ms) == em, f"{what}, frame {f}: markers"
        assert [int(r["candidate_index"]) for r in ms] == ei, f"{what}, frame {f}: candidate indices"
        assert flags[pos: pos + c].tolist() == ef, f"{what}, frame {f}: flags"
        pos += c


def _check_invariant(ctx, markers, per, flags, what, least_inverted=1):
    """flags[i] == (tapped decode_ok[candidate_index] == 2) for every delivered marker of the last (tapped) batch"""
    assert len(flags) == len(markers) == int(per.sum()), what
    assert set(np.unique(flags).tolist()) <= {0, 1}, what
    pos = 0
    for f, c in enumerate(per.tolist()):
        dec = ctx.homographies(f, with_patches=False)[3]
        for i in range(pos, pos + c):
            assert int(markers[i]["frame"]) == f
            assert int(flags[i]) == int(dec[int(markers[i]["candidate_index"])] == 2), f"{what}: marker {i} of frame {f}"
        pos += c
    assert int(flags.sum()) >= least_inverted, f"{what}: no inverted marker was delivered, the case proves nothing"


# ---- 1. mode DARK ------------------------------------------------------------------------------------------------------------------------
def test_mode_dark_after_both_is_a_context_that_never_set_it(oracle):
    from aruco3_amd import _lib

    nb, _, codes = du.table(FOUND)
    tau = du.tau_of(FOUND)
    grey, _ = du.found_frames(FOUND)
    frames = np.ascontiguousarray(np.concatenate([grey[:4], _found_frames(4)]))
    args = _args(frames)
    cap = 128 * len(frames)
    det0, never = _detector(FOUND, both=False)
    det1, ctx = _detector(FOUND, both=False)
    assert ctx.get_marker_polarity() == _lib.POLARITY_DARK
    ctx.set_marker_polarity(_lib.POLARITY_BOTH)
    assert ctx.get_marker_polarity() == _lib.POLARITY_BOTH
    with pytest.raises(_lib.A3Error) as e:
        ctx.set_marker_polarity(2)
    assert e.value.code == _lib.ERR_INVALID and ctx.get_marker_polarity() == _lib.POLARITY_BOTH
    ctx.set_debug_taps(True)
    m, per = ctx.detect_batch(*args, out_cap=cap)
    assert int(ctx.marker_flags().sum()) > 0
    ctx.set_marker_polarity(_lib.POLARITY_DARK)
    never.set_debug_taps(True)
    m0, per0 = never.detect_batch(*args, out_cap=cap)
    m1, per1 = ctx.detect_batch(*args, out_cap=cap)
    assert marker_tuples(m1) == marker_tuples(m0) and per1.tolist() == per0.tolist()   # (every field; a record's 4 padding bytes are not data)
    for c in (ctx, never):
        with pytest.raises(_lib.A3Error, match="A3_POLARITY_BOTH") as e:
            c.marker_flags()
        assert e.value.code == _lib.ERR_INVALID
    cfg = iu.oracle_config(oracle, True, nb)
    for f, ms in enumerate(_split(m1, per1)):
        ref = oracle.detect(frames[f], codes, nb, tau, config=cfg)
        assert markers_of_hip(ms) == markers_of_oracle(ref), f
        for c in (ctx, never):
            _, ok, tapped, dec = c.homographies(f, with_patches=False)
            assert dec.tolist() == ref["decode_ok"].tolist() and tapped.tolist() == ref["codes"].tolist(), f
            assert 2 not in dec.tolist()
    # the argument checks that need a context
    L = _lib.load()
    import ctypes as C

    n = C.c_size_t(5)
    assert L.a3_get_marker_flags(ctx.handle, None, 3, C.byref(n)) == _lib.ERR_INVALID
    assert L.a3_get_marker_flags(ctx.handle, None, 0, None) == _lib.ERR_INVALID
    assert L.a3_get_marker_polarity(ctx.handle, None) == _lib.ERR_INVALID
    ctx.set_marker_polarity(_lib.POLARITY_BOTH)
    ctx.detect_batch(*args, out_cap=cap)
    total = len(m)
    short = (C.c_uint32 * 1)()
    assert total > 1 and L.a3_get_marker_flags(ctx.handle, short, 1, C.byref(n)) == _lib.ERR_CAPACITY and n.value == total
    ctx.submit(*args, out_cap=cap)
    with pytest.raises(_lib.A3Error) as e:      # refused between submit and collect
        ctx.marker_flags()
    assert e.value.code == _lib.ERR_INVALID
    ctx.collect()
    assert ctx.marker_flags().tolist() == _flags_of(m, per, ctx)


def _flags_of(markers, per, ctx):
    """the flags the tapped decode_ok of the last batch imply for `markers`"""
    out, pos = [], 0
    for f, c in enumerate(per.tolist()):
        dec = ctx.homographies(f, with_patches=False)[3]
        out += [int(dec[int(markers[i]["candidate_index"])] == 2) for i in range(pos, pos + c)]
        pos += c
    return out


# ---- 2. injected quads -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", INJECTED)
def test_injected_quads_on_complemented_frames(name):
    """every pattern of family a, complemented, from each of its four start corners: what k_decode<256, 256, false, true> makes of it"""
    nb, _, codes = du.table(name)
    tau = du.tau_of(name)
    cap = 1024
    seen = set()
    for filt in (True, False):
        det, ctx = _detector(name, filt, config=du.detector_config(filt, nb))
        ctx.set_debug_taps(True)
        for fi, (img, quads, views, _) in enumerate(du.injected_frames(name)):
            what = f"{name}, filter {filt}, frame {fi}"
            exp = [iu.expect_view_both(1 - np.asarray(v), codes) for v in views]
            want = [(m, int(inv)) for m, inv in ((du.expected_marker(e, q, tau, filt), inv) for (e, inv), q in zip(exp, quads)) if m is not None]
            frames = np.ascontiguousarray(iu.complemented(img)[None])
            args = _args(frames)
            ctx.detect_batch(*args, out_cap=cap)      # (the hook is one-shot: a batch the library runs twice would lose it)
            ctx.debug_inject_candidates(quads)
            m, per = ctx.detect_batch(*args, out_cap=cap)
            flags = ctx.marker_flags()
            assert ctx.candidates(0).tolist() == quads.tolist(), what
            _, ok, tapped, dec = ctx.homographies(0, with_patches=False)
            assert ok.all(), what
            assert dec.tolist() == [e.decode_ok for e, _ in exp], what + ": decode_ok"
            assert [[int(c) for c in r] for r in tapped] == [e.codes for e, _ in exp], what + ": codes4"
            assert markers_of_hip(m) == [w[0] for w in want], what + ": markers"
            assert flags.tolist() == [w[1] for w in want], what + ": flags"
            assert [int(r["candidate_index"]) for r in m] == [k for k, (e, _) in enumerate(exp) if e.accepted(tau, filt)], what
            assert per.tolist() == [len(want)], what
            seen |= set(dec.tolist())
        del det
    assert seen == {0, 2}        # a complemented frame holds nothing that reads dark


# ---- 3. found quads ----------------------------------------------------------------------------------------------------------------------
def test_found_quads_in_small_and_large_batches_and_as_yuyv(oracle):
    n = du.FOUND_FRAMES
    assert n >= 65
    frames = _found_frames(n)
    want = _expected(oracle, frames)
    assert sum(sum(w[2]) for w in want) > n and any(0 in w[2] and 1 in w[2] for w in want)     # inverted markers, and frames with both kinds
    det, ctx = _detector(FOUND)
    cap = 128 * n
    m, per = ctx.detect_batch(*_args(frames), out_cap=cap)                    # 65 frames or more: the one-wave tail
    flags = ctx.marker_flags()
    _check_found(m, per, flags, want, "whole batch")
    part = np.ascontiguousarray(frames[:64])
    mp, pp = ctx.detect_batch(*_args(part), out_cap=cap)                      # at most 64 frames: the all-waves tail
    _check_found(mp, pp, ctx.marker_flags(), want[:64], "64 frames")
    for count, what in ((n, "YUYV, whole batch"), (8, "YUYV, 8 frames")):     # the luma rule: equal to L8, in both tail forms
        sub = np.ascontiguousarray(frames[:count])
        yargs, keep = _yuyv_args(sub)
        my, py = ctx.detect_batch(*yargs, out_cap=cap)
        _check_found(my, py, ctx.marker_flags(), want[:count], what)
        del keep


# ---- 4. the invariant through every path ---------------------------------------------------------------------------------------------------
def test_flags_follow_the_tapped_decode_ok_with_threshold_windows():
    frames = _found_frames(4)
    det, ctx = _detector(FOUND, threshold_windows=(7, 15))
    ctx.set_debug_taps(True)
    m, per = ctx.detect_batch(*_args(frames), out_cap=512)
    _check_invariant(ctx, m, per, ctx.marker_flags(), "threshold windows (7, 15)")


def test_flags_follow_the_tapped_decode_ok_with_a_reduction():
    from aruco3_amd.aruco import Reduction

    frames = _found_frames(4)
    det, ctx = _detector(FOUND, reduction=Reduction(2))
    ctx.set_debug_taps(True)
    m, per = ctx.detect_batch(*_args(frames), out_cap=512)
    _check_invariant(ctx, m, per, ctx.marker_flags(), "Reduction(2)")


def test_flags_follow_the_tapped_decode_ok_with_a_rectification():
    from aruco3_amd import CameraIntrinsics
    from aruco3_amd.aruco import Rectification

    frames = _found_frames(4)
    t = np.deg2rad(2.0)
    rot = np.array([[np.cos(t), 0.0, np.sin(t)], [0.0, 1.0, 0.0], [-np.sin(t), 0.0, np.cos(t)]])
    cam = CameraIntrinsics(du.W, du.H, 700.0, 700.0, 320.0, 240.0)
    det, ctx = _detector(FOUND, rectification=Rectification(cam, rotation=rot, fill=128))
    ctx.set_debug_taps(True)
    m, per = ctx.detect_batch(*_args(frames), out_cap=512)
    _check_invariant(ctx, m, per, ctx.marker_flags(), "Rectification")


def test_flags_behind_the_recovery_merge():
    """BoardRecovery on: the marker list the flags are made for is k_recover_merge's.  On the board scene as drawn (dark markers, mode
    BOTH) frame 1's damaged marker is recovered and its flag follows its quad: decode_ok 1, flag 0; with a recovery that compares no
    bits the notched marker comes too: its border was mixed, decode_ok 0, flag 0.  On the wholly complemented scene every delivered
    marker is flagged.  The recovered INVERTED marker is test_a_recovered_inverted_markers_flag_follows_its_quad's."""
    from aruco3_amd import _lib
    from tests import recover_scene as rs

    board = rs.board()
    d = rs.DICT
    ctx = _lib.Context(rs.detector_config()._c(), d.code_list, d.num_bits, d._tau)
    ctx.set_board(board.ids, board.corners)
    ctx.set_board_recovery(ctx.default_recover_config())
    ctx.set_marker_polarity(_lib.POLARITY_BOTH)
    ctx.set_debug_taps(True)
    frames = np.ascontiguousarray(rs.frames())
    m, per = ctx.detect_batch(*_args(frames), out_cap=256)
    flags = ctx.marker_flags()
    assert ctx.recovered_counts(len(frames)).tolist() == [0, 1, 0]
    _check_invariant(ctx, m, per, flags, "BoardRecovery, as drawn", least_inverted=0)
    k = int(per[0] + per[1]) - 1                  # frame 1's recovered marker is the tail of its segment
    dec = ctx.homographies(1, with_patches=False)[3]
    assert int(m[k]["id"]) == rs.FIRST_ID + rs.DAMAGED_SLOT and int(dec[int(m[k]["candidate_index"])]) == 1 and int(flags[k]) == 0
    cfg = ctx.default_recover_config()
    cfg.max_hamming = 255
    ctx.set_board_recovery(cfg)
    m, per = ctx.detect_batch(*_args(frames), out_cap=256)
    flags = ctx.marker_flags()
    assert ctx.recovered_counts(len(frames)).tolist() == [0, 2, 0]
    _check_invariant(ctx, m, per, flags, "BoardRecovery, max_hamming 255", least_inverted=0)
    dec = ctx.homographies(1, with_patches=False)[3]
    end = int(per[0] + per[1])
    tail = {int(m[i]["id"]): (int(dec[int(m[i]["candidate_index"])]), int(flags[i])) for i in range(end - 2, end)}
    assert tail == {rs.FIRST_ID + rs.DAMAGED_SLOT: (1, 0), rs.FIRST_ID + rs.NOTCHED_SLOT: (0, 0)}
    inv = np.ascontiguousarray(iu.complemented(rs.frames()))
    m, per = ctx.detect_batch(*_args(inv), out_cap=256)
    flags = ctx.marker_flags()
    _check_invariant(ctx, m, per, flags, "BoardRecovery, complemented", least_inverted=6)
    assert int(flags.sum()) == len(m)
    ctx.close()


def test_a_recovered_inverted_markers_flag_follows_its_quad(oracle):
    """tests/inverted_util.py's board scene (bright-on-dark markers on a bright board, frame 1 with one marker damaged by tau cells):
    the merged list, the recovered counts and the flags are what the recovery contract makes of the numpy rule on the oracle's
    candidates -- k_recover compares the complemented codes4 -- the recovered marker's candidate has decode_ok 2 and its flag is 1, and
    the edge fit refines it with the inverted sign"""
    from aruco3_amd import _lib
    from tests import edge_refine_oracle as ero
    from tests import inverted_edge_oracle as ieo
    from tests import recover_cases
    from tests import recover_scene as rs

    board, frames = iu.board_scene()
    d = rs.DICT
    want, wper, wrec, wflags, wdec = iu.expected_recovery(oracle, frames, board, d, rs.oracle_config(oracle), 2, iu.RECOVER_DISTANCE_PX,
                                                          recover_cases.MAX_HAMMING)
    assert wrec == [0, 1, 0]
    ctx = _lib.Context(rs.detector_config()._c(), d.code_list, d.num_bits, d._tau)
    ctx.set_board(board.ids, board.corners)
    cfg = ctx.default_recover_config()
    assert cfg.max_hamming == recover_cases.MAX_HAMMING
    cfg.max_distance_px = iu.RECOVER_DISTANCE_PX
    ctx.set_board_recovery(cfg)
    ctx.set_marker_polarity(_lib.POLARITY_BOTH)
    ctx.set_corner_refinement(_lib.RefineConfig(_lib.REFINE_EDGES, 10, 0.4, 30, 0.01))   # (ero.config(10, 0.4) as the library's record)
    ctx.set_debug_taps(True)
    m, per = ctx.detect_batch(*_args(frames), out_cap=256)
    flags = ctx.marker_flags()
    assert marker_tuples(m) == want and per.tolist() == wper
    assert ctx.recovered_counts(len(frames)).tolist() == wrec
    assert flags.tolist() == wflags
    _check_invariant(ctx, m, per, flags, "BoardRecovery, inverted board scene", least_inverted=len(m))
    k = int(per[0] + per[1]) - 1                  # frame 1's recovered marker is the tail of its segment
    dec = ctx.homographies(1, with_patches=False)[3]
    assert int(m[k]["id"]) == rs.FIRST_ID + rs.DAMAGED_SLOT and 0 < int(m[k]["hamming_distance"]) <= recover_cases.MAX_HAMMING
    assert int(dec[int(m[k]["candidate_index"])]) == 2 and wdec[k] == 2 and int(flags[k]) == 1
    refined = ctx.refined_corners()
    pos = 0
    for f, c in enumerate(per.tolist()):
        corners = [tuple(int(v) for v in r["corners"]) for r in m[pos: pos + c]]
        assert refined[pos: pos + c].tobytes() == ieo.refine_markers(frames[f], corners, rs.N, ero.config(10, 0.4), flags[pos: pos + c]).tobytes(), f
        pos += c
    assert (refined[k] != np.array(m[k]["corners"], np.float32).reshape(4, 2)).any()      # refined, not reverted
    ctx.close()


def test_flags_of_a_batch_in_chunks():
    frames = _found_frames(8)
    det, ctx = _detector(FOUND)
    ctx.set_debug_taps(True)
    m0, per0 = ctx.detect_batch(*_args(frames), out_cap=1024)
    f0 = ctx.marker_flags()
    assert ctx.stats()["chunks"] == 1
    darts = ctx.stats()["darts"]
    det2, small = _detector(FOUND)
    small.set_pool_limits(max_darts=int(darts * 0.3), max_points=0)
    small.set_debug_taps(True)
    m, per = small.detect_batch(*_args(frames), out_cap=1024)
    assert small.stats()["chunks"] >= 2
    assert marker_tuples(m) == marker_tuples(m0) and per.tolist() == per0.tolist()
    flags = small.marker_flags()
    assert flags.tolist() == f0.tolist()
    _check_invariant(small, m, per, flags, "chunks")


def test_flags_of_a_list_longer_than_its_guess(oracle):
    """a fresh context guesses 64 markers: its first batch holds more, the whole list and its flags are fetched again"""
    frames = _found_frames(24)
    want = _expected(oracle, frames)
    assert sum(len(w[0]) for w in want) > 64
    det, ctx = _detector(FOUND)
    m, per = ctx.detect_batch(*_args(frames), out_cap=4096)
    _check_found(m, per, ctx.marker_flags(), want, "re-fetch")
    det2, tapped = _detector(FOUND)
    tapped.set_debug_taps(True)
    m2, per2 = tapped.detect_batch(*_args(frames), out_cap=4096)
    _check_invariant(tapped, m2, per2, tapped.marker_flags(), "re-fetch, tapped")


def test_flags_through_submit_collect_and_the_batch_queue(oracle):
    from aruco3_amd.aruco import BatchQueue

    frames = _found_frames(6)
    want = _expected(oracle, frames)
    det, ctx = _detector(FOUND)
    ctx.set_debug_taps(True)
    ctx.submit(*_args(frames), out_cap=1024)
    m, per = ctx.collect()
    flags = ctx.marker_flags()
    _check_invariant(ctx, m, per, flags, "submit / collect")
    _check_found(m, per, flags, want, "submit / collect")
    q = BatchQueue(det, depth=2)
    other = np.ascontiguousarray(frames[::-1])
    for _ in range(2):   # every context twice
        q.submit(frames[..., None])
        q.submit(other[..., None])
        for dets, w in ((q.collect(), want), (q.collect(), want[::-1])):
            for d, (em, _, ef) in zip(dets, w):
                assert [(x.id, x.code, tuple(x.corners), x.hamming_distance) for x in d.markers] == [t[:4] for t in em]
                assert [int(x.inverted) for x in d.markers] == ef
    q.close()


# ---- 5. edge refinement ------------------------------------------------------------------------------------------------------------------
def test_edge_fit_of_an_inverted_quad_on_a_complemented_scene():
    """tests/edge_refine_cases.py's slanted scene, complemented: a bright quad on a dark ground, its inner quad handed in as the one
    candidate; filter off, so the all-lit matrix is accepted (read inverted, code 0) and refined with the opposite sign"""
    from aruco3_amd.aruco import CornerRefinement, DetectorConfig
    from tests import edge_refine_cases as ec
    from tests import edge_refine_oracle as ero
    from tests import inverted_edge_oracle as ieo

    grey = np.ascontiguousarray(255 - ec.slanted_frame())
    quad = np.rint(ec.square(80.3, 59.6, 32.0, 17.0)).astype(np.uint32)      # 3 px inside the bright quad: a flat patch
    nb = du.table(FOUND)[0]
    cells = du.side_cells(nb) + 2
    det, ctx = _detector(FOUND, False, config=DetectorConfig(filter_high_bit_errors=False), refinement=CornerRefinement.edges(10, 0.0))
    det._apply_refinement(ctx)
    ctx.set_debug_taps(True)
    args = _args(grey[None])
    ctx.detect_batch(*args, out_cap=64)
    ctx.debug_inject_candidates(quad[None])
    m, per = ctx.detect_batch(*args, out_cap=64)
    assert per.tolist() == [1] and ctx.marker_flags().tolist() == [1]
    assert ctx.homographies(0, with_patches=False)[3].tolist() == [2]
    corners = [tuple(int(v) for v in m[0]["corners"])]
    got = ctx.refined_corners()
    want = ieo.refine_markers(grey, corners, cells, ero.config(10, 0.0), [1])
    assert got.tobytes() == want.tobytes()
    start = np.array(corners[0], np.float32).reshape(4, 2)
    assert (want[0] != start).any()                                            # the fit moved the corners out to the edge ...
    rot = int(m[0]["rotation"])
    assert np.abs(want[0] - np.roll(ec.SLANTED, -rot, axis=0)).max() < 0.5     # ... of the drawn quad
    dark = ieo.refine_markers(grey, corners, cells, ero.config(10, 0.0), [0])
    assert dark.tobytes() == start[None].tobytes()                             # the dark-inside fit finds no edge here and reverts


@pytest.mark.parametrize("scene,win_half,relative_win,iterations", [("slanted", 5, 0.4, 30), ("slanted", 10, 0.0, 1), ("border", 5, 0.0, 30),
                                                                     ("border", 10, 0.4, 30), ("faint", 5, 0.0, 30)])
def test_edge_fit_on_more_complemented_scenes(scene, win_half, relative_win, iterations):
    """further frames of tests/edge_refine_cases.py, complemented, at other settings: the quad 3 px inside the bright one is handed in,
    read inverted (a flat patch: every cell lit) and refined as the polarity oracle refines it -- the cell-size range, one pass only,
    a side along the frame border, and a contrast below the live level (the marker reverts)"""
    from aruco3_amd import _lib
    from aruco3_amd.aruco import DetectorConfig
    from tests import edge_refine_cases as ec
    from tests import edge_refine_oracle as ero
    from tests import inverted_edge_oracle as ieo

    if scene == "border":
        grey, drawn = ec.border_frame(), ec.BORDER
        quad = np.rint(drawn + np.array([[3, 3], [-3, 3], [-3, -3], [3, -3]])).astype(np.uint32)
    else:
        grey = ec.scenes()["faint"][0] if scene == "faint" else ec.slanted_frame()
        quad = np.rint(ec.square(80.3, 59.6, 32.0, 17.0)).astype(np.uint32)
    grey = np.ascontiguousarray(255 - grey)
    cells = du.side_cells(du.table(FOUND)[0]) + 2
    cfg = ero.config(win_half, relative_win, max_iterations=iterations)
    det, ctx = _detector(FOUND, False, config=DetectorConfig(filter_high_bit_errors=False))
    ctx.set_corner_refinement(_lib.RefineConfig(_lib.REFINE_EDGES, cfg.win_half, cfg.relative_win, cfg.max_iterations, cfg.min_shift))
    ctx.set_debug_taps(True)
    args = _args(grey[None])
    ctx.detect_batch(*args, out_cap=64)
    ctx.debug_inject_candidates(quad[None])
    m, per = ctx.detect_batch(*args, out_cap=64)
    assert per.tolist() == [1] and ctx.marker_flags().tolist() == [1]
    corners = [tuple(int(v) for v in m[0]["corners"])]
    want = ieo.refine_markers(grey, corners, cells, cfg, [1])
    assert ctx.refined_corners().tobytes() == want.tobytes()
    moved = bool((want[0] != np.array(corners[0], np.float32).reshape(4, 2)).any())
    assert moved == (scene != "faint")


def test_edge_fit_on_mixed_frames(oracle):
    from aruco3_amd.aruco import CornerRefinement
    from tests import edge_refine_oracle as ero
    from tests import inverted_edge_oracle as ieo

    frames = _found_frames(4)
    want = _expected(oracle, frames)
    nb = du.table(FOUND)[0]
    cells = du.side_cells(nb) + 2
    det, ctx = _detector(FOUND, refinement=CornerRefinement.edges(10, 0.4))
    det._apply_refinement(ctx)
    m, per = ctx.detect_batch(*_args(frames), out_cap=512)
    flags = ctx.marker_flags()
    _check_found(m, per, flags, want, "edge refinement on")
    refined = ctx.refined_corners()
    assert len(refined) == len(m)
    cfg = ero.config(10, 0.4)
    pos, n_dark, n_inv, moved = 0, 0, 0, 0
    for f, c in enumerate(per.tolist()):
        corners = [tuple(int(v) for v in r["corners"]) for r in m[pos: pos + c]]
        fl = flags[pos: pos + c]
        assert refined[pos: pos + c].tobytes() == ieo.refine_markers(frames[f], corners, cells, cfg, fl).tobytes(), f
        dark = [q for q, x in zip(corners, fl.tolist()) if not x]
        if dark:   # dark markers: the existing oracle
            assert refined[pos: pos + c][fl == 0].tobytes() == ero.refine_markers(frames[f], dark, cells, cfg).tobytes(), f
        n_dark += len(dark)
        n_inv += int(fl.sum())
        moved += int((refined[pos: pos + c][fl == 1] != np.array(corners, np.float32).reshape(-1, 4, 2)[fl == 1]).any(axis=(1, 2)).sum())
        pos += c
    assert n_dark >= 2 and n_inv >= 4 and moved >= n_inv // 2      # inverted markers were refined, not merely reverted


# ---- 6. Python ---------------------------------------------------------------------------------------------------------------------------
def test_detector_returns_marker_inverted(oracle):
    from aruco3_amd.aruco import Detector

    frames = _found_frames(4)
    want = _expected(oracle, frames)
    today = _expected(oracle, frames, both=False)
    d = du.dictionary(FOUND)
    det = Detector(iu.detector_config(True, d.num_bits), d, inverted_markers=True)
    for dets in (det.detect_batch(frames[..., None]), [x for x, _ in det.detect_batch_with_pose(frames[..., None], 40.0)]):
        for got, (em, _, ef) in zip(dets, want):
            assert [(x.id, x.code, tuple(x.corners), x.hamming_distance) for x in got.markers] == [t[:4] for t in em]
            assert [int(x.inverted) for x in got.markers] == ef
    plain = Detector(iu.detector_config(True, d.num_bits), d)
    for got, (em, _, _) in zip(plain.detect_batch(frames[..., None]), today):
        assert [(x.id, x.code, tuple(x.corners), x.hamming_distance) for x in got.markers] == [t[:4] for t in em]
        assert not any(x.inverted for x in got.markers)
    assert sum(len(w[0]) for w in today) < sum(len(w[0]) for w in want)
