"""Inverted markers without a GPU: the rule of tests/inverted_util.py on the oracle's own stages.  On the complement of every
family-b frame of tests/damage_util.py, every pattern that the dark expectation accepts is found and read inverted with the same id,
code and distance -- all of them, no allowance; on the frames as drawn the rule's dark reads are the oracle's marker list.  The stages
ahead of the bit matrix (threshold, contours, quads, discard, warp) are the oracle's and do not know about polarity: this is the check
that they need not."""
import functools

import numpy as np
import pytest

from tests import damage_util as du
from tests import inverted_util as iu
from tests.util import markers_of_oracle


def _slot_of(quad, squares):
    """the slot whose marker square has every corner within 2 px of a corner of `quad` (the quiet zone's quad lies QUIET px out)"""
    q = np.asarray(quad, dtype=np.int64).reshape(4, 2)
    for s, (x0, y0, x1, y1) in enumerate(squares):
        sq = np.array([[x0, y0], [x1, y0], [x1, y1], [x0, y1]])
        if all(np.abs(sq - p).max(axis=1).min() <= 2 for p in q):
            return s
    return None


def _squares(count, nb):
    return [(x0 + du.QUIET, y0 + du.QUIET, x1 - du.QUIET, y1 - du.QUIET) for x0, y0, x1, y1 in iu.slot_rects(count, nb)]


@functools.lru_cache(maxsize=None)
def _survey(oracle_mod, name):
    """every family-b frame of `name`, as drawn and complemented -> the counts the tests assert on"""
    oracle = oracle_mod
    nb, _, codes = du.table(name)
    tau = du.tau_of(name)
    frames, which = du.found_frames(name)
    cfg = iu.oracle_config(oracle, True, nb)
    out = {"want": 0, "got": 0, "missing": [], "dark_mismatch": [], "false_inverted": 0, "dark_total": 0, "inverted_dark_reads": 0}
    for f, frame in enumerate(frames):
        squares = _squares(len(which[f]), nb)
        ref = oracle.detect(frame, codes, nb, tau, config=cfg)
        markers, idx, flags, _ = iu.expect_frame(oracle, ref, codes, nb, tau, True)
        dark = [m for m, fl in zip(markers, flags) if not fl]
        if dark != markers_of_oracle(ref):
            out["dark_mismatch"].append(f)
        out["dark_total"] += len(dark)
        out["false_inverted"] += sum(flags)
        dark_by_slot = {}
        for m, k, fl in zip(markers, idx, flags):
            s = _slot_of(ref["candidates"][k], squares)
            if s is not None and not fl:
                dark_by_slot[s] = (m[0], m[1], m[3])
        # the dark expectation of the drawing itself must have been delivered (tests/test_decode_damage.py shows that it is)
        for s, pi in enumerate(which[f]):
            assert (s in dark_by_slot) == du.patterns(name)[pi].expect.accepted(tau, True), (name, f, s)
        inv = iu.complemented(frame)
        ref_i = oracle.detect(inv, codes, nb, tau, config=cfg)
        markers_i, idx_i, flags_i, _ = iu.expect_frame(oracle, ref_i, codes, nb, tau, True)
        inv_by_slot = {}
        for m, k, fl in zip(markers_i, idx_i, flags_i):
            s = _slot_of(ref_i["candidates"][k], squares)
            if s is not None:
                if fl:
                    inv_by_slot[s] = (m[0], m[1], m[3])
                else:
                    out["inverted_dark_reads"] += 1
        for s, want in dark_by_slot.items():
            out["want"] += 1
            if inv_by_slot.get(s) == want:
                out["got"] += 1
            else:
                out["missing"].append((f, s, want, inv_by_slot.get(s)))
    return out


@pytest.mark.parametrize("name", iu.DICTS)
def test_every_accepted_pattern_is_read_inverted_from_the_complement(oracle, name):
    r = _survey(oracle, name)
    print(f"{name}: {r['got']} of {r['want']} accepted patterns read inverted with the same id, code and distance; "
          f"{r['false_inverted']} inverted reads beside {r['dark_total']} dark ones on the frames as drawn")
    assert r["want"] > 0
    assert r["got"] == r["want"], r["missing"][:5]
    assert r["inverted_dark_reads"] == 0          # no marker square of a complemented frame reads dark


@pytest.mark.parametrize("name", iu.DICTS)
def test_dark_reads_of_the_rule_are_the_oracles_markers(oracle, name):
    r = _survey(oracle, name)
    assert r["dark_mismatch"] == []
    if name in ("ARUCO", "APRILTAG_16H5"):       # small tau: no white quiet zone passes the filter (include/aruco3_hip.h)
        assert r["false_inverted"] == 0


@pytest.mark.parametrize("name", iu.DICTS)
def test_flat_matrices_and_the_failed_projection(oracle, name):
    nb, _, codes = du.table(name)
    n = du.side_cells(nb) + 2
    zero_codes = du.expect_codes([0, 0, 0, 0], codes)
    e, inv = iu.expect_view_both(np.zeros((n, n), np.uint8), codes)          # all black: read dark, the interior's code is 0
    assert (e.decode_ok, inv, e.codes, e.id, e.distance) == (1, False, [0, 0, 0, 0], zero_codes.id, zero_codes.distance)
    e, inv = iu.expect_view_both(np.ones((n, n), np.uint8), codes)           # all white: read inverted, complemented to all black
    assert (e.decode_ok, inv, e.codes, e.id, e.distance) == (2, True, [0, 0, 0, 0], zero_codes.id, zero_codes.distance)
    # quirk Q4: a failed projection is a 1 x 1 black patch, its matrix all black: dark, never inverted
    bits = iu.bits_of_patch(oracle, np.full((7, 7), 255, np.uint8), False, n)
    assert bits.shape == (n, n) and not bits.any()
    e, inv = iu.expect_view_both(bits, codes)
    assert e.decode_ok == 1 and not inv
    # a mixed border: no codes in either mode
    m = np.zeros((n, n), np.uint8)
    m[0, :] = 1
    assert iu.expect_view_both(m, codes)[0].decode_ok == 0 and iu.expect_view_dark(m, codes)[0].decode_ok == 0
    m = np.ones((n, n), np.uint8)
    m[n - 1, 1] = 0
    assert iu.expect_view_both(m, codes)[0].decode_ok == 0
    # mode DARK never reads an all-lit border
    assert iu.expect_view_dark(np.ones((n, n), np.uint8), codes)[0].decode_ok == 0


def test_mixed_frames_hold_both_kinds_and_cut_no_marker(oracle):
    name = "ARUCO"
    nb, _, codes = du.table(name)
    tau = du.tau_of(name)
    frames, which = du.found_frames(name)
    frame, inv = iu.mixed(frames[0], len(which[0]), nb, 7)
    assert inv.any() and not inv.all()
    rects = iu.slot_rects(len(which[0]), nb)
    for a in range(len(rects)):
        for b in range(a + 1, len(rects)):
            (ax0, ay0, ax1, ay1), (bx0, by0, bx1, by1) = rects[a], rects[b]
            assert ax1 <= bx0 or bx1 <= ax0 or ay1 <= by0 or by1 <= ay0
    ref = oracle.detect(frame, codes, nb, tau, config=iu.oracle_config(oracle, True, nb))
    markers, idx, flags, _ = iu.expect_frame(oracle, ref, codes, nb, tau, True)
    squares = _squares(len(which[0]), nb)
    for m, k, fl in zip(markers, idx, flags):
        s = _slot_of(ref["candidates"][k], squares)
        if s is not None:
            assert bool(fl) == bool(inv[s])
    ps = du.patterns(name)
    for s, pi in enumerate(which[0]):
        if ps[pi].expect.accepted(tau, True):
            assert any(_slot_of(ref["candidates"][k], squares) == s for k in idx), s


def test_the_board_scene_holds_a_recovered_inverted_marker(oracle):
    """what tests/test_gpu_inverted.py holds the recovery path to: in frame 1 the damaged marker's quad reads inverted, is refused by
    the filter and is placed by the board; the notched marker's border is mixed and it stays out"""
    from tests import recover_cases
    from tests import recover_scene as rs

    b, frames = iu.board_scene()
    merged, per, rec, flags, decs = iu.expected_recovery(oracle, frames, b, rs.DICT, rs.oracle_config(oracle), 2, iu.RECOVER_DISTANCE_PX,
                                                         recover_cases.MAX_HAMMING)
    assert rec == [0, 1, 0] and per == [6, 5, 1]
    assert flags == [1] * len(merged) and decs == [2] * len(merged)
    tail = merged[per[0] + per[1] - 1]
    assert tail[1] == rs.FIRST_ID + rs.DAMAGED_SLOT and 0 < tail[4] <= recover_cases.MAX_HAMMING
    assert sorted(m[1] for m in merged[per[0]: per[0] + per[1]]) == [10, 11, 12, 13, 15]
