"""The board-aided marker recovery (a3_set_board_recovery / a3_recover_markers, include/aruco3_hip.h) without a GPU: the CPU
restatement tests/recover_oracle.c against designed lists whose outcome the contract fixes (tests/recover_cases.py), the derived
default of max_hamming against an exact binomial sum, the refusals of the Python front end, and the three declarations of the ABI
(header, ctypes, Rust) against each other.  tests/test_gpu_recover.py holds the device kernel to the same oracle on the same lists."""
import ctypes as C
import json
import math
import re
from pathlib import Path

import numpy as np
import pytest

from tests import recover_cases, recover_oracle

ROOT = Path(__file__).resolve().parent.parent
HEADER = ROOT / "include" / "aruco3_hip.h"
CASES = recover_cases.designed()


def exact_default(bits: int) -> int:
    """the largest h with P[a uniformly random `bits`-bit code lies within h of a fixed code] < 1e-3, in integers; 0 when none"""
    best = 0
    for h in range(bits + 1):
        if sum(math.comb(bits, k) for k in range(h + 1)) * 1000 < 2 ** bits:
            best = h
    return best


@pytest.mark.parametrize("case", CASES, ids=[c.name for c in CASES])
def test_designed_case(case):
    got = case.oracle()
    assert [(int(m["id"]), int(m["candidate_index"]), int(m["rotation"]), int(m["hamming_distance"])) for m in got] == case.expect
    for m in got:
        c, r = int(m["candidate_index"]), int(m["rotation"])
        assert int(m["frame"]) == 0
        assert np.array_equal(m["corners"].reshape(4, 2), np.roll(case.candidates[c], -r, axis=0))   # rotate_left(r)
        assert int(m["code"]) == (int(case.codes4[c, r]) if case.has_codes[c] else 0)
        if case.max_hamming != recover_cases.NO_BITS:
            slot_code = int(case.dictionary.code_list[int(m["id"])])
            assert int(m["hamming_distance"]) == bin(int(m["code"]) ^ slot_code).count("1") <= case.max_hamming


def test_designed_cases_cover_what_they_claim():
    names = {c.name for c in CASES}
    assert {"code_at_tau", "code_at_max_hamming", "code_beyond_max_hamming", "codeless_with_bits", "codeless_no_bits", "distance_at_bound",
            "distance_one_ulp_beyond", "four_shifts", "tie_lowest_candidate", "tie_lowest_shift", "claim_smaller_d2", "claim_tie_lowest_slot",
            "min_markers_not_met", "collinear_corners", "behind_the_camera"} <= names
    by = {c.name: c for c in CASES}
    # the two distance cases differ by one ulp of the bound and by nothing else
    a, b = by["distance_at_bound"], by["distance_one_ulp_beyond"]
    assert np.nextafter(np.float32(a.max_distance_px), np.float32(0)) == np.float32(b.max_distance_px)
    assert np.array_equal(a.candidates, b.candidates) and np.array_equal(a.detected_corners, b.detected_corners)
    # tau is what the decoder refuses, and the default takes it
    assert recover_cases.DICT._tau == recover_cases.TAU <= recover_cases.MAX_HAMMING
    # the collinear frame has no homography; the frame behind the camera has one, and skips the marker
    line = by["collinear_corners"]
    assert not recover_oracle.expected_corners(line.board, line.detected_ids, line.detected_corners, 1)[0]
    deep = by["behind_the_camera"]
    have, e, ok = recover_oracle.expected_corners(deep.board, deep.detected_ids, deep.detected_corners, deep.min_markers)
    assert have and not ok[4]
    assert recover_cases.pair_d2(e[4], deep.candidates[0], 0) <= deep.max_distance_px ** 2   # it would be taken, were it not skipped


def test_big_case_recovers_what_it_planted():
    case = recover_cases.big_case()
    got = case.oracle()
    assert len(case.board) == 1024 and len(case.candidates) == 2048
    assert 100 < len(got) < len(case.board) - len(case.detected_ids)   # damaged beyond the default and codeless quads stay out
    assert np.all(np.diff(got["candidate_index"].astype(np.int64)) > 0)   # candidate order
    assert np.unique(got["id"]).size == len(got) and not set(got["id"].tolist()) & set(case.detected_ids.tolist())


def test_rendered_frames_hold_what_they_were_drawn_for(oracle):
    """the three frames of tests/recover_scene.py through the CPU oracle: frame 1's damaged marker is refused by the decoder at
    distance tau and recovered under the derived default; its notched one has no code and is recovered only without bits"""
    from tests import recover_scene as rs

    for b, imgs in ((rs.board(), rs.frames()), (rs.charuco_board(), rs.charuco_frames())):
        merged, per, rec = rs.expected(oracle, imgs, b, 2, 10.0, recover_cases.MAX_HAMMING)
        assert (per, rec) == ([6, 5, 1], [0, 1, 0])
        tail = [t for t in merged if t[0] == 1][-1]
        assert (tail[1], tail[4]) == (int(b.ids[rs.DAMAGED_SLOT]), recover_cases.TAU)
        merged, per, rec = rs.expected(oracle, imgs, b, 2, 10.0, recover_cases.NO_BITS)
        assert (per, rec) == ([6, 6, 1], [0, 2, 0])
        assert [t[1] for t in merged if t[0] == 1][-2:] == [int(b.ids[rs.DAMAGED_SLOT]), int(b.ids[rs.NOTCHED_SLOT])]
        assert rs.expected(oracle, imgs, b, 5, 10.0, recover_cases.NO_BITS)[2] == [0, 0, 0]   # frame 1 shows four intact markers


def test_default_max_hamming_is_the_binomial_tail():
    index = json.loads((ROOT / "aruco3_amd" / "data" / "dictionaries.json").read_text())
    text = HEADER.read_text()
    stated = text[text.index("For the named dictionaries:"):]
    stated = re.sub(r"\n\s*\*", " ", stated[:stated.index("*/")])   # (the comment's line starts)
    groups = re.findall(r"(\d+) bits \(([^)]*)\) (\d+)", stated)
    assert len(groups) == 4
    named = {}
    for bits, names, h in groups:
        assert exact_default(int(bits)) == int(h) == recover_cases.DEFAULT_HAMMING[int(bits)], bits
        for n in re.split(r"[,\s]+", names.replace("APRILTAG_36H9 / 36H10 / 36H11", "APRILTAG_36H9, APRILTAG_36H10, APRILTAG_36H11")):
            if n:
                named[n] = int(bits)
    assert named == {k: v["num_bits"] for k, v in index.items()}   # every named dictionary, under its bit count
    assert [exact_default(b) for b in (1, 4, 9, 10)] == [0, 0, 0, 0]   # spaces too small for any h: exact matches only


def test_python_front_end_refusals():
    import aruco3_amd
    from aruco3_amd.aruco import Detector, Marker
    from aruco3_amd.board import BoardRecovery

    assert aruco3_amd.BoardRecovery is BoardRecovery and callable(aruco3_amd.recover_markers)
    r = BoardRecovery()
    assert (r.max_distance_px, r.max_hamming, r.min_markers) == (10.0, None, 2)
    for bad in (dict(max_distance_px=0.0), dict(max_distance_px=-1.0), dict(max_distance_px=float("nan")), dict(max_distance_px=float("inf")),
                dict(min_markers=0), dict(min_markers=1.5), dict(max_hamming=256), dict(max_hamming=-1), dict(max_hamming=2.5)):
        with pytest.raises(ValueError):
            BoardRecovery(**bad)
    with pytest.raises(ValueError, match="needs a board"):
        Detector(recovery=BoardRecovery())
    d = Detector(board=recover_cases.grid(), recovery=BoardRecovery(max_hamming=255))
    assert d.recovery.max_hamming == 255
    assert Marker(1, 2, [(0, 0)] * 4, 0).recovered is False


def _strip(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_header_ctypes_and_rust_agree():
    from aruco3_amd import _lib

    header = _strip(HEADER.read_text())
    body = re.search(r"typedef struct a3_recover_config \{(.*?)\} a3_recover_config;", header, flags=re.S).group(1)
    fields = [re.sub(r"\[.*?\]", "", d.split()[-1]) for d in body.split(";") if d.strip()]
    assert fields == ["mode", "min_markers", "max_distance_px", "max_hamming", "reserved"]
    assert [f[0] for f in _lib.RecoverConfig._fields_] == fields and C.sizeof(_lib.RecoverConfig) == 16
    assert _lib.RecoverConfig.max_distance_px.offset == 8 and _lib.RecoverConfig.max_hamming.offset == 12 and _lib.RecoverConfig.reserved.offset == 13
    rust = re.sub(r"//[^\n]*", "", (ROOT / "integration" / "aruco3_hip.rs").read_text())
    m = re.search(r"#\[repr\(C\)\]\s*#\[derive\([^\]]*\)\]\s*pub struct A3RecoverConfig \{(.*?)\}", rust, flags=re.S)
    assert re.findall(r"pub\s+([a-z0-9_]+)\s*:\s*([^,\n]+)", m.group(1)) == [("mode", "u32"), ("min_markers", "u32"), ("max_distance_px", "f32"),
                                                                              ("max_hamming", "u8"), ("reserved", "[u8; 3]")]
    L = _lib.load()
    arity = {"a3_default_recover_config": 2, "a3_set_board_recovery": 2, "a3_get_board_recovery": 2, "a3_get_recovered_counts": 3,
             "a3_recover_markers": 12}
    for name, n in arity.items():
        c = re.search(r"\b%s\s*\(([^;{]*?)\)\s*;" % name, header, flags=re.S).group(1)
        r = re.search(r"pub\s+fn\s+%s\s*\((.*?)\)\s*->\s*c_int;" % name, rust, flags=re.S).group(1)
        assert len(c.split(",")) == len(r.split(",")) == len(getattr(L, name).argtypes) == n, name
        assert name in _lib.SYMBOLS and getattr(L, name).restype is C.c_int
    assert re.search(r"#define A3_ABI_VERSION 5\b", header)   # additive: the version stays
    assert C.sizeof(_lib.MarkerRec) == recover_oracle.MARKER_DTYPE.itemsize == 56
