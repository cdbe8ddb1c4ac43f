"""Designed lists for the board-aided marker recovery (a3_recover_markers, include/aruco3_hip.h): boards of 4-6 markers, at most 8
rejected quads each, and what the contract makes of them.  tests/test_oracle_recover.py holds the CPU oracle to the designed outcome,
tests/test_gpu_recover.py holds the device to the oracle on the same lists.  TEST INFRASTRUCTURE ONLY."""
from dataclasses import dataclass, field
from typing import List, Optional, Tuple

import numpy as np

from aruco3_amd.board import Board, GridBoard
from aruco3_amd.dictionaries import ARDictionary
from tests import recover_oracle

NO_BITS = recover_oracle.NO_BITS
DEFAULT_HAMMING = {16: 1, 25: 4, 36: 8, 64: 19}   # include/aruco3_hip.h, per bit count of the named dictionaries
DICT = ARDictionary.new_from_named_dict("ARUCO")   # 25 bits, tau 3
TAU = 3
MAX_HAMMING = DEFAULT_HAMMING[25]
BIG_DICT = ARDictionary.new_from_named_dict("ARTAG")   # 36 bits, 1024 codes: a board of A3_BOARD_MAX_MARKERS markers


CAMERA = ((3.1, 0.2, 120.0), (0.15, -2.9, 90.0), (0.0008, -0.0005, 1.0))
# a camera whose horizon crosses the board at X = 80, and which maps what lies behind it back into the frame
DEEP_CAMERA = ((-3.1, 0.2, 300.0), (-3.0, -2.9, 200.0), (-1.0 / 80.0, 0.0, 1.0))


def project(xy, m=CAMERA):
    """the designed camera: board (X, Y), y up -> pixels"""
    X, Y = np.asarray(xy, np.float64)[..., 0], np.asarray(xy, np.float64)[..., 1]
    u, v, w = (r[0] * X + r[1] * Y + r[2] for r in m)
    return np.stack([u / w, v / w], axis=-1)


def pixels(xy, m=CAMERA):
    return np.rint(project(xy, m)).astype(np.uint32)


@dataclass
class Case:
    name: str
    board: Board
    detected_ids: np.ndarray          # (n,)
    detected_corners: np.ndarray      # (n, 4, 2) uint32
    candidates: np.ndarray            # (m, 4, 2) uint32
    codes4: np.ndarray                # (m, 4) uint64
    has_codes: np.ndarray             # (m,) uint8
    min_markers: int = 2
    max_distance_px: float = 10.0
    max_hamming: int = MAX_HAMMING
    expect: List[Tuple[int, int, int, int]] = field(default_factory=list)   # (id, candidate_index, rotation, hamming_distance) in order
    dictionary: ARDictionary = DICT

    def oracle(self):
        return recover_oracle.recover_markers(self.board, self.dictionary.code_list, self.detected_ids, self.detected_corners, self.candidates, self.codes4,
                                              self.has_codes, self.min_markers, self.max_distance_px, self.max_hamming)


def flip(code: int, h: int) -> int:
    """`code` with its h lowest bits flipped"""
    return int(code) ^ ((1 << h) - 1)


def quad(corners, r: int, offset=(0, 0)):
    """a quad whose corner (j + r) mod 4 is corners[j] + offset: shift r aligns it with the board"""
    c = np.asarray(corners, np.int64) + np.asarray(offset, np.int64)
    return np.roll(c, r, axis=0).astype(np.uint32)


def codes_for(id_: int, r: int, h: Optional[int], dictionary: ARDictionary = DICT):
    """four rotated codes whose r-th is h bits from the marker's code and whose others are every bit away; h None: no codes"""
    if h is None:
        return [0, 0, 0, 0], 0
    far = int(dictionary.code_list[id_]) ^ ((1 << dictionary.num_bits) - 1)
    out = [far] * 4
    out[r] = flip(int(dictionary.code_list[id_]), h)
    return out, 1


def build(name, board, detected_slots, cands, g=CAMERA, **cfg) -> Case:
    """cands: (slot, shift, offset, hamming bits or None) per rejected quad, sitting at the designed camera's view of that board slot"""
    ids = np.asarray(board.ids, np.uint32)
    det = np.asarray(detected_slots, np.int64).reshape(-1)
    q, k, h = [], [], []
    for slot, r, offset, bits in cands:
        q.append(quad(pixels(board.corners[slot], g), r, offset))
        c4, has = codes_for(int(ids[slot]), r, bits)
        k.append(c4); h.append(has)
    return Case(name, board, ids[det], pixels(board.corners[det], g).reshape(-1, 4, 2), np.asarray(q, np.uint32).reshape(-1, 4, 2),
                np.asarray(k, np.uint64).reshape(-1, 4), np.asarray(h, np.uint8).reshape(-1), **cfg)


def grid():
    return GridBoard(3, 2, 40.0, 10.0)   # ids 0..5, slots = ids


def smallest_bound(d2: float) -> np.float32:
    """the smallest float f with (double)f * (double)f >= d2"""
    f = np.float32(np.sqrt(d2))
    while float(f) * float(f) < d2:
        f = np.nextafter(f, np.float32(np.inf))
    while float(np.nextafter(f, np.float32(0))) ** 2 >= d2:
        f = np.nextafter(f, np.float32(0))
    return f


def pair_d2(e, q, r: int) -> float:
    """d2(m, c, r) of the contract in the contract's arithmetic"""
    d2 = 0.0
    for j in range(4):
        s = (j + r) & 3
        dx, dy = float(e[j][0]) - float(q[s][0]), float(e[j][1]) - float(q[s][1])
        d = dx * dx + dy * dy
        d2 = d if d > d2 else d2
    return d2


def designed() -> List[Case]:
    out = []
    b = grid()
    det = [0, 1, 3, 4]
    # ---- the bit test ----
    out.append(build("code_at_tau", b, det, [(2, 1, (1, -1), TAU)], expect=[(2, 0, 1, TAU)]))
    out.append(build("code_at_max_hamming", b, det, [(2, 0, (0, 0), MAX_HAMMING)], expect=[(2, 0, 0, MAX_HAMMING)]))
    out.append(build("code_beyond_max_hamming", b, det, [(2, 0, (0, 0), MAX_HAMMING + 1)], expect=[]))
    wrong = build("wrong_shift_has_the_code", b, det, [(2, 0, (0, 0), 0)], expect=[])   # (the geometry fixes the rotation)
    wrong.codes4[0] = np.roll(wrong.codes4[0], 1)
    out.append(wrong)
    out.append(build("codeless_with_bits", b, det, [(2, 2, (0, 0), None)], expect=[]))
    out.append(build("codeless_no_bits", b, det, [(2, 2, (0, 0), None)], max_hamming=NO_BITS, expect=[(2, 0, 2, NO_BITS)]))
    out.append(build("coded_no_bits", b, det, [(5, 3, (2, 2), 25)], max_hamming=NO_BITS, expect=[(5, 0, 3, NO_BITS)]))
    # ---- the distance test: at the bound, and one ulp of the bound below it ----
    near = build("distance_at_bound", b, det, [(2, 0, (3, -4), 0)])
    have, e, ok = recover_oracle.expected_corners(b, near.detected_ids, near.detected_corners, near.min_markers)
    assert have and ok[2]
    bound = smallest_bound(pair_d2(e[2], near.candidates[0], 0))
    near.max_distance_px = float(bound)
    near.expect = [(2, 0, 0, 0)]
    out.append(near)
    far = build("distance_one_ulp_beyond", b, det, [(2, 0, (3, -4), 0)], max_distance_px=float(np.nextafter(bound, np.float32(0))), expect=[])
    out.append(far)
    # ---- every shift, several markers, quads that match nothing ----
    out.append(build("four_shifts", b, [0, 4], [(1, 0, (0, 1), 0), (2, 1, (1, 0), 1), (3, 2, (-1, 0), 2), (5, 3, (0, -1), 3),
                                                (1, 0, (40, 40), 0), (2, 0, (0, 0), None)],
                     expect=[(1, 0, 0, 0), (2, 1, 1, 1), (3, 2, 2, 2), (5, 3, 3, 3)]))
    # ---- ties of a marker's choice: the lowest candidate, then the lowest shift ----
    out.append(build("tie_lowest_candidate", b, det, [(2, 0, (40, 0), 0), (2, 1, (2, 1), 0), (2, 1, (2, 1), 0)], expect=[(2, 1, 1, 0)]))
    point = build("tie_lowest_shift", b, det, [(2, 0, (0, 0), None)], max_hamming=NO_BITS, max_distance_px=200.0, expect=[(2, 0, 0, NO_BITS)])
    point.candidates[0, :, :] = point.candidates[0, 0, :]   # four equal corners: every shift is equally far
    out.append(point)
    # ---- two missing markers claim one candidate ----
    out.append(build("claim_smaller_d2", b, det, [(2, 0, (1, 1), None)], max_hamming=NO_BITS, max_distance_px=400.0, expect=[(2, 0, 0, NO_BITS)]))
    c = np.asarray(b.corners, np.float32)
    twins = Board([0, 1, 3, 4, 9, 7], np.concatenate([c[[0, 1, 3, 4]], c[[2, 2]]]))   # ids 9 and 7 printed on the same spot
    out.append(build("claim_tie_lowest_slot", twins, [0, 1, 2, 3], [(5, 0, (1, 0), None)], max_hamming=NO_BITS, expect=[(9, 0, 0, NO_BITS)]))
    # ---- frames without a homography ----
    out.append(build("min_markers_not_met", b, [0], [(2, 0, (0, 0), 0)], expect=[]))
    out.append(build("min_markers_met_by_one", b, [0], [(1, 0, (0, 0), 0)], min_markers=1, max_distance_px=40.0, expect=[(1, 0, 0, 0)]))
    line = build("collinear_corners", b, [0], [(2, 0, (0, 0), 0)], min_markers=1, max_distance_px=1000.0, max_hamming=NO_BITS, expect=[])
    line.detected_corners[0] = np.array([(100, 100), (140, 120), (180, 140), (220, 160)], np.uint32)
    out.append(line)
    dup = build("repeated_id_is_not_used", b, [0, 1, 1], [(2, 0, (0, 0), 0)], expect=[])   # one usable marker is left: below min_markers
    out.append(dup)
    # ---- a board marker behind the camera: its quad sits exactly where the homography mirrors it to ----
    side = 16.0
    sq = lambda x, y: [(x, y), (x + side, y), (x + side, y - side), (x, y - side)]   # noqa: E731
    deep = Board([0, 1, 2, 3, 4], [sq(0, 0), sq(24, 0), sq(0, -24), sq(24, -24), sq(100, -12)])
    behind = build("behind_the_camera", deep, [0, 1, 2, 3], [(0, 0, (0, 0), None)], g=DEEP_CAMERA, max_hamming=NO_BITS, max_distance_px=4.0, expect=[])
    have, e, ok = recover_oracle.expected_corners(deep, behind.detected_ids, behind.detected_corners, behind.min_markers)
    assert have and not ok[4] and np.all(np.isfinite(e[4])) and np.all(e[4] >= 0) and np.all(e[4] < 65535)
    behind.candidates[0] = np.rint(e[4]).astype(np.uint32)   # feasible at once, were the marker not skipped
    out.append(behind)
    for case in out:
        assert 4 <= len(case.board) <= 6 and len(case.candidates) <= 8, case.name
    return out


def big_case(n_board: int = 1024, n_cand: int = 2048, seed: int = 7):
    """one frame beyond the LDS-sized cases: a 32 x 32 board of which every fourth marker is detected, its other markers' quads (shifted,
    some with damaged codes, some without codes) scattered among quads that match nothing"""
    rng = np.random.default_rng(seed)
    side = int(round(n_board ** 0.5))
    board = GridBoard(side, side, 4.0, 1.0)
    n_board = len(board)
    ids = np.asarray(board.ids, np.uint32)
    view = lambda xy: np.rint(np.stack([100.0 + 12.0 * np.asarray(xy)[..., 0] + 0.3 * np.asarray(xy)[..., 1],   # noqa: E731
                                        30.0 + 0.2 * np.asarray(xy)[..., 0] - 12.0 * np.asarray(xy)[..., 1]], axis=-1)).astype(np.uint32)
    det = np.arange(0, n_board, 4)
    missing = np.setdiff1d(np.arange(n_board), det)
    q = rng.integers(2500, 60000, size=(n_cand, 4, 2)).astype(np.uint32)   # far from the board's view
    k = rng.integers(0, 1 << 36, size=(n_cand, 4)).astype(np.uint64)
    h = np.ones(n_cand, np.uint8)
    where = rng.permutation(n_cand)[:missing.size]
    for slot, c in zip(missing, where):
        r = int(rng.integers(0, 4))
        q[c] = quad(view(board.corners[slot]), r, rng.integers(-2, 3, size=2))
        bits = int(rng.integers(0, 11))   # 9 and 10 are beyond the default
        c4, _ = codes_for(int(ids[slot]), r, bits, BIG_DICT)
        k[c] = c4
        if rng.integers(0, 8) == 0:
            h[c] = 0
    return Case("big", board, ids[det], view(board.corners[det]).reshape(-1, 4, 2), q, k, h, max_hamming=DEFAULT_HAMMING[36], dictionary=BIG_DICT)
