"""The decode stage's error-correcting lookup on DAMAGED markers, CPU half: the oracle against an expectation in plain numpy
(tests/damage_util.py), and the conditions on the inputs that keep this from thinning into another clean-marker test.
tests/test_gpu_decode_damage.py runs the same frames and quads through k_decode.

What every other test feeds the lookup is a clean marker: the minimum is 0 and unique, so neither tie rule (lowest index among
codes, earliest among rotations), nor the `< tau` boundary, nor the corner rotation under an inexact match can matter.  Counted once (a snapshot of this commit, asserted nowhere)
with the oracle over the synthetic frames the existing GPU tests decode -- BASELINE configs 1, 2, 4 and 5 (42, 32, 3 and 2 frames:
the most any test renders) and the 68 seeds of the config fuzz: 517 accepted markers, 495 of them at Hamming distance 0, 22 at a
distance above 0 (9 at 1, 4 at 2, 2 at 3, 7 between 5 and 10 under sigma 8 noise or odd sample sizes), 6 of those with a tied minimum, and
nothing placed at `tau - 1` / `tau` or at a lane-set, wave or trip boundary of the scan (`test_what_clean_frames_leave_out` keeps a
sample of that count in the suite).  Here (`pytest -rA` prints the table per dictionary; again a snapshot): 5376 patterns over 21 tables, 4567 of them
(85 %) at distance >= 1, up to 35 cells; 860 with the minimum tied over codes, 1038 with it tied over rotations; every pattern is shown
to the decoder from each of its four corners (21 504 quads handed in) and again through the contour stage (1484 frames).

Three families of frames (damage_util draws them):
  a  quads handed in (`oracle.detect(..., quads=)`, on the device `debug_inject_candidates`): the sampled bits are a known quantity,
     every quad's four codes must be the numpy rotations of the drawn pattern;
  b  the same drawings found by the contour stage, 66 frames or more per table: the expectation is per candidate, from the four codes
     it reports, and every drawn pattern must be among them;
  c  damaged tables through the synthetic renderer (rotation, perspective, noise, paper), detected with the TRUE table.
All equalities are exact.
"""
import numpy as np
import pytest

from tests import damage_util as du
from tests.util import markers_of_oracle


# ------------------------------------------------------------------------------------------------------------------
# the helper against the reference's own known answers (the ones test_oracle_kat.py quotes)
# ------------------------------------------------------------------------------------------------------------------
def test_helper_find_nearest_known_answers(dicts):
    """src/dictionaries.rs:245-281"""
    codes = dicts.new_from_named_dict("ARUCO_DEFAULT").code_list
    near = lambda c: du.find_nearest(codes, c)[:2]
    assert near(0x1084210) == (0, 0)
    assert near(0x1084209) == (2, 0)
    assert near(0b00000001_00001000_01000010_00001001) == (2, 0)
    assert near(0b00000001_00001000_01000010_10001001) == (2, 1)
    assert near(0x1084217) == (1, 0)
    idx, dist = near(0b01100001_00001000_01000010_00001001)          # try_find_nearest: a 2-bit error is inside tau = 3
    assert dist < 3 and idx == 2
    idx, dist = near(int("11111111" "0000100" "01000010" "00001001", 2))   # (the reference's literal, 7-digit group and all)
    assert not dist < 3
    assert du.numpy_tau(codes) == 3                                   # src/dictionaries.rs:239-243
    assert du.popcount(np.array([0xFFFFFFFF, 0xFFFFFFFFFFFFFFFF, 0], dtype=np.uint64)).tolist() == [32, 64, 0]   # src/lib.rs:28-40


def test_helper_bit_rotate_known_answers():
    """src/aruco.rs:414-444: rotate_bit_matrix is np.rot90(m, 1); the four codes are read row-major, first cell = most significant bit"""
    pre = np.array([[1, 1, 1], [1, 0, 0], [0, 1, 0]], dtype=np.uint8)
    post = np.array([[1, 0, 0], [1, 0, 1], [1, 1, 0]], dtype=np.uint8)
    assert np.array_equal(np.rot90(pre, 1), post)
    pre = np.array([[1, 1, 1, 1], [1, 1, 1, 0], [1, 1, 0, 0], [1, 0, 0, 0]], dtype=np.uint8)
    post = np.array([[1, 0, 0, 0], [1, 1, 0, 0], [1, 1, 1, 0], [1, 1, 1, 1]], dtype=np.uint8)
    assert np.array_equal(np.rot90(pre, 1), post)
    assert du.rotated_codes(pre) == [0b1111_1110_1100_1000, 0b1000_1100_1110_1111, 0b0001_0011_0111_1111, 0b1111_0111_0011_0001]
    assert du.code_of(du.matrix_of(0x1084217, 25)) == 0x1084217 and du.matrix_of(1 << 24, 25)[0, 0] == 1
    assert du.rotate_left([(0, 0), (1, 0), (1, 1), (0, 1)], 1) == ((1, 0), (1, 1), (0, 1), (0, 0))   # Vec::rotate_left


def test_helper_tie_rules():
    """lowest index among equal codes; the earliest among equal rotations; a later rotation only when strictly nearer"""
    sym = 0b000_010_000                                   # the same under every rotation
    e = du.expect_codes([sym] * 4, np.array([0b111_111_111, sym, sym], dtype=np.uint64))
    assert (e.id, e.distance, e.rotation, e.code_tie, e.tied, e.rotation_tie) == (1, 0, 0, True, (1, 2), True)
    e = du.expect_codes([0b11, 0b01, 0b00, 0b00], np.array([0], dtype=np.uint64))
    assert (e.rotation, e.distance, e.rotation_tie, e.code_tie) == (2, 0, True, False)
    lit = np.zeros((5, 5), np.uint8)
    lit[4, 2] = 1
    assert du.expect_view(lit, np.array([0], dtype=np.uint64)).decode_ok == 0


# ------------------------------------------------------------------------------------------------------------------
# conditions on the inputs, from numpy alone
# ------------------------------------------------------------------------------------------------------------------
def test_dictionaries_are_the_ones_named():
    from aruco3_amd.dictionaries import _load

    index, _ = _load()
    for name, count, bits, tau in (("APRILTAG_16H5", 30, 16, 5), ("ARUCO_MIP_16H3", 250, 16, 3), ("ARUCO", 1023, 25, 3), ("ARUCO_MIP_36H12", 250, 36, 12),
                                   ("APRILTAG_36H10", 2320, 36, 10), ("APRILTAG_36H9", 5329, 36, 9), ("CHILITAGS", 1024, 64, 5), ("ARTAG", 1024, 36, 0)):
        nb, t, codes = du.table(name)
        assert (len(codes), nb, t) == (count, bits, tau) == (index[name]["count"], index[name]["num_bits"], index[name]["tau"]), name
    assert [len(du.table(f"HAND_LEN_{n}")[2]) for n in du.HAND_LENGTHS] == [1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049]
    for name in du.HAND:
        codes = du.table(name)[2]
        if name != "HAND_DUPLICATES":
            assert len(set(codes.tolist())) == len(codes), name
    codes = du.table("HAND_DUPLICATES")[2]
    for lo, hi in du.DUPLICATES:
        assert codes[lo] == codes[hi] and int((codes == codes[lo]).sum()) == 2
    nb, _, codes = du.table("HAND_SELF_ROTATION")
    a, b = du.SELF_ROTATION
    assert du.code_of(np.rot90(du.matrix_of(codes[a], nb), 1)) == int(codes[b]) != int(codes[a])
    # ARTAG declares tau 0 = "compute it"; the table holds one code twice, so the minimum pairwise distance IS 0: with the filter on
    # nothing is ever accepted (`distance < 0`), and every pattern near that code is a tie between two indices
    codes = du.table("ARTAG")[2]
    assert du.tau_of("ARTAG") == du.numpy_tau(codes) == 0 and len(set(codes.tolist())) == len(codes) - 1


@pytest.mark.parametrize("name", du.ALL)
def test_patterns_cover_every_class_the_dictionary_admits(name):
    """per dictionary: a pattern in every class it admits, at least half of all patterns at distance >= 1; the report of `-rA`"""
    s = du.summary(name)
    ps = du.patterns(name)
    nb, _, codes = du.table(name)
    tau = du.tau_of(name)
    print(f"{name}: {len(codes)} codes of {nb} bits, tau {tau}: {s['patterns']} patterns, {s['damaged']} at distance >= 1 "
          f"({100.0 * s['damaged'] / s['patterns']:.0f} %), largest distance {s['max_distance']}, {s['code_ties']} with the minimum tied over codes, "
          f"{s['rotation_ties']} tied over rotations")
    print("   " + ", ".join(f"{k} {v}" for k, v in sorted(s["classes"].items())))
    missing = du.admitted_classes(name) - set(s["classes"])
    assert not missing, f"{name}: no pattern of class {sorted(missing)}"
    assert 2 * s["damaged"] >= s["patterns"]
    # the classes mean what they say (from numpy's lookup, not from how the pattern was made)
    for p in ps:
        e = p.expect
        if "boundary_accept" in p.tags:
            assert e.distance == tau - 1
        if "boundary_reject" in p.tags:
            assert e.distance == tau and not e.accepted(tau, True) and e.accepted(tau, False)
        if p.tags & {"border_left", "border_right", "border_top", "border_bottom"}:
            assert e.decode_ok == 0 and int(p.cells[1:-1, 1:-1].sum()) == int(p.cells.sum()) - 1
        if "code_tie" in p.tags:
            assert len(e.tied) > 1 and e.id == min(e.tied)
        for d in range(tau + 2):
            if f"flip_{d}" in p.tags:
                assert e.distance <= d
    if name == "HAND_DUPLICATES":
        for lo, hi in du.DUPLICATES:
            hit = [p for p in ps if f"duplicate_{lo}_{hi}" in p.tags]
            assert {p.expect.distance for p in hit if p.expect.id == lo and hi in p.expect.tied} >= {0, 1, 2}, (lo, hi)
            assert not [p for p in hit if p.expect.id == hi]
    if name == "HAND_SELF_ROTATION":
        hit = [p for p in ps if "self_rotation" in p.tags and "flip_0" in p.tags]
        assert hit and all(p.expect.rotation_tie and p.expect.distance == 0 for p in hit)
        assert {p.expect.id for p in hit} == set(du.SELF_ROTATION)
    if len(codes) > 2048:
        assert [p for p in ps if "code_tie_trips" in p.tags and p.expect.id < 2048]


def test_ties_over_the_whole_module():
    """at least 100 patterns whose minimum is not unique over codes and 20 whose minimum is not unique over rotations (there are
    about ten times as many); the named dictionaries alone yield them too"""
    tot = {k: sum(du.summary(n)[k] for n in du.ALL) for k in ("patterns", "damaged", "code_ties", "rotation_ties")}
    named = {k: sum(du.summary(n)[k] for n in du.NAMED) for k in ("code_ties", "rotation_ties")}
    print(f"all tables: {tot}; the named ones alone: {named}")
    assert tot["code_ties"] >= 100 and tot["rotation_ties"] >= 20
    assert named["code_ties"] >= 100 and named["rotation_ties"] >= 20
    assert 2 * tot["damaged"] >= tot["patterns"]


# ------------------------------------------------------------------------------------------------------------------
# family a: quads handed in
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", du.ALL)
def test_injected_quads_oracle_equals_numpy(oracle, name):
    """every quad's codes are the numpy rotations of the drawn pattern (no case dropped), decode_ok and the marker records are
    numpy's, filter on and off, L8 and RGB8"""
    nb, _, codes = du.table(name)
    tau = du.tau_of(name)
    n_quads = 0
    for img, quads, views, _ in du.injected_frames(name):
        exp = [du.expect_view(v, codes) for v in views]
        for filt in (True, False):
            want = [m for m in (du.expected_marker(e, q, tau, filt) for e, q in zip(exp, quads)) if m is not None]
            for frame in (img, du.as_rgb(img)):
                res = oracle.detect(frame, codes, nb, tau, config=du.oracle_config(oracle, filt, nb), quads=quads)
                assert res["candidates"].tolist() == quads.tolist()                # discard_too_near kept every quad, in order
                assert res["homography_ok"].all()
                assert res["decode_ok"].tolist() == [e.decode_ok for e in exp]
                assert [[int(c) for c in row] for row in res["codes"]] == [e.codes for e in exp]
                assert markers_of_oracle(res) == want
                assert [m["candidate_index"] for m in res["markers"]] == [k for k, e in enumerate(exp) if e.accepted(tau, filt)]
        n_quads += len(quads)
    assert n_quads == 4 * len(du.patterns(name))


# ------------------------------------------------------------------------------------------------------------------
# family b: the same drawings, found by the contour stage
# ------------------------------------------------------------------------------------------------------------------
def appears(p, square, res):
    """a drawn pattern is among a frame's candidates: its four codes from some corner, or, with a lit border cell, a candidate on
    its square (corners within two pixels) that fails the border test"""
    if p.expect.decode_ok:
        cs = p.expect.codes
        rows = {tuple(int(c) for c in r) for r, ok in zip(res["codes"], res["decode_ok"]) if ok}
        return any(tuple(cs[j:] + cs[:j]) in rows for j in range(4))
    sq = np.asarray(square, dtype=np.int64)
    for q, ok in zip(res["candidates"].astype(np.int64), res["decode_ok"]):
        if not ok and all(np.abs(sq - c).max(axis=1).min() <= 2 for c in q):
            return True
    return False


@pytest.mark.parametrize("name", du.ALL)
def test_found_quads_oracle_equals_numpy(oracle, name):
    nb, _, codes = du.table(name)
    tau = du.tau_of(name)
    ps = du.patterns(name)
    frames, which = du.found_frames(name)
    assert len(frames) >= 65 and len({f.tobytes() for f in frames}) == len(frames)        # more than 64 DIFFERENT frames: `few` is off
    assert set().union(*map(set, which)) == set(range(len(ps)))                            # every pattern is drawn
    seen = set()
    for f, img in enumerate(frames):
        squares = du.draw_frame([ps[i] for i in which[f]], nb, "b")[1]
        on = oracle.detect(img, codes, nb, tau, config=du.oracle_config(oracle, True, nb))
        off = oracle.detect(img, codes, nb, tau, config=du.oracle_config(oracle, False, nb))
        assert on["codes"].tolist() == off["codes"].tolist() and on["candidates"].tolist() == off["candidates"].tolist()
        for i, sq in zip(which[f], squares):
            assert appears(ps[i], sq, on), f"{name}: frame {f}: pattern {i} {sorted(ps[i].tags)} is not among the candidates"
            if not ps[i].expect.decode_ok:
                seen |= ps[i].tags
        for res, filt in ((on, True), (off, False)):
            want, idx, exps = du.expected_of_candidates(res, codes, tau, filt)
            assert markers_of_oracle(res) == want, (name, f, filt)
            assert [m["candidate_index"] for m in res["markers"]] == idx
        for e in exps:
            seen |= du.tags_of(e, tau)
    made = {t for p in ps for t in p.tags if t.startswith(("flip_", "orient_", "index_", "duplicate_", "self_", "all_", "searched_"))}
    missing = du.admitted_classes(name) - seen - made
    assert not missing, f"{name}: after detection no candidate of class {sorted(missing)}"


# ------------------------------------------------------------------------------------------------------------------
# family c: damaged tables through the renderer
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", du.FAMILY_C)
def test_rendered_damage_oracle_recovers_the_drawn_ids(oracle, name):
    """the nearest-code rule holds for every candidate; with sigma 0, at least 90 % of the drawn markers damaged by d < tau / 2 cells
    come back with the id that was drawn and hamming_distance == d (the rest: the reference's own drop-outs, quirks Q2 / Q3)"""
    nb, _, codes = du.table(name)
    tau = du.tau_of(name)
    damaged, d = du.damaged_table(name)
    assert du.popcount(damaged ^ codes).tolist() == d.tolist() and set(d.tolist()) == set(range(tau + 2))
    want = got = 0
    for sigma in (0, 6):
        for paper in (True, False):
            for img, truth in du.family_c_frames(name, sigma, paper):
                for filt in (True, False):
                    cfg = oracle.Config.default()
                    cfg.filter_high_bit_errors = int(filt)
                    cfg.min_corner_separation_factor = du.C_SEPARATION
                    res = oracle.detect(img, codes, nb, tau, config=cfg)
                    exp, idx, _ = du.expected_of_candidates(res, codes, tau, filt)
                    assert markers_of_oracle(res) == exp and [m["candidate_index"] for m in res["markers"]] == idx
                    if sigma == 0 and filt:
                        w, g = du.recovered(markers_of_oracle(res), truth, d, tau)
                        want += w
                        got += len(g)
    print(f"{name}: {got} of {want} drawn markers with d < tau / 2 recovered with their id and distance")
    assert want >= 20 and got >= 0.9 * want


# ------------------------------------------------------------------------------------------------------------------
# the gap this closes, as a count
# ------------------------------------------------------------------------------------------------------------------
def test_what_clean_frames_leave_out(oracle, dicts):
    """prints (`-rA`) what the frames the rest of the suite decodes give the lookup, here for BASELINE configs 1 and 2, five frames
    each: accepted markers by Hamming distance and how many of them have a tied minimum.  A report, not a bound on the renderer."""
    from aruco3_amd import synth

    d = dicts.new_from_named_dict("ARUCO_DEFAULT")
    hist, ties = {}, 0
    for config in (1, 2):
        frames, _ = synth.config_frames(config, 5)
        for img in frames:
            res = oracle.detect(img, d.code_list, d.num_bits, d._tau)
            for m in res["markers"]:
                hist[m["hamming_distance"]] = hist.get(m["hamming_distance"], 0) + 1
                e = du.expect_codes(res["codes"][m["candidate_index"]], d.code_list)
                ties += e.code_tie or e.rotation_tie
                assert (m["id"], m["hamming_distance"], m["rotation"]) == (e.id, e.distance, e.rotation)
    print(f"clean frames: accepted markers by Hamming distance {hist}, {ties} with a tied minimum")
    assert sum(hist.values()) > 0


# ------------------------------------------------------------------------------------------------------------------
# why families a and b do not run 36- and 64-bit tables at the default sample size
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ("ARUCO_MIP_36H12", "CHILITAGS"))
def test_default_sample_size_cannot_deliver_every_pattern(oracle, name):
    """damage_util.sample_size's reason, measured on the oracle: at homography_sample_size 49 some quads of family a are misread, and
    every misread cell is a WHITE cell that the triangle resize of the Otsu-binarised patch leaves at 127 or less (at exactly 126
    for the 36-bit table), never a black one read white; test_injected_quads_oracle_equals_numpy shows none at 48 / 50"""
    nb, _, codes = du.table(name)
    tau, n = du.tau_of(name), du.side_cells(nb) + 2
    cfg = du.oracle_config(oracle, True, nb)
    cfg.homography_sample_size = 49
    white, black, misread, total = [], [], 0, 0
    for img, quads, views, _ in du.injected_frames(name):
        res = oracle.detect(img, codes, nb, tau, config=cfg, quads=quads)
        for k, v in enumerate(views):
            patch = res["homographies"][k]
            r = oracle.resize_triangle((patch > oracle.otsu_level(patch)).astype(np.uint8) * 255, n, n)
            wrong = (r > 127) != (v == 1)
            e = du.expect_view(v, codes)
            if e.decode_ok:         # (a lit border cell leaves no codes to compare; the cells are still measured)
                assert bool(wrong.any()) == ([int(c) for c in res["codes"][k]] != e.codes or int(res["decode_ok"][k]) != 1)
            total += 1
            misread += bool(wrong.any())
            white += r[wrong & (v == 1)].tolist()
            black += r[wrong & (v == 0)].tolist()
    print(f"{name} at sample size 49: {misread} of {total} quads misread; white cells read at {sorted(set(white))}, black cells at {sorted(set(black))}")
    assert misread > 0 and not black and max(white) <= 127
    if nb == 36:
        assert set(white) == {126}
