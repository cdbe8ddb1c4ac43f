"""The inputs of tests/test_gpu_contour_quads.py, checked without a GPU (tests/quad_cases.py): the composition of the oracle's functions that
serves as the expectation IS the oracle's contour-to-candidate stage on whole scenes; the exact model of the kernel's Douglas-Peucker
keeps what the oracle keeps on every border; every table is inside the contract of a3_debug_contour_quads; and the borders make the kernel
execute every event of the census in both group widths.  Each plausible fault, switched on in the model, changes the expected output of
some border: that is why the GPU test would fail on a kernel with that fault.  These are conditions on the inputs, fixed here; the GPU test
relies on them and measures nothing of the kind.

Two things the census cannot hold, and why:
  * winding_flipped.  The hull (Graham scan, a stack kept while orientation == -1) leaves its four points with every turn
    (q - p) x (r - q) > 0, so for a strictly convex quad (p1 - p0) x (p2 - p0) > 0 too and enforce_clockwise_corners never swaps behind it:
    inside the range where the reference's 32-bit products are defined the winding fix of this stage is the identity, and dropping it
    changes no output (test_the_winding_fix_is_the_identity_behind_the_hull holds that on every case and on random quads; the fix itself
    has its own reference vectors through a3_debug_clockwise).
  * win_full_trip for the 16-lane form: its borders have at most 64 points, so a chord visits at most 63 and its one trip of 4 x 16
    is always a partial one."""
from fractions import Fraction

import numpy as np
import pytest

from tests import contour_scenes as S
from tests import quad_cases as qc

SCENES = ("prune_bound", "edges", "blobs_sparse", "nested_rings", "noise", "anomaly")


@pytest.mark.parametrize("scene", SCENES)
def test_composition_is_the_oracles_candidate_stage(scene, oracle, dicts):
    """expected_quad() over find_contours(thresholded) reproduces oracle.detect's candidates_pre, their order and its three reject counters"""
    h, w = 120, 160
    d = dicts.new_from_named_dict("ARUCO_DEFAULT")
    res = oracle.detect(S.SCENES[scene](h, w, 3), d.code_list, d.num_bits, d._tau)
    cs, _, _ = oracle.find_contours(res["thresholded"])
    assert len(cs) == res["n_contours"] and len(cs) > 3
    mel = S.min_edge_length(h, w)
    quads, starts, stats = [], [], {"reject_point_count": 0, "reject_convexity": 0, "reject_edge_length": 0, "accepted": 0}
    for c in cs:
        cls, quad = qc.expected_quad(oracle, c, 0.05, mel)
        stats[cls] += 1
        if quad is not None:
            quads.append(quad)
            starts.append(int(c[0][1]) * w + int(c[0][0]))
        assert qc.is_closed_walk(c)
        kept, mcls, mquad = qc.model(c, 0.05, mel, oracle=oracle)
        assert mcls == cls and (quad is None or np.array_equal(mquad, quad))
    assert (stats["reject_point_count"], stats["reject_convexity"], stats["reject_edge_length"]) == res["stats"]
    assert np.array_equal(np.array(quads, dtype=np.int64).reshape(-1, 4, 2), res["candidates_pre"])
    assert starts == res["candidates_pre_start"].tolist()


def test_model_and_oracle_keep_the_same_indices(oracle):
    cases = qc.distinct_cases()
    assert len(cases) > 3000
    for name, b, ef, mel in cases:
        kept, cls, quad = qc.model(b.pts, ef, mel, oracle=oracle)
        ecls, equad = qc.border_result(b, ef, mel)
        assert cls == ecls and (equad is None or np.array_equal(quad, equad)), (name, b.name)
        want = qc.oracle_kept(oracle, b.pts, ef)
        if kept is None:                         # the kernel stops at the fourth split: the oracle goes on to five vertices or more
            assert len(want) > 4, (name, b.name)
        else:
            assert [0] + sorted(kept) == want, (name, b.name)


@pytest.mark.parametrize("name", sorted(qc.launches()))
def test_every_table_is_inside_the_hooks_contract(name):
    L = qc.launches()[name]
    rec, pool = L.tables()
    assert 1 <= L.width <= 65536 and 1 <= L.height <= 65536 and 1 <= L.max_cand <= 65536 and L.n_frames >= 1
    assert (L.first_frame + L.n_frames) * L.max_cand <= 1 << 24 and len(pool) < 1 << 30
    n, base, frame = rec["n"].astype(np.int64), rec["point_base"].astype(np.int64), rec["frame"].astype(np.int64)
    assert (n >= 1).all() and (base + n <= len(pool)).all()
    assert ((frame >= L.first_frame) & (frame < L.first_frame + L.n_frames)).all()
    assert ((pool & 0xFFFF) < L.width).all() and ((pool >> 16) < L.height).all()
    pairs = frame << 32 | rec["start_key"].astype(np.int64)
    assert len(np.unique(pairs)) == len(pairs)
    assert not np.all(np.diff(rec["start_key"].astype(np.int64)) > 0) or len(rec) < 3          # keys are not the record order
    assert min(L.ctr_contours, L.max_contours) <= len(rec)
    for frame_, b in L.borders:
        assert b.pts.min() >= 0 and qc.is_closed_walk(b.pts), b.name
    for f, e in qc.expected(name).items():                # what the reference's 32-bit dx*dx + dy*dy can hold
        q = e[:, 1:].reshape(-1, 4, 2)
        assert (np.abs(q - np.roll(q, 1, axis=1)) < 1 << 15).all()


def test_walks_are_what_they_claim():
    assert qc.is_closed_walk([(0, 0), (1, 1), (2, 1), (1, 0)]) and not qc.is_closed_walk([(0, 0), (2, 0), (1, 1)])
    assert not qc.is_closed_walk([(0, 0), (1, 0), (2, 0), (3, 0)])            # open: the last and the first are apart
    w = qc.walk(qc.BIG_QUAD)
    assert qc.is_closed_walk(w) and 65000 < len(w) < 66000 and w.max() == 16383 and w.min() == 3
    for v in qc.BIG_QUAD:                       # every vertex is visited exactly
        assert (w == v).all(axis=1).any()
    lg = qc.large_walks()
    assert lg["far_quad"].pts.max(axis=0).tolist() == [65535, 65535] and np.ptp(lg["far_quad"].pts, axis=0).max() < 1 << 15
    assert lg["far_pentagon"].pts.max(axis=0).tolist() == [65535, 65535] and np.ptp(lg["far_pentagon"].pts, axis=0).max() < 1 << 15


def test_lengths_orientations_and_both_border_kinds():
    sb = qc.small_borders()
    for n in qc.LENGTHS_16 + qc.LENGTHS_64:
        got = [b for name, b in sb.items() if name.startswith(f"block{n}_o")]
        assert len(got) == 8 and all(b.n == n for b in got), n
    assert {1, 2, 3, 4, 5, 6, 7, 8, 16, 17, 18, 32, 33, 34, 48, 49, 50, 63, 64} <= set(qc.LENGTHS_16)
    assert {65, 66, 128, 129, 130, 255, 256, 257, 258, 511, 512, 513, 514, 1025, 1026, 4097} <= set(qc.LENGTHS_64)
    assert qc.block(64).shape == (17, 17) and sorted(qc.block(66).shape) == [17, 18]
    holes = [b for name, b in sb.items() if "_hole_" in name]
    assert sum(b.n <= 64 for b in holes) >= 50 and sum(b.n > 64 for b in holes) >= 50          # hole borders in both group widths
    # the eight orientations differ in start, direction of travel and the signs of the numerators
    tri = [sb[f"triangle_s2_o{k}"].pts for k in range(8)]
    assert len({t.tobytes() for t in tri}) == 8
    signs = set()
    for t in tri:
        d = np.roll(t, -1, axis=0) - t
        signs.add(int(np.sign((d[:, 0] * np.roll(d[:, 1], -1) - d[:, 1] * np.roll(d[:, 0], -1)).sum())))
    assert signs == {1} or signs == {-1}        # outer borders all travel one way round; the hole borders travel the other way
    d = np.roll(sb["triangle_s2_hole_o0"].pts, -1, axis=0) - sb["triangle_s2_hole_o0"].pts
    assert int(np.sign((d[:, 0] * np.roll(d[:, 1], -1) - d[:, 1] * np.roll(d[:, 0], -1)).sum())) not in signs


# (w, h, b, bw, px) -> n, (num, den) of the band chord, ratio - 1 (exact), class
BUMP_FACTS = {
    (3, 6, 4, 1, 1): (20, (1, 1), Fraction(0), "reject_point_count"),
    (8, 2, 3, 1, 3): (20, (5, 25), Fraction(0), "reject_convexity"),
    (9, 2, 2, 4, 4): (20, (5, 25), Fraction(0), "accepted"),
    (4, 15, 4, 1, 2): (40, (2, 1), Fraction(0), "reject_point_count"),
    (5, 24, 4, 1, 3): (60, (3, 1), Fraction(0), "reject_point_count"),
    (6, 33, 4, 1, 4): (80, (4, 1), Fraction(0), "reject_point_count"),
    (10, 39, 4, 1, 5): (100, (5, 1), Fraction(0), "reject_point_count"),
    (5, 12, 4, 1, 3): (36, (9, 25), Fraction(-81064793292668929, 1642875177895785385404520646836225), "accepted"),
    (8, 9, 4, 1, 3): (36, (9, 25), Fraction(-81064793292668929, 1642875177895785385404520646836225), "reject_point_count"),
    (6, 2, 3, 3, 1): (16, (4, 25), Fraction(-36028797018963969, 324518553658426762811953039540225), "reject_point_count"),
    (6, 9, 4, 4, 1): (32, (8, 25), Fraction(-36028797018963969, 324518553658426762811953039540225), "accepted"),
    (7, 5, 3, 3, 1): (24, (6, 25), Fraction(-13510798882111489, 45635421608216271964680197505025), "accepted"),
}
# index into WALK_BAND_CASES -> n, (num, den), ratio - 1, class
WALK_FACTS = {
    0: (172, (430, 2500), Fraction(48413695994232831, 585971489955498992428155062452225), "accepted"),
    1: (172, (430, 2500), Fraction(48413695994232831, 585971489955498992428155062452225), "reject_point_count"),
    2: (55, (99, 225), Fraction(37154696925806591, 345117875912135417402780521857025), "accepted"),
    3: (55, (99, 225), Fraction(37154696925806591, 345117875912135417402780521857025), "reject_point_count"),
    4: (72, (36, 100), Fraction(-81064793292668929, 1642875177895785385404520646836225), "accepted"),
    5: (84, (42, 100), Fraction(-47287796087390209, 559033914700649213347842200961025), "accepted"),
    6: (84, (42, 100), Fraction(-47287796087390209, 559033914700649213347842200961025), "reject_point_count"),
}


def test_band_cases_are_band_cases(oracle):
    """each committed border makes Douglas-Peucker evaluate exactly one chord inside the band, with the ratio stated"""
    sb = qc.small_borders()
    assert set(BUMP_FACTS) == set(qc.BUMP_BAND_CASES) and len(WALK_FACTS) == len(qc.WALK_BAND_CASES)
    rows = []
    for c, (n, chord, off, cls) in BUMP_FACTS.items():
        b, log = sb["bump_%d_%d_%d_%d_%d" % c], []
        got = qc.model(b.pts, 0.05, 0, oracle=oracle, band_log=log)
        assert b.n == n and [(num, den) for num, den, _ in log] == [chord] and log[0][2] - 1 == off and got[1] == cls, c
        rows.append((b.name, 0.05, n, chord, off, cls))
    walks = {b.name: (ef, b) for ef, bs in qc.hand_walks().items() for b in bs}
    for i, (n, chord, off, cls) in WALK_FACTS.items():
        ef, b = walks[f"walk_band_{i}"]
        log = []
        got = qc.model(b.pts, ef, 0, oracle=oracle, band_log=log)
        assert ef == qc.WALK_BAND_CASES[i][0] and b.n == n and [(num, den) for num, den, _ in log] == [chord] and log[0][2] - 1 == off and got[1] == cls, i
        # the double n * eps_factor lies below the rational: exactly far, not far by the reference's expression, far by the squared doubles
        if i < 4:
            assert off > 0 and qc.model(b.pts, ef, 0, mutant="band_squared_only", oracle=oracle)[1] != cls
        else:
            assert off < 0
        rows.append((b.name, ef, n, chord, off, cls))
    for r in rows:
        print("band case %-22s eps_factor %.2f n %3d (num, den) %-12s ratio - 1 = %+.3e  %s" % (r[0], r[1], r[2], r[3], float(r[4]), r[5]))
    for lo, hi in ((1, 64), (65, 1 << 30)):          # ratio exactly 1 and ratio off 1, chords along an axis and in a 3-4-5 direction
        mine = [r for r in rows if lo <= r[2] <= hi]
        assert any(r[4] == 0 for r in mine) and any(r[4] != 0 for r in mine)
    assert {r[2] for r in rows if r[4] == 0} >= {20, 40, 60, 100} and {r[2] for r in rows if r[4] < 0} >= {36, 72, 84} and any(r[2] == 36 and r[5] == "accepted" for r in rows)
    assert any(r[3][1] == 1 for r in rows) and any(r[3][1] == 25 for r in rows)


def test_launch_structure(oracle):
    L = qc.launches()
    # both widths in one launch, interleaved, more borders than groups of either width at the smallest grid
    for name in ("mixed_min_grid", "mixed_max_grid"):
        n = np.array([b.n for _, b in L[name].borders])
        short = n <= qc.K_SMALL
        assert (~short).sum() > qc.MIN_GRID[0] and short.sum() > qc.MIN_GRID[1] and len(n) > qc.MIN_GRID[1]
        assert np.count_nonzero(short[1:] != short[:-1]) > 300
        assert L[name].first_frame == 2 and L[name].n_frames == 3 and {f for f, _ in L[name].borders} == {2, 3, 4}
        frames = np.array([f for f, _ in L[name].borders])
        assert np.count_nonzero(frames[1:] != frames[:-1]) > 500
        assert all(len(e) > 100 for e in qc.expected(name).values())
    a, b = L["mixed_min_grid"], L["mixed_max_grid"]
    assert a.n_darts == 0 and b.n_darts == 1 << 23 and a.borders is b.borders and np.array_equal(a.keys, b.keys)
    # one wave, four unlike borders
    classes = [qc.border_result(bd, 0.05, 0)[0] for _, bd in L["neighbours"].borders[:4]]
    assert [bd.n for _, bd in L["neighbours"].borders[:4]] == [1, 32, 22, 36] and classes == ["reject_point_count", "accepted", "reject_point_count", "accepted"]
    cen = qc.new_census()
    log = []
    qc.model(L["neighbours"].borders[2][1].pts, 0.05, 0, census=cen, oracle=oracle)
    qc.model(L["neighbours"].borders[3][1].pts, 0.05, 0, oracle=oracle, band_log=log)
    assert cen["fourth_split_with_work_left"] == 1 and len(log) == 1
    # tables cut short by either count
    for name in ("max_contours_below", "ctr_contours_below"):
        assert 100 < L[name].considered() < len(L[name].borders) and 100 < len(qc.expected(name)[0]) < len(qc.expected("small_near")[0])
    assert L["max_contours_below"].max_contours < len(L["max_contours_below"].borders) == L["max_contours_below"].ctr_contours
    assert L["ctr_contours_below"].ctr_contours < len(L["ctr_contours_below"].borders) == L["ctr_contours_below"].max_contours
    # one frame of three overflows its table
    e = qc.expected("cand_overflow")
    assert len(e[1]) > L["cand_overflow"].max_cand and 0 < len(e[0]) <= L["cand_overflow"].max_cand and 0 < len(e[2]) <= L["cand_overflow"].max_cand
    # stale tables: flags set, borders that would yield quads
    for name in ("stale_point_pool", "stale_contour_table"):
        assert L[name].considered() == 0 and len(qc.expected(name)[0]) == 0
        assert sum(qc.border_result(bd, 0.05, 0)[1] is not None for _, bd in L[name].borders) > 50
        assert L[name].ctr_contours == len(L[name].borders)          # nothing beyond the table: a kernel that read on would still read records
    # the edge filter flips on the same borders, in both widths
    e0, eq, plus = qc.expected("mel_0")[0], qc.expected("mel_eq")[0], qc.expected("mel_plus1")[0]
    assert len(e0) == len(L["mel_0"].borders) and sorted(e0[:, 1:].tolist()) == sorted(eq[:, 1:].tolist()) and len(plus) == 0
    q = e0[:, 1:].reshape(-1, 4, 2)
    assert (((q - np.roll(q, 1, axis=1)) ** 2).sum(axis=2).min(axis=1) == qc.MEL_SIDE).all()
    assert {qc.width_of(bd.n) for _, bd in L["mel_eq"].borders} == {16, 64}
    # 24-bit and 64-bit numerators on the same walks; the pentagons are rejected
    assert (L["large_14"].width, L["large_64"].width) == (16384, 16385) and L["large_14"].borders == L["large_64"].borders
    for name in ("large_14", "large_64", "large_far"):
        assert len(qc.expected(name)[0]) == 1
        assert [qc.border_result(bd, 0.05, 1000)[0] for _, bd in L[name].borders] == ["accepted", "reject_point_count"]
    assert np.array_equal(qc.expected("large_14")[0][:, 1:], qc.expected("large_64")[0][:, 1:])
    pool = L["small_far14"].tables()[1]
    assert (pool & 0xFFFF).max() == 16383 and (pool >> 16).max() == 16383
    pool = L["small_far64"].tables()[1]
    assert (pool & 0xFFFF).max() == 65535 and (pool >> 16).max() == 65535


def test_the_winding_fix_is_the_identity_behind_the_hull(oracle):
    rng = np.random.default_rng(5)
    n_hulls = 0
    quads = [q for _, b, ef, mel in qc.distinct_cases() for q in [qc.border_result(b, ef, mel)[1]] if q is not None]
    for _ in range(4000):
        ext = int(rng.choice([4, 40, 3000, 32767]))
        quads.append(rng.integers(0, ext + 1, size=(4, 2)) + int(rng.integers(0, 65536 - ext)))
    for q in quads:
        hull = oracle.convex_hull(np.asarray(q, dtype=np.uint32))
        if len(hull) == 4:
            n_hulls += 1
            assert np.array_equal(oracle.enforce_clockwise_corners(hull)[0], hull)
    assert n_hulls > 3000


# What the committed cases make the kernel execute, per group width, as model() counts it: the floors of test_census_floors.
FLOORS = {
    16: {"borders": 2222, "chords": 13385, "chords_zero": 3451, "chords_pa_eq_pb": 38, "band_ratio_one": 50, "band_ratio_not_one": 44,
         "tie_chords": 3504, "win_u0": 5701, "win_u1": 694, "win_u2": 44, "win_u3": 4, "win_last_partial_trip": 6443, "win_full_trip": 0,
         "fourth_split_with_work_left": 292, "reject_point_count": 1343, "reject_convexity": 143, "reject_edge_length": 3, "accepted": 733,
         "winding_flipped": 0},
    64: {"borders": 1030, "chords": 6478, "chords_zero": 1516, "chords_pa_eq_pb": 3, "band_ratio_one": 6, "band_ratio_not_one": 15,
         "tie_chords": 1732, "win_u0": 2217, "win_u1": 637, "win_u2": 114, "win_u3": 102, "win_last_partial_trip": 2620, "win_full_trip": 450,
         "fourth_split_with_work_left": 118, "reject_point_count": 453, "reject_convexity": 83, "reject_edge_length": 4, "accepted": 490,
         "winding_flipped": 0},
}
IMPOSSIBLE = {16: {"win_full_trip", "winding_flipped"}, 64: {"winding_flipped"}}       # (module docstring)
SPANS = {16: {1, 15, 16, 17, 63}, 64: {1, 63, 64, 65, 255, 256, 257, 511, 512, 513}}   # points a chord's arg-max visits: 1, G-1, G, G+1, 4G-1, 4G, 4G+1 ...


def _census(oracle):
    cen = {16: qc.new_census(), 64: qc.new_census()}
    for w in cen:
        cen[w]["_spans"] = set()
    for _, b, ef, mel in qc.distinct_cases():
        qc.model(b.pts, ef, mel, census=cen[qc.width_of(b.n)], oracle=oracle)
    return cen


def test_census_floors_per_group_width(oracle):
    cen = _census(oracle)
    print("%-28s %8s %8s" % ("event", "16-lane", "wave"))
    for key in qc.CENSUS_KEYS:
        print("%-28s %8d %8d" % (key, cen[16][key], cen[64][key]))
    for w in (16, 64):
        assert SPANS[w] <= cen[w]["_spans"], (w, sorted(SPANS[w] - cen[w]["_spans"]))
        for key in qc.CENSUS_KEYS:
            if key in IMPOSSIBLE[w]:
                assert cen[w][key] == 0, (w, key)
            else:
                assert cen[w][key] >= max(1, FLOORS[w][key]), (w, key, cen[w][key])


@pytest.mark.parametrize("mutant", qc.MUTANTS)
def test_every_fault_changes_some_expected_output(mutant, oracle):
    hits = {16: [], 64: []}
    for name, b, ef, mel in qc.distinct_cases():
        _, cls, quad = qc.model(b.pts, ef, mel, mutant=mutant, oracle=oracle)
        ecls, equad = qc.border_result(b, ef, mel)
        if cls != ecls or (equad is not None and not np.array_equal(quad, equad)):
            hits[qc.width_of(b.n)].append(b.name)
    print("mutant %-24s changes %4d 16-lane and %4d wave borders, e.g. %s" % (mutant, len(hits[16]), len(hits[64]), (hits[16] + hits[64])[:2]))
    if mutant == "no_winding_fix":      # the identity behind a hull (module docstring): no border can tell
        assert not hits[16] and not hits[64]
    else:
        assert hits[16] and hits[64]
