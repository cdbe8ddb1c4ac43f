"""The inputs of tests/test_gpu_frame_candidates.py, checked without a GPU: on every frame of every launch the numpy model of
discard_too_near (tests/candidates_util.py, written from src/aruco.rs:187-232) and the oracle keep the same quads, every builder
reaches the branch of the walk it was built for, and each of the kernel's three forms is fed every event of the census at least
once.  These are conditions on the inputs, fixed here; the GPU test relies on them and measures nothing of the kind."""
import numpy as np
import pytest

from tests import candidates_util as cu

LAUNCHES = sorted(cu.launches())


@pytest.mark.parametrize("name", LAUNCHES)
def test_model_and_oracle_keep_the_same_quads(name, oracle):
    L = cu.launches()[name]
    for fr, e in zip(L.frames, cu.expected(name, oracle)):
        if e is None:
            assert fr.count > L.max_cand and len(fr.records) == L.max_cand
            continue
        assert len(fr.records) == fr.count == len(e["sorted"])
        keys = fr.records["start_key"]
        assert len(np.unique(keys)) == len(keys)
        if fr.count >= 2:       # keys as the contour stage makes them: anywhere in u32, never the record order
            assert keys.min() == 0 and keys.max() == 0xFFFFFFFF and not np.all(np.diff(keys.astype(np.int64)) > 0)
        assert np.array_equal(e["kept"], e["model_kept"]), fr.name
        assert np.array_equal(e["fin"], e["sorted"][e["kept"]]), fr.name


def test_reference_vector_leaves_one(oracle):
    """test_drop_too_near, src/aruco.rs:446-459"""
    for keys in (np.arange(4), np.array([7, 0xFFFFFFFF, 0, 9])):
        _, kept, _ = cu.model(cu.REFERENCE_VECTOR, keys, 10.0)
        assert len(kept) == 1
    assert len(oracle.discard_too_near(cu.REFERENCE_VECTOR.astype(np.uint32), 10.0)[1]) == 1


def test_model_follows_the_walk_on_hand_made_rows():
    sq = cu.square
    # i (smaller) meets a bigger close j: i dies, j stays; a close smaller quad behind j survives row i and is killed by row j
    _, kept, c = cu.model(np.array([sq(100, 100, 40), sq(100, 100, 45), sq(100, 100, 38)]), [1, 2, 3], 25.0)
    assert kept.tolist() == [1] and c["i_dies"] == 1 and c["survivor_behind_bigger"] == 1 and c["kills_then_dies"] == 0
    # equal perimeters: the earlier one wins
    _, kept, c = cu.model(np.array([sq(100, 100, 40), sq(103, 100, 40)]), [5, 9], 25.0)
    assert kept.tolist() == [0] and c["ties"] == 1
    # keys decide the order, not the record order
    _, kept, _ = cu.model(np.array([sq(100, 100, 40), sq(103, 100, 40)]), [9, 5], 25.0)
    order, _, _ = cu.model(np.array([sq(100, 100, 40), sq(103, 100, 40)]), [9, 5], 25.0)
    assert order.tolist() == [1, 0] and kept.tolist() == [0]
    # strict <: a mean corner distance of exactly 5.0 is not close at 5.0
    pair = np.array([sq(100, 100, 40), np.array(sq(100, 100, 40)) + (3, 4)])
    assert cu.model(pair, [0, 1], 5.0)[1].tolist() == [0, 1] and cu.model(pair, [0, 1], 5.0)[2]["knife_pairs"] == 1
    assert cu.model(pair, [0, 1], cu.MIN_DISTANCES[4])[1].tolist() == [0]
    assert cu.model(pair, [0, 1], cu.MIN_DISTANCES[2])[1].tolist() == [0, 1]


def _census(name, frame_prefix, oracle):
    L = cu.launches()[name]
    hits = [(fr, e) for fr, e in zip(L.frames, cu.expected(name, oracle)) if fr.name.startswith(frame_prefix)]
    assert hits, (name, frame_prefix)
    return hits


MD = {md: m for m, md in enumerate(cu.MIN_DISTANCES)}


@pytest.mark.parametrize("form", ["reg", "lds", "big"])
def test_every_builder_reaches_what_it_is_for(form, oracle):
    at25 = f"builders_{form}_md{MD[25.0]}"
    for fr, e in _census(at25, "far_apart", oracle):                   # nothing close: nothing dies
        assert len(e["kept"]) == fr.count and e["census"]["i_dies"] == 0
    for fr, e in _census(at25, "clusters", oracle):                    # both directions of the comparison, dead quads met again
        assert e["census"]["i_dies"] >= 5 and e["census"]["kills_then_dies"] >= 1 and e["census"]["dead_j_skipped"] >= 1
    for fr, e in _census(at25, "ties", oracle):
        assert e["census"]["ties"] >= 10 and e["census"]["i_dies"] == 0
    for fr, e in _census(at25, "masked", oracle):                      # a dead bigger j in front of a row it would have killed
        assert e["census"]["dead_j_skipped_bigger"] == 1 and 1 in e["kept"]
        gap = int(fr.name.split("_")[1])
        assert form == "reg" or gap >= 63                                # j = 2 + gap: beyond row 1's first 64-quad trip from 64 on
    for fr, e in _census(at25, "late_bigger", oracle):
        c = e["census"]
        v = [int(x) for x in fr.name.split("_")[2:]]
        gap = v[0] if form == "reg" else 63 + 64 * v[0] + v[1]           # quads between i and the first bigger one, all killed by row i
        assert c["kills_then_dies"] >= (2 if gap else 1) and c["survivor_behind_bigger"] >= 1, fr.name
        assert c["i_dies_gap64"] == (gap >= 64) and c["i_dies_gap128"] == (gap >= 128), fr.name
    for md in (5.0, 10.0):                                               # the strict `<` at exactly the mean distance
        below, at, above = (f"builders_{form}_md{MD[md] + d}" for d in (-1, 0, 1))
        for (fr, eb), (_, ea), (_, eu) in zip(_census(below, "knife", oracle), _census(at, "knife", oracle), _census(above, "knife", oracle)):
            assert ea["census"]["knife_pairs"] >= 1
            assert np.array_equal(eb["kept"], ea["kept"]) and len(eu["kept"]) < len(ea["kept"]), fr.name
    for fr, e in _census(f"builders_{form}_md{MD[0.0]}", "duplicates", oracle):
        assert len(e["kept"]) == fr.count                                # 0 < 0.0 is false: all kept
    for fr, e in _census(f"builders_{form}_md{MD[cu.TINY]}", "duplicates", oracle):
        n_dup = int(np.count_nonzero((e["sorted"] == np.array(cu.square(700, 700, 33))).all(axis=(1, 2))))
        assert n_dup >= 20 and len(e["kept"]) == fr.count - n_dup + 1     # the first of them is kept
    for fr, e in _census(at25, "corners", oracle):
        assert e["sorted"].min() == 0 and e["sorted"].max() == 65535
    for fr, e in _census(f"builders_{form}_md{MD[1e9]}", "", oracle):   # everything is close to everything: one survivor
        assert len(e["kept"]) == 1


def test_shapes_cover_every_form_and_edge():
    from aruco3_amd import _lib

    assert _lib.CAND_DTYPE == cu.CAND_DTYPE and _lib.CAND_DTYPE.itemsize == 20 and _lib.PROJ_DTYPE.itemsize == 40    # a3_internal.h
    L = cu.launches()
    for table in cu.TABLES:
        counts = [fr.count for fr in L[f"sweep_{table}"].frames]
        assert set(cu.COUNTS + (table, table + 1)) <= set(counts), table
        assert set(cu.CLUSTER_COUNTS[table]) <= set(counts)
    assert sorted(c for t in cu.TABLES for c in cu.CLUSTER_COUNTS[t]) == [40, 64, 65, 300, 1500, 6144, 7000, 12288]
    for table in (1024, 6145):
        m = L[f"many_frames_{table}"]
        counts = [fr.count for fr in m.frames]
        assert len(counts) == 70 and m.S == 49 and counts.count(0) >= 2 and sum(c > table for c in counts) == 2
        assert set(counts) - {table + 1, table + 300} <= set(cu.COUNTS + (table,))
    assert L["builders_lds_md8_no_projections"].S == 0 and L["builders_lds_md8_no_projections"].frames is L["builders_lds_md8"].frames
    assert L["builders_lds_6144"].max_cand == cu.LDS_SLOTS and L["builders_big_md0"].max_cand == cu.LDS_SLOTS + 1
    assert max(len(fr.records) for l in L.values() for fr in l.frames) == 12288


# floors the GPU test relies on: every census event at least once in each form.  The register walk holds at most 64 quads, so a
# first bigger neighbour 64 or more places behind i cannot occur in it.
IMPOSSIBLE = {"reg": {"i_dies_gap64", "i_dies_gap128"}, "lds": set(), "big": set()}


def test_census_floors_per_kernel_form(oracle):
    total = cu.census_by_form(oracle)
    for form, census in total.items():
        print(form, census)
    for form, census in total.items():
        for key, n in census.items():
            if key in IMPOSSIBLE[form]:
                assert n == 0, (form, key)
            else:
                assert n >= 1, (form, key)
