"""k_frame_candidates as the pipeline launches it (a3_debug_frame_candidates: one call of launch_frame_candidates), held against the
oracle on hand-made candidate tables, exactly: integers and bits.  Per frame pre_xy is the quads sorted by start key; fin_count and
fin_xy are oracle.discard_too_near's survivors in order (tests/candidates_util.py's numpy model is the second opinion: the CPU test
tests/test_candidate_cases.py holds the two equal on these very inputs); an overflowed frame yields nothing; the work list tiles
[0, sum fin_count) with one contiguous range f*max_cand + 0, 1, 2 ... per frame; with S = 49 proj[w] is
oracle.from_control_points of the quad at work index w, flag and inverse bit for bit (the inverse is compared where the flag is
set: a failed solve leaves it unwritten).  Every slot the kernel has no business writing must come back as the 0xFF the hook
filled it with.

All three forms of the walk -- registers (2..64 quads), LDS (65 and more, tables up to 6144), through memory (tables above) -- get
every builder at every min_distance (0.0, the smallest positive float, 5.0 and 10.0 with their float32 neighbours, 25.0, 1e9), the
counts 0, 1, 2, 3, 63..66, 127..129, 1024, max_cand, max_cand + 1 in tables of 1024, 6144, 6145 and 12288, clusters of 40 to 12288
quads, and two launches of 70 frames.  What the walks execute on these inputs (tests/test_candidate_cases.py prints and floors it):

  form  i_dies  gap>=64  gap>=128  kills_then_dies  survivor_behind_bigger  dead_j_skipped  ..._bigger   ties  knife_pairs
  reg      695        0         0              331                     546             642         636    743          675
  lds     7033     4250      3335             3675                    6314            7837        7637   3904        12275
  big    17720    14992     13833             9251                   16285           16879       16673   3061        12268

(the register walk holds 64 quads: no gap of 64 exists in it).  GPU only."""
import numpy as np
import pytest

from tests import candidates_util as cu

pytestmark = pytest.mark.gpu
LAUNCHES = list(cu.launches())


@pytest.fixture(scope="module")
def ctx(dicts):
    from aruco3_amd.aruco import Detector, DetectorConfig

    return Detector(DetectorConfig(), dicts.new_from_named_dict("ARUCO"))._context()


_ran = {}


def _run(ctx, name):
    """one launch of the kernel per name, shared by the tests that look at it"""
    if name not in _ran:
        L = cu.launches()[name]
        counts = np.array([fr.count for fr in L.frames], dtype=np.uint32)
        records = np.concatenate([fr.records for fr in L.frames])
        _ran[name] = ctx.debug_frame_candidates(counts, records, L.max_cand, L.min_distance, L.S)
    return _ran[name]


def _check(L, got, want, oracle):
    n, mc = len(L.frames), L.max_cand
    assert got["pre_xy"].shape == (n, mc, 8) and got["fin_count"].shape == (n,)
    fin_count = got["fin_count"].astype(np.int64)
    for f, (fr, e) in enumerate(zip(L.frames, want)):
        pre, fin = got["pre_xy"][f], got["fin_xy"][f]
        if e is None:                                       # overflowed: nothing ordered, nothing kept
            assert fin_count[f] == 0, (fr.name, fin_count[f])
            assert (pre == 0xFFFF).all() and (fin == 0xFFFF).all(), fr.name
            continue
        c, m = fr.count, len(e["kept"])
        assert np.array_equal(pre[:c].reshape(c, 4, 2), e["sorted"]), fr.name
        assert (pre[c:] == 0xFFFF).all(), fr.name
        assert fin_count[f] == m, (fr.name, int(fin_count[f]), m)
        assert np.array_equal(fin[:m].reshape(m, 4, 2), e["fin"]), fr.name
        assert np.array_equal(e["kept"], e["model_kept"]), fr.name
        assert (fin[m:] == 0xFFFF).all(), fr.name
    # the work list: sum fin_count entries, one contiguous range per frame, in whatever order the frames arrived
    total = int(fin_count.sum())
    work = got["work"].astype(np.int64)
    assert got["work_count"] == total
    assert (work[total:] == 0xFFFFFFFF).all()
    frames_of, pos_of = work[:total] // mc, work[:total] % mc
    starts = {}
    covered = np.zeros(total, dtype=bool)
    for f in np.nonzero(fin_count)[0]:
        w = np.nonzero(frames_of == f)[0]
        assert len(w) == fin_count[f] and np.array_equal(w, np.arange(w[0], w[0] + len(w))), L.frames[f].name
        assert np.array_equal(pos_of[w], np.arange(len(w))), L.frames[f].name
        starts[int(f)] = int(w[0])
        covered[w] = True
    assert covered.all()
    if not L.S:
        assert got["proj"] is None
        return
    proj = got["proj"]
    assert (proj[total:].view(np.uint8) == 0xFF).all()
    S = np.float32(L.S)
    to = np.array([0, 0, S, 0, S, S, 0, S], dtype=np.float32)
    solved = {}
    for f, w0 in starts.items():
        for pos, quad in enumerate(want[f]["fin"].reshape(-1, 8)):
            key = quad.tobytes()
            if key not in solved:
                ok, _, inv = oracle.from_control_points(quad.astype(np.float32), to)
                solved[key] = (int(ok), inv.view(np.uint32).copy())
            ok, inv = solved[key]
            r = proj[w0 + pos]
            assert int(r["ok"]) == ok, (L.frames[f].name, pos, quad)
            if ok:
                assert np.array_equal(r["inv"].view(np.uint32), inv), (L.frames[f].name, pos, quad, r["inv"], inv.view(np.float32))


@pytest.mark.parametrize("name", LAUNCHES)
def test_frame_candidates_equal_the_oracle(name, ctx, oracle):
    L = cu.launches()[name]
    _check(L, _run(ctx, name), cu.expected(name, oracle), oracle)


def test_without_projections_the_rest_is_unchanged(ctx, oracle):
    a, b = _run(ctx, "builders_lds_md8"), _run(ctx, "builders_lds_md8_no_projections")
    assert a["proj"] is not None and b["proj"] is None
    for k in ("pre_xy", "fin_xy", "fin_count"):
        assert np.array_equal(a[k], b[k]), k
    assert a["work_count"] == b["work_count"] and np.array_equal(np.sort(a["work"]), np.sort(b["work"]))


def test_reference_vector_through_shuffled_keys(ctx, oracle):
    """test_drop_too_near (src/aruco.rs:446-459) leaves one quad -- here with keys that are not the record order"""
    rec = np.zeros(4, dtype=cu.CAND_DTYPE)
    rec["xy"] = cu.REFERENCE_VECTOR.reshape(4, 8)
    rec["start_key"] = [7, 0xFFFFFFFF, 0, 9]
    got = ctx.debug_frame_candidates([4], rec, 1024, 10.0, 0)
    assert got["fin_count"].tolist() == [1] and got["work_count"] == 1 and got["work"][0] == 0
    srt = cu.REFERENCE_VECTOR[[2, 0, 3, 1]]
    assert np.array_equal(got["pre_xy"][0, :4].reshape(4, 4, 2), srt)
    want, kept = oracle.discard_too_near(srt.astype(np.uint32), 10.0)
    assert np.array_equal(got["fin_xy"][0, :1].reshape(1, 4, 2), want)


def test_hook_refuses_what_the_kernel_cannot_take(ctx):
    from aruco3_amd import _lib

    rec = np.zeros(2, dtype=cu.CAND_DTYPE)
    rec["start_key"] = [5, 6]
    for counts, records, max_cand, word in (([], rec[:0], 1024, "n_frames"), ([2], rec, 0, "max_cand"), ([2], rec, 65537, "max_cand")):
        with pytest.raises(_lib.A3Error) as e:
            ctx.debug_frame_candidates(counts, records, max_cand, 25.0, 0)
        assert word in str(e.value), str(e.value)
    rec["start_key"] = [5, 5]
    with pytest.raises(_lib.A3Error) as e:
        ctx.debug_frame_candidates([0, 2], rec, 1024, 25.0, 0)
    assert "unique" in str(e.value)
    rec["start_key"] = [5, 6]      # the same key in two frames is fine
    got = ctx.debug_frame_candidates([1, 1], np.array([rec[0], rec[0]]), 65536, 25.0, 0)
    assert got["fin_count"].tolist() == [1, 1] and sorted(got["work"][:2].tolist()) == [0, 65536]
