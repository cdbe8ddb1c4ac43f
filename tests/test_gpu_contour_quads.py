"""k_contour_quads as the pipeline launches it (a3_debug_contour_quads: one call of launch_contour_quads), held against the oracle on
hand-made borders, exactly: per frame the records the kernel wrote, sorted by start key, equal the expected records sorted by start key,
integer for integer (the slot order is an atomic's and no part of the contract); cand_count is the expected count; every other slot and
everything of a frame below first_frame is still the 0xFF the hook filled it with; err_flags is 0.  The expectation is the oracle's own
approximate_polygon_dp, convex_hull, edge filter and enforce_clockwise_corners, composed per border (tests/quad_cases.py).

The borders are chosen for the kernel's control flow: every length at which the arg-max's trips change (1 .. 64 in the 16-lane form, 65 ..
4097 in the wave form), eight orientations, outer and hole borders, every reject class, chords inside the nine-digit band of the distance
test with ratio exactly 1 and 1e-16 off it, ties along whole rectangle sides, rejections at the fourth split, coordinates against
16383 (24-bit products near 2^28) and against 65535, walks of 65 000 points across the whole 2^14 range at widths 16384 and 16385, both
group widths interleaved in one launch at the smallest and the largest grid, three frames from first_frame 2, tables cut short by
max_contours and by the device's count, a frame that overflows its candidate table, and stale tables behind kErrPointPool and
kErrContourTable.  tests/test_quad_cases.py counts, without a GPU, what these inputs make the kernel execute and shows that each plausible
fault -- ties to the largest index, >= for >, the band decided by the squared comparison, no rejection at the fourth split, an unsquared
edge filter, no hull -- changes the expected output of some border in each width.  GPU only."""
import numpy as np
import pytest

from tests import quad_cases as qc

pytestmark = pytest.mark.gpu
PLAIN = [n for n in sorted(qc.launches()) if n not in ("cand_overflow",)]


@pytest.fixture(scope="module")
def ctx(dicts):
    from aruco3_amd.aruco import Detector, DetectorConfig

    return Detector(DetectorConfig(), dicts.new_from_named_dict("ARUCO"))._context()


_ran = {}


def _run(ctx, name):
    """one launch of the kernel per name, shared by the tests that look at it"""
    if name not in _ran:
        L = qc.launches()[name]
        rec, pool = L.tables()
        _ran[name] = ctx.debug_contour_quads(L.width, L.height, rec, pool, **L.kwargs())
    return _ran[name]


def _rows(cands):
    """written records of one frame's table as (m, 9) int64 rows of key and xy[8], sorted; and the mask of written slots"""
    written = ~(cands.view(np.uint8).reshape(len(cands), -1) == 0xFF).all(axis=1)
    c = cands[written]
    rows = np.concatenate([c["start_key"].astype(np.int64)[:, None], c["xy"].astype(np.int64)], axis=1)
    return rows[np.lexsort(rows.T[::-1])], written


def _check_untouched(L, got):
    assert got["cand_count"].shape == (L.first_frame + L.n_frames,) and got["cands"].shape == (L.first_frame + L.n_frames, L.max_cand)
    assert (got["cand_count"][:L.first_frame] == 0xFFFFFFFF).all()
    assert (got["cands"][:L.first_frame].view(np.uint8) == 0xFF).all()


@pytest.mark.parametrize("name", PLAIN)
def test_contour_quads_equal_the_oracle(name, ctx):
    L = qc.launches()[name]
    got, want = _run(ctx, name), qc.expected(name)
    _check_untouched(L, got)
    assert got["err_flags"] == 0
    for f, e in want.items():
        rows, written = _rows(got["cands"][f])
        assert int(got["cand_count"][f]) == len(e), (name, f, int(got["cand_count"][f]), len(e))
        assert written[:len(e)].all() and not written[len(e):].any(), (name, f)      # the first count slots and no other
        assert np.array_equal(rows, e), (name, f, rows[:3], e[:3])


def test_both_grids_give_the_same_output(ctx):
    a, b = _run(ctx, "mixed_min_grid"), _run(ctx, "mixed_max_grid")
    assert np.array_equal(a["cand_count"], b["cand_count"])
    for f in range(2, 5):
        assert np.array_equal(_rows(a["cands"][f])[0], _rows(b["cands"][f])[0])


def test_24_bit_and_64_bit_numerators_agree(ctx):
    a, b = _run(ctx, "large_14"), _run(ctx, "large_64")
    ra, rb = _rows(a["cands"][0])[0], _rows(b["cands"][0])[0]
    assert len(ra) == 1 and np.array_equal(ra[:, 1:], rb[:, 1:])


def test_overflowed_frame_counts_all_and_keeps_the_table(ctx):
    L = qc.launches()["cand_overflow"]
    got, want = _run(ctx, "cand_overflow"), qc.expected("cand_overflow")
    _check_untouched(L, got)
    assert got["err_flags"] == qc.ERR_CAND_TABLE
    for f, e in want.items():
        rows, written = _rows(got["cands"][f])
        assert int(got["cand_count"][f]) == len(e), f                                # every candidate is counted
        if len(e) <= L.max_cand:
            assert written[:len(e)].all() and not written[len(e):].any() and np.array_equal(rows, e), f
        else:                                                                        # exactly max_cand slots, each a distinct expected record
            assert written.all() and len(np.unique(rows, axis=0)) == L.max_cand
            assert {tuple(r) for r in rows.tolist()} <= {tuple(r) for r in e.tolist()}


@pytest.mark.parametrize("name", ["stale_point_pool", "stale_contour_table"])
def test_stale_tables_are_not_read(name, ctx):
    got = _run(ctx, name)
    assert got["err_flags"] == 0 and (got["cand_count"] == 0).all()
    assert (got["cands"].view(np.uint8) == 0xFF).all()


def test_hook_refuses_what_the_kernel_cannot_take(ctx):
    from aruco3_amd import _lib

    sq = qc.walk([(1, 1), (9, 1), (9, 9), (1, 9)])
    pool = (sq[:, 0] | sq[:, 1] << 16).astype(np.uint32)

    def rec(*rows):
        return np.array(list(rows), dtype=qc.CONTOUR_DTYPE)

    ok = ctx.debug_contour_quads(16, 16, rec((0, 7, 0, len(pool))), pool)
    assert ok["cand_count"].tolist() == [1] and ok["err_flags"] == 0
    bad = (
        (dict(), rec((0, 7, 0, 0)), "n == 0"),
        (dict(), rec((0, 7, 1, len(pool))), "beyond the pool"),
        (dict(), rec((1, 7, 0, len(pool))), "frame"),
        (dict(first_frame=1), rec((0, 7, 0, len(pool))), "frame"),
        (dict(), rec((0, 7, 0, 4), (0, 7, 4, 4)), "unique"),
        (dict(max_cand=0), rec((0, 7, 0, len(pool))), "max_cand"),
        (dict(ctr_contours=2, max_contours=2), rec((0, 7, 0, len(pool))), "records must be given"),
    )
    for kw, r, word in bad:
        with pytest.raises(_lib.A3Error) as e:
            ctx.debug_contour_quads(16, 16, r, pool, **kw)
        assert word in str(e.value), str(e.value)
    for w, h in ((9, 16), (16, 9), (0, 16), (16, 65537)):
        with pytest.raises(_lib.A3Error) as e:
            ctx.debug_contour_quads(w, h, rec((0, 7, 0, len(pool))), pool)
        assert "width" in str(e.value), str(e.value)
    two = ctx.debug_contour_quads(16, 16, rec((0, 7, 0, len(pool)), (1, 7, 0, len(pool))), pool, n_frames=2)      # one key in two frames is fine
    assert two["cand_count"].tolist() == [1, 1]
