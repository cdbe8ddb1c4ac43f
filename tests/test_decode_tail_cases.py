"""The designed patches of tests/decode_tail_util.py, CPU half: the oracle delivers every one of them exactly and keeps every quad, the two
numpy models equal the oracle's own otsu_level, resize_triangle and homography_to_code_permutations on them, and the cases reach what
tests/test_gpu_decode_tail.py claims for them -- counted with models that are deliberately wrong in one respect each.  No GPU.

What the seeded searches found (test_summary prints the counts per tag and shape):
  * exact ties: 600 symmetric histograms per S give 68 / 65 / 57 (S = 48 / 50 / 200) with two thresholds of bit-equal, maximal f64
    variance; every shape at those S keeps 10 or more with the tied thresholds in different quarters of 0..255 and 6 or more in one
    quarter but different runs of four, all of them with a grey between the tied thresholds;
  * f32: a pixel moved off an exact tie opens a gap of 1e-3 of the variance, and seeded few-level histograms do not come closer: a
    trial of 12 000 such draws at S = 48 found none that f32 arithmetic decides differently, so the builder does not draw them.  What
    does come within f32's reach are the symmetric histograms whose mirrored thresholds end a few ulps apart in f64 instead of
    bit-equal: 10 000 draws per S give 192 / 193 / 185 in which f32 picks the other threshold and 59 / 43 / 46 in which the later
    threshold wins by those ulps.  Every shape at S = 48, 50, 200 keeps 8 + 4 of them, and 10 or more f32 cases in all;
  * `>= 0.0` for `> 0.0` cannot be noticed by any patch: test_ge_zero_is_the_same_level says why;
  * resize: every shape with S > n has 8 or more patches in which some variant changes the outcome (1000 patches per source searched, 200
    at S = 199 and 200, and the few half-cell patches where a cell's centre lies between two samples); no shape has to be listed as
    empty.  Truncation is noticed at every such shape, `>= 127` at all but (8, 7); fused multiply-add, pass order and f64
    accumulation at (48, 8) -- six samples a cell: 127.5 is reached exactly, and only the rounding of the reference's own operation
    order decides -- in 3 to 12 cases each, and fused multiply-add and f64 accumulation in the half-cell patches of (200, 6).
    (5, 10) upsamples and is no shape of the resize condition."""
import numpy as np
import pytest

from tests import damage_util as du
from tests import decode_tail_util as tu


@pytest.mark.parametrize("shape", tu.SHAPES, ids=tu.shape_id)
def test_oracle_delivers_the_designed_patches(oracle, shape):
    """every later claim about a histogram rests on this: the oracle's patch of every tile IS the designed one, and every quad is kept, in
    order"""
    S, n = shape
    assert du.table(tu.DICT_OF_N[n])[0] == (n - 2) ** 2
    seen = 0
    for index, (img, quads, chunk) in enumerate(tu.mosaics(shape)):
        ref = tu.reference(oracle, shape, index)
        assert ref["candidates"].tolist() == quads.tolist(), f"{shape} mosaic {index}: quads dropped or reordered"
        assert ref["homography_ok"].all()
        for k, c in enumerate(chunk):
            got = ref["homographies"][k]
            if not np.array_equal(got, c.patch):
                y, x = np.argwhere(got != c.patch)[0]
                raise AssertionError(f"{shape} mosaic {index} tile {k} {sorted(c.tags)}: delivered {got[y, x]} for {c.patch[y, x]} at ({x}, {y}), "
                                     f"{int((got != c.patch).sum())} samples differ")
        seen += len(chunk)
        assert img.shape[0] <= 1000 and img.shape[1] <= 1300
    assert seen == len(tu.cases(shape)) > 0


@pytest.mark.parametrize("shape", tu.SHAPES, ids=tu.shape_id)
def test_models_equal_the_oracle(oracle, shape):
    """the Otsu model is oracle.otsu_level, the resize model oracle.resize_triangle cell for cell (on the binarised patch and on the grey
    one), model plus rotation is oracle.homography_to_code_permutations and the oracle's whole detect, flag and four codes"""
    S, n = shape
    pos = 0
    cs = tu.cases(shape)
    for index, (_, _, chunk) in enumerate(tu.mosaics(shape)):
        ref = tu.reference(oracle, shape, index)
        for k, c in enumerate(chunk):
            what = f"{shape} case {pos} {sorted(c.tags)}"
            assert c is cs[pos]
            assert c.level == oracle.otsu_level(c.patch), what
            binary = np.where(c.patch > c.level, 255, 0).astype(np.uint8)
            for src in (binary, c.patch):
                assert np.array_equal(tu.resize_u8(src[None], n)[0], oracle.resize_triangle(src, n, n)), what
            codes = oracle.homography_to_code_permutations(c.patch, n)
            ok, want = c.outcome
            assert (codes is not None) == bool(ok), what
            assert codes is None or tuple(int(v) for v in codes) == want, what
            assert int(ref["decode_ok"][k]) == ok and tuple(int(v) for v in ref["codes"][k]) == want, what
            pos += 1
    assert pos == len(cs)


def test_ge_zero_is_the_same_level():
    """`bv >= 0.0 ? bt : 0` for `bv > 0.0 ? bt : 0` changes no level, so no case can notice it -- the one variant of the list that is
    none.  A threshold counts only with pixels on both sides of it; their means then differ by 1 / S^2 or more and its variance is
    1 * 1 * S^-4 >= 6e-10 or more, never 0.0 or below.  Without such a threshold (a flat patch) the best variance is the scan's
    identity, below 0.0 under either test, and the first-of-equals rule would name threshold 0 anyway.  Asserted on every case and on
    the smallest variance a patch can have."""
    for shape in tu.SHAPES:
        cs = tu.cases(shape)
        hists = np.stack([tu.histogram(c.patch) for c in cs])
        assert np.array_equal(tu.otsu_levels(hists, "ge_zero"), tu.otsu_levels(hists))
        assert not any("ge_zero" in c.noticed for c in cs)
    h = np.zeros(256, np.int64)
    h[254], h[255] = 200 * 200 // 2, 200 * 200 // 2
    v = tu.otsu_variances(h)[0]
    assert v.max() > 0.0 and tu.otsu_levels(h[None])[0] == 254
    flat = np.zeros(256, np.int64)
    flat[128] = 49 * 49
    assert tu.otsu_variances(flat).max() < 0.0 and tu.otsu_levels(flat[None], "ge_zero")[0] == 0


def _count(shape, pred):
    return sum(1 for c in tu.cases(shape) if pred(c))


def test_otsu_conditions():
    """exact ties per S in 48, 50, 200 (asserted for every shape at that S): 8 or more across quarters -- the s_var[] loop of `<256, 256>` --
    and 4 or more inside a quarter across runs of four -- wave_best_var_to63 of `<256, 64>` (and of `<256, 256>`, whose lanes hold one
    threshold each) --, each with a grey between the tied thresholds so that the wrong tie rule changes the flag or the codes; 4 or more
    f32 cases at S = 48; every variant but `>= 0.0` noticed"""
    noticed = set()
    for shape in tu.SHAPES:
        noticed |= set().union(*(c.noticed for c in tu.cases(shape)))
        if shape[0] not in tu.TIE_SIZES:
            continue
        q = _count(shape, lambda c: "tie_quarters" in c.tags and {"last_of_equals", "higher_quarter"} <= c.noticed)
        r = _count(shape, lambda c: "tie_runs" in c.tags and {"last_of_equals", "higher_run_of_4"} <= c.noticed)
        assert q >= 8 and r >= 4, (shape, q, r)
        for c in tu.cases(shape):
            if {"tie_quarters", "tie_runs"} & c.tags:
                h = tu.histogram(c.patch)
                assert h[c.tied[0] + 1: c.tied[-1] + 1].any() and c.level == c.tied[0], shape
        later = _count(shape, lambda c: "near_tie_later_wins" in c.tags)
        assert later >= 1, shape
        if shape[0] == tu.F32_SIZE:
            assert _count(shape, lambda c: "f32" in c.noticed) >= 4, shape
    assert noticed >= set(tu.OTSU_VARIANTS) - {"ge_zero"}


def test_resize_conditions():
    """every resize variant is noticed somewhere; every shape with S > n has 8 or more cases in which some variant changes the flag or a
    code, and plain ones with a cell at 126..129"""
    noticed, short = set(), []
    larger = [s for s in tu.SHAPES if s[0] > s[1]]
    for shape in larger:
        noticed |= set().union(*(c.noticed for c in tu.cases(shape)))
        if _count(shape, lambda c: "resize" in c.tags and c.noticed & set(tu.RESIZE_VARIANTS)) < 8:
            short.append(shape)
        assert _count(shape, lambda c: "cell_at_cut" in c.tags and not c.noticed & set(tu.RESIZE_VARIANTS)) >= 1, shape
        assert tu.resize_search(shape)[1] == 3 * tu.RESIZE_BUDGET[shape[0] >= 199] + len(tu.half_cell_patches(shape))
    assert noticed >= set(tu.RESIZE_VARIANTS)
    assert short == []          # (the module docstring would have to list a shape that falls short; a quarter of them at the most)


def test_every_group_of_patches_is_present():
    for shape in tu.SHAPES:
        S, n = shape
        tags = set().union(*(c.tags for c in tu.cases(shape)))
        want = {"flat_0", "flat_1", "flat_128", "flat_255", "no_level"}
        if S >= 2:
            want |= {"one_pixel_0", "one_pixel_255", "adjacent_0_1", "adjacent_63_64", "adjacent_127_128", "adjacent_254_255", "adjacent_3_4"}
        if S % n == 0:
            want |= {"cell_grey"}
        if S >= n:
            want |= {"dictionary_code", "dictionary_missed"}
        if S == 200:
            want |= {"largest_sums"}
        if S <= 11:
            want |= {"random_small"}
        assert want <= tags, (shape, want - tags)
        accepted = 0
        if S >= n:      # real codes are accepted as markers; the others pass the border test and miss every code by tau or more
            _, _, codes = du.table(tu.DICT_OF_N[n])
            tau = du.tau_of(tu.DICT_OF_N[n])
            for c in tu.cases(shape):
                if "dictionary" in c.tags:
                    assert c.outcome[0] == 1, shape
                    e = du.expect_codes(c.outcome[1], codes)
                    if "dictionary_missed" in c.tags:
                        assert e.distance >= tau, (shape, e.distance)
                    elif S % n == 0 or S >= 48:     # (the few samples of S = n + 1 put two on one cell: the code is read shifted)
                        assert e.distance < tau, (shape, e.distance)
                        accepted += 1
            assert accepted == 2 or (S < 48 and S % n), shape


def test_summary():
    for group, shapes in tu.SHAPE_GROUPS.items():
        for shape in shapes:
            s = tu.summary(shape)
            print(f"{group} {shape}: {s['cases']} cases in {len(tu.mosaics(shape))} mosaics; noticed {s['noticed']}; tags {s['tags']}")
            assert s["cases"] >= 16
