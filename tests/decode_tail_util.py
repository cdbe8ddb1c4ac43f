"""Designed patches for the middle of the decode stage -- the Otsu level, the binarisation `> level`, the two-pass f32 triangle resize and
`round > 127` -- delivered exactly.  Shared by tests/test_decode_tail_cases.py (oracle, CPU: delivery, the models, the counts of what the
cases reach) and tests/test_gpu_decode_tail.py (k_decode in both instantiations).

Delivery.  An L8 frame holds a grid of tiles, each an S x S patch blown up to k x k constant blocks.  The quad handed to the decode stage
is (x0, y0), (x0 + kS, y0), (x0 + kS, y0 + kS), (x0, y0 + kS): sample (x, y) of the warp falls on (x0 + kx, y0 + ky), and the tile is
drawn so that this pixel is the centre of block (x, y).  k = 3 up to S = 50, k = 1 from S = 199.  Every claim made here about a
histogram rests on test_decode_tail_cases.py asserting that the oracle's patches ARE the designed ones.

Models.  otsu_* and resize_* restate the two steps in numpy with the oracle's operations in the oracle's order (oracle/a3_oracle.c:
a3o_otsu_level, resize_weights, a3o_resize_triangle), vectorised over patches so that thousands can be searched.  Their VARIANTS are
deliberately wrong in one respect each; they are never compared with the device, only used to count which cases would notice a
kernel that is wrong in that respect (`noticed`: the flag or the four codes of the case come out differently).

Builders.  All seeded, cached per shape, every case tagged with what it reaches.  `tie_*`: histograms symmetric about a centre reach
bit-equal f64 variances at two thresholds with different background weights; which of the two the scan keeps is decided by k_decode's
three layers of "first strict maximum" (a lane's run, wave_best_var_to63, the loop over s_var[] in `<256, 256>`).  `near_tie`: the
same histograms where the two variances end a few ulps apart instead: the only near ties f32 arithmetic decides differently."""
import functools
from dataclasses import dataclass, field

import numpy as np

from tests import damage_util as du

DICT_OF_N = {6: "APRILTAG_16H5", 7: "ARUCO", 8: "HAND_TAU_12", 10: "CHILITAGS"}      # 16-, 25-, 36- and 64-bit codes (damage_util.table; HAND_TAU_12:
#   every other code of ARUCO_MIP_36H12 with its tau -- the dense 36-bit tables leave no pattern tau from all of their codes)
SHAPE_GROUPS = {
    "default S": ((49, 7), (49, 8), (49, 10), (49, 6)),
    "whole cells": ((48, 6), (48, 8), (50, 10)),
    "copy branch and its neighbours": ((7, 7), (6, 7), (8, 7), (10, 10), (9, 10), (11, 10)),
    "tiny": ((1, 7), (2, 8), (3, 10), (5, 10)),
    "largest": ((199, 7), (200, 6), (200, 10)),
}
SHAPES = tuple(s for g in SHAPE_GROUPS.values() for s in g)
TIE_SIZES = (48, 50, 200)            # the S at which exact ties are harvested
F32_SIZE = 48                        # the S at which the number of f32 cases is a condition
OTSU_VARIANTS = ("last_of_equals", "higher_run_of_4", "higher_quarter", "f32", "ge_zero")
RESIZE_VARIANTS = ("fma", "horizontal_first", "f64_accumulate", "ge_127", "truncate")
SEPARATION = 0.001                   # min_corner_separation_factor: a pixel or so; tiles lie a block and a gap apart
GAP, BACKGROUND = 8, 128


def shape_id(shape):
    return f"S{shape[0]}-n{shape[1]}"


def block(S):
    return 1 if S >= 199 else 3


# ------------------------------------------------------------------------------------------------------------------
# Otsu: the model and its variants, over a batch of histograms [N, 256]
# ------------------------------------------------------------------------------------------------------------------
_T = np.arange(256, dtype=np.int64)


def histogram(patch):
    return np.bincount(np.asarray(patch, dtype=np.uint8).reshape(-1), minlength=256).astype(np.int64)


def otsu_variances(hists, dtype=np.float64):
    """-> (variance per threshold [N, 256] in `dtype`, -1 where the reference's weight tests skip the threshold).  Prefix sums are exact
    integers; the floating-point operations are a3o_otsu_level's, in its order."""
    h = np.atleast_2d(np.asarray(hists, dtype=np.int64))
    bw, bs = np.cumsum(h, axis=1), np.cumsum(h * _T, axis=1)
    total, tsum = bw[:, -1:], bs[:, -1:]
    fw = total - bw
    valid = (bw != 0) & (fw != 0)
    f = dtype
    with np.errstate(divide="ignore", invalid="ignore"):
        bsum = bs.astype(f)
        fsum = tsum.astype(f) - bsum
        diff = bsum / bw.astype(f) - fsum / fw.astype(f)
        v = bw.astype(f) * fw.astype(f) * (diff * diff)
    return np.where(valid, v, f(-1.0))


def _first_max(v):
    """first strict maximum above 0.0 of every row"""
    return np.where(v.max(axis=1) > 0.0, np.argmax(v, axis=1), 0)


def otsu_levels(hists, variant=None):
    """the level of every histogram: the model (variant None), or the model wrong in one respect"""
    v = otsu_variances(hists, np.float32 if variant == "f32" else np.float64)
    n = len(v)
    rows = np.arange(n)
    if variant in (None, "f32"):
        return _first_max(v)
    m = v.max(axis=1)
    if variant == "ge_zero":                 # `>= 0.0`: provably the same level (test_decode_tail_cases.py says why)
        return np.where(m >= 0.0, np.argmax(v, axis=1), 0)
    if variant == "last_of_equals":
        return np.where(m > 0.0, 255 - np.argmax(v[:, ::-1], axis=1), 0)
    group = {"higher_run_of_4": 4, "higher_quarter": 64}[variant]
    g = v.reshape(n, 256 // group, group)
    gt = np.argmax(g, axis=2)                                    # first maximum inside a run ...
    gm = g.max(axis=2)
    last = gm.shape[1] - 1 - np.argmax(gm[:, ::-1], axis=1)      # ... the HIGHER run among equals
    return np.where(m > 0.0, last * group + gt[rows, last], 0)


def tied_thresholds(hist):
    """present greys at which the f64 variance equals the maximum (a grey absent from the patch repeats its predecessor's variance: not a
    threshold of its own)"""
    v = otsu_variances(hist)[0]
    if v.max() <= 0.0:
        return []
    return [int(t) for t in np.flatnonzero((v == v.max()) & (np.asarray(hist) > 0))]


# ------------------------------------------------------------------------------------------------------------------
# resize: the model and its variants, over a batch of binarised patches [N, S, S] (0 / 255)
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def resize_weights(in_len, out_len):
    """image::imageops::resize's weights as the oracle's resize_weights computes them, every operation in f32 -> [(left, weights)]"""
    f = np.float32
    ratio = f(in_len) / f(out_len)
    sratio = f(1.0) if ratio < f(1.0) else ratio
    support = f(1.0) * sratio
    out = []
    for o in range(out_len):
        inp = (f(o) + f(0.5)) * ratio
        left = min(max(int(np.floor(inp - support)), 0), in_len - 1)
        right = min(max(int(np.ceil(inp + support)), left + 1), in_len)
        inp = inp - f(0.5)
        ws, s = [], f(0.0)
        for i in range(left, right):
            x = (f(i) - inp) / sratio
            w = f(1.0) - abs(x) if abs(x) < f(1.0) else f(0.0)
            ws.append(w)
            s = s + w
        out.append((left, np.array([w / s for w in ws], dtype=f)))
    return out


def _pass(img, out_len, axis, mode):
    """one pass of the resize along `axis` of [N, rows, cols] f32, tap by tap"""
    img = np.moveaxis(img, axis, 1)
    acc_t = np.float64 if mode in ("f64_accumulate", "fma") else np.float32
    res = np.empty((img.shape[0], out_len, img.shape[2]), dtype=np.float32)
    for o, (left, ws) in enumerate(resize_weights(img.shape[1], out_len)):
        t = np.zeros((img.shape[0], img.shape[2]), dtype=acc_t)
        for k, w in enumerate(ws):
            if mode == "fma":       # one rounding per tap: the product of two f32 is exact in f64
                t = (t + img[:, left + k, :].astype(np.float64) * np.float64(w)).astype(np.float32).astype(np.float64)
            elif mode == "f64_accumulate":
                t = t + img[:, left + k, :].astype(np.float64) * np.float64(w)
            else:
                t = t + img[:, left + k, :] * w
        res[:, o, :] = t.astype(np.float32)
    return np.moveaxis(res, 1, axis)


def resize_values(binary, n, variant=None):
    """[N, S, S] u8 -> the clamped f32 value of every one of the n x n cells before rounding (None: the patch is copied)"""
    b = np.asarray(binary)
    if b.shape[1] == n:
        return None
    x = b.astype(np.float32)
    mode = variant if variant in ("fma", "f64_accumulate") else None
    order = (2, 1) if variant == "horizontal_first" else (1, 2)          # the reference: vertical pass first
    for axis in order:
        x = _pass(x, n, axis, mode)
    return np.clip(x, np.float32(0.0), np.float32(255.0))


def resize_bits(binary, n, variant=None):
    """[N, S, S] u8 (0 / 255) -> the n x n bit matrices, [N, n, n] u8"""
    c = resize_values(binary, n, variant)
    if c is None:
        r = np.asarray(binary).astype(np.int64)
    elif variant == "truncate":
        r = c.astype(np.int64)
    else:
        r = np.floor(c.astype(np.float64) + 0.5).astype(np.int64)        # round half away from zero (c >= 0)
    return (r >= 127 if variant == "ge_127" else r > 127).astype(np.uint8)


def resize_u8(patches, n):
    """the model's resize of grey patches as oracle.resize_triangle returns it: u8"""
    c = resize_values(patches, n)
    if c is None:
        return np.asarray(patches, dtype=np.uint8).copy()
    return np.floor(c.astype(np.float64) + 0.5).astype(np.uint8)


# ------------------------------------------------------------------------------------------------------------------
# the tail as a whole: level, binarisation, resize, border test, four codes
# ------------------------------------------------------------------------------------------------------------------
def outcomes(patches, n, otsu_variant=None, resize_variant=None, levels=None):
    """[N, S, S] u8 -> [(decode_ok, (four codes))] per patch"""
    patches = np.asarray(patches, dtype=np.uint8)
    if levels is None:
        levels = otsu_levels(np.stack([histogram(p) for p in patches]), otsu_variant)
    binary = np.where(patches > np.asarray(levels).reshape(-1, 1, 1), 255, 0).astype(np.uint8)
    bits = resize_bits(binary, n, resize_variant)
    out = []
    for m in bits:
        if m[0].any() or m[-1].any() or m[:, 0].any() or m[:, -1].any():
            out.append((0, (0, 0, 0, 0)))
        else:
            out.append((1, tuple(du.rotated_codes(m[1:-1, 1:-1]))))
    return out


@dataclass
class Case:
    patch: np.ndarray                      # S x S u8, as designed
    tags: set = field(default_factory=set)
    level: int = 0                         # the model's Otsu level of the designed histogram
    outcome: tuple = None                  # (decode_ok, codes) by the model
    noticed: set = field(default_factory=set)   # the variants under which the outcome differs
    tied: tuple = ()                       # thresholds of equal, maximal f64 variance


def classify(patches, tags, n, resize=True):
    """-> [Case] with level, outcome, `noticed` and the tags that follow from the histogram alone (resize False: the Otsu variants only)"""
    patches = np.asarray(patches, dtype=np.uint8)
    if len(patches) == 0:
        return []
    hists = np.stack([histogram(p) for p in patches])
    level = otsu_levels(hists)
    base = outcomes(patches, n, levels=level)
    cases = [Case(p, set(t), int(l), o) for p, t, l, o in zip(patches, tags, level, base)]
    for v in OTSU_VARIANTS:
        lv = otsu_levels(hists, v)
        idx = np.flatnonzero(lv != level)
        if len(idx):
            for i, o in zip(idx, outcomes(patches[idx], n, levels=lv[idx])):
                if o != base[i]:
                    cases[i].noticed.add(v)
    for v in RESIZE_VARIANTS if resize else ():
        for i, o in enumerate(outcomes(patches, n, resize_variant=v, levels=level)):
            if o != base[i]:
                cases[i].noticed.add(v)
    for c, h in zip(cases, hists):
        c.tied = tuple(tied_thresholds(h))
        if len(c.tied) > 1:
            lo, hi = c.tied[0], c.tied[-1]
            between = bool(h[lo + 1: hi + 1].any())         # a grey above the first tied threshold, at or below the last
            if lo // 64 != hi // 64:
                c.tags.add("tie_quarters" if between else "tie_quarters_unseen")
            elif lo // 4 != hi // 4:
                c.tags.add("tie_runs" if between else "tie_runs_unseen")
            else:
                c.tags.add("tie_same_run")
        if (h > 0).sum() < 2:
            c.tags.add("no_level")
        vals = resize_values(np.where(c.patch > c.level, 255, 0).astype(np.uint8)[None], n)
        if vals is not None and ((vals > 125.5) & (vals < 129.5)).any():
            c.tags.add("cell_at_cut")
        if c.noticed & set(RESIZE_VARIANTS):
            c.tags.add("resize_noticed")
        if "f32" in c.noticed:
            c.tags.add("f32_noticed")
    return cases


# ------------------------------------------------------------------------------------------------------------------
# layouts
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _order(S, n):
    """sample positions, perimeter cells first, then the interior cell by cell: greys laid out ascending along it put the lowest on
    the perimeter and fill whole cells with one grey where the counts allow"""
    cell = np.minimum(np.arange(S) * n // S, n - 1) if S >= n else np.arange(S)
    cy, cx = np.meshgrid(cell, cell, indexing="ij")
    m = cell.max()
    rim = (cy == 0) | (cx == 0) | (cy == m) | (cx == m)
    key = np.where(rim, -1, cy * n + cx).reshape(-1)
    return np.argsort(key, kind="stable")


def rim_samples(S, n):
    """samples of an S x S patch that lie in the perimeter cells"""
    cell = np.minimum(np.arange(S) * n // S, n - 1)
    inner = int(((cell > 0) & (cell < n - 1)).sum())
    return S * S - inner * inner


def lay_histogram(hist, S, n):
    """a patch with this histogram: greys ascending along _order"""
    hist = np.asarray(hist, dtype=np.int64)
    assert hist.sum() == S * S
    p = np.empty(S * S, dtype=np.uint8)
    p[_order(S, n)] = np.repeat(np.arange(256, dtype=np.uint8), hist)
    return p.reshape(S, S)


def lay_cells(cells, S):
    """an n x n matrix of greys painted over S samples a side (S >= n): sample x lies in cell x * n // S"""
    n = cells.shape[0]
    at = np.minimum(np.arange(S) * n // S, n - 1)
    return np.asarray(cells, dtype=np.uint8)[np.ix_(at, at)]


# ------------------------------------------------------------------------------------------------------------------
# builders
# ------------------------------------------------------------------------------------------------------------------
def _seed(shape, salt):
    return shape[0] * 1000 + shape[1] * 10 + salt


def _flat(shape):
    S, n = shape
    return [(np.full((S, S), g, np.uint8), {"flat", f"flat_{g}"}) for g in (0, 1, 128, 255)]


def _extreme(shape):
    S, n = shape
    out = []
    if S >= 2:
        for lone, rest in ((0, 255), (255, 0)):
            h = np.zeros(256, np.int64)
            h[lone], h[rest] = 1, S * S - 1
            out.append((lay_histogram(h, S, n), {"extreme", f"one_pixel_{lone}"}))
        for g in (0, 63, 127, 254, 3):
            h = np.zeros(256, np.int64)
            h[g] = rim_samples(S, n) if S >= n else S * S // 2       # the perimeter cells: the lower grey
            h[g + 1] = S * S - h[g]
            out.append((lay_histogram(h, S, n), {"extreme", "adjacent_greys", f"adjacent_{g}_{g + 1}"}))
    if S == 200:      # the largest prefix sums a patch can have
        for low in (1, S * S // 2):
            h = np.zeros(256, np.int64)
            h[254], h[255] = low, S * S - low
            out.append((lay_histogram(h, S, n), {"extreme", "largest_sums"}))
    return out


def _cell_grey(shape):
    """every cell one grey, the perimeter the lowest grey present: it stays black at any level, so the codes show which interior cells lie
    above the level.  Greys of the interior: a few levels, adjacent ones among them (`>` against `>=`)."""
    S, n = shape
    if S % n:
        return []
    rng = np.random.default_rng(_seed(shape, 1))
    out = []
    for i in range(8):
        k = int(rng.integers(3, 7))
        lo = int(rng.integers(0, 120))
        greys = rng.choice(np.arange(lo + 1, 255), size=k, replace=False)
        if i % 2:
            greys = np.append(greys, greys[0] + 1)
        greys = np.unique(greys)
        cells = np.full((n, n), lo, dtype=np.uint8)
        inner = rng.choice(greys, size=(n - 2, n - 2))
        inner.reshape(-1)[: len(greys)] = greys                  # every grey present
        cells[1:-1, 1:-1] = inner
        out.append((lay_cells(cells, S), {"cell_grey"}))
    return out


def symmetric_histograms(S, draws, seed):
    """seeded histograms of S x S patches, symmetric about a centre: 2-4 pairs of levels a, c - a with equal counts.  Thresholds t and
    c - 1 - t split them into mirrored classes: equal variances in exact arithmetic, bit-equal or a few ulps apart in f64"""
    rng = np.random.default_rng(seed)
    hs = np.zeros((draws, 256), np.int64)
    for i in range(draws):
        pairs = int(rng.integers(2, 5))
        if i % 3 == 0:       # everything inside one quarter of 0..255
            q = int(rng.integers(0, 4))
            lo, hi = 64 * q, 64 * q + 63
        else:
            lo, hi = 0, 255
        span = int(rng.integers(4 * pairs, hi - lo + 1))
        base = int(rng.integers(lo, hi - span + 1))
        a = rng.choice(np.arange(0, (span + 1) // 2), size=pairs, replace=False)     # offsets of the lower levels, mirrored about span / 2
        cuts = np.sort(rng.choice(np.arange(1, S * S // 2), size=pairs - 1, replace=False))
        counts = np.diff(np.concatenate([[0], cuts, [S * S // 2]]))
        for off, c in zip(a, counts):
            hs[i, base + off] += c
            hs[i, base + span - off] += c
    return hs


TIE_DRAWS, NEAR_TIE_DRAWS = 600, 10000


@functools.lru_cache(maxsize=None)
def tie_histograms(S):
    """exact distant ties: of TIE_DRAWS symmetric histograms, those in which two thresholds reach the same maximal f64 variance"""
    hs = symmetric_histograms(S, TIE_DRAWS, S * 7 + 1)
    v = otsu_variances(hs)
    tied = ((v == v.max(axis=1, keepdims=True)) & (hs > 0)).sum(axis=1) > 1
    return hs[tied]


@functools.lru_cache(maxsize=None)
def near_tie_histograms(S):
    """near ties: of NEAR_TIE_DRAWS symmetric histograms, those whose two best thresholds are NOT bit-equal in f64 but within 1e-12 of
    one another -> (those in which f32 arithmetic picks another level, those in which the later threshold wins by those few ulps)"""
    hs = symmetric_histograms(S, NEAR_TIE_DRAWS, S * 7 + 2)
    v = np.where(hs > 0, otsu_variances(hs), -1.0)           # thresholds of their own only
    top = np.sort(v, axis=1)[:, -2:]
    near = (top[:, 0] > 0.0) & (top[:, 0] < top[:, 1]) & (top[:, 1] - top[:, 0] < 1e-12 * top[:, 1])
    hs, v = hs[near], v[near]
    level, level32 = otsu_levels(hs), otsu_levels(hs, "f32")
    second = np.argsort(v, axis=1)[:, -2]
    return hs[level32 != level], hs[(level32 == level) & (second < level)]


def _selected(shape, hists, tag, wants, cap=60):
    """lay the first `cap` histograms out and keep, per (tag, variants that must notice, how many), the first that qualify"""
    S, n = shape
    hists = hists[:cap]
    found = classify([lay_histogram(h, S, n) for h in hists], [{tag} for _ in hists], n, resize=False)
    out, taken = [], set()
    for need_tag, variants, want in wants:
        got = 0
        for i, c in enumerate(found):
            if got < want and (need_tag is None or need_tag in c.tags) and set(variants) <= c.noticed:
                got += 1
                if i not in taken:
                    taken.add(i)
                    out.append((c.patch, {tag}))
    return out


def _ties(shape):
    if shape[0] not in TIE_SIZES:
        return []
    return _selected(shape, tie_histograms(shape[0]), "tie", (("tie_quarters", ("last_of_equals", "higher_quarter"), 10),
                                                              ("tie_runs", ("last_of_equals", "higher_run_of_4"), 6), (None, ("f32",), 6)), cap=100)


def _near_ties(shape):
    if shape[0] not in TIE_SIZES:
        return []
    f32, later = near_tie_histograms(shape[0])
    return (_selected(shape, f32, "near_tie", ((None, ("f32",), 8),)) +
            [(p, t | {"near_tie_later_wins"}) for p, t in _selected(shape, later, "near_tie", ((None, (), 4),), cap=4)])


def _random_small(shape):
    """S <= 11: seeded patches of two to four greys and binary ones -- at S = 1 and 2 together with the flat ones most of what there is"""
    S, n = shape
    if S > 11:
        return []
    rng = np.random.default_rng(_seed(shape, 3))
    out = []
    for i in range(12):
        greys = rng.choice(256, size=int(rng.integers(2, 5)), replace=False) if i % 2 else np.array([0, 255])
        p = rng.choice(greys, size=(S, S)).astype(np.uint8)
        if S >= n:                         # a black perimeter: the interior shows in the codes
            p[0], p[-1], p[:, 0], p[:, -1] = greys.min(), greys.min(), greys.min(), greys.min()
        out.append((p, {"random_small"}))
    return out


RESIZE_HITS = {}
RESIZE_BUDGET = {True: 200, False: 1000}       # patches searched per source: S >= 199, smaller


def _resize_sources(shape, count, rng):
    """binary patches (0 / 255: the level is out of the picture), a black perimeter band so that the interior shows in the codes"""
    S, n = shape
    cell = S / n
    band = max(1, int(np.ceil(cell)))
    noise = rng.integers(0, 2, size=(count, S, S), dtype=np.uint8)
    for a in (noise[:, :band], noise[:, -band:], noise[:, :, :band], noise[:, :, -band:]):
        a[...] = 0
    moved, flipped = np.zeros((count, S, S), np.uint8), np.zeros((count, S, S), np.uint8)
    for i in range(count):
        cells = np.zeros((n, n), np.uint8)
        cells[1:-1, 1:-1] = rng.integers(0, 2, size=(n - 2, n - 2))
        edges = np.clip(np.round(np.arange(n + 1) * cell).astype(int) + np.concatenate([[0], rng.integers(-2, 3, size=n - 1), [0]]), 0, S)
        edges = np.maximum.accumulate(edges)
        at = np.clip(np.searchsorted(edges, np.arange(S), side="right") - 1, 0, n - 1)
        moved[i] = cells[np.ix_(at, at)]
        f = lay_cells(cells, S).copy()
        flip = rng.random((S, S)) < 0.08
        flip[:band] = flip[-band:] = False
        flip[:, :band] = flip[:, -band:] = False
        flipped[i] = f ^ flip.astype(np.uint8)
    return (("noise", noise * np.uint8(255)), ("moved_boundaries", moved * np.uint8(255)), ("flipped_samples", flipped * np.uint8(255)))


def half_cell_patches(shape):
    """a white rectangle over the interior whose one edge runs through the CENTRE of a column of cells, where that centre lies between two
    samples: the cells of that column whose vertical support is all white then hold exactly half of the horizontal weights -- 127.5 in
    exact arithmetic, so that nothing but the f32 rounding of the reference's own operation order decides the bit.  Every such column,
    turned four ways -> [m, S, S] (empty where no cell centre lies between samples)"""
    S, n = shape
    lo, hi = -(-S // n), (n - 1) * S // n
    out = []
    for j in range(1, n - 2):
        if (2 * j + 1) * S % (2 * n) == 0:
            p = np.zeros((S, S), np.uint8)
            p[lo: hi, (2 * j + 1) * S // (2 * n): hi] = 255
            out += [np.rot90(p, t) for t in range(4)]
    return np.array(out, dtype=np.uint8).reshape(-1, S, S)


@functools.lru_cache(maxsize=None)
def resize_search(shape):
    """-> ([(patch, tags)], patches searched): binary patches in which a resize variant changes the outcome (two per variant and source
    first, up to eight per source), and a few plain ones with a cell at 126..129"""
    S, n = shape
    if S <= n:
        return [], 0
    rng = np.random.default_rng(_seed(shape, 4))
    count = RESIZE_BUDGET[S >= 199]
    out, searched = [], 0
    for name, patches in _resize_sources(shape, count, rng) + (("half_cells", half_cell_patches(shape)),):
        if len(patches) == 0:
            continue
        searched += len(patches)
        level = np.zeros(len(patches), np.int64)                 # (0 / 255 patches: the level is 0 whenever both are present)
        base = outcomes(patches, n, levels=level)
        hits = {v: np.array([o != b for o, b in zip(outcomes(patches, n, resize_variant=v, levels=level), base)]) for v in RESIZE_VARIANTS}
        take = []
        for v in RESIZE_VARIANTS:                                # two per variant first, then any up to eight
            take += [i for i in np.flatnonzero(hits[v]).tolist() if i not in take][:2]
        hit = np.any(list(hits.values()), axis=0)
        take += [i for i in np.flatnonzero(hit).tolist() if i not in take][: max(0, 8 - len(take))]
        vals = resize_values(patches, n)
        near = ((vals > 125.5) & (vals < 129.5)).any(axis=(1, 2)) & ~hit
        out += [(patches[i], {"resize", name}) for i in sorted(take)]
        out += [(patches[i], {"resize", name, "plain"}) for i in np.flatnonzero(near)[:1]]
        RESIZE_HITS[(shape, name)] = {v: int(h.sum()) for v, h in hits.items()}
    return out, searched


def _dictionary(shape):
    """real codes of the shape's dictionary, white cells from a high set of greys and black ones from a low set: these decode to markers;
    seeded random interiors that the model reads at tau or more from every code under every rotation: these pass the border test and
    are refused by the filter"""
    S, n = shape
    if S < n:
        return []
    nb, _, codes = du.table(DICT_OF_N[n])
    tau = du.tau_of(DICT_OF_N[n])
    rng = np.random.default_rng(_seed(shape, 5))
    out = []

    def paint(m, turn):
        cells = rng.integers(10, 60, size=(n, n))
        cells[1:-1, 1:-1] = np.where(np.rot90(m, turn) != 0, rng.integers(180, 250, size=m.shape), cells[1:-1, 1:-1])
        return lay_cells(cells.astype(np.uint8), S)

    for i in range(2):
        out.append((paint(du.matrix_of(int(codes[int(rng.integers(0, len(codes)))]), nb), i + 1), {"dictionary", "dictionary_code"}))
    # random damage rarely ends tau from every code of a dense table under every rotation: a walk that never lets the distance fall does
    k = n - 2
    every = np.array([du.code_of(np.rot90(du.matrix_of(int(c), nb), r)) for c in codes for r in range(4)], dtype=np.uint64)

    def nearest(m):
        return int(du.popcount(every ^ np.uint64(du.code_of(m))).min())

    missed = 0
    for _ in range(20):
        m = rng.integers(0, 2, size=(k, k)).astype(np.uint8)
        d = nearest(m)
        for _ in range(3000):
            if d >= tau:
                break
            y, x = int(rng.integers(0, k)), int(rng.integers(0, k))
            m[y, x] ^= 1
            d2 = nearest(m)
            if d2 >= d:
                d = d2
            else:
                m[y, x] ^= 1
        p = paint(m, 0)
        ok, cs = outcomes(p[None], n)[0]
        if ok and du.expect_codes(cs, codes).distance >= tau:
            out.append((p, {"dictionary", "dictionary_missed"}))
            missed += 1
            if missed == 2:
                break
    return out


BUILDERS = (_flat, _extreme, _cell_grey, _ties, _near_ties, _random_small, lambda s: resize_search(s)[0], _dictionary)


@functools.lru_cache(maxsize=None)
def cases(shape):
    """every case of one shape, classified by the models -> [Case]"""
    made = [pt for b in BUILDERS for pt in b(shape)]
    out = classify([p for p, _ in made], [t for _, t in made], shape[1])
    for c in out:
        c.patch.setflags(write=False)
    return out


def summary(shape):
    """counts for the report: cases per tag and per noticed variant"""
    tags, noticed = {}, {}
    for c in cases(shape):
        for t in c.tags:
            tags[t] = tags.get(t, 0) + 1
        for v in c.noticed:
            noticed[v] = noticed.get(v, 0) + 1
    return {"cases": len(cases(shape)), "tags": dict(sorted(tags.items())), "noticed": dict(sorted(noticed.items()))}


# ------------------------------------------------------------------------------------------------------------------
# mosaics
# ------------------------------------------------------------------------------------------------------------------
def grid(S):
    """-> (columns, rows) of tiles a mosaic holds"""
    return (2, 2) if S >= 199 else (8, 6)


@functools.lru_cache(maxsize=None)
def mosaics(shape):
    """-> [(L8 frame, quads [m, 4, 2] u32, the cases of the tiles in quad order)]; every mosaic of a shape has the same size"""
    S, n = shape
    k = block(S)
    cols, rows = grid(S)
    pitch = k * S + GAP
    W, H = GAP + cols * pitch + 2, GAP + rows * pitch + 2
    cs = cases(shape)
    out = []
    for f0 in range(0, len(cs), cols * rows):
        chunk = cs[f0: f0 + cols * rows]
        img = np.full((H, W), BACKGROUND, dtype=np.uint8)
        quads = []
        for s, c in enumerate(chunk):
            x0, y0 = GAP + (s % cols) * pitch, GAP + (s // cols) * pitch
            # block (x, y) covers x0 + kx - k // 2 .. x0 + kx + k // 2: sample (x, y) lands on its centre
            a, b = y0 - k // 2, x0 - k // 2
            img[a: a + k * S, b: b + k * S] = np.repeat(np.repeat(c.patch, k, axis=0), k, axis=1)
            quads.append([[x0, y0], [x0 + k * S, y0], [x0 + k * S, y0 + k * S], [x0, y0 + k * S]])
        img.setflags(write=False)
        out.append((img, np.array(quads, dtype=np.uint32), chunk))
    return out


def oracle_config(oracle, S):
    cfg = oracle.Config.default()
    cfg.homography_sample_size = S
    cfg.min_corner_separation_factor = SEPARATION
    return cfg


def detector_config(S):
    from aruco3_amd.aruco import DetectorConfig

    return DetectorConfig(min_corner_separation_factor=SEPARATION, homography_sample_size=S)


_REFS = {}


def reference(oracle, shape, index):
    """the oracle on mosaic `index` of a shape with its quads: computed once, shared by every test, never written to"""
    key = (shape, index)
    if key not in _REFS:
        nb, _, codes = du.table(DICT_OF_N[shape[1]])
        img, quads, _ = mosaics(shape)[index]
        _REFS[key] = oracle.detect(img, codes, nb, du.tau_of(DICT_OF_N[shape[1]]), config=oracle_config(oracle, shape[0]), quads=quads)
    return _REFS[key]
