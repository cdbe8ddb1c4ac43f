"""Independent cross-checks of the oracle's image stages (parity UNPINNED for stages C, D, E, G, H, K, L -- the reference
holds no image fixture and cannot be built here).  None of this pins the oracle to the crates' bytes; it checks the restatement against
implementations and definitions that were NOT written from the same reading of the crates:
  * resize(.., Triangle) (image 0.25) against Pillow's BILINEAR resize -- the same filter family and sampling convention
    (support scaled by the ratio, centre (o + 0.5) * ratio, weights normalised) in Pillow's own fixed-point arithmetic: within one level;
  * otsu_level (imageproc, A8) against the definition -- the threshold that maximises the between-class variance, first maximum;
  * adaptive_threshold (A2) against a direct window loop;
  * find_contours (A3) against the topology scipy.ndimage.label reports: one outer border per 8-connected foreground component, one
    hole border per 4-connected background component that does not reach the frame, and the union of all border points = the foreground
    pixels with a background 4-neighbour (images whose foreground keeps off columns 0 and W - 1, where A3's guards do not bite);
  * warp_into (imageproc, A7) against the plain bilinear sample in float64 of the same f32 inverse map, without the three truncations;
  * into_luma8 (A1) against the integers of its definition for every RGB triple."""
import numpy as np
import pytest
from scipy import ndimage

PIL = pytest.importorskip("PIL.Image")


def _rng(seed):
    return np.random.default_rng(seed)


@pytest.mark.parametrize("n", [6, 7, 8, 10])
def test_triangle_resize_agrees_with_pillows_bilinear_within_one_level(oracle, n):
    worst = 0
    for seed in range(40):
        r = _rng(seed)
        if seed % 2:       # a thresholded patch (what the pipeline feeds it): 0 / 255 in blobs
            patch = (ndimage.uniform_filter(r.random((49, 49)), 5) > 0.5).astype(np.uint8) * 255
        else:
            patch = r.integers(0, 256, (49, 49), dtype=np.uint8)
        got = oracle.resize_triangle(patch, n, n).astype(np.int32)
        ref = np.asarray(PIL.fromarray(patch, mode="L").resize((n, n), resample=PIL.BILINEAR, reducing_gap=None), dtype=np.int32)
        worst = max(worst, int(np.abs(got - ref).max()))
    assert worst <= 1, worst


def test_otsu_level_is_the_first_maximum_of_the_between_class_variance(oracle):
    for seed in range(60):
        r = _rng(100 + seed)
        kind = seed % 3
        if kind == 0:
            img = r.integers(0, 256, (49, 49), dtype=np.uint8)
        elif kind == 1:     # two humps
            img = np.clip(np.where(r.random((49, 49)) < 0.4, r.normal(60, 12, (49, 49)), r.normal(190, 20, (49, 49))), 0, 255).astype(np.uint8)
        else:               # few levels (ties)
            img = r.choice(np.array([0, 17, 200, 255], dtype=np.uint8), (49, 49))
        hist = np.bincount(img.reshape(-1), minlength=256).astype(np.float64)
        lv = np.arange(256, dtype=np.float64)
        best, best_t = 0.0, 0
        for t in range(256):
            wb, wf = hist[: t + 1].sum(), hist[t + 1:].sum()
            if wb == 0 or wf == 0:
                continue
            mb, mf = (hist[: t + 1] * lv[: t + 1]).sum() / wb, (hist[t + 1:] * lv[t + 1:]).sum() / wf
            v = wb * wf * (mb - mf) ** 2
            if v > best:
                best, best_t = v, t
        assert oracle.otsu_level(img) == best_t, seed


def test_adaptive_threshold_against_a_window_loop(oracle):
    r = _rng(7)
    img = r.integers(0, 256, (37, 53), dtype=np.uint8)
    img[10:20, 5:30] = 200            # a uniform region: pixel == mean -> white (quirk Q3)
    for radius in (1, 3, 7, 9):
        got = oracle.adaptive_threshold(img, radius)
        h, w = img.shape
        want = np.zeros_like(img)
        for y in range(h):
            y0, y1 = max(0, y - radius), min(h - 1, y + radius)
            for x in range(w):
                x0, x1 = max(0, x - radius), min(w - 1, x + radius)
                win = img[y0: y1 + 1, x0: x1 + 1].astype(np.uint64)
                want[y, x] = 255 if int(img[y, x]) >= int(win.sum()) // win.size else 0
        assert np.array_equal(got, want), radius


def _blobs(seed, h=96, w=128, density=0.5, smooth=3):
    r = _rng(seed)
    img = (ndimage.uniform_filter(r.random((h, w)), smooth) > density).astype(np.uint8) * 255
    img[:, 0] = 0; img[:, -1] = 0     # A3's x > 0 / x + 1 < W guards never bite
    return img


@pytest.mark.parametrize("seed,smooth,density", [(s, sm, de) for s in range(6) for sm, de in ((1, 0.5), (3, 0.5), (5, 0.48), (2, 0.62))])
def test_find_contours_topology_against_connected_components(oracle, seed, smooth, density):
    img = _blobs(seed, smooth=smooth, density=density)
    h, w = img.shape
    contours, btype, parent = oracle.find_contours(img)
    fg = img > 0
    _, n_fg = ndimage.label(fg, structure=np.ones((3, 3), int))                       # 8-connected foreground
    lab_bg, n_bg = ndimage.label(~fg, structure=[[0, 1, 0], [1, 1, 1], [0, 1, 0]])    # 4-connected background
    rim = np.zeros_like(fg); rim[0, :] = rim[-1, :] = rim[:, 0] = rim[:, -1] = True
    outside = set(np.unique(lab_bg[rim & ~fg])) - {0}
    n_holes = n_bg - len(outside)
    bt = np.asarray(btype)
    assert int((bt == 0).sum()) == n_fg, "one outer border per 8-connected component"
    assert int((bt == 1).sum()) == n_holes, "one hole border per enclosed 4-connected background component"
    # every border point is a foreground pixel; together they are exactly the foreground pixels with a background 4-neighbour (the frame counts as background)
    pts = np.concatenate([np.asarray(c).reshape(-1, 2) for c in contours]) if len(contours) else np.zeros((0, 2), int)
    on_border = np.zeros_like(fg)
    on_border[pts[:, 1], pts[:, 0]] = True
    padded = np.pad(fg, 1)
    has_bg4 = fg & ~(padded[:-2, 1:-1] & padded[2:, 1:-1] & padded[1:-1, :-2] & padded[1:-1, 2:])
    assert np.array_equal(on_border, has_bg4)
    # consecutive points of a border are 8-neighbours, and so are its last and first; discovery order is raster order of the start points
    starts = []
    for c in contours:
        c = np.asarray(c, dtype=np.int64).reshape(-1, 2)
        if len(c) > 1:
            d = np.abs(np.diff(np.vstack([c, c[:1]]), axis=0)).max(axis=1)
            assert d.max() == 1
        starts.append(int(c[0][1]) * w + int(c[0][0]))
    assert starts == sorted(starts)


def _solve_longdouble(frm, to):
    """the same 8 x 8 DLT system solved in extended precision with full pivoting: what ANY correct f64 solver approximates"""
    A = np.zeros((8, 8), np.longdouble); b = np.zeros(8, np.longdouble)
    for i in range(4):
        xf, yf, x, y = (np.longdouble(v) for v in (frm[2 * i], frm[2 * i + 1], to[2 * i], to[2 * i + 1]))
        A[2 * i] = [0, 0, 0, -xf, -yf, -1, y * xf, y * yf]
        A[2 * i + 1] = [xf, yf, 1, 0, 0, 0, -x * xf, -x * yf]
        b[2 * i], b[2 * i + 1] = -y, x
    n = 8
    perm = list(range(n))
    for k in range(n):
        sub = np.abs(A[k:, k:])
        r, c = np.unravel_index(np.argmax(sub), sub.shape)
        r += k; c += k
        A[[k, r]] = A[[r, k]]; b[[k, r]] = b[[r, k]]
        A[:, [k, c]] = A[:, [c, k]]; perm[k], perm[c] = perm[c], perm[k]
        for i in range(k + 1, n):
            f = A[i, k] / A[k, k]
            A[i, k:] -= f * A[k, k:]; b[i] -= f * b[k]
    x = np.zeros(n, np.longdouble)
    for i in range(n - 1, -1, -1):
        x[i] = (b[i] - (A[i, i + 1:] * x[i + 1:]).sum()) / A[i, i]
    out = np.zeros(n, np.longdouble)
    for i, p in enumerate(perm):
        out[p] = x[i]
    return out


def test_control_point_solve_is_insensitive_to_the_solver(oracle):
    """VERDICT r05 'least certain restatement': oracle/a3_oracle.c solves the 8 x 8 system by LU with partial pivoting in f64; imageproc
    0.25.0 may take another nalgebra path.  Measured here: the f32 matrix the pipeline uses (the f64 solution rounded to f32) is the
    same as that of an extended-precision solve in all but a few entries per thousand, those differ by one f32 ulp, and the warped
    49 x 49 patch then differs in at most a handful of pixels by one grey level -- never enough to move a bit of the 7 x 7 grid."""
    r = _rng(11)
    S = 49
    to = np.array([0, 0, S, 0, S, S, 0, S], np.float32)
    grey = r.integers(0, 256, (480, 640), dtype=np.uint8)
    entries = diff_entries = 0
    worst_ulp = 0
    patch_px = patch_diff = 0
    for case in range(3000):
        c = r.uniform([80, 80], [560, 400]); side = r.uniform(30, 140); ang = r.uniform(0, 2 * np.pi)
        base = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], float) * side / 2
        rot = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        quad = np.rint(base @ rot.T * r.uniform(0.8, 1.2, (4, 1)) + c).astype(np.float32).reshape(8)      # integer corners, as the pipeline's
        ok, t, inv = oracle.from_control_points(quad, to)
        assert ok
        ref = _solve_longdouble(quad.astype(np.float64), to.astype(np.float64)).astype(np.float64).astype(np.float32)
        got = t[:8]
        entries += 8
        d = got.view(np.int32).astype(np.int64) - ref.view(np.int32).astype(np.int64)
        tiny = np.abs(ref) < 1e-9          # an entry that is exactly 0 (two corners in one column): the f64 LU leaves 1e-17 there -- times a
        assert np.abs(got[tiny]).max(initial=0.0) < 1e-12          # coordinate below 2^16 that is nothing next to the row's other terms
        d[tiny] = 0
        diff_entries += int((d != 0).sum())
        worst_ulp = max(worst_ulp, int(np.abs(d).max()))
        if (d != 0).any() and patch_px < 49 * 49 * 40:
            # what such a difference does downstream: invert the alternative matrix the oracle's way and warp with both
            t2 = np.concatenate([ref, [1.0]]).astype(np.float32)
            m = t2.reshape(3, 3).astype(np.float32)
            cof = np.array([[m[1, 1] * m[2, 2] - m[1, 2] * m[2, 1], -(m[0, 1] * m[2, 2] - m[0, 2] * m[2, 1]), m[0, 1] * m[1, 2] - m[0, 2] * m[1, 1]],
                            [-(m[1, 0] * m[2, 2] - m[1, 2] * m[2, 0]), m[0, 0] * m[2, 2] - m[0, 2] * m[2, 0], -(m[0, 0] * m[1, 2] - m[0, 2] * m[1, 0])],
                            [m[1, 0] * m[2, 1] - m[1, 1] * m[2, 0], -(m[0, 0] * m[2, 1] - m[0, 1] * m[2, 0]), m[0, 0] * m[1, 1] - m[0, 1] * m[1, 0]]], np.float32)
            inv2 = (cof / cof[2, 2]).astype(np.float32).reshape(9)
            pa, pb = oracle.warp_into(grey, inv, S, S), oracle.warp_into(grey, inv2, S, S)
            patch_px += S * S
            patch_diff += int((pa != pb).sum())
            assert np.abs(pa.astype(int) - pb.astype(int)).max() <= 255       # (noise image: a tap moved across a pixel edge may change a level a lot)
    assert worst_ulp <= 1, worst_ulp
    assert diff_entries <= entries * 0.02, (diff_entries, entries)
    if patch_px:
        assert patch_diff <= patch_px * 0.01, (patch_diff, patch_px)
    print(f"solver sensitivity: {diff_entries}/{entries} f32 entries differ (by {worst_ulp} ulp at most); {patch_diff}/{patch_px} patch pixels differ on a noise image")


def _bilinear_f64(img, inv, S):
    """(values f64 [S, S], inside bool [S, S]): the f32 matrix `inv` applied to the output pixels in f64, imageproc's inside test, and the
    bilinear sample with nothing truncated"""
    h, w = img.shape
    m = np.asarray(inv, dtype=np.float32).astype(np.float64)
    xs, ys = np.meshgrid(np.arange(S, dtype=np.float64), np.arange(S, dtype=np.float64))
    den = m[6] * xs + m[7] * ys + m[8]
    px, py = (m[0] * xs + m[1] * ys + m[2]) / den, (m[3] * xs + m[4] * ys + m[5]) / den
    left, top = np.floor(px), np.floor(py)
    inside = (left >= 0) & (left + 1 < w) & (top >= 0) & (top + 1 < h)
    l, t = np.where(inside, left, 0).astype(np.int64), np.where(inside, top, 0).astype(np.int64)
    rw, bw = px - left, py - top
    f = img.astype(np.float64)
    r, b = np.minimum(l + 1, w - 1), np.minimum(t + 1, h - 1)
    v = (1 - bw) * ((1 - rw) * f[t, l] + rw * f[t, r]) + bw * ((1 - rw) * f[b, l] + rw * f[b, r])
    return v, inside


def test_warp_into_against_a_float64_bilinear_sample(oracle):
    """imageproc truncates to u8 three times per sample (the two horizontal lerps, then the vertical one): each costs less than a level
    (row values in (T - 1, T] and (B - 1, B] blend to (V - 1, V], the last truncation gives (V - 2, V]), so the oracle's patch lies within
    2.0 grey levels of the untruncated value wherever both call the sample inside.  The two can disagree about inside / outside only where
    the f32 and the f64 evaluation of the map fall on different sides of an edge of the frame: a few pixels in a million at most (none
    of these 960 400); the cap of 1e-4 is a condition on the inputs, far above that.  The oracle's verdict is read off its patch: 0 is
    outside, and a sample whose untruncated value is below 2 may be 0 either way."""
    r = _rng(21)
    S, w, h = 49, 160, 120
    noise = r.integers(0, 256, (h, w), dtype=np.uint8)
    yy, xx = np.mgrid[0:h, 0:w]
    smooth = np.clip(127.5 + 80 * np.sin(xx / 9.0) * np.cos(yy / 13.0) + 40 * np.sin((xx + yy) / 23.0), 0, 255).astype(np.uint8)
    to = np.array([0, 0, S, 0, S, S, 0, S], np.float32)
    pixels = disagree = 0
    worst = 0.0
    for case in range(400):
        img = noise if case % 2 == 0 else smooth
        c = r.uniform([20, 20], [w - 20, h - 20]); side = r.uniform(8, 110); ang = r.uniform(0, 2 * np.pi)
        base = np.array([[-1, -1], [1, -1], [1, 1], [-1, 1]], float) * side / 2
        rot = np.array([[np.cos(ang), -np.sin(ang)], [np.sin(ang), np.cos(ang)]])
        quad = np.clip(np.rint(base @ rot.T * r.uniform(0.6, 1.4, (4, 1)) + c), 0, 65535).astype(np.float32).reshape(8)   # some reach past the frame
        ok, _, inv = oracle.from_control_points(quad, to)
        if not ok:
            continue
        got = oracle.warp_into(img, inv, S, S).astype(np.float64)
        ref, inside = _bilinear_f64(img, inv, S)
        got_inside = got != 0        # (an inside sample of value 0 counts as agreeing with either verdict below)
        both = inside & got_inside
        disagree += int((got_inside & ~inside).sum()) + int((inside & ~got_inside & (ref >= 2.0)).sum())
        pixels += S * S
        if both.any():
            worst = max(worst, float(np.abs(got - ref)[both].max()))
    print(f"warp_into vs float64 bilinear: worst {worst:.3f} levels over {pixels} pixels, inside / outside disagreement {disagree}")
    assert pixels == 400 * S * S
    assert worst <= 2.0, worst
    assert disagree <= pixels * 1e-4, (disagree, pixels)


def test_to_luma8_is_the_integer_definition_for_every_rgb_triple(oracle):
    """L = (2126 R + 7152 G + 722 B) / 10000, truncating, for all 2^24 triples; the same with an alpha byte that must not matter"""
    g, b = np.meshgrid(np.arange(256, dtype=np.uint32), np.arange(256, dtype=np.uint32), indexing="ij")
    rng = _rng(5)
    for r0 in range(0, 256, 16):
        rgb = np.empty((16 * 256, 256, 3), dtype=np.uint8)
        rr = np.repeat(np.arange(r0, r0 + 16, dtype=np.uint32), 256)[:, None]
        rgb[..., 0] = rr
        rgb[..., 1] = np.tile(g, (16, 1))
        rgb[..., 2] = np.tile(b, (16, 1))
        want = ((2126 * rgb[..., 0].astype(np.uint64) + 7152 * rgb[..., 1].astype(np.uint64) + 722 * rgb[..., 2].astype(np.uint64)) // 10000).astype(np.uint8)
        assert np.array_equal(oracle.to_luma8(rgb), want), r0
        rgba = np.concatenate([rgb, rng.integers(0, 256, rgb.shape[:2] + (1,), dtype=np.uint8)], axis=2)
        assert np.array_equal(oracle.to_luma8(rgba), want), r0
