"""The threshold tests' own footing, without a GPU: tests/threshold_util.py's numpy reference against the CPU oracle on every batch
tests/test_gpu_threshold_paths.py runs, and that those batches would show a kernel with one of three plain mistakes -- the comparison
one count off, a window one column short, the unclipped area -- so that passing the GPU module means something."""
import numpy as np
import pytest

from tests import threshold_util as tu


def _rid(r):
    return f"r{r}"


@pytest.fixture(scope="module", params=tu.ALL_RADII, ids=_rid)
def rendered(request):
    """every batch of one radius, rendered and thresholded by the reference once: [(case, names, pixels, grey, image, margin)]"""
    out = []
    for c in tu.cases_of(request.param):
        names, px, grey = c.frames()
        thr, margin = tu.reference(grey, c.radius)
        assert np.abs(margin).max() < 2**31
        out.append((c, names, px, grey, thr, margin.astype(np.int32)))
    return request.param, out


def test_reference_equals_oracle(rendered, oracle):
    """into_luma8 and adaptive_threshold of oracle/a3_oracle.c (u32, per pixel) give what the numpy versions give, frame by frame"""
    radius, batches = rendered
    for c, names, px, grey, thr, _ in batches:
        for i, name in enumerate(names):
            img = px[i, ..., 0] if c.fmt == "L8" else (px[i][..., [2, 1, 0, 3]] if c.fmt == "BGRA8" else px[i])
            assert np.array_equal(oracle.to_luma8(img), grey[i]), (c.id, name)
            if not name.startswith("noise") and c.fmt != "L8":
                assert np.array_equal(grey[i], px[i, ..., 0]), (c.id, name)   # R = G = B comes through unchanged
            assert np.array_equal(oracle.adaptive_threshold(grey[i], radius), thr[i]), (c.id, name)


def _wrong_short_window(grey, radius):
    """the window one column short on the right"""
    h, w = grey.shape[-2:]
    y0, y1 = tu.windows(h, radius)
    x0, x1 = tu.windows(w, radius)
    x1 = np.minimum(np.arange(w, dtype=np.int64) + int(radius), w - 1)
    area = (y1 - y0)[:, None] * (x1 - x0)[None, :]
    return (grey.astype(np.int64) + 1) * area - tu.box_sums(grey, y0, y1, x0, x1) > 0


def _wrong_unclipped_area(grey, radius):
    """(2R+1)^2 for the area wherever the window is clipped.  (Capped at 2^40: from 255 x the frame's pixels on every larger area gives
    the same image, and (2^32)^2 does not fit an int64.)"""
    h, w = grey.shape[-2:]
    y0, y1 = tu.windows(h, radius)
    x0, x1 = tu.windows(w, radius)
    area = min((2 * int(radius) + 1) ** 2, 1 << 40)
    return (grey.astype(np.int64) + 1) * area - tu.box_sums(grey, y0, y1, x0, x1) > 0


def test_contents_discriminate(rendered):
    """Three wrong thresholds against the right one.  `margin >= 0` must show on a knife frame; the two wrong window shapes must show on
    at least one knife, impulse or noise frame of the radius."""
    radius, batches = rendered
    seen = {"ge": False, "short": False, "area": False}
    for c, names, _, grey, thr, margin in batches:
        right = thr > 0
        for i, name in enumerate(names):
            if not name.startswith(("knife", "impulses", "noise")):
                continue
            if name.startswith("knife"):
                seen["ge"] |= bool(((margin[i] >= 0) != right[i]).any())
            seen["short"] |= bool((_wrong_short_window(grey[i], radius) != right[i]).any())
            seen["area"] |= bool((_wrong_unclipped_area(grey[i], radius) != right[i]).any())
    assert all(seen.values()), (radius, seen)


def test_knife_condition(rendered):
    """Every knife frame of 10 000 pixels or more holds at least 8 pixels ON the comparison's boundary (margin 0: black, and white under
    `<=`) and at least 8 one count inside it (margin 1: white, and black if a count is lost).

    Where one window covers the whole frame (radius >= max(h, w) - 1: the brute-force radii from 200 on at 140 x 150) no frame can hold
    both: every pixel sees the same sum S over the same area N, so a pixel's margin is (L + 1) N - S, and two margins differ by a
    multiple of N.  There the two knife frames share the work -- knife(0) has as many highs as lows, every low pixel at margin 0;
    knife(253) one high fewer, every low pixel at margin 1 -- and each must hold its 8."""
    radius, batches = rendered
    for c, names, _, _, _, margin in batches:
        if c.h * c.w < 10000:
            continue
        counts = {name: (int((margin[i] == 0).sum()), int((margin[i] == 1).sum())) for i, name in enumerate(names) if name.startswith("knife")}
        assert counts, c.id
        if tu.window_covers_frame(c.h, c.w, radius):
            assert counts["knife0"][0] >= 8 and counts["knife253"][1] >= 8, (c.id, counts)
        else:
            assert all(z >= 8 and o >= 8 for z, o in counts.values()), (c.id, counts)


@pytest.mark.parametrize("radius", tu.K1_RADII)
def test_impulses_blacken_their_footprints(radius):
    """the impulse frames are what their docstring says: disjoint footprints, black exactly there, at the lanes' and strips' edges"""
    R = radius
    for h, w in ((100, 1009), (100, 1985), (2 * R + 1, 1008), (R, 17), (1, 17)):
        rows = tu.k1_geometry(10, w, h, R)[2]
        sites = tu.impulse_sites(h, w, R, rows)
        cover = np.zeros((h, w), np.int32)
        for y, x in sites:
            cover[max(y - R, 0): y + R + 1, max(x - R, 0): x + R + 1] += 1
        assert sites and cover.max() == 1
        g = tu.impulses(R, rows)(None, h, w)
        black = cover == 1
        black[tuple(np.array(sites).T)] = False
        assert np.array_equal(tu.reference(g, R)[0] == 0, black)
        if h == 100:
            xs, ys = {x for _, x in sites}, {y for y, _ in sites}
            assert {x for x in range(1, w) if x % 16 in (0, 15)} <= xs
            assert {x for x in (975, 976, 991, 992, 1007, 1008) if x < w} <= xs
            assert set(range(R)) | set(range(w - R, w)) <= xs
            assert set(range(R)) | set(range(h - R, h)) | {0, 16, 17, 33, 34, 50, 51, 67, 68, 84, 85, 99} <= ys
