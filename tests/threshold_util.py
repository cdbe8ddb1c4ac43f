"""The threshold stage's test inputs: a plain reference, frame contents that sit on the comparison's boundary, and the one table of
(radius, shape, format, contents) that tests/test_threshold_reference.py (CPU: the reference against the oracle, and that the
contents discriminate) and tests/test_gpu_threshold_paths.py (the kernels against the reference) both walk.  No GPU in here.

    white iff L >= floor(sum / area) over the window clipped to the image  <=>  margin = (L + 1) * area - sum > 0
"""
import numpy as np

FORMATS = ("RGB8", "RGBA8", "BGRA8", "L8")
CHANNELS = {"RGB8": 3, "RGBA8": 4, "BGRA8": 4, "L8": 1}


# ---- the reference ---------------------------------------------------------------------------------------------------------
def windows(n, radius):
    """first and one-past-last index of the window around every position 0..n-1, clipped to 0..n-1"""
    i = np.arange(n, dtype=np.int64)
    return np.maximum(i - int(radius), 0), np.minimum(i + int(radius), n - 1) + 1


def box_sums(grey, y0, y1, x0, x1):
    """sum of grey over rows y0[y] .. y1[y] - 1 and columns x0[x] .. x1[x] - 1 for every (y, x), from an integral image in int64;
    grey may carry leading batch axes"""
    g = np.asarray(grey).astype(np.int64)
    I = np.zeros(g.shape[:-2] + (g.shape[-2] + 1, g.shape[-1] + 1), np.int64)
    I[..., 1:, 1:] = g.cumsum(-2).cumsum(-1)
    Y0, Y1, X0, X1 = y0[:, None], y1[:, None], x0[None, :], x1[None, :]
    return I[..., Y1, X1] - I[..., Y0, X1] - I[..., Y1, X0] + I[..., Y0, X0]


def reference(grey, radius):
    """adaptive_threshold(grey, radius) in numpy and int64 -> (image of 0 / 255, margin).  Written apart from oracle/a3_oracle.c
    (u32, a loop per pixel); tests/test_threshold_reference.py holds the two against each other."""
    g = np.asarray(grey)
    h, w = g.shape[-2:]
    y0, y1 = windows(h, radius)
    x0, x1 = windows(w, radius)
    area = (y1 - y0)[:, None] * (x1 - x0)[None, :]
    margin = (g.astype(np.int64) + 1) * area - box_sums(g, y0, y1, x0, x1)
    return np.where(margin > 0, 255, 0).astype(np.uint8), margin


def window_covers_frame(h, w, radius):
    """every pixel's clipped window is the whole frame"""
    return radius >= max(h, w) - 1


# ---- the strip choice of the two fused kernels ------------------------------------------------------------------------------
# Mirrors of aruco3_amd/csrc/a3_threshold_plan.h, for building test shapes without a compiler; tests/test_threshold_plan.py holds them
# against the compiled planner on every shape the tables below use.
K1_STRIP_COLS = 992    # T_OUT: output columns per wave
K1_FLUSH_ROWS = 128    # kFlushRows: rows of result bits a wave parks in LDS between bursts of stores
RING_LDS_ROWS8 = 19    # kRingLdsRows8: rows of ring a wave may keep in LDS with two waves per SIMD


def _strips(n, w, h, radius, out_cols, slots):
    """plan_strips: time ~ rounds x (rows per strip + 2R), strips of at least 16 rows, the smaller strip count on a tie"""
    strips_x = -(-w // out_cols)
    cols = strips_x * n
    best_sy, best_cost = 1, None
    for sy in range(1, max(1, h // 16) + 1):
        rows = -(-h // sy)
        waves = cols * -(-h // rows)
        cost = -(-waves // slots) * (rows + 2 * radius)
        if best_cost is None or cost < best_cost:
            best_sy, best_cost = sy, cost
    rows_per_wave = -(-h // best_sy)
    return strips_x, -(-h // rows_per_wave), rows_per_wave


def k1_geometry(n, w, h, radius):
    """(strips_x, strips_y, rows_per_wave) of radii 1..7 for n frames of w x h: plan_k1, 2048 wave slots.  A wave flushes its parked
    rows every min(K1_FLUSH_ROWS, rows_per_wave) rows (rounded up to the row loop's unroll), and odd strips walk upwards."""
    return _strips(n, w, h, radius, K1_STRIP_COLS, 2048)


def ring_geometry(n, w, h, radius, fmt="RGB8", fast=True):
    """(strips_x, strips_y, rows_per_wave, flush_rows) of radii 8..31: plan_ring.  fast: vector loads (aligned layout, w % 16 == 0).
    Eight waves per CU while the ring's LDS part is at most RING_LDS_ROWS8 rows, else four; a wave's parked rows share its part of the
    160 KB with the ring."""
    last8 = 19 if not fast else {"L8": 28, "YUYV8": 27, "UYVY8": 27, "RGB8": 26}.get(fmt, 24)
    reg = radius if radius + 1 <= RING_LDS_ROWS8 or radius > last8 else 2 * radius + 1 - RING_LDS_ROWS8
    nb = 2 * radius + 1 - reg
    wpc = 8 if nb <= RING_LDS_ROWS8 else 4
    sx, sy, rows = _strips(n, w, h, radius, (60 if radius > 15 else 62) * 16, 256 * wpc)
    room = (160 * 1024 // wpc - 64 - nb * 1024) // 128 - 3
    return sx, sy, rows, max(1, min(K1_FLUSH_ROWS, rows, room))


# ---- contents: grey planes as functions of (rng, h, w) ---------------------------------------------------------------------
def noise(rng, h, w):
    return rng.integers(0, 256, (h, w), dtype=np.uint8)


def ramp(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return ((xx * 3 + yy * 5) % 256).astype(np.uint8)


def all255(rng, h, w):
    return np.full((h, w), 255, np.uint8)


def all0(rng, h, w):
    return np.zeros((h, w), np.uint8)


def knife(v, tilt=0):
    """Every pixel v + 1, a random eighth v ("lows") and another eighth, less `tilt` pixels, v + 2 ("highs").  A low pixel's margin is
    the number of lows minus the number of highs in its window, so many pixels sit at margin 0 and 1: on the boundary of
    sum < (L + 1) * area and one count inside it.  Where one window covers the whole frame every low pixel's margin IS `tilt` -- the
    margins of two grey levels then differ by multiples of the frame's area, and no single frame can hold both a 0 and a 1 -- so the
    table runs knife(0) with tilt 0 and knife(253) with tilt 1."""
    def f(rng, h, w):
        n = h * w
        k = n // 8
        order = rng.permutation(n)
        g = np.full(n, v + 1, np.uint8)
        g[order[:k]] = v
        g[order[k: max(k, 2 * k - tilt)]] = v + 2
        return g.reshape(h, w)
    return f


def impulse_sites(h, w, radius, row_strips):
    """[(y, x)] of single pixels with pairwise disjoint (2R+1)^2 footprints, placed at: both sides of every lane boundary
    (x = 15, 16 mod 16), both sides of the column strip's seam (975, 976, 991, 992, 1007, 1008), the first and last R rows and columns,
    the first and last row of every row strip (row_strips: rows per strip)."""
    R = int(radius)
    xs = [x for x in (975, 976, 991, 992, 1007, 1008) if x < w]
    xs += [x for x in range(w) if x % 16 in (15, 0) and x > 0]
    ys = []
    for s in range(0, h, row_strips):
        ys += [s, min(s + row_strips, h) - 1]
    xs, ys = list(dict.fromkeys(xs)), list(dict.fromkeys(ys))
    blocked = np.zeros((h, w), bool)   # centres whose footprint would touch one already placed
    sites = []

    def place(y, x):
        if not (0 <= y < h and 0 <= x < w) or blocked[y, x]:
            return False
        blocked[max(y - 2 * R, 0): y + 2 * R + 1, max(x - 2 * R, 0): x + 2 * R + 1] = True
        sites.append((y, x))
        return True

    # the borders first, on diagonals that keep the footprints apart: column k and column w - 1 - k in a band of rows of their own,
    # row k and row h - 1 - k in a band of columns of their own (what does not fit a small frame is left out)
    for k in range(R):
        place(k * (2 * R + 1) + R, k)
        place(k * (2 * R + 1) + R, w - 1 - k)
    for k in range(R):
        place(k, 4 * R + 2 + k * (2 * R + 1))
        place(h - 1 - k, 4 * R + 2 + k * (2 * R + 1))
    for i, x in enumerate(xs):          # every interesting column once, at an interesting row where one is free
        for j in range(len(ys)):
            if place(ys[(i + j) % len(ys)], x):
                break
    for j, y in enumerate(ys):          # every interesting row once more
        for i in range(len(xs)):
            if place(y, xs[(7 * j + i) % len(xs)]):
                break
    return sites


def impulses(radius, row_strips):
    """255 at impulse_sites on a background of 0, radii 1..7: the area is at most 225 < 255, so the mean of a window that holds an impulse
    is at least 1 and of any other 0 -- the black pixels are exactly the footprints (less the impulses themselves, which are white)."""
    def f(rng, h, w):
        g = np.zeros((h, w), np.uint8)
        for y, x in impulse_sites(h, w, radius, row_strips):
            g[y, x] = 255
        return g
    return f


def stripes_cols(rng, h, w):
    return np.broadcast_to(((np.arange(w) & 1) * 255).astype(np.uint8)[None, :], (h, w)).copy()


def stripes_rows(rng, h, w):
    return np.broadcast_to(((np.arange(h) & 1) * 255).astype(np.uint8)[:, None], (h, w)).copy()


def checkerboard(rng, h, w):
    yy, xx = np.mgrid[0:h, 0:w]
    return (((xx + yy) & 1) * 255).astype(np.uint8)


# ---- the table -------------------------------------------------------------------------------------------------------------
class Case:
    """One batch: `contents` (name -> function) rendered at h x w in one pixel format, thresholded with `radius`."""

    def __init__(self, path, radius, h, w, fmt, contents, salt=0):
        self.path, self.radius, self.h, self.w, self.fmt, self.contents, self.salt = path, radius, h, w, fmt, contents, salt

    @property
    def id(self):
        return f"{self.path}-r{self.radius}-{self.h}x{self.w}-{self.fmt}"

    def greys(self):
        """{name: grey plane}; every content draws from a generator of its own, so dropping one changes no other"""
        out = {}
        for i, (name, fn) in enumerate(self.contents.items()):
            rng = np.random.default_rng([self.radius % (1 << 32), self.h, self.w, FORMATS.index(self.fmt), i, self.salt])
            out[name] = fn(rng, self.h, self.w)
        return out

    def frames(self):
        """(names, pixels (n, h, w, channels), grey planes (n, h, w)).  `noise` is drawn per channel (the luma weights and the byte order
        count); every other content has R = G = B = the grey level, which into_luma8 returns unchanged (2126 + 7152 + 722 = 10000),
        so the knife stays on its edge in every format.  The fourth byte is noise: nobody may read it."""
        greys = self.greys()
        c = CHANNELS[self.fmt]
        rng = np.random.default_rng([self.radius % (1 << 32), self.h, self.w, FORMATS.index(self.fmt), 99, self.salt])
        px = np.empty((len(greys), self.h, self.w, c), np.uint8)
        for i, (name, g) in enumerate(greys.items()):
            if c == 1:
                px[i, ..., 0] = g
                continue
            px[i, ..., :3] = rng.integers(0, 256, (self.h, self.w, 3), dtype=np.uint8) if name.startswith("noise") else g[..., None]
            if c == 4:
                px[i, ..., 3] = rng.integers(0, 256, (self.h, self.w), dtype=np.uint8)
        grey = np.stack([luma(px[i], self.fmt) for i in range(len(greys))])
        return list(greys), px, grey


def luma(px, fmt):
    """into_luma8 of one frame (h, w, channels) in numpy: (2126 R + 7152 G + 722 B) / 10000, truncating"""
    if CHANNELS[fmt] == 1:
        return px[..., 0].copy()
    p = px.astype(np.int64)
    r, b = (p[..., 2], p[..., 0]) if fmt == "BGRA8" else (p[..., 0], p[..., 2])
    return ((2126 * r + 7152 * p[..., 1] + 722 * b) // 10000).astype(np.uint8)


K1_RADII = (1, 2, 3, 4, 5, 6, 7)
RING_RADII = (8, 15, 16, 19, 27, 31)   # 19: the first with 19 rows of ring in LDS and a longer register part; 27: RGB8 back at R | R + 1
SEPARABLE_RADII = (32, 33, 64, 127, 128)
BRUTE_RADII = (129, 200, 1000, 65535, 2**31 - 1)
ALL_RADII = K1_RADII + RING_RADII + SEPARABLE_RADII + BRUTE_RADII

K1_WIDTHS = (1, 15, 16, 17, 64, 991, 992, 993, 1008, 1009, 1985)   # 993: a second column strip; 1985: a third


def k1_heights(R):
    # 100 rows: six strips of 17 rows, alternately walking down and up, and the FAST row loop overruns each into clamped rows
    return sorted({1, R, R + 1, 2 * R, 2 * R + 1, 2 * R + 2, 33, 100})


def k1_contents(R, h, w, n=10):
    rows = k1_geometry(n, w, h, R)[2]
    return {"noise": noise, "ramp": ramp, "all255": all255, "all0": all0, "knife0": knife(0), "knife253": knife(253, 1),
            "impulses": impulses(R, rows), "stripes_cols": stripes_cols, "stripes_rows": stripes_rows, "checkerboard": checkerboard}


def k1_cases(R):
    """radii 1..7: every height at widths 17 and 1008, every width at heights 2R+1 and 100; all four formats at widths 1008 and 1009"""
    shapes = [(h, w) for h in k1_heights(R) for w in (17, 1008)] + [(h, w) for h in (2 * R + 1, 100) for w in K1_WIDTHS]
    out = []
    for h, w in dict.fromkeys(shapes):
        for fmt in (FORMATS if w in (1008, 1009) else ("RGB8",)):
            out.append(Case("k1", R, h, w, fmt, k1_contents(R, h, w)))
    return out


def ring_cases(R):
    """radii 8..31 on what tests/test_gpu_parity.py::test_threshold_windows_8_to_31 leaves out: the comparison's boundary and the
    largest sums, per-pixel loads (1009) and vector loads with a second column strip (1040)"""
    contents = {"knife0": knife(0), "knife253": knife(253, 1), "all255": all255, "all0": all0, "stripes_cols": stripes_cols,
                "stripes_rows": stripes_rows, "checkerboard": checkerboard}
    return [Case("ring", R, 40, 1009, "RGB8", contents), Case("ring", R, 129, 1040, "RGB8", contents)]


# seeds: (radius, h, w) -> salt, chosen so that the reference alone finds at least 8 pixels at margin 0 and 8 at margin 1 on the knife
# frames of the large windows (tests/test_threshold_reference.py asserts it), where few distinct windows exist
SALTS = {(127, 129, 300): 1, (128, 129, 300): 1, (129, 140, 150): 5}


BIG_CONTENTS = {"noise": noise, "ramp": ramp, "all255": all255, "all0": all0, "knife0": knife(0), "knife253": knife(253, 1)}


def separable_cases(R):
    """radii 32..128.  40 x 1009 BGRA: W % 4 != 0, the byte loads of k_hsum_generic; 130 x 1028: two of its workgroups per row with
    the apron across column 1024, and two row strips of k_vsum_threshold_generic with H no multiple of 8; 257 x 260: row sums of exactly
    65535 on all255 at R = 128"""
    return [Case("separable", R, h, w, fmt, BIG_CONTENTS, SALTS.get((R, h, w), 0))
            for h, w, fmt in ((129, 300, "RGB8"), (40, 1009, "BGRA8"), (130, 1028, "L8"), (257, 260, "L8"), (1, 16, "RGB8"), (5, 3, "RGB8"))]


def brute_cases(R):
    """radii above 128: work per pixel grows with the clipped window's area, so small frames only"""
    return [Case("brute", R, h, w, "RGB8", BIG_CONTENTS, SALTS.get((R, h, w), 0)) for h, w in ((1, 16), (5, 3), (40, 30), (140, 150))]


def layout_cases(R):
    """radii 1..7 on 100 x 1008 (vector loads where the layout is aligned) and 100 x 1009, each run in every layout of LAYOUTS"""
    rows = k1_geometry(4, 1008, 100, R)[2]
    contents = {"noise": noise, "knife100": knife(100), "impulses": impulses(R, rows), "checkerboard": checkerboard}
    return [Case("layout", R, 100, w, "RGB8", contents) for w in (1008, 1009)]


# name -> (bytes of padding behind every row, bytes between frames, offset of the first pixel from a 16-byte aligned address)
LAYOUTS = {
    "packed": (0, 0, 0),          # vector loads where W % 16 == 0
    "rows+32": (32, 0, 0),        # padded, still aligned
    "rows+20,base+3": (20, 64, 3),   # nothing aligned: per-pixel loads
    "frames+8": (0, 8, 0),        # only the frame stride is no multiple of 16
}


def _flush_contents(n):
    return {f"{'knife100' if i & 1 else 'noise'}_{i}": (knife(100) if i & 1 else noise) for i in range(n)}


def flush_cases(R):
    """radii 1..7, the parked rows' flush: 2048 frames of 16 x 300 are one strip of 300 rows per wave (two bursts of 128 rows and a
    remainder), 1024 frames of 16 x 260 two strips of 130 rows (a burst and a remainder of 2; the second walks upwards) -- by
    k1_geometry, which tests/test_threshold_plan.py checks.  Noise in even frames, knife(100) in odd ones."""
    return [Case("flush", R, 300, 16, "L8", _flush_contents(2048)), Case("flush", R, 260, 16, "L8", _flush_contents(1024))]


RING_FLUSH_RADII = (8, 31)


def ring_flush_cases(R):
    """the ring kernel's parked rows with strips taller than a burst, contents as flush_cases.  R = 8 (2048 wave slots, bursts of 84
    rows): 2048 frames of 16 x 300 are one strip of 300 rows, 1024 of 16 x 260 two strips of 130, the second walking upwards.  R = 31
    (1024 wave slots, bursts of 60 rows): 1024 frames of 16 x 200 are one strip of 200 rows, 512 of 16 x 260 two strips of 130 -- by
    ring_geometry, which tests/test_threshold_plan.py checks."""
    shapes = {8: ((2048, 300), (1024, 260)), 31: ((1024, 200), (512, 260))}[R]
    return [Case("ringflush", R, h, 16, "L8", _flush_contents(n)) for n, h in shapes]


def cases_of(radius):
    """every batch the GPU module runs with this radius"""
    if radius in K1_RADII:
        return k1_cases(radius) + layout_cases(radius) + flush_cases(radius)
    if radius in RING_RADII:
        return ring_cases(radius) + (ring_flush_cases(radius) if radius in RING_FLUSH_RADII else [])
    return separable_cases(radius) if radius in SEPARABLE_RADII else brute_cases(radius)
