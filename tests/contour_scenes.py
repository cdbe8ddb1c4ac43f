"""Deterministic scenes for the contour stage (numpy only, no GPU).

Every generator takes (h, w, seed) and returns an L8 frame of h x w.  The structured scenes are painted in two grey levels,
LIGHT where the intended foreground lies and DARK elsewhere.  The window-7 adaptive threshold (foreground iff grey >= the
window's mean) turns them into exactly that foreground as long as every dark pixel lies within 7 pixels of a light one (a
uniform dark area is its own mean and thresholds to foreground).  The generators keep to that rule; `intended()` returns the
painted foreground, and tests/test_contour_scenes.py checks the threshold against it.

Tile geometry the scenes aim at (aruco3_amd/csrc/k_contours.hip): a dart tile of the contour graph covers 4 words x 64 rows,
i.e. 256 x 64 pixels, so borders that cross x = 256 k and y = 64 k change tiles there.
"""
import numpy as np

LIGHT, DARK = 210, 20
TILE_W, TILE_H = 256, 64


def paint(fg):
    return np.where(fg, LIGHT, DARK).astype(np.uint8)


def intended(frame):
    """the foreground a structured scene was painted with"""
    return frame == LIGHT


def min_edge_length(h, w, factor=0.2):
    """src/aruco.rs: (min(w, h) as f32 * min_side_length_factor) as u32"""
    return int(np.float32(min(h, w)) * np.float32(factor))


# ------------------------------------------------------------------------------------------------------------------
# long borders
# ------------------------------------------------------------------------------------------------------------------
def serpentine(h, w, seed, width=1, period=4):
    """one connected stroke `width` px thick: rows every `period` px, joined alternately at the left and right ends.  Its
    outer border visits every stroke pixel from both sides: about 2 h w / period points."""
    fg = np.zeros((h, w), bool)
    y0 = seed % max(1, min(period - width + 1, h))
    rows = list(range(y0, h - width + 1, period)) or [0]
    right = bool(seed & 4)
    for i, y in enumerate(rows):
        fg[y:y + width, :] = True
        if i + 1 < len(rows):
            x = slice(w - width, w) if right else slice(0, width)
            fg[y:rows[i + 1] + width, x] = True
            right = not right
    return paint(fg)


def serpentine2(h, w, seed):
    return serpentine(h, w, seed, width=2, period=5)


def spiral(h, w, seed, gap=3):
    """one connected 1-px square spiral, walls `gap` px apart, from the frame's edge inwards: its border runs through tiles in
    all four directions"""
    fg = np.zeros((h, w), bool)
    m = seed % 3
    top, left, bottom, right = m, m, h - 1 - m, w - 1 - m
    if bottom < top or right < left:
        fg[h // 2, w // 2] = True
        return paint(fg)
    step = gap + 1
    y, x = top, left
    fg[y, x] = True
    while True:
        if right < x: break
        fg[y, x:right + 1] = True; x = right                       # east
        top += step
        if bottom < y: break
        fg[y:bottom + 1, x] = True; y = bottom                      # south
        right -= step
        if x < left or right < left: break
        fg[y, left:x + 1] = True; x = left                          # west
        bottom -= step
        if y < top or bottom < top: break
        fg[top:y + 1, x] = True; y = top                            # north
        left += step
        if right < left: break
    return paint(fg)


# ------------------------------------------------------------------------------------------------------------------
# nesting, diagonal contacts, tile boundaries, frame edges
# ------------------------------------------------------------------------------------------------------------------
def nested_rings(h, w, seed):
    """concentric rectangular rings, light (2 px) and dark (2 or 3 px: a 1-px dark ring would let the light rings on either side
    touch diagonally at its corners) in turn: every ring is an outer border inside the hole of the ring around it, so the border
    tree is as deep as twice the number of rings.  (With 1-px light rings the reference's parents do not chain: the outer border
    of every ring names the first hole as its parent.)"""
    rng = np.random.default_rng(seed)
    fg = np.zeros((h, w), bool)
    o = 0
    while 2 * o < min(h, w):
        t = 2
        fg[o:h - o, o:w - o] = True
        o += t
        if 2 * o >= min(h, w):
            break
        d = 2 + int(rng.random() < 0.2)
        fg[o:h - o, o:w - o] = False
        o += d
    return paint(fg)


def checkerboard(h, w, seed, cell=1):
    """cells of `cell` px: light cells touch only at their corners (the 8-connectivity cases of the dart sweep)"""
    y, x = np.mgrid[0:h, 0:w]
    ph = seed % (2 * cell)
    return paint(((y + ph) // cell + (x + ph // 2) // cell) % 2 == 0)


def comb(h, w, seed):
    """two interleaved combs: teeth hang from a spine on row 0 and stand on a spine on row h-1, one tooth every 2 columns
    alternately from the top and the bottom.  The top teeth end at y = 64 j + r with r in -2..2, so their borders turn on
    either side of a tile row boundary; the teeth's phase (seed % 4) puts a tooth on x = 255, 256 or 257 mod 256 (phases 3, 0
    and 1), and both spines cross every tile column boundary."""
    rng = np.random.default_rng(seed)
    fg = np.zeros((h, w), bool)
    fg[0, :] = True
    if h < 8:
        return paint(fg)
    fg[h - 1, :] = True
    ph = seed % 4
    ends = {}
    for x in range(ph % 4, w, 4):                        # top teeth
        j = int(rng.integers(1, max(2, (h - 6) // TILE_H + 1)))
        e = min(TILE_H * j + int(rng.integers(-2, 3)), h - 8)
        e = max(e, 4)
        ends[x] = e
        fg[0:e + 1, x] = True
    for x in range((ph + 2) % 4, w, 4):                  # bottom teeth, reaching up to 3 px short of their neighbours' ends
        near = [ends[v] for v in (x - 2, x + 2) if v in ends] or [4]
        top = max(min(near) - 3, 2)
        fg[top:h, x] = True
    return paint(fg)


def edges(h, w, seed):
    """a light frame with thin dark bars and dark outlines touching column 0, column w-1, row 0 and row h-1, plus the column-0
    start anomaly of tests/test_gpu_shard_taps.py (dark pixels at (1, 3) and (0, 4))"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), LIGHT, np.uint8)
    for k in range(4 + int(rng.integers(0, 4))):
        t = int(rng.integers(1, 6))
        side = k if k < 4 else int(rng.integers(0, 4))
        if side < 2 and h > 2:       # a bar from the left (0) or right (1) edge
            y = int(rng.integers(0, h)); ln = int(rng.integers(1, max(2, w // 2)))
            xs = slice(0, ln) if side == 0 else slice(max(0, w - ln), w)
            img[y:y + t, xs] = DARK
        elif w > 2:                  # from the top (2) or bottom (3) edge
            x = int(rng.integers(0, w)); ln = int(rng.integers(1, max(2, h // 2)))
            ys = slice(0, ln) if side == 2 else slice(max(0, h - ln), h)
            img[ys, x:x + t] = DARK
    for _ in range(int(rng.integers(1, 4))):   # dark outlines (hole borders with an island inside) cut by the frame's edge
        y0, x0 = int(rng.integers(-4, max(1, h - 2))), int(rng.integers(-4, max(1, w - 2)))
        hh, ww = int(rng.integers(3, 24)), int(rng.integers(3, 24))
        y1, x1 = y0 + hh, x0 + ww
        for yy in (y0, y1):
            if 0 <= yy < h: img[yy, max(0, x0):max(0, min(w, x1 + 1))] = DARK
        for xx in (x0, x1):
            if 0 <= xx < w: img[max(0, y0):max(0, min(h, y1 + 1)), xx] = DARK
    if h > 5 and w > 2:
        img[3, 1] = DARK; img[4, 0] = DARK
    return img


def anomaly(h, w, seed):
    """the column-0 start anomaly (test_start_resolution_fast_and_full_paths): a light frame -- one component, first pixel
    (0, 0) -- whose outer border has events only where two dark pixels touch column 0 diagonally, so that its natural start
    does not fire; plus dark specks away from the frame's edge and one dark outline"""
    rng = np.random.default_rng(seed)
    img = np.full((h, w), LIGHT, np.uint8)
    if h > 12 and w > 12:
        sp = rng.random((h, w)) < 0.07
        sp[:10, :10] = False
        sp[:2, :] = False; sp[-2:, :] = False; sp[:, :2] = False; sp[:, -2:] = False
        img[sp] = DARK
    if h > 5 and w > 2:
        img[3, 1] = DARK; img[4, 0] = DARK
    return img


def specks(h, w, seed):
    """isolated light pixels and 2-pixel diagonal pairs on a lattice of pitch 3 (no two lattice sites are 8-neighbours), on
    dark; the corner sites are always lit so that no dark pixel lies further than 7 px from a light one"""
    rng = np.random.default_rng(seed)
    fg = np.zeros((h, w), bool)
    for y in range(0, h, 3):
        for x in range(0, w, 3):
            r = rng.random()
            corner = (y < 3 or y >= h - 3) and (x < 3 or x >= w - 3)
            if r < 0.4 or corner:
                fg[y, x] = True
            elif r < 0.7:
                fg[y, x] = True
                if y + 1 < h and x + 1 < w and y % 6 == 0:
                    fg[y + 1, x + 1] = True
                elif y + 1 < h and x >= 1:
                    fg[y + 1, x - 1] = True
    return paint(fg)


# ------------------------------------------------------------------------------------------------------------------
# the length bound of the product path's pruning (k_cycle_select, k_local_contract): kept iff n >= 5 and n^2 >= 8 mel
# ------------------------------------------------------------------------------------------------------------------
def _diamond(fg, cy, cx, r):
    h, w = fg.shape
    for dy in range(-r, r + 1):
        k = r - abs(dy)
        y = cy + dy
        if 0 <= y < h:
            fg[y, max(0, cx - k):max(0, min(w, cx + k + 1))] = True


def prune_bound(h, w, seed):
    """filled diamonds of radius r (a border of n = 4 r points along four straight diagonals, whose hull edges are 2 r^2 long
    squared: a candidate iff 2 r^2 >= mel, which is n^2 >= 8 mel -- the pruning bound itself) for r around the bound, axis-aligned
    squares and k x (k + 1) rectangles whose border lengths 4 k - 4 and 4 k - 2 lie around it, and polyominoes with borders of 4, 5 and 6 points.  One speck per
    cell corner keeps the dark area within reach of light."""
    rng = np.random.default_rng(seed)
    mel = min_edge_length(h, w)
    r0 = max(1, int(np.ceil(np.sqrt(mel / 2.0))))
    k0 = max(2, int(np.ceil(np.sqrt(8.0 * mel) / 4.0)) + 1)
    shapes = []
    for r in (r0 - 1, r0, r0 + 1, r0 + 2):
        if r >= 1:
            shapes.append(("d", r))
    for k in (k0 - 1, k0, k0 + 1):
        shapes += [("s", k), ("r", k)]
    polys = [("p", 4), ("p", 1), ("p", 0), ("p", 2), ("p", 3)]
    shapes = polys + shapes if mel < 8 else shapes + polys     # small frames hold few cells: the short borders first
    cell = 2 * (r0 + 2) + 4
    cell = max(cell, k0 + 5, 8)
    fg = np.zeros((h, w), bool)
    i = int(rng.integers(0, len(shapes))) if seed else 0
    for y0 in range(0, h - cell + 1, cell):
        for x0 in range(0, w - cell + 1, cell):
            kind, v = shapes[i % len(shapes)]
            i += 1
            c = cell // 2
            if kind == "d":
                _diamond(fg, y0 + c, x0 + c, v)
            elif kind == "s":
                fg[y0 + 2:y0 + 2 + v, x0 + 2:x0 + 2 + v] = True
            elif kind == "r":       # k x (k + 1): a border of 4 k - 2 points, between two squares'
                fg[y0 + 2:y0 + 2 + v, x0 + 2:x0 + 3 + v] = True
            else:   # 2x2 square (4 points), L-tromino, 2x3 block, a 3-pixel diagonal, a P-pentomino (5 points)
                yy, xx = y0 + 2, x0 + 2
                if v == 0: fg[yy:yy + 2, xx:xx + 2] = True
                elif v == 1: fg[yy, xx:xx + 2] = True; fg[yy + 1, xx] = True
                elif v == 2: fg[yy:yy + 2, xx:xx + 3] = True
                elif v == 3: fg[yy, xx] = fg[yy + 1, xx + 1] = fg[yy + 2, xx + 2] = True
                else: fg[yy, xx:xx + 3] = True; fg[yy + 1, xx + 1:xx + 3] = True
    # specks on a pitch-6 lattice where nothing else is within 2 px
    near = np.zeros((h + 4, w + 4), bool)
    for dy in range(5):
        for dx in range(5):
            near[dy:dy + h, dx:dx + w] |= fg
    near = near[2:h + 2, 2:w + 2]
    for y in range(0, h, 6):
        for x in range(0, w, 6):
            if not near[y, x]:
                fg[y, x] = True
    return paint(fg)


# ------------------------------------------------------------------------------------------------------------------
# fields
# ------------------------------------------------------------------------------------------------------------------
def _box(a, k):
    """mean over a (2k+1)^2 window, edges replicated"""
    if k <= 0:
        return a
    p = np.pad(a, k, mode="edge")
    c = np.cumsum(np.cumsum(p, 0), 1)
    c = np.pad(c, ((1, 0), (1, 0)))
    n = 2 * k + 1
    h, w = a.shape
    return (c[n:n + h, n:n + w] - c[0:h, n:n + w] - c[n:n + h, 0:w] + c[0:h, 0:w]) / (n * n)


def blobs(h, w, seed, density=0.5, smooth=1):
    """a smoothed random field thresholded at `density` and painted (as in tests/test_oracle_crosscheck.py)"""
    rng = np.random.default_rng(seed)
    return paint(_box(rng.random((h, w)), smooth) > density)


def blobs_sparse(h, w, seed):
    return blobs(h, w, seed, density=0.56, smooth=2)


def blobs_dense(h, w, seed):
    return blobs(h, w, seed, density=0.44, smooth=1)


def noise(h, w, seed):
    """uniform noise, the reference bench's recipe: thousands of tiny borders and one giant component"""
    return np.random.default_rng(seed).integers(0, 256, size=(h, w), dtype=np.uint8)


def blank(h, w, seed):
    return np.full((h, w), LIGHT, np.uint8)


STRUCTURED = {
    "serpentine": serpentine, "serpentine2": serpentine2, "spiral": spiral, "nested_rings": nested_rings,
    "checker1": lambda h, w, s: checkerboard(h, w, s, 1), "checker2": lambda h, w, s: checkerboard(h, w, s, 2),
    "checker3": lambda h, w, s: checkerboard(h, w, s, 3), "comb": comb, "specks": specks, "prune_bound": prune_bound,
}
SCENES = dict(STRUCTURED, edges=edges, anomaly=anomaly, blobs=blobs, blobs_sparse=blobs_sparse, blobs_dense=blobs_dense,
              noise=noise, blank=blank)
