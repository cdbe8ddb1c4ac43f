"""Damaged markers for the decode stage: an expectation in plain numpy, patterns that clean markers cannot deliver, and frames
that deliver those patterns bit for bit.  Shared by tests/test_decode_damage.py (oracle, CPU) and tests/test_gpu_decode_damage.py.

The expectation is written from the algorithm, not from k_decode and not from oracle/a3_oracle.c:
  * src/aruco.rs:287-292   any lit cell on the perimeter of the bit matrix -> no codes at all;
  * src/aruco.rs:296-310   four codes: the interior read row-major, first cell = most significant bit, `rotate_bit_matrix` between them;
  * src/aruco.rs:315-326   `rotate_bit_matrix` = 90 degrees counter-clockwise, i.e. np.rot90(m, 1) (test_bit_rotate's two matrices pin it);
  * src/dictionaries.rs:160-196  `find_nearest`: brute force, a strictly smaller distance replaces the best -> lowest index among equals;
  * src/aruco.rs:83-92     over the four rotations, the first with a strictly smaller distance;
  * src/aruco.rs:96-103    accepted iff the filter is off or distance < tau; corners.rotate_left(rotation).

Drawing.  A pattern is an n x n cell matrix (n = sqrt(num_bits) + 2, perimeter included) painted axis-aligned with cells of a whole
number of pixels, a white quiet zone and a flat background.  The quad handed to the decode stage is the marker's own square
(x0, y0) .. (x0 + n * cell, y0 + n * cell); starting the quad at corner j shows the decoder np.rot90(pattern, j).
Where the contour stage has to find the quads itself (family b) its corners lie up to a pixel off that square, so those frames are
drawn larger, with the cell grid a pixel up and left of the square and a black rim under a lit border cell (see CELL and draw_frame).
The warp samples the square homography_sample_size times a side; `sample_size` says why 36- and 64-bit tables run at 48 and 50.
An interior without a single white cell would make the warped patch flat, and Otsu's level of a flat patch is 0: everything reads
white and the border test fails (that is the reference's behaviour, not a bit pattern anybody drew).  Such a pattern carries a white
speck, a ninth of one cell, in the middle of an interior cell: the patch then has two levels and every CELL still reads black.
"""
import functools
from dataclasses import dataclass, field

import numpy as np

NAMED = ("APRILTAG_16H5", "ARUCO_MIP_16H3", "ARUCO", "ARUCO_MIP_36H12", "APRILTAG_36H10", "APRILTAG_36H9", "CHILITAGS", "ARTAG")
HAND_LENGTHS = (1, 63, 64, 65, 511, 512, 513, 2047, 2048, 2049)
HAND = tuple(f"HAND_LEN_{n}" for n in HAND_LENGTHS) + ("HAND_DUPLICATES", "HAND_SELF_ROTATION", "HAND_TAU_12")
ALL = NAMED + HAND
# the scan of k_decode: 64 or 256 threads, 8 codes per thread and trip -> a wave is 64 consecutive indices, a lane-set 64 / 256,
# a trip 512 / 2048
BOUNDARIES = (64, 256, 512, 2048)
# the same code at two indices: either side of a lane-set, a wave and a trip boundary of both scans, and far apart
DUPLICATES = ((63, 64), (255, 256), (511, 512), (2047, 2048), (3, 2051), (70, 700))
SELF_ROTATION = (5, 40)          # HAND_SELF_ROTATION: a code and its own 90-degree rotation

W, H = 640, 480
BLACK, WHITE, BACKGROUND = 25, 235, 150
QUIET = 8


# ------------------------------------------------------------------------------------------------------------------
# the expectation
# ------------------------------------------------------------------------------------------------------------------
_POP8 = np.array([bin(i).count("1") for i in range(256)], dtype=np.uint8)


def popcount(a):
    """bits set in every element of a uint64 array"""
    a = np.ascontiguousarray(a, dtype=np.uint64)
    if hasattr(np, "bitwise_count"):
        return np.bitwise_count(a).astype(np.int64)
    return _POP8[a.view(np.uint8).reshape(a.shape + (8,))].sum(axis=-1, dtype=np.int64)


def side_cells(num_bits):
    k = int(round(num_bits ** 0.5))
    assert k * k == num_bits
    return k


def code_of(m):
    """a k x k bit matrix read row-major, first cell = most significant bit (src/aruco.rs:296-308)"""
    v = 0
    for b in np.asarray(m).reshape(-1).tolist():
        v = (v << 1) | int(b)
    return v


def matrix_of(code, num_bits):
    k = side_cells(num_bits)
    return np.array([(int(code) >> (num_bits - 1 - i)) & 1 for i in range(num_bits)], dtype=np.uint8).reshape(k, k)


def rotated_codes(interior):
    """the four codes of homography_to_code_permutations: rotate_bit_matrix applied 0..3 times"""
    return [code_of(np.rot90(interior, r)) for r in range(4)]


def find_nearest(codes, c):
    """-> (index, distance, how many codes are at that distance)"""
    d = popcount(np.asarray(codes, dtype=np.uint64) ^ np.uint64(c))
    i = int(np.argmin(d))                       # lowest index among equals
    return i, int(d[i]), int((d == d[i]).sum())


def numpy_tau(codes):
    """ARDictionary::new with tau 0 (src/dictionaries.rs:116-138): the minimum pairwise distance"""
    codes = np.asarray(codes, dtype=np.uint64)
    best = 255
    for i in range(len(codes) - 1):
        best = min(best, int(popcount(codes[i + 1:] ^ codes[i]).min()))
    return best


@dataclass
class Expect:
    decode_ok: int
    codes: list                       # the four codes (zeros when the border test fails)
    per_rotation: list = None         # (index, distance, ties) per rotation
    rotation: int = 0
    id: int = 0
    distance: int = 0
    code: int = 0
    code_tie: bool = False            # more than one code at the minimum, at the winning rotation
    tied: tuple = ()                  # the indices tied there
    rotation_tie: bool = False        # the minimum is reached under more than one rotation

    def accepted(self, tau, filt):
        return bool(self.decode_ok and (not filt or self.distance < tau))


def expect_codes(cs, codes):
    """the lookup of the four rotated codes `cs`: nearest code per rotation, then the first rotation with a strictly smaller distance"""
    cs = [int(c) for c in cs]
    per = [find_nearest(codes, c) for c in cs]
    best = None
    for r, (i, d, _) in enumerate(per):
        if best is None or d < best[1]:         # the first strictly smaller distance
            best = (i, d, r)
    i, d, r = best
    dist = popcount(np.asarray(codes, dtype=np.uint64) ^ np.uint64(cs[r]))
    tied = tuple(np.flatnonzero(dist == d).tolist())
    return Expect(1, cs, per, r, i, d, cs[r], len(tied) > 1, tied, sum(1 for p in per if p[1] == d) > 1)


def expect_view(view, codes):
    """what the decode stage must make of the n x n cell matrix `view` (perimeter included)"""
    view = np.asarray(view)
    if view[0].any() or view[-1].any() or view[:, 0].any() or view[:, -1].any():
        return Expect(0, [0, 0, 0, 0])
    return expect_codes(rotated_codes(view[1:-1, 1:-1]), codes)


def rotate_left(quad, r):
    q = [tuple(int(v) for v in p) for p in np.asarray(quad).reshape(4, 2).tolist()]
    return tuple(q[r:] + q[:r])


def expected_marker(e, quad, tau, filt):
    """(id, code, corners, hamming_distance, rotation) as tests.util.markers_of_* give them, or None"""
    if not e.accepted(tau, filt):
        return None
    return (e.id, e.code, rotate_left(quad, e.rotation), e.distance, e.rotation)


def expected_of_candidates(res, codes, tau, filt):
    """numpy applied to the four codes each candidate reports (`res`: "codes", "decode_ok", "candidates" of one frame, from the
    oracle or from the device's taps) -> (marker tuples, their candidate indices, the expectation per candidate)"""
    out, idx, exps = [], [], []
    for k, (row, ok, q) in enumerate(zip(res["codes"], res["decode_ok"], res["candidates"])):
        e = expect_codes(row, codes) if ok else Expect(0, [0, 0, 0, 0])
        exps.append(e)
        m = expected_marker(e, q, tau, filt)
        if m is not None:
            out.append(m)
            idx.append(k)
    return out, idx, exps


# ------------------------------------------------------------------------------------------------------------------
# dictionaries
# ------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def table(name):
    """-> (num_bits, tau as the table declares it (0: computed), codes).  Hand-made tables: 25-bit codes, tau 3, but for HAND_TAU_12."""
    from aruco3_amd.dictionaries import ARDictionary

    if name in NAMED:
        d = ARDictionary.new_from_named_dict(name)
        return d.num_bits, d._tau, d.code_list.copy()
    rng = np.random.default_rng(abs(hash_name(name)))
    if name.startswith("HAND_LEN_"):
        n = int(name.rsplit("_", 1)[1])
        return 25, 3, _distinct(rng, n, 25)
    if name == "HAND_DUPLICATES":
        codes = _distinct(rng, 2100, 25)
        for lo, hi in DUPLICATES:
            codes[hi] = codes[lo]
        return 25, 3, codes
    if name == "HAND_SELF_ROTATION":
        codes = _distinct(rng, 100, 25)
        a, b = SELF_ROTATION
        while True:
            m = matrix_of(int(codes[a]), 25)
            r = code_of(np.rot90(m, 1))
            if r != int(codes[a]) and r not in codes.tolist():
                break
            codes[a] += np.uint64(1)
        codes[b] = np.uint64(r)
        return 25, 3, codes
    if name == "HAND_TAU_12":
        # ARUCO_MIP_36H12 is dense: no pattern 12 cells from all of its codes under every rotation was found (300 walks of 3000
        # single-cell flips that never let the distance fall all end at 11; a search, not a proof), so its own `< tau` is only met
        # from below here; every other code of it, with the same tau, leaves room for patterns at exactly 12
        return 36, 12, ARDictionary.new_from_named_dict("ARUCO_MIP_36H12").code_list[::2].copy()
    raise KeyError(name)


def hash_name(name):
    return sum((i + 1) * ord(c) for i, c in enumerate(name)) * 7919 + 17


def _distinct(rng, n, num_bits):
    seen, out = set(), []
    while len(out) < n:
        c = int(rng.integers(1, 1 << num_bits))
        if c not in seen:
            seen.add(c)
            out.append(c)
    return np.array(out, dtype=np.uint64)


@functools.lru_cache(maxsize=None)
def tau_of(name):
    """the tau the detector works with: the table's, or numpy's minimum pairwise distance where the table says 0"""
    _, tau, codes = table(name)
    return tau if tau else numpy_tau(codes)


def dictionary(name):
    """the ARDictionary the detector and the oracle are given (tau as the table declares it: 0 = computed on the device)"""
    from aruco3_amd.dictionaries import ARDictionary

    nb, tau, codes = table(name)
    return ARDictionary(nb, tau, codes.copy(), name)


def boundary_indices(n_codes):
    """first, last, and either side of the first and the last multiple of 64, 256, 512 and 2048 the table reaches -> {index: tags}"""
    out = {0: {"index_first"}}
    out.setdefault(n_codes - 1, set()).add("index_last")
    for m in BOUNDARIES:
        if n_codes > m:
            for mult in sorted({m, (n_codes - 1) // m * m}):
                out.setdefault(mult - 1, set()).add(f"index_below_{m}")
                out.setdefault(mult, set()).add(f"index_at_{m}")
    return out


def admitted_classes(name):
    """every class of pattern the dictionary `name` admits (a 30-code table has no index 2048, a one-code table no code tie)"""
    nb, _, codes = table(name)
    n, tau = len(codes), tau_of(name)
    out = {f"flip_{d}" for d in range(tau + 2)} | {f"orient_{o}" for o in range(4)} | set().union(*boundary_indices(n).values())
    if name != "ARUCO_MIP_36H12":          # (see HAND_TAU_12 in table())
        out.add("boundary_reject")
    out |= {"rotation_tie", "rotation_1", "rotation_2", "rotation_3", "border_left", "border_right", "border_top",
            "border_bottom", "all_black", "all_white"}
    if tau >= 1:
        out.add("boundary_accept")
    if n >= 2:
        out.add("code_tie")
    if n > 64:
        out.add("code_tie_waves")
    if n > 2048:
        out.add("code_tie_trips")
    if name == "HAND_DUPLICATES":
        out |= {f"duplicate_{lo}_{hi}" for lo, hi in DUPLICATES}
    if name == "HAND_SELF_ROTATION":
        out.add("self_rotation")
    return out


# ------------------------------------------------------------------------------------------------------------------
# patterns
# ------------------------------------------------------------------------------------------------------------------
@dataclass
class Pattern:
    cells: np.ndarray                 # n x n, perimeter included, as drawn
    tags: set = field(default_factory=set)
    expect: Expect = None             # of the pattern as drawn (quad started at its top-left corner)


def _framed(interior):
    k = interior.shape[0]
    m = np.zeros((k + 2, k + 2), dtype=np.uint8)
    m[1:-1, 1:-1] = interior
    return m


def _flip(rng, interior, d):
    m = interior.copy().reshape(-1)
    for i in rng.choice(m.size, size=d, replace=False).tolist():
        m[i] ^= 1
    return m.reshape(interior.shape)


def _midpoint(rng, a, b):
    """a with half of the cells flipped in which it differs from b (None when they differ in an odd number of cells, or in none)"""
    diff = np.flatnonzero(a.reshape(-1) != b.reshape(-1))
    if diff.size == 0 or diff.size % 2:
        return None
    m = a.copy().reshape(-1)
    for i in rng.choice(diff, size=diff.size // 2, replace=False).tolist():
        m[i] ^= 1
    return m.reshape(a.shape)


def tags_of(e, tau):
    """the classes that follow from an expectation alone, not from how a pattern was made"""
    t = set()
    if not e.decode_ok:
        return t
    if e.distance >= 1:
        t.add(f"rotation_{e.rotation}")               # a best rotation at a non-zero distance
    if e.distance == tau:
        t.add("boundary_reject")
    if tau >= 1 and e.distance == tau - 1:
        t.add("boundary_accept")
    if e.code_tie:
        t.add("code_tie")
        if len({(i % 256) // 64 for i in e.tied}) > 1:
            t.add("code_tie_waves")
        if len({i // 2048 for i in e.tied}) > 1:
            t.add("code_tie_trips")
    if e.rotation_tie:
        t.add("rotation_tie")
    return t


def _classify(p, codes, tau):
    p.expect = expect_view(p.cells, codes)
    p.tags |= tags_of(p.expect, tau)
    return p


@functools.lru_cache(maxsize=None)
def patterns(name):
    """the seeded search of one dictionary -> [Pattern]"""
    nb, _, codes = table(name)
    tau, n, k = tau_of(name), len(codes), side_cells(nb)
    rng = np.random.default_rng(hash_name(name) + 1)
    mats = [None] * n

    def mat(i):
        if mats[i] is None:
            mats[i] = matrix_of(int(codes[i]), nb)
        return mats[i]

    out = []

    def add(interior, orient, *tags, cells=None):
        # drawn turned back by `orient` quarter turns: rotation `orient` of what the decoder reads is `interior` again
        c = _framed(np.rot90(interior, -orient)) if cells is None else cells
        p = _classify(Pattern(c, set(tags) | ({f"orient_{orient}"} if cells is None else set())), codes, tau)
        out.append(p)
        return p

    # d cells flipped from a code, d = 0 .. tau + 1, four orientations, at the indices where the scan changes lane-set, wave or trip
    idx = boundary_indices(n)
    if name == "HAND_DUPLICATES":
        for lo, hi in DUPLICATES:
            idx.setdefault(hi, set()).add(f"duplicate_{lo}_{hi}")   # damaged from the HIGHER index: the lower one must be reported
    if name == "HAND_SELF_ROTATION":
        for i in SELF_ROTATION:
            idx.setdefault(i, set()).add("self_rotation")
    for i, tags in sorted(idx.items()):
        for d in range(tau + 2):
            for o in range(4):
                add(_flip(rng, mat(i), d), o, f"flip_{d}", *tags)

    # the exact boundary, measured to the NEAREST code under any rotation: tau - 1 (accepted) and tau (rejected with the filter on).
    # Random damage rarely ends that far from every code of a dense table: a walk that never lets the distance fall gets there.
    shifts = np.arange(nb - 1, -1, -1, dtype=np.uint64)
    bits = ((codes[:, None] >> shifts[None, :]) & np.uint64(1)).reshape(n, k, k)
    rot = {r: (np.rot90(bits, r, axes=(1, 2)).reshape(n, nb) << shifts[None, :]).sum(axis=1, dtype=np.uint64) for r in (1, 2, 3)}
    every = np.concatenate([codes, rot[1], rot[2], rot[3]])     # pattern turned by r against a code = pattern against the code turned back

    def nearest_any(m):
        return int(popcount(every ^ np.uint64(code_of(m))).min())

    for want, tag in ((tau - 1, "boundary_accept"), (tau, "boundary_reject")):
        if want < 0:
            continue
        for got in range(8):
            m = _flip(rng, mat(int(rng.integers(0, n))), min(want, nb))
            d = nearest_any(m)
            for _ in range(4000):
                if d >= want:
                    break
                y, x = int(rng.integers(0, k)), int(rng.integers(0, k))
                m[y, x] ^= 1
                d2 = nearest_any(m)
                if d2 >= d:
                    d = d2
                else:
                    m[y, x] ^= 1
            if d == want:
                assert expect_view(_framed(m), codes).distance == want
                add(m, got % 4, f"searched_{tag}")

    # code ties: half of the cells flipped in which a code differs from a close one -- the closest at all, the closest in another
    # wave, the closest in another trip of the 256-thread scan
    if n >= 2:
        index = np.arange(n)
        for which, other in (("any", lambda i: index != i), ("wave", lambda i: (index % 256) // 64 != (i % 256) // 64),
                             ("trip", lambda i: index // 2048 != i // 2048)):
            got = 0
            for _ in range(300):
                i = int(rng.integers(0, n))
                d = popcount(codes ^ codes[i])
                ok = other(i) & (d % 2 == 0) & (d > 0)
                if not ok.any():
                    continue
                j = int(np.flatnonzero(ok)[np.argmin(d[ok])])
                m = _midpoint(rng, mat(i), mat(j))
                e = expect_view(_framed(m), codes)
                need = {"any": True, "wave": len({(t % 256) // 64 for t in e.tied}) > 1, "trip": len({t // 2048 for t in e.tied}) > 1}[which]
                if e.code_tie and need:
                    add(m, got % 4, f"searched_code_tie_{which}")
                    got += 1
                    if got == 8:
                        break

    # rotation ties: half-way between a code and another code turned by one, two or three quarter turns
    got = 0
    for _ in range(300):
        i, r = int(rng.integers(0, n)), int(rng.integers(1, 4))
        d = popcount(rot[r] ^ codes[i])
        ok = (d % 2 == 0) & (d > 0)
        if not ok.any():
            continue
        j = int(np.flatnonzero(ok)[np.argmin(d[ok])])
        m = _midpoint(rng, mat(i), np.rot90(mat(j), r))
        if expect_view(_framed(m), codes).rotation_tie:
            add(m, got % 4, "searched_rotation_tie")
            got += 1
            if got == 8:
                break

    # one lit border cell on each side (rejected before any lookup), all-black and all-white interiors
    base = _framed(mat(int(rng.integers(0, n))))
    last = k + 1
    for tag, (y, x) in (("border_left", (int(rng.integers(1, last)), 0)), ("border_right", (int(rng.integers(1, last)), last)),
                        ("border_top", (0, int(rng.integers(1, last)))), ("border_bottom", (last, int(rng.integers(1, last)))),
                        ("border_top", (0, 0)), ("border_bottom", (last, last))):
        c = base.copy()
        c[y, x] = 1
        add(None, 0, tag, cells=c)
    add(np.zeros((k, k), np.uint8), 0, "all_black")
    add(np.ones((k, k), np.uint8), 0, "all_white")
    return out


def summary(name):
    """counts for the report: patterns per class, the share at distance >= 1, tied minima"""
    ps = patterns(name)
    per = {}
    for p in ps:
        for t in p.tags:
            per[t] = per.get(t, 0) + 1
    dec = [p for p in ps if p.expect.decode_ok]
    return {"patterns": len(ps), "classes": per, "damaged": sum(1 for p in dec if p.expect.distance >= 1),
            "code_ties": sum(1 for p in dec if p.expect.code_tie), "rotation_ties": sum(1 for p in dec if p.expect.rotation_tie),
            "max_distance": max(p.expect.distance for p in dec)}


# ------------------------------------------------------------------------------------------------------------------
# frames
# ------------------------------------------------------------------------------------------------------------------
def sample_size(num_bits):
    """homography_sample_size of families a and b: the multiple of the cell count nearest the default 49.  With 49 samples across 8
    or 10 cells a cell is 6 or 7 (4 or 5) samples wide depending on where it lies, and the reference's own triangle resize then reads
    some white cells with black neighbours at 127 of 255 or less, under its `> 127`, whatever the size of a cell in pixels: not every bit
    pattern can be delivered (test_decode_damage.py::test_default_sample_size_cannot_deliver_every_pattern measures it: 1 % of the
    quads of ARUCO_MIP_36H12, every misread cell at 126; 4 in 10 of CHILITAGS').  Family c runs at the default."""
    n = side_cells(num_bits) + 2
    return {6: 48, 7: 49, 8: 48, 10: 50}[n]


# family a (quads handed in: exact) packs small markers; family b (quads found by the contour stage, whose corners lie up to a
# pixel off the square's) draws them large, one sample of the warp at least three pixels wide, with the cell grid moved one pixel
# up and left inside the black square: a sample then stays a pixel or more clear of every cell boundary wherever in [-1, 1] the
# found corner lies, and the found quads read the drawn bits as well
CELL = {"a": {6: 14, 7: 12, 8: 12, 10: 12}, "b": {6: 25, 7: 21, 8: 18, 10: 16}}
GRID_SHIFT = {"a": 0, "b": 1}


def geometry(num_bits, family="a"):
    """-> (cell size in pixels, columns, rows) of the regular grid a 640 x 480 frame holds"""
    n = side_cells(num_bits) + 2
    cell = CELL[family][n]
    pitch = n * cell + 2 * QUIET + 6
    return cell, W // pitch, H // pitch


def per_frame(num_bits, family="a"):
    _, cols, rows = geometry(num_bits, family)
    return cols * rows


def draw_frame(ps, num_bits, family="a"):
    """-> (L8 frame, [quad 4 x 2 (x, y) from the top-left corner clockwise] per pattern)"""
    cell, cols, rows = geometry(num_bits, family)
    n = side_cells(num_bits) + 2
    side = n * cell
    assert len(ps) <= cols * rows
    img = np.full((H, W), BACKGROUND, dtype=np.uint8)
    quads = []
    at = np.clip((np.arange(side) + GRID_SHIFT[family]) // cell, 0, n - 1)      # the cell a pixel of the square lies in
    for s, p in enumerate(ps):
        cx, cy = (s % cols * 2 + 1) * W // (2 * cols), (s // cols * 2 + 1) * H // (2 * rows)
        x0, y0 = cx - side // 2, cy - side // 2
        assert x0 - QUIET >= 0 and y0 - QUIET >= 0 and x0 + side + QUIET <= W and y0 + side + QUIET <= H
        img[y0 - QUIET: y0 + side + QUIET, x0 - QUIET: x0 + side + QUIET] = WHITE
        img[y0: y0 + side, x0: x0 + side] = np.where(p.cells[np.ix_(at, at)] != 0, WHITE, BLACK)
        if family == "b":
            # a lit cell on the perimeter keeps a two-pixel black rim along the square's outline: the contour stage still finds the
            # square (an open notch, or a lit corner, joins the quiet zone and leaves no quad), the cell still reads white
            for rim in (img[y0: y0 + 2, x0: x0 + side], img[y0 + side - 2: y0 + side, x0: x0 + side],
                        img[y0: y0 + side, x0: x0 + 2], img[y0: y0 + side, x0 + side - 2: x0 + side]):
                rim[...] = BLACK
        if not p.cells.any():                 # a flat patch has no Otsu level: see the module docstring
            a, b = y0 + cell + cell // 3, x0 + cell + cell // 3
            img[a: a + cell // 3, b: b + cell // 3] = WHITE
        quads.append(np.array([[x0, y0], [x0 + side, y0], [x0 + side, y0 + side], [x0, y0 + side]], dtype=np.uint32))
    return img, quads


def as_rgb(grey):
    """the same frame as RGB8, tinted so that the luma weights matter"""
    g = grey.astype(np.float32)
    return np.rint(np.stack([g, g * 0.98, g * 0.94], axis=-1)).astype(np.uint8)


@functools.lru_cache(maxsize=None)
def injected_frames(name):
    """family a -> [(L8 frame, quads [m, 4, 2], views: the cell matrix each quad shows, pattern index of each quad)]: every pattern's
    quad started at each of its four corners"""
    nb = table(name)[0]
    ps, g = patterns(name), per_frame(nb)
    out = []
    for f0 in range(0, len(ps), g):
        chunk = ps[f0: f0 + g]
        img, quads = draw_frame(chunk, nb)
        qs, views, which = [], [], []
        for s, (p, q) in enumerate(zip(chunk, quads)):
            for j in range(4):
                qs.append(np.roll(q, -j, axis=0))
                views.append(np.rot90(p.cells, j))
                which.append(f0 + s)
        out.append((img, np.stack(qs), views, which))
    return out


FOUND_FRAMES = 66


def found_frames(name):
    """family b -> (L8 frames [FOUND_FRAMES or more, H, W], [pattern indices per frame]): the same drawings, nothing injected; every
    pattern is drawn at least once, every frame holds a different window of a seeded shuffle"""
    nb = table(name)[0]
    ps, g = patterns(name), per_frame(nb, "b")
    rng = np.random.default_rng(hash_name(name) + 2)
    order = rng.permutation(len(ps))
    first = -(-len(ps) // g)                     # frames that hold the shuffle once; the rest are fresh draws from it
    frames, which = [], []
    for f in range(max(FOUND_FRAMES, first)):
        ids = order[f * g: (f + 1) * g].tolist() if f < first else rng.choice(len(ps), size=min(g, len(ps)), replace=False).tolist()
        frames.append(draw_frame([ps[i] for i in ids], nb, "b")[0])
        which.append(ids)
    return np.stack(frames), which


def oracle_config(oracle, filt, num_bits):
    cfg = oracle.Config.default()
    cfg.homography_sample_size = sample_size(num_bits)
    cfg.min_corner_separation_factor = 0.01      # packed quads, the same square from four corners: discard_too_near keeps them all
    cfg.filter_high_bit_errors = int(filt)
    return cfg


def detector_config(filt, num_bits):
    from aruco3_amd.aruco import DetectorConfig

    return DetectorConfig(min_corner_separation_factor=0.01, homography_sample_size=sample_size(num_bits), filter_high_bit_errors=bool(filt))


# ------------------------------------------------------------------------------------------------------------------
# family c: damaged tables through the renderer, nothing injected, nothing axis-aligned
# ------------------------------------------------------------------------------------------------------------------
# (not CHILITAGS: 49 samples across its 10 cells read a lone flipped cell back as its neighbours about every other time, in the
# reference as in the oracle, so `hamming_distance == d` is not what the reference itself delivers there)
FAMILY_C = ("APRILTAG_16H5", "ARUCO", "ARUCO_MIP_36H12", "APRILTAG_36H10")
C_W, C_H = 800, 600
C_FRAMES = {0: 30, 6: 10}      # frames per (sigma, paper): the 90 % bar is taken over the sigma-0 ones


@functools.lru_cache(maxsize=None)
def damaged_table(name):
    """-> (the dictionary's codes with d cells flipped per entry, d per entry): d spread over 0 .. tau + 1"""
    nb, _, codes = table(name)
    tau = tau_of(name)
    rng = np.random.default_rng(hash_name(name) + 3)
    d = rng.permutation(len(codes)) % (tau + 2)
    out = codes.copy()
    for i in range(len(codes)):
        for b in rng.choice(nb, size=int(d[i]), replace=False).tolist():
            out[i] ^= np.uint64(1 << b)
    return out, d


def family_c_frames(name, sigma, paper):
    """-> [(RGB8 frame, [TruthMarker])]: the renderer picks the cells from the DAMAGED table, the ids it reports stay the true ones"""
    from aruco3_amd import synth

    nb = table(name)[0]
    spec = synth.SynthSpec(C_W, C_H, n_markers=(1, 2), side=(260.0, 340.0), min_center_sep=400.0, perspective=0.2, noise_sigma=float(sigma),
                           background="gradient" if paper else "flat", paper=bool(paper), supersample=2)
    seed0 = hash_name(name) * 10 + int(sigma) * 2 + int(paper)
    return [synth.render_frame(spec, damaged_table(name)[0], nb, seed0 * 100 + i) for i in range(C_FRAMES[int(sigma)])]


C_SEPARATION = 0.02   # min_corner_separation_factor of family c: with paper off the white quiet zone is a quad of its own, a cell's
#                       width outside the marker's, and at the default 0.1 discard_too_near keeps that one (the longer perimeter) alone


def recovered(markers, truth, damage, tau):
    """of the drawn markers damaged by d < tau / 2 cells: (how many, which of them (frame-local index) the marker tuples `markers`
    report with the id that was drawn and hamming_distance == d).  A marker belongs to the drawn quad its centre lies nearest."""
    want, got = 0, []
    for k, t in enumerate(truth):
        d = int(damage[t.id])
        if not 2 * d < tau:
            continue
        want += 1
        c = np.asarray(t.corners, dtype=np.float64).mean(axis=0)
        for m in markers:
            mc = np.asarray(m[2], dtype=np.float64).mean(axis=0)
            if np.hypot(*(mc - c)) < 12.0 and m[0] == t.id and m[3] == d:
                got.append(k)
                break
    return want, got
