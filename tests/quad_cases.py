"""Hand-made borders for k_contour_quads (aruco3_amd/csrc/k_contours.hip), what the oracle makes of them, and an exact model of the
kernel's Douglas-Peucker that counts what they make the kernel execute.  numpy, fractions and the C oracle; no GPU.

Three pieces, used by tests/test_quad_cases.py (CPU) and tests/test_gpu_contour_quads.py (GPU):

  expected_quad()  the specification: the oracle's own approximate_polygon_dp, convex_hull, the squared-edge filter in the reference's
                   form and enforce_clockwise_corners, composed per border as contours_to_candidates (src/aruco.rs:124-166) composes them.
  model()          Douglas-Peucker as the kernel walks it -- the same work list, the arg-max by (|num|, smallest index), the test of
                   num / sqrt(den) > eps -- in Python integers and Fractions: eps is the exact value of the double n * eps_factor, so
                   num^2 against eps^2 den is decided exactly.  Where the two sides agree to nine digits (the kernel's third branch) it
                   evaluates the reference's expression in doubles, as the kernel does; everywhere else the exact comparison and that
                   expression must agree, which model() asserts.  It is the second opinion on the kept indices, the bookkeeper of the
                   coverage table (census keys below, per group width), and it takes a switch per plausible fault (MUTANTS) so that the
                   CPU test can show each fault changes the expected output of some case without running a wrong kernel.
  launches()       the tables the GPU test hands a3_debug_contour_quads, one Launch per call.

Borders are closed 8-connected walks: small ones traced by oracle.find_contours on painted shapes (as traced, and translated: a
translated border is a border), large ones walked analytically round convex polygons."""
import math
from fractions import Fraction
from functools import lru_cache

import numpy as np

CONTOUR_DTYPE = np.dtype([("frame", "<u4"), ("start_key", "<u4"), ("point_base", "<u4"), ("n", "<u4")])   # a3_debug_contour
CAND_DTYPE = np.dtype([("start_key", "<u4"), ("xy", "<u2", (8,))])                                        # a3_debug_cand
K_SMALL = 64                       # kSmallBorder: borders of at most 64 points go to 16-lane groups, longer ones to whole waves
ERR_POINT_POOL, ERR_CONTOUR_TABLE, ERR_CAND_TABLE = 2, 4, 8
MIN_GRID = (160, 1024)             # launch_contour_quads' smallest grid: wave groups, 16-lane groups
BAND = Fraction(1, 10 ** 9)

MUTANTS = ("tie_largest_index", "ge_for_gt", "band_squared_only", "no_fourth_split_reject", "edge_unsquared", "no_hull", "no_winding_fix")
CENSUS_KEYS = ("borders", "chords", "chords_zero", "chords_pa_eq_pb", "band_ratio_one", "band_ratio_not_one", "tie_chords",
               "win_u0", "win_u1", "win_u2", "win_u3", "win_last_partial_trip", "win_full_trip", "fourth_split_with_work_left",
               "reject_point_count", "reject_convexity", "reject_edge_length", "accepted", "winding_flipped")


def width_of(n):
    return 16 if n <= K_SMALL else 64


# ------------------------------------------------------------------------------------------------------------------------------------
# the specification: the oracle's functions, composed
# ------------------------------------------------------------------------------------------------------------------------------------
def expected_quad(oracle, pts, eps_factor, mel):
    """-> ("accepted", quad 4 x 2) or (reject class, None), as contours_to_candidates + enforce_clockwise_corners decide it"""
    pts = np.ascontiguousarray(pts, dtype=np.uint32).reshape(-1, 2)
    n = len(pts)
    poly = oracle.approximate_polygon_dp(pts, n * eps_factor, True)
    if len(poly) != 4:
        return "reject_point_count", None
    hull = oracle.convex_hull(poly)
    if len(hull) != 4:
        return "reject_convexity", None
    cmin = mel + 1
    h = hull.astype(np.int64)
    for i in range(4):
        dx, dy = h[i] - h[(i + 1) % 4]
        assert abs(dx) < 1 << 15 and abs(dy) < 1 << 15, "the reference's 32-bit dx*dx + dy*dy is not defined here"
        cmin = min(cmin, int(dx * dx + dy * dy))
    if cmin < mel:
        return "reject_edge_length", None
    return "accepted", oracle.enforce_clockwise_corners(hull)[0].astype(np.int64)


def oracle_kept(oracle, pts, eps_factor):
    """the indices approximate_polygon_dp keeps (closed: without the last point), found from its vertices in walk order"""
    pts = np.ascontiguousarray(pts, dtype=np.uint32).reshape(-1, 2)
    poly = oracle.approximate_polygon_dp(pts, len(pts) * eps_factor, True)
    out, i = [], 0
    for v in poly:            # kept vertices come in increasing index order; match each to its first occurrence from i on
        while not (pts[i] == v).all():
            i += 1
        out.append(i)
        i += 1
    return out


# ------------------------------------------------------------------------------------------------------------------------------------
# the model
# ------------------------------------------------------------------------------------------------------------------------------------
def new_census():
    return dict.fromkeys(CENSUS_KEYS, 0)


def _far(num, den, eps, e2, mutant, census, band_log=None):
    """the kernel's distance test for the farthest point of a chord: num / sqrt(den) > eps"""
    exact = Fraction(num * num) - e2 * den          # sign of num^2 - eps^2 den
    ratio_off = abs(Fraction(num * num) / (e2 * den) - 1) if e2 else None
    reference = num / math.sqrt(den) > eps          # f64, correctly rounded division and square root: the reference's expression
    if ratio_off is not None and ratio_off < BAND:
        if census is not None:
            census["band_ratio_one" if exact == 0 else "band_ratio_not_one"] += 1
        if band_log is not None:
            band_log.append((num, den, Fraction(num * num) / (e2 * den)))
        if mutant == "band_squared_only":
            dn, dd = float(num), float(den)
            return dn * dn > eps * eps * dd, True
        far = reference
        in_band = True
    else:
        assert reference == (exact > 0), (num, den, eps)       # outside the band the squared comparison is the reference's answer
        far, in_band = exact > 0, False
    if mutant == "ge_for_gt":
        far = far or exact == 0
    return far, in_band


def model(pts, eps_factor, mel, mutant=None, census=None, oracle=None, band_log=None):
    """-> (kept indices without 0 in the order the kernel finds them -- None when it rejects in Douglas-Peucker --, class, quad or None).
    census: a dict of CENSUS_KEYS to add to.  band_log: a list that receives (num, den, exact ratio
    num^2 / (eps^2 den)) of every chord in the band.  The steps behind Douglas-Peucker are the oracle's (hull, winding) unless a mutant drops them."""
    assert mutant is None or mutant in MUTANTS
    p = np.ascontiguousarray(pts, dtype=np.int64).reshape(-1, 2)
    n = len(p)
    G = width_of(n)
    eps = float(n) * float(eps_factor)
    e2 = Fraction(eps) ** 2
    x, y = p[:, 0], p[:, 1]
    if census is not None:
        census["borders"] += 1
    work, kept, reject = [(0, n - 1)], [], False
    while work and not reject:
        a, b = work.pop()
        la, lb = int(y[a] - y[b]), int(x[b] - x[a])
        lc = int(x[a]) * int(y[b]) - int(x[b]) * int(y[a])
        if census is not None:
            census["chords"] += 1
            census["chords_pa_eq_pb"] += la == 0 and lb == 0
            if "_spans" in census:
                census["_spans"].add(b - a)         # the points the arg-max visits: a + 1 .. b
        if b == a:
            if census is not None:
                census["chords_zero"] += 1
            continue
        nums = np.abs(la * x[a + 1:b + 1] + lb * y[a + 1:b + 1] + lc)
        num = int(nums.max())
        if num == 0:
            if census is not None:
                census["chords_zero"] += 1
            continue
        at = np.nonzero(nums == num)[0]
        off = int(at[-1] if mutant == "tie_largest_index" else at[0])
        far, _ = _far(num, la * la + lb * lb, eps, e2, mutant, census, band_log)
        if census is not None:
            census["tie_chords"] += len(at) > 1
            if far:      # where the winner sat in the kernel's visiting order: four loads per trip, G apart; trips 4 G apart
                census[f"win_u{off // G % 4}"] += 1
                last_trip, partial = (b - a - 1) // (4 * G), (b - a) % (4 * G) != 0
                census["win_last_partial_trip" if off // (4 * G) == last_trip and partial else "win_full_trip"] += 1
        if not far:
            continue
        index = a + 1 + off
        if len(kept) == 3:
            if mutant == "no_fourth_split_reject":
                continue
            if census is not None and work:
                census["fourth_split_with_work_left"] += 1
            reject = True
            break
        kept.append(index)
        work.append((a, index))
        work.append((index, b))
    if reject or len(kept) != 3:
        if census is not None:
            census["reject_point_count"] += 1
        return (None if reject else kept), "reject_point_count", None
    quad = p[[0] + sorted(kept)]
    if mutant != "no_hull":
        hull = oracle.convex_hull(quad.astype(np.uint32)).astype(np.int64)
        if len(hull) != 4:
            if census is not None:
                census["reject_convexity"] += 1
            return kept, "reject_convexity", None
        quad = hull
    d2 = [int(((quad[i] - quad[(i + 1) % 4]) ** 2).sum()) for i in range(4)]
    short = min(math.isqrt(d) for d in d2) < mel if mutant == "edge_unsquared" else min(min(d2), mel + 1) < mel
    if short:
        if census is not None:
            census["reject_edge_length"] += 1
        return kept, "reject_edge_length", None
    (x0, y0), (x1, y1), (x2, y2) = quad[0], quad[1], quad[2]
    flip = (x1 - x0) * (y2 - y0) - (y1 - y0) * (x2 - x0) < 0
    if flip and mutant != "no_winding_fix":
        quad = quad[[0, 3, 2, 1]]
    if census is not None:
        census["accepted"] += 1
        census["winding_flipped"] += bool(flip)
    return kept, "accepted", quad


# ------------------------------------------------------------------------------------------------------------------------------------
# borders
# ------------------------------------------------------------------------------------------------------------------------------------
def is_closed_walk(pts):
    """consecutive points, and the last and the first, are 8-neighbours or equal"""
    p = np.asarray(pts, dtype=np.int64).reshape(-1, 2)
    return bool((np.abs(p - np.roll(p, -1, axis=0)).max(axis=1) <= 1).all())


def walk(vertices):
    """the closed 8-connected walk round a polygon: a digital line (one point per step of the longer axis, the shorter one rounded to
    nearest) from each vertex to the next, every vertex visited exactly, starting at the first"""
    v = np.asarray(vertices, dtype=np.int64)
    out = []
    for p, q in zip(v, np.roll(v, -1, axis=0)):
        d = q - p
        steps = int(np.abs(d).max())
        i = np.arange(steps, dtype=np.int64)[:, None]
        out.append(p + np.sign(d) * ((2 * i * np.abs(d) + steps) // (2 * steps)) if steps else p[None, :])
    return np.concatenate(out)


def fill_poly(vertices, shape):
    """pixels on or inside a polygon (even-odd rule on pixel centres, plus its outline as walk() draws it)"""
    v = np.asarray(vertices, dtype=np.float64)
    yy, xx = np.mgrid[0:shape[0], 0:shape[1]]
    inside = np.zeros(shape, bool)
    for (x0, y0), (x1, y1) in zip(v, np.roll(v, -1, axis=0)):
        if y0 == y1:
            continue
        crosses = ((y0 <= yy) != (y1 <= yy)) & (xx < x0 + (yy - y0) * (x1 - x0) / (y1 - y0))
        inside ^= crosses
    w = walk(vertices)
    inside[w[:, 1], w[:, 0]] = True
    return inside


def trace(oracle, fg):
    """oracle.find_contours on a painted shape with a one-pixel margin -> [(points n x 2 int64 in the shape's coordinates + 1, is_hole)]"""
    cs, bt, _ = oracle.find_contours(np.where(np.pad(np.asarray(fg, bool), 1), 255, 0).astype(np.uint8))
    return [(c.astype(np.int64), bool(t)) for c, t in zip(cs, bt)]


def orientations(fg):
    """the eight orientations of the square"""
    out = []
    for k in range(4):
        r = np.rot90(fg, k)
        out += [r, r[:, ::-1]]
    return [np.ascontiguousarray(o) for o in out]


def block(n):
    """a painted shape whose outer border has exactly n points: single pixels and dominoes, an L-tromino, then w x h blocks (border
    2 (w + h) - 4), for odd n with one corner pixel cut.  A 17 x 17 block gives 64, an 18 x 17 block 66, each less a corner 63 and 65."""
    if n == 1: return np.ones((1, 1), bool)
    if n == 2: return np.ones((1, 2), bool)
    if n == 3: return np.array([[1, 1], [1, 0]], bool)
    s = (n + (n & 1) + 4) // 2                    # w + h
    h = s // 2
    fg = np.ones((h, s - h), bool)
    if n & 1:
        fg[-1, -1] = False
    return fg


def ring(fg):
    """the shape as a hole: a 2-pixel frame of foreground round it, the shape itself background"""
    return ~np.pad(~np.asarray(fg, bool), 2)


def _oracle():
    from oracle import a3oracle

    a3oracle.build()
    return a3oracle


class Border:
    """one closed walk: name, points (n x 2 int64, non-negative) and what it was built for"""
    def __init__(self, name, pts, hand_made=False):
        self.name, self.pts, self.hand_made = name, np.ascontiguousarray(pts, dtype=np.int64).reshape(-1, 2), hand_made
        self.n = len(self.pts)

    def at(self, dx, dy, tag):
        return Border(f"{self.name}@{tag}", self.pts + (dx, dy), self.hand_made)

    def against(self, corner, tag):
        """translated so that its largest coordinates are corner - 1"""
        mx, my = self.pts.max(axis=0)
        return self.at(corner - 1 - mx, corner - 1 - my, tag)


LENGTHS_16 = (1, 2, 3, 4, 5, 6, 7, 8, 16, 17, 18, 32, 33, 34, 48, 49, 50, 63, 64)
LENGTHS_64 = (65, 66, 128, 129, 130, 255, 256, 257, 258, 511, 512, 513, 514, 1025, 1026, 4097)
RING_BLOCKS = (1, 2, 3, 4, 6, 8, 16, 17, 30, 31, 32, 33, 34, 48, 60, 62, 63, 64, 65, 66, 128, 129, 256, 257)


def _polygons(s):
    """painted polygons at scale s, by the number of vertices Douglas-Peucker is meant to find"""
    shape = (9 * s + 2, 11 * s + 2)
    plus = np.zeros((9 * s, 9 * s), bool)
    plus[3 * s:6 * s, :] = True
    plus[:, 3 * s:6 * s] = True
    ell = np.zeros((8 * s, 8 * s), bool)
    ell[:, :3 * s] = True
    ell[5 * s:, :] = True
    yy, xx = np.mgrid[0:8 * s + 1, 0:8 * s + 1]
    return {
        "triangle": fill_poly([(0, 0), (10 * s, 0), (0, 8 * s)], shape),
        "sliver": fill_poly([(0, 0), (10 * s, s), (0, 2 * s)], shape),
        "pentagon": fill_poly([(4 * s, 0), (8 * s, 3 * s), (6 * s, 8 * s), (2 * s, 8 * s), (0, 3 * s)], shape),
        "hexagon": fill_poly([(2 * s, 0), (6 * s, 0), (8 * s, 4 * s), (6 * s, 8 * s), (2 * s, 8 * s), (0, 4 * s)], shape),
        "ell": ell, "plus": plus, "disk": (yy - 4 * s) ** 2 + (xx - 4 * s) ** 2 <= (4 * s) ** 2,
        "arrowhead": fill_poly([(0, 0), (10 * s, 4 * s), (0, 8 * s), (3 * s, 4 * s)], shape),
        "deep_arrowhead": fill_poly([(0, 0), (10 * s, 4 * s), (0, 8 * s), (6 * s, 4 * s)], shape),
        "kite": fill_poly([(3 * s, 0), (10 * s, 4 * s), (3 * s, 8 * s), (0, 4 * s)], shape),
        "slanted": fill_poly([(0, s), (9 * s, 0), (10 * s, 7 * s), (2 * s, 8 * s)], shape),
    }


# Band cases, found by a search with model() and committed as literals.  A w x h block with a bump b high and bw wide standing on its top
# side px from the left; traced as painted (no other orientation: the start point decides which chords exist).  Each makes Douglas-
# Peucker evaluate a chord whose num^2 and eps^2 den agree to nine digits at eps_factor 0.05; tests/test_quad_cases.py proves it.
#   (w, h, b, bw, px): n, (num, den) of the band chord, num^2 / (eps^2 den) - 1
BUMP_BAND_CASES = (
    (3, 6, 4, 1, 1),       # n = 20, (1, 1): eps = 1.0, ratio exactly 1, chord along an axis
    (8, 2, 3, 1, 3),       # n = 20, (5, 25): ratio exactly 1, chord in a 3-4-5 direction; rejected for convexity
    (9, 2, 2, 4, 4),       # n = 20, (5, 25): ratio exactly 1; ends with exactly four vertices
    (4, 15, 4, 1, 2),      # n = 40, (2, 1): ratio exactly 1
    (5, 24, 4, 1, 3),      # n = 60, (3, 1): ratio exactly 1
    (6, 33, 4, 1, 4),      # n = 80, (4, 1): ratio exactly 1 (wave form)
    (10, 39, 4, 1, 5),     # n = 100, (5, 1): ratio exactly 1 (wave form)
    (5, 12, 4, 1, 3),      # n = 36, (9, 25): -4.9e-17 -- n * 0.05 is not 9/5; ends with exactly four vertices
    (8, 9, 4, 1, 3),       # n = 36, (9, 25): -4.9e-17
    (6, 2, 3, 3, 1),       # n = 16, (4, 25): -1.1e-16
    (6, 9, 4, 4, 1),       # n = 32, (8, 25): -1.1e-16; four vertices
    (7, 5, 3, 3, 1),       # n = 24, (6, 25): -3.0e-16; four vertices
)
# Hand-made walks (walk() round these vertices) with a chord in a 3-4-5 direction whose farthest point lies at the rational n * eps_factor
# exactly.  In the first four the double n * eps_factor is SMALLER than that rational: num^2 > eps^2 den by 1e-16, yet num / sqrt(den) > eps is false
# in doubles -- and dn * dn > eps * eps * den, the squared comparison on its own, is true.  Only the reference's expression decides.
#   (eps_factor, vertices): n, (num, den), ratio - 1
WALK_BAND_CASES = (
    (0.05, ((0, 0), (40, 6), (11, -5), (0, -24), (42, -12))),      # n = 172, (430, 2500), +8.3e-17: wave form, accepted
    (0.05, ((0, 0), (31, -42), (12, -53), (1, -82), (5, -77))),    # n = 172, (430, 2500), +8.3e-17: wave form, rejected (point count)
    (0.12, ((0, 0), (9, -2), (12, 5), (0, 10), (10, 17))),         # n = 55, (99, 225), +1.1e-16: 16-lane form, accepted
    (0.12, ((0, 0), (21, 5), (20, 14), (9, 14), (10, 11))),        # n = 55, (99, 225), +1.1e-16: 16-lane form, rejected (point count)
    # ... and wave-form walks where the double lies above the rational (as in the bump cases): not far by either reckoning
    (0.05, ((0, 0), (14, 4), (4, 21), (10, 23), (10, 29))),        # n = 72, (36, 100), -4.9e-17: accepted
    (0.05, ((0, 0), (1, 23), (13, 28), (13, 35), (7, 36))),        # n = 84, (42, 100), -8.5e-17: accepted
    (0.05, ((0, 0), (-2, -1), (-30, 30), (-37, 30), (-38, 24))),   # n = 84, (42, 100), -8.5e-17: rejected (point count)
)


SPAN_ONE_WALK = ((0, 0), (1, 1), (35, 0), (17, -12))


def bump(w, h, b, bw, px):
    fg = np.zeros((h + b, w), bool)
    fg[b:, :] = True
    fg[:b, px:px + bw] = True
    return fg


@lru_cache(maxsize=None)
def small_borders():
    """every small border, as traced (coordinates from 1 up): name -> Border"""
    o = _oracle()
    out = []

    def add(name, fg, holes=False):
        for k, img in enumerate(orientations(fg)):
            for pts, is_hole in trace(o, ring(img) if holes else img):
                if is_hole == holes:
                    out.append(Border(f"{name}{'_hole' if holes else ''}_o{k}", pts))

    for n in LENGTHS_16 + LENGTHS_64:
        add(f"block{n}", block(n))
    for m in RING_BLOCKS:
        add(f"block{m}", block(m), holes=True)
    for s in (1, 2, 4, 9):
        for name, fg in _polygons(s).items():
            add(f"{name}_s{s}", fg)
            if s <= 4:
                add(f"{name}_s{s}", fg, holes=True)
    for s in (12, 13):                                       # smallest squared hull edge 121 and 144 in both group widths
        for t in (s, s + 8, 40, 60):
            add(f"rect{s}x{t}", np.ones((s, t), bool))
    for c in BUMP_BAND_CASES:
        for pts, is_hole in trace(o, bump(*c)):
            out.append(Border("bump_%d_%d_%d_%d_%d" % c, pts))
    return {b.name: b for b in out}


@lru_cache(maxsize=None)
def hand_walks():
    """eps_factor -> hand-made walks: the band walks above, and walks whose last point is their first (pa == pb on the first chord)"""
    out = {0.05: [], 0.12: [], 0.01: []}
    # A wave-form chord that visits ONE point (b - a = 1) needs a kept point next to a chord end, i.e. a point within sqrt(2) of a
    # line and yet farther than eps from it: impossible from 65 points on at eps_factor 0.05 (eps >= 3.25).  At 0.01 this walk of
    # 70 points (eps = 0.7) keeps its point 1, one step from its start, and then evaluates the chord (0, 1).
    w = walk(SPAN_ONE_WALK)
    out[0.01].append(Border("span_one", w - w.min(axis=0) + 1, hand_made=True))
    for i, (ef, v) in enumerate(WALK_BAND_CASES):
        w = walk(v)
        out[ef].append(Border(f"walk_band_{i}", w - w.min(axis=0) + 1, hand_made=True))
    for n_side in (5, 30):                                   # n = 4 * side + 1: 21 and 121 points
        w = walk([(0, 0), (n_side, 0), (n_side, n_side), (0, n_side)])
        out[0.05].append(Border(f"closed_twice_{len(w) + 1}", np.concatenate([w, w[:1]]) + 1, hand_made=True))
    return out


# large walks: Bresenham-like walks round convex polygons, about 65 000 points each
BIG_QUAD = ((3, 5), (16380, 40), (16383, 16379), (20, 16350))
BIG_PENTAGON = ((3, 5), (9000, 2), (16383, 7000), (12000, 16383), (10, 12000))
FAR_QUAD = ((0, 300), (32000, 0), (32700, 31000), (900, 32767))          # extent below 2^15, placed against (65535, 65535)
FAR_PENTAGON = ((0, 300), (20000, 0), (32700, 15000), (25000, 32767), (900, 30000))


@lru_cache(maxsize=None)
def large_walks():
    return {"big_quad": Border("big_quad", walk(BIG_QUAD), True), "big_pentagon": Border("big_pentagon", walk(BIG_PENTAGON), True),
            "far_quad": Border("far_quad", walk(FAR_QUAD), True).against(65536, "far64"),
            "far_pentagon": Border("far_pentagon", walk(FAR_PENTAGON), True).against(65536, "far64")}


# ------------------------------------------------------------------------------------------------------------------------------------
# launches
# ------------------------------------------------------------------------------------------------------------------------------------
class Launch:
    """one call of a3_debug_contour_quads: borders = [(frame, Border)] in record order; the rest are the hook's arguments"""
    def __init__(self, name, borders, width, height, eps_factor=0.05, mel=0, n_darts=0, first_frame=0, n_frames=1, max_cand=4096,
                 max_contours=None, ctr_contours=None, ctr_err_flags=0, seed=0):
        self.name, self.borders, self.width, self.height, self.eps_factor, self.mel = name, borders, width, height, eps_factor, mel
        self.n_darts, self.first_frame, self.n_frames, self.max_cand, self.ctr_err_flags = n_darts, first_frame, n_frames, max_cand, ctr_err_flags
        self.max_contours = len(borders) if max_contours is None else max_contours
        self.ctr_contours = len(borders) if ctr_contours is None else ctr_contours
        # start keys: unique (a bijection of the record index), all over u32, never in record order
        self.keys = (np.random.default_rng(seed).permutation(len(borders)).astype(np.uint64) * 2654435761 + 12345) % (1 << 32)

    def considered(self):
        """the records the kernel looks at"""
        if self.ctr_err_flags & (ERR_POINT_POOL | ERR_CONTOUR_TABLE):
            return 0
        return min(self.ctr_contours, self.max_contours, len(self.borders))

    def tables(self):
        rec = np.zeros(len(self.borders), dtype=CONTOUR_DTYPE)
        pool, base = [], 0
        for i, (frame, b) in enumerate(self.borders):
            rec[i] = (frame, self.keys[i], base, b.n)
            pool.append((b.pts[:, 0] | (b.pts[:, 1] << 16)).astype(np.uint32))
            base += b.n
        return rec, np.concatenate(pool) if pool else np.zeros(0, np.uint32)

    def kwargs(self):
        return dict(eps_factor=self.eps_factor, min_edge_length=self.mel, n_darts=self.n_darts, first_frame=self.first_frame,
                    n_frames=self.n_frames, max_cand=self.max_cand, max_contours=self.max_contours, ctr_contours=self.ctr_contours,
                    ctr_err_flags=self.ctr_err_flags)


MAX_GRID_DARTS = 1 << 23
MEL_SIDE = 121          # (12 - 1)^2: the smallest squared hull edge of the 12 x t blocks


def _mixed(rng):
    """more than 160 long and more than 1024 short borders, the widths interleaved, spread over three frames and over the 2^14 range"""
    small = list(small_borders().values()) + hand_walks()[0.05]
    short = [b for b in small if b.n <= K_SMALL]
    long_ = [b for b in small if K_SMALL < b.n <= 600]
    out, si, li = [], 0, 0
    while si < 1100 or li < 180:
        for _ in range(6):
            b = short[si % len(short)]
            si += 1
            out.append((2 + int(rng.integers(0, 3)), b.at(int(rng.integers(0, 16000)), int(rng.integers(0, 16000)), f"m{si}")))
        b = long_[li % len(long_)]
        li += 1
        out.append((2 + int(rng.integers(0, 3)), b.at(int(rng.integers(0, 15000)), int(rng.integers(0, 15000)), f"m{li}")))
    return out


@lru_cache(maxsize=None)
def launches():
    small = list(small_borders().values())
    walks = hand_walks()
    lg = large_walks()
    by = small_borders()
    L = {}

    def add(name, borders, *a, **k):
        L[name] = Launch(name, borders, *a, seed=len(L) + 1, **k)

    near = small + walks[0.05]
    add("small_near", [(0, b) for b in near], 16384, 16384)
    add("small_far14", [(0, b.against(16384, "far14")) for b in near], 16384, 16384)         # 24-bit products near 2^28
    add("small_far64", [(0, b.against(65536, "far64")) for b in near], 65536, 65536)         # la x in 32 bits would overflow
    add("walks_eps12", [(0, b) for b in walks[0.12]] + [(0, b.against(65536, "far64")) for b in walks[0.12]], 65536, 65536, eps_factor=0.12)
    add("walks_eps01", [(0, b) for b in walks[0.01]] + [(0, b.against(16384, "far14")) for b in walks[0.01]], 16384, 16384, eps_factor=0.01)
    rects = [b for b in small if b.name.startswith("rect12x")]
    for name, mel in (("mel_0", 0), ("mel_eq", MEL_SIDE), ("mel_plus1", MEL_SIDE + 1)):
        add(name, [(0, b) for b in rects], 640, 480, mel=mel)
    add("large_14", [(0, lg["big_quad"]), (0, lg["big_pentagon"])], 16384, 16384, mel=1000)
    add("large_64", [(0, lg["big_quad"]), (0, lg["big_pentagon"])], 16385, 16385, mel=1000)
    add("large_far", [(0, lg["far_quad"]), (0, lg["far_pentagon"])], 65536, 65536, mel=1000)
    mixed = _mixed(np.random.default_rng(7))
    add("mixed_min_grid", mixed, 16384, 16384, first_frame=2, n_frames=3, max_cand=2048)
    add("mixed_max_grid", mixed, 16384, 16384, first_frame=2, n_frames=3, max_cand=2048, n_darts=MAX_GRID_DARTS)
    L["mixed_max_grid"].keys = L["mixed_min_grid"].keys
    # four 16-lane groups of one wave on borders as unlike as can be: a single point, a quad, a rejection at the fourth split with
    # chords left, a border that enters the band
    unlike = [by["block1_o0"], by["block32_o3"], by["pentagon_s1_o3"], by["bump_5_12_4_1_3"]]
    add("neighbours", [(0, unlike[i % 4].at(40 * i, 17 * i, f"u{i}")) for i in range(64)], 4096, 4096)
    add("max_contours_below", [(0, b) for b in near], 16384, 16384, max_contours=len(near) // 2)
    add("ctr_contours_below", [(0, b) for b in near], 16384, 16384, ctr_contours=len(near) // 3)
    quads = [b for b in small if b.name.startswith("block") and "hole" not in b.name and 16 <= b.n <= 130]
    add("cand_overflow", [((1 if i % 3 else (0 if i % 2 else 2)), b) for i, b in enumerate(quads)], 640, 480, n_frames=3, max_cand=32)
    add("stale_point_pool", [(0, b) for b in quads], 640, 480, ctr_err_flags=ERR_POINT_POOL)
    add("stale_contour_table", [(0, b) for b in quads], 640, 480, ctr_err_flags=ERR_CONTOUR_TABLE | 1)
    return L


_results = {}


def border_result(b, eps_factor, mel):
    """(class, quad) by the oracle, once per distinct border"""
    key = (b.pts.tobytes(), eps_factor, mel)
    if key not in _results:
        _results[key] = expected_quad(_oracle(), b.pts, eps_factor, mel)
    return _results[key]


def expected(name):
    """per frame of the launch (first_frame .. first_frame + n_frames - 1): the expected records sorted by start key, as an
    (m, 9) int64 array of key and xy[8]"""
    L = launches()[name]
    rows = {f: [] for f in range(L.first_frame, L.first_frame + L.n_frames)}
    for i in range(L.considered()):
        frame, b = L.borders[i]
        cls, quad = border_result(b, L.eps_factor, L.mel)
        if quad is not None:
            rows[frame].append([int(L.keys[i])] + [int(v) for v in quad.reshape(8)])
    return {f: np.array(sorted(r), dtype=np.int64).reshape(-1, 9) for f, r in rows.items()}


def distinct_cases():
    """every distinct (border, eps_factor, mel) over all launches, among the records the kernel looks at"""
    seen, out = set(), []
    for L in launches().values():
        for i in range(L.considered()):
            b = L.borders[i][1]
            key = (b.pts.tobytes(), L.eps_factor, L.mel)
            if key not in seen:
                seen.add(key)
                out.append((L.name, b, L.eps_factor, L.mel))
    return out
