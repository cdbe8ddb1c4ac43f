"""Designed inputs for sub-pixel corner refinement (k_refine_corners), shared by tests/test_refine_cases.py (the CPU restatement: what
each input reaches, and that each of the oracle's deliberately wrong variants is told from the contract) and
tests/test_gpu_refine_cases.py (the kernel, bit for bit against the oracle).  A case is a small grey frame (at most 96 x 80), float32
starts, a RefineConfig and one cell size per start or None.  The census is built from the oracle's trace
(refine_oracle.refine_corners_trace).  Nothing here comes from the library under test.  TEST INFRASTRUCTURE ONLY."""
import functools
from collections import namedtuple

import numpy as np

from tests import refine_oracle as refo
from tests.edge_refine_cases import render, square

Case = namedtuple("Case", "name group grey starts cfg cell")

WINDOWS = tuple(range(1, 11))
W, H = 96, 80

# ---- converging corners: a rotated dark square at a sub-pixel position ----
SQUARE = square(47.3, 39.6, 20.0, 17.0)
_OFFSETS = np.array([[0.3, 0.1], [-0.2, 0.25], [0.15, -0.3], [-0.25, -0.2]])   # in windows
CONVERGING_CONFIGS = ((30, 0.01), (1, 0.0), (3, 0.0), (100, 0.0), (0, 0.01))   # (max_iterations, min_shift)


def cfg(win_half, relative_win=0.0, max_iterations=30, min_shift=0.01) -> refo.RefineConfig:
    return refo.RefineConfig(1, win_half, relative_win, max_iterations, min_shift)


@functools.lru_cache(maxsize=None)
def square_frame() -> np.ndarray:
    g = render([SQUARE], w=W, h=H)
    g.setflags(write=False)
    return g


def converging_starts(w) -> np.ndarray:
    """16 starts: every analytic corner of SQUARE + each of four offsets of up to 0.3 windows; start k belongs to corner k // 4"""
    return (SQUARE[:, None, :] + _OFFSETS[None] * w).reshape(-1, 2).astype(np.float32)


# ---- revert and far travel: an axis-aligned dark square, pixels 30..59 x 30..49, corners at (29.5 | 59.5, 29.5 | 49.5) ----
BOX = (29.5, 29.5, 59.5, 49.5)


def box_frame() -> np.ndarray:
    g = np.full((H, W), 220, np.uint8)
    g[30:50, 30:60] = 30
    return g


def box_starts(w) -> np.ndarray:
    """per corner of BOX two starts, outward along the diagonal: w + 0.25 away (reverts on its second step) and w - 0.25 away (travels
    nearly the whole window and stays); start 2k reverts, start 2k + 1 stays"""
    out = []
    for cx, sx in ((BOX[0], -1.0), (BOX[2], 1.0)):
        for cy, sy in ((BOX[1], -1.0), (BOX[3], 1.0)):
            for d in (w + 0.25, w - 0.25):
                out.append([cx + sx * d, cy + sy * d])
    return np.array(out, np.float32)


# ---- exactly singular ----
def singular_frames():
    flat = np.full((40, 56), 117, np.uint8)
    vertical = np.full((40, 56), 220, np.uint8)
    vertical[:, 28:] = 30
    horizontal = np.full((40, 56), 220, np.uint8)
    horizontal[20:, :] = 30
    return {"flat": flat, "vertical_edge": vertical, "horizontal_edge": horizontal}


SINGULAR_STARTS = np.array([[27.5, 19.5], [26.25, 18.0], [29.0, 21.75], [20.3, 12.6]], np.float32)

# ---- frame borders ----
BW, BH = 64, 48


def border_frames(d):
    """-> {"corners": four dark rectangles of 20 x 14, one in each frame corner with its outer corner d px from both frame edges,
    "edges": a dark cross whose eight outer corners lie d px from one frame edge each}, with their start lists (the integer corners
    and fractional neighbours)"""
    a = np.full((BH, BW), 220, np.uint8)
    for x in (d, BW - d - 20):
        for y in (d, BH - d - 14):
            a[y: y + 14, x: x + 20] = 30
    sa = [[x + ox, y + oy] for x in (d, BW - 1 - d) for y in (d, BH - 1 - d) for ox, oy in ((0.0, 0.0), (0.4, -0.3))]
    b = np.full((BH, BW), 220, np.uint8)
    b[16:32, d: BW - d] = 30
    b[d: BH - d, 20:44] = 30
    sb = [[x, y] for x in (d, BW - 1 - d) for y in (16, 31)] + [[x, y] for x in (20, 43) for y in (d, BH - 1 - d)]
    sb += [[d + 0.3, 16.4], [43.3, BH - 1 - d - 0.4]]
    return {"corners": (a, np.array(sa, np.float32)), "edges": (b, np.array(sb, np.float32))}


# starts off the frame whose windows reach into it, and starts 64 px outside (the most a3_refine_corners admits)
OUTSIDE_STARTS = np.array([[-0.5, 3.2], [-3.75, -2.5], [-0.25, -0.75], [BW - 0.5, 3.2], [BW + 2.75, BH + 1.5], [5.5, BH - 0.5], [BW - 1 + 0.6, BH - 1 + 0.9],
                           [-64.0, -64.0], [BW + 64.0, BH + 64.0], [-64.0, 10.0], [10.0, BH + 64.0]], np.float32)
N_FAR_OUTSIDE = 4   # (the last four of OUTSIDE_STARTS)

# ---- frames smaller than the tile ----
SMALL_SIZES = ((1, 1), (7, 5), (40, 3))   # (width, height)


def small_case(width, height, seed):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 256, (height, width), dtype=np.uint8)
    fixed = [[0.0, 0.0], [width - 1.0, height - 1.0], [width - 1.0, 0.0], [0.0, height - 1.0], [(width - 1) / 2.0, (height - 1) / 2.0 + 0.25],
             [-2.5, -1.25], [width + 3.5, height + 0.75], [-0.5, height - 0.5], [-64.0, height + 64.0]]
    rnd = np.stack([rng.uniform(-3.0, width + 2.0, 40), rng.uniform(-3.0, height + 2.0, 40)], axis=1)
    return g, np.concatenate([np.array(fixed), rnd]).astype(np.float32)


# ---- relative window: win_half 10, relative_win 0.4; floorf(0.4 * cell) = 0, 1, 2, 3, 9, 10, 11, 1e6, NaN, and 4 .. 8, and 3.6 ----
CELLS = np.array([1.0, 23.0, 5.5, 28.0, 3.0, 25.5, 8.0, 2.5e6, np.nan, 10.5, 20.5, 13.0, 18.0, 15.5, 9.0], np.float32)
CELL_WINDOWS = (2, 9, 2, 10, 2, 10, 3, 10, 2, 4, 8, 5, 7, 6, 3)   # the contract's window of each


def relative_starts(n) -> np.ndarray:
    """n starts within 0.6 px of SQUARE's corners (corner k % 4, one of 16 offsets), and their cells CELLS[k % 15]: every corner meets
    every cell, and four consecutive starts have four different cells"""
    base = (SQUARE[None, :, :] + _OFFSETS[:, None, :] * 2.0).reshape(-1, 2)   # (offset-major: consecutive starts are different corners)
    k = np.arange(n)
    return base[k % 16].astype(np.float32), CELLS[k % 15]


LONG_N = 4 * 1024 + 7


@functools.lru_cache(maxsize=None)
def cases():
    """every case, in one tuple.  Groups: converging, revert, singular, border, small, relative, launch"""
    out = []
    sq, box = square_frame(), box_frame()
    for w in WINDOWS:
        for it, eps in CONVERGING_CONFIGS:
            out.append(Case(f"converging_w{w}_it{it}", "converging", sq, converging_starts(w), cfg(w, 0.0, it, eps), None))
        out.append(Case(f"revert_w{w}", "revert", box, box_starts(w), cfg(w), None))
        for name, g in singular_frames().items():
            out.append(Case(f"{name}_w{w}", "singular", g, SINGULAR_STARTS, cfg(w), None))
        for d in (0, 1, 2):
            for name, (g, st) in border_frames(d).items():
                if name == "corners":
                    st = np.concatenate([st, OUTSIDE_STARTS])
                out.append(Case(f"border_{name}_d{d}_w{w}", "border", g, st, cfg(w), None))
    for i, (width, height) in enumerate(SMALL_SIZES):
        g, st = small_case(width, height, 11 + i)
        for w in (1, 10):
            out.append(Case(f"small_{width}x{height}_w{w}", "small", g, st, cfg(w), None))
    st, cell = relative_starts(60)
    out.append(Case("relative", "relative", sq, st, cfg(10, 0.4), cell))
    for n in (1, 2, 3):
        out.append(Case(f"launch_n{n}", "launch", sq, converging_starts(5)[:n], cfg(5), None))
        out.append(Case(f"launch_n{n}_mixed", "launch", sq, relative_starts(n)[0], cfg(10, 0.4), relative_starts(n)[1]))
    st, cell = relative_starts(LONG_N)
    out.append(Case("launch_long", "launch", sq, st, cfg(10, 0.4), cell))
    for c in out:
        c.grey.setflags(write=False)
        c.starts.setflags(write=False)
    assert len({c.name for c in out}) == len(out)
    return tuple(out)


def by_name(name) -> Case:
    return next(c for c in cases() if c.name == name)


@functools.lru_cache(maxsize=None)
def trace(variant=0):
    """name -> refine_oracle.refine_corners_trace of the case under the variant (0: the contract)"""
    return {c.name: refo.refine_corners_trace(c.grey, c.starts, c.cfg, c.cell, variant) for c in cases()}


@functools.lru_cache(maxsize=None)
def expected():
    """name -> a3o_refine_corners of the case: what the kernel is held to"""
    out = {c.name: refo.refine_corners(c.grey, c.starts, c.cfg, c.cell) for c in cases()}
    for v in out.values():
        v.setflags(write=False)
    return out


def census():
    """what the cases reach under the contract: {"exits": {w: {exit name: corners}}, "stay_excursion": {w: the largest excursion of a
    corner that did not revert}, "cell_windows": the windows chosen through cell_px}"""
    exits = {w: {e: 0 for e in refo.EXITS} for w in WINDOWS}
    stay = {w: 0.0 for w in WINDOWS}
    cell_windows = set()
    for c in cases():
        t = trace()[c.name]
        for w, e, far in zip(t["w"], t["exit"], t["excursion"]):
            exits[int(w)][refo.EXITS[e]] += 1
            if refo.EXITS[e] != "revert":
                stay[int(w)] = max(stay[int(w)], float(far))
        if c.cell is not None and c.cfg.relative_win > 0.0:
            cell_windows |= {int(w) for w in t["w"]}
    return {"exits": exits, "stay_excursion": stay, "cell_windows": cell_windows}
