"""The designed inputs of tests/refine_cases.py on the CPU restatement of sub-pixel corner refinement (tests/refine_oracle.c): the traced
entry equals the plain one bit for bit, every input reaches what it was designed for (the census), each deliberately wrong variant of
the oracle is told from the contract by at least one corner (so a kernel with that mistake fails tests/test_gpu_refine_cases.py), one
iteration agrees with a plain float64 statement of the contract, and refinement improves on rounded starts.  No GPU."""
import time

import numpy as np
import pytest

from tests import refine_cases as rcs
from tests import refine_oracle as refo

EXIT = {name: k for k, name in enumerate(refo.EXITS)}


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _group(group):
    return [c for c in rcs.cases() if c.group == group]


def test_cases_are_small_deterministic_and_quick():
    t0 = time.perf_counter()
    again = rcs.cases.__wrapped__()
    assert [c.name for c in again] == [c.name for c in rcs.cases()]
    for a, b in zip(again, rcs.cases()):
        assert np.array_equal(a.grey, b.grey) and np.array_equal(_bits(a.starts), _bits(b.starts))
        assert (a.cell is None) == (b.cell is None) and (a.cell is None or np.array_equal(_bits(a.cell), _bits(b.cell)))
        assert a.grey.shape[0] <= 80 and a.grey.shape[1] <= 96 and a.starts.dtype == np.float32
        # every start is one a3_refine_corners admits: finite, at most 64 px outside the frame
        h, w = a.grey.shape
        assert np.all((a.starts >= -64.0) & (a.starts <= np.array([w, h], np.float32) + 64.0))
    rcs.trace()
    assert time.perf_counter() - t0 < 20.0   # (about a second where this was written)


def test_trace_equals_the_plain_oracle_on_every_case():
    tr, want = rcs.trace(), rcs.expected()
    for c in rcs.cases():
        t = tr[c.name]
        assert np.array_equal(_bits(t["xy"]), _bits(want[c.name])), c.name
        assert np.all((t["w"] >= 1) & (t["w"] <= c.cfg.win_half)) and np.all(t["iters"] <= c.cfg.max_iterations), c.name
        if c.cell is None:
            assert np.all(t["w"] == c.cfg.win_half), c.name
        if c.cfg.max_iterations == 0:   # the result is the start
            assert np.array_equal(_bits(t["xy"]), _bits(c.starts)) and np.all(t["exit"] == EXIT["cap"]) and np.all(t["iters"] == 0), c.name
        gone = (t["exit"] == EXIT["revert"]) | ((t["exit"] == EXIT["det0"]) & (t["iters"] == 1))
        assert np.array_equal(_bits(t["xy"][gone]), _bits(c.starts[gone])), c.name   # a revert and a flat first window keep the start
        assert np.all(t["excursion"] <= t["w"]), c.name   # no estimate is kept farther than w from its start
        assert np.all(np.isfinite(t["xy"])), c.name


def test_census():
    cen = rcs.census()
    for w in rcs.WINDOWS:
        for e in ("det0", "revert", "converged", "cap"):
            assert cen["exits"][w][e] >= 1, (w, e, cen["exits"][w])
        # unreachable: the five sums are bounded by 441 * 510^2 (the weights are at most 1, a gradient at most 255 - 0 ... a bilinear
        # difference of two grey levels), so det is far below FLT_MAX and never NaN
        assert cen["exits"][w]["nonfinite"] == 0
        assert cen["stay_excursion"][w] >= w - 0.5, (w, cen["stay_excursion"][w])
    assert cen["cell_windows"] >= set(range(2, 11))


def test_each_input_reaches_what_it_was_designed_for():
    tr = rcs.trace()
    for w in rcs.WINDOWS:
        # revert and far travel, about all four corners of the box: the starts w + 0.25 away revert on their second step, those w - 0.25
        # away travel nearly the whole window, toward each side of the tile, and stay
        t = tr[f"revert_w{w}"]
        st = rcs.box_starts(w)
        assert np.all(t["exit"][0::2] == EXIT["revert"]) and np.all(t["iters"][0::2] == 2), (w, t["exit"], t["iters"])
        assert np.all(t["exit"][1::2] == EXIT["converged"]) and np.all(t["excursion"][1::2] >= w - 0.5), (w, t["exit"], t["excursion"])
        signs = {tuple(np.sign(d).astype(int)) for d in (t["xy"][1::2] - st[1::2])}
        assert signs == {(1, 1), (1, -1), (-1, 1), (-1, -1)}, (w, signs)
        corners = np.array([[x, y] for x in (rcs.BOX[0], rcs.BOX[2]) for y in (rcs.BOX[1], rcs.BOX[3])])
        assert np.abs(t["xy"][1::2] - corners).max() < 0.3, (w, t["xy"][1::2])
        # exactly singular: a flat frame, and straight edges where gradients are present but c2 == b == 0 or a == b == 0
        for name in rcs.singular_frames():
            t = tr[f"{name}_w{w}"]
            assert np.all(t["exit"] == EXIT["det0"]) and np.all(t["iters"] == 1), (name, w)
        # the converging corners converge on their corner, in more than one step, unless the cap ends them first
        t = tr[f"converging_w{w}_it30"]
        done = t["exit"] == EXIT["converged"]
        assert done.sum() >= 12 and np.all(t["iters"][done] >= 2), (w, t["exit"], t["iters"])
        assert np.abs(t["xy"][done] - np.repeat(rcs.SQUARE, 4, axis=0)[done]).max() < (0.8 if w == 1 else 0.35), w
        for it in (1, 3, 100):
            t = tr[f"converging_w{w}_it{it}"]
            capped = t["exit"] == EXIT["cap"]
            assert np.all(t["iters"][capped] == it) and (capped.sum() >= 4 or it == 100), (w, it, t["exit"])
        # frame borders: 64 px outside the tile is one replicated value; the windows of the nearer outside starts reach the frame
        for d in (0, 1, 2):
            t = tr[f"border_corners_d{d}_w{w}"]
            assert np.all(t["exit"][-rcs.N_FAR_OUTSIDE:] == EXIT["det0"]), (d, w)
    for w in rcs.WINDOWS:   # (at every window some start off the frame sees a rectangle's corner and iterates)
        near = np.concatenate([tr[f"border_corners_d{d}_w{w}"]["exit"][8: -rcs.N_FAR_OUTSIDE] for d in (0, 1, 2)])
        print(f"w {w}: {int(np.sum(near != EXIT['det0']))} of {len(near)} starts off the frame iterate")
        assert np.sum(near != EXIT["det0"]) >= 1, w
    # the relative window: each cell picks the window the contract states, and groups of four corners have four different windows
    for name in ("relative", "launch_long"):
        t = tr[name]
        assert np.array_equal(t["w"], np.array(rcs.CELL_WINDOWS)[np.arange(len(t["w"])) % 15]), name
        groups = t["w"][: len(t["w"]) // 4 * 4].reshape(-1, 4)
        assert sum(len(set(g)) == 4 for g in groups.tolist()) >= len(groups) // 4, name
    assert len(tr["launch_long"]["w"]) == 4 * 1024 + 7 and set(tr["launch_long"]["w"].tolist()) == set(range(2, 11))


def test_each_wrong_variant_is_told_from_the_contract():
    """Variants 3 .. 9 each change the bits of at least one corner and leave at least one case as it is: a kernel with that mistake
    fails tests/test_gpu_refine_cases.py, and not on every input.

    Variants 1 (the tile one column and row short) and 2 (its origin from a truncation) change no corner, here or anywhere: an estimate
    stays within w of q0 and a sample within w + 1 of an estimate, so the samples read columns floor(q0) - 2w - 1 .. floor(q0) + 2w + 2
    (the float sum c + i can round up to the integer floor(q0) + 2w + 2, whose right neighbour then has the weight 0).  Either variant
    only takes the tile's guard column from one side, which a3_subpix.h keeps for no read that counts.  This is asserted, as the
    proof of that header's sizing argument on the estimates that travel the whole window; variant 9, one column further in, is the
    mistake that can be seen."""
    base = rcs.trace()
    for v in refo.VARIANTS:
        tv = rcs.trace(v)
        changed = [n for n in base if not np.array_equal(_bits(tv[n]["xy"]), _bits(base[n]["xy"]))]
        print(f"variant {v}: {len(changed)} of {len(base)} cases change")
        if v in (1, 2):
            assert changed == [], (v, changed[:4])
        else:
            assert 1 <= len(changed) < len(base), (v, len(changed))
    # variant 8 is the relative window's: the cases with cell sizes tell it, and only they
    t8 = rcs.trace(8)
    assert {rcs.by_name(n).group for n in base if not np.array_equal(t8[n]["w"], base[n]["w"])} == {"relative", "launch"}


# ---- one iteration against a plain float64 statement of the contract (the text at the top of tests/refine_oracle.c) ----

def _sample64(grey, x, y):
    """bilinear grey level at float64 (x, y) arrays, border replicate"""
    h, w = grey.shape
    x0, y0 = np.floor(x), np.floor(y)
    fx, fy = x - x0, y - y0
    xa, xb = np.clip(x0, 0, w - 1).astype(int), np.clip(x0 + 1, 0, w - 1).astype(int)
    ya, yb = np.clip(y0, 0, h - 1).astype(int), np.clip(y0 + 1, 0, h - 1).astype(int)
    g = grey.astype(np.float64)
    return (1 - fy) * ((1 - fx) * g[ya, xa] + fx * g[ya, xb]) + fy * ((1 - fx) * g[yb, xa] + fx * g[yb, xb])


def _step64(grey, cx, cy, w):
    """one iteration from (cx, cy) in float64, sums in numpy's order over the whole window -> the new estimate"""
    i, j = np.meshgrid(np.arange(-w, w + 1, dtype=np.float64), np.arange(-w, w + 1, dtype=np.float64))
    m = np.exp(-(i * i) / (w * w)) * np.exp(-(j * j) / (w * w))
    gx = _sample64(grey, cx + i + 1, cy + j) - _sample64(grey, cx + i - 1, cy + j)
    gy = _sample64(grey, cx + i, cy + j + 1) - _sample64(grey, cx + i, cy + j - 1)
    a, b, c2 = np.sum(gx * gx * m), np.sum(gx * gy * m), np.sum(gy * gy * m)
    bb1, bb2 = np.sum(gx * gx * m * i + gx * gy * m * j), np.sum(gx * gy * m * i + gy * gy * m * j)
    det = a * c2 - b * b
    return cx + (c2 * bb1 - b * bb2) / det, cy + (-b * bb1 + a * bb2) / det


def _step_gaps():
    """-> (the largest |oracle - float64| of one step over the converging starts, the share of starts skipped as reverts)"""
    gap, skipped, total = 0.0, 0, 0
    for w in rcs.WINDOWS:
        c = rcs.by_name(f"converging_w{w}_it1")
        assert c.cfg.max_iterations == 1 and c.cfg.min_shift == 0.0
        t = rcs.trace()[c.name]
        for k, (x, y) in enumerate(c.starts):
            total += 1
            if t["exit"][k] == EXIT["revert"]:
                skipped += 1
                continue
            assert t["iters"][k] == 1 and t["exit"][k] in (EXIT["cap"], EXIT["converged"])
            nx, ny = _step64(c.grey, float(x), float(y), w)
            gap = max(gap, abs(float(t["xy"][k, 0]) - nx), abs(float(t["xy"][k, 1]) - ny))
    return gap, skipped / total


STEP_GAP = 6.9e-6   # px: the measured largest gap, rounded up (see the docstring below)


def test_one_step_equals_a_float64_statement():
    """One step of the oracle (float32, per lane and butterfly, (float)exp weights) from the 160 converging starts (16 at each window)
    against the same step in float64 with plain sums.  Measured: the largest difference is 6.85e-6 px (gcc 13, glibc), and none of
    the starts reverts on its first step.  The bound is four times the measured gap (other compilers' exp and sum orders), 2.8e-5 px,
    and must stay far below the 0.01 px min_shift: it is asserted to be under a hundredth of it.  The kernel is tied to this through
    bit equality with the oracle."""
    gap, share = _step_gaps()
    print(f"one step, oracle against float64: largest gap {gap:.3e} px, {share:.3f} of the starts skipped as reverts")
    assert share <= 0.1
    assert gap <= 4.0 * STEP_GAP
    assert 4.0 * STEP_GAP < 0.01 / 100.0


def _accuracy(w):
    start = np.rint(rcs.SQUARE).astype(np.float32)
    got = refo.refine_corners(rcs.square_frame(), start, rcs.cfg(w))
    return np.linalg.norm(start - rcs.SQUARE, axis=1), np.linalg.norm(got - rcs.SQUARE, axis=1)


@pytest.mark.parametrize("w,worst", [(3, 0.27), (5, 0.28), (10, 0.35)])
def test_refined_corners_improve_on_rounded_starts(w, worst):
    """SQUARE's four analytic corners, refined from their rounded positions, which are 0.374, 0.422, 0.600 and 0.348 px off.  The
    thresholds are the oracle's measured numbers with a margin, as in tests/test_oracle_refine.py (whose docstring says why a
    box-filtered edge leaves about 0.2 px): refined, the corners are 0.237, 0.229, 0.181, 0.211 px off at w = 3; 0.253, 0.239, 0.177,
    0.214 at w = 5; 0.320, 0.288, 0.225, 0.286 at w = 10 (the wider window weighs more of the one-pixel-wide edges).  Every corner is
    nearer than its start.  (At w = 1 the window does not reach from a start 0.6 px off: not asserted.)"""
    e_int, e_ref = _accuracy(w)
    print(f"w {w}: rounded starts {np.round(e_int, 3).tolist()} px off, refined {np.round(e_ref, 3).tolist()}")
    assert e_ref.max() <= worst
    assert np.all(e_ref < e_int)
