"""Edge-fit corner refinement (A3_REFINE_EDGES) on its CPU restatement (tests/edge_refine_oracle.c, an extension beyond the reference):
accuracy against the synthetic renderer's true corners beside SUBPIX (tests/refine_oracle.c), corners mapped up from reduced planes,
the hand-made scenes of tests/edge_refine_cases.py, and the Python surface.

Absolute thresholds are the oracle's measured numbers with a margin (3 frames per config, search range from win_half 10):

    config   corners   edge fit median / p90 / p99 (px)   reverted   SUBPIX median (px)   thresholds median / p90
    1        48        0.150 / 0.176 / 0.182              0          0.175                0.17 / 0.20
    2        56        0.027 / 0.065 / 0.101              0          0.194                0.04 / 0.09
    4        41        0.039 / 0.088 / 1.364              4.9 %      0.185                0.05 / 0.11

(config 1 is axis-aligned, and the renderer's 3 x supersampling quantises such an edge to thirds of a pixel: that bounds both methods
there.  Config 4's reverted corners are one malformed quad.)  Reduced starts, config 2 at win_half 10: factor 2 median 0.023,
factor 3 median 0.027, none reverted; SUBPIX leaves 0 and 2 corners at their start."""
import ctypes as C

import numpy as np
import pytest

from tests import edge_refine_cases as ec
from tests import edge_refine_oracle as ero
from tests import refine_oracle as refo

N_FRAMES = 3
THRESHOLDS = {1: (0.17, 0.20), 2: (0.04, 0.09), 4: (0.05, 0.11)}


def _cells(d):
    return int(np.ceil(np.sqrt(d.num_bits))) + 2


def _errors(oracle, config, factor=1):
    """the frames, matching and start corners of tests/test_oracle_refine.py's _errors (start "detection"); with a factor the oracle
    detects on the reduced plane and the mapped corners start the refinement on the full-size grey.
    -> errors of the integer, SUBPIX and edge-fit corners, corners that the edge fit reverted, corners SUBPIX left at the start"""
    from aruco3_amd import ARDictionary, synth
    from tests import reduced_cases as rcs

    frames, truths = synth.config_frames(config, N_FRAMES)
    _, name = synth.config_spec(config)
    d = ARDictionary.new_from_named_dict(name)
    cells = _cells(d)
    e_int, e_sub, e_edge, reverted, stayed = [], [], [], 0, 0
    for f in range(N_FRAMES):
        if factor == 1:
            res = oracle.detect(frames[f], d.code_list, d.num_bits, d._tau)
            grey = res["grey"]
            quads = [np.asarray(m["corners"]).reshape(8) for m in res["markers"]]
            sub = refo.refine_markers(grey, quads, cells)
        else:
            grey = oracle.to_luma8(np.ascontiguousarray(frames[f]))
            res = oracle.detect(rcs.reduce(frames[f], factor), d.code_list, d.num_bits, d._tau)
            quads = [np.array(rcs.map_corners(np.asarray(m["corners"]).reshape(4, 2), factor)).reshape(8) for m in res["markers"]]
            sub = refo.refine_markers(grey, quads, cells, refo.RefineConfig(1, 10, 0.4, 30, 0.01))
        edge = ero.refine_markers(grey, quads, cells, ero.config(win_half=10))
        allt = np.concatenate([np.asarray(t.corners) for t in truths[f]])
        for q, s, e in zip(quads, sub, edge):
            ic = np.asarray(q, dtype=np.float64).reshape(4, 2)
            for k in range(4):
                j = int(np.argmin(np.linalg.norm(allt - ic[k], axis=1)))
                if np.linalg.norm(allt[j] - ic[k]) > 3.0 * factor:
                    continue   # (a corner that belongs to no true marker corner)
                e_int.append(np.linalg.norm(ic[k] - allt[j]))
                e_sub.append(np.linalg.norm(s[k] - allt[j]))
                e_edge.append(np.linalg.norm(e[k] - allt[j]))
                reverted += int(np.array_equal(e, ic.astype(np.float32)))   # (a marker reverts whole)
                stayed += int(np.array_equal(s[k], ic[k].astype(np.float32)))
    return np.array(e_int), np.array(e_sub), np.array(e_edge), reverted, stayed


@pytest.fixture(scope="module")
def unreduced(oracle):
    return {c: _errors(oracle, c) for c in (1, 2, 4)}


@pytest.mark.parametrize("config", [1, 2, 4])
def test_accuracy_against_the_renderers_truth(unreduced, config):
    e_int, e_sub, e_edge, reverted, _ = unreduced[config]
    med, p90 = THRESHOLDS[config]
    assert len(e_edge) >= 40
    print(f"config {config}: {len(e_edge)} corners, integer median {np.median(e_int):.3f}, SUBPIX median {np.median(e_sub):.3f} "
          f"p90 {np.percentile(e_sub, 90):.3f}, edge fit median {np.median(e_edge):.3f} p90 {np.percentile(e_edge, 90):.3f} "
          f"p99 {np.percentile(e_edge, 99):.3f}, reverted {reverted}")
    if config == 1:
        assert np.median(e_edge) <= np.median(e_sub)
    else:
        assert np.median(e_edge) <= 0.5 * np.median(e_sub)
    assert np.median(e_edge) <= med and np.percentile(e_edge, 90) <= p90
    assert reverted <= 0.10 * len(e_edge)


@pytest.mark.parametrize("factor", [2, 3])
def test_reduced_starts(oracle, unreduced, factor):
    e_int, e_sub, e_edge, reverted, stayed = _errors(oracle, 2, factor)
    assert len(e_edge) >= 40
    print(f"config 2 at factor {factor}: {len(e_edge)} corners, mapped median {np.median(e_int):.3f}, SUBPIX median {np.median(e_sub):.3f} "
          f"({stayed} at the start), edge fit median {np.median(e_edge):.3f} p90 {np.percentile(e_edge, 90):.3f} ({reverted} reverted)")
    assert reverted <= stayed
    assert np.median(e_edge) <= 2.0 * np.median(unreduced[2][2])


# ---- hand-made scenes ----

def _run(name):
    grey, quads, cfg, cell = ec.scenes()[name]
    return quads, ero.refine_quads(grey, quads, cfg, cell)


def _same_bits(a, b):
    return np.array_equal(np.asarray(a, np.float32).view(np.uint32), np.asarray(b, np.float32).view(np.uint32))


@pytest.mark.parametrize("name", ["flat", "faint", "far", "no_pass", "short_side"])
def test_the_start_is_returned(name):
    """no gradient; contrast 15, below the live level; one corner 30 px off (every corner reverts, not that one alone); max_iterations
    0; sides of 2.8 px"""
    quads, got = _run(name)
    assert _same_bits(got, quads)


# Measured: 0.051 - 0.115 px from either start, every pass count.  Larger than config 2's errors because the square is slanted by
# 17 degrees (a pixel-phase period of 3.27 px along a side) and its stations are 3.28 px apart: every station of a side sees the edge
# at nearly the same pixel phase, so the phase error of the bilinear gradient does not average out along the side.
SLANTED_BOUND = 0.15


def test_slanted_square_from_a_cut_corner():
    """a start with one corner 6 px along its side (as approximate_polygon_dp cuts one) and the others within 1 px: all four corners
    come out within SLANTED_BOUND of the analytic corners, where SUBPIX at win_half 5 leaves the cut corner where it was"""
    quads, got = _run("slanted")
    for q, g in zip(quads, got):
        err = np.linalg.norm(g.astype(np.float64) - ec.SLANTED, axis=1)
        print("start off by", np.linalg.norm(q - ec.SLANTED, axis=1).round(3), "-> off by", err.round(3))
        assert err.max() <= SLANTED_BOUND
    start = ec.slanted_start()
    assert np.linalg.norm(start[0] - ec.SLANTED[0]) > 5.9
    sub = refo.refine_corners(ec.slanted_frame(), start, refo.RefineConfig(1, 5, 0.0, 30, 0.01))
    assert _same_bits(sub[0], start[0])
    assert np.abs(sub[1:] - start[1:]).max() > 0.1
    # the relative range (r = 3 and 2 from the given cell sizes) still finds the sides: the passes walk the cut corner in
    quads, got = _run("slanted_relative")
    assert np.linalg.norm(got.astype(np.float64) - ec.SLANTED, axis=2).max() <= SLANTED_BOUND


def test_one_pass_moves_and_more_passes_settle():
    quads, one = _run("one_pass")
    _, many = _run("slanted")
    assert np.abs(one - quads).max() > 0.4 and not _same_bits(one, many)
    assert np.abs(one - many).max() < 0.2


def test_side_next_to_the_frame_border():
    """border replicate: the samples of the top side's stations reach past row 0; the result is finite, within 2r of the start and on
    the square"""
    grey, quads, cfg, _ = ec.scenes()["border"]
    _, got = _run("border")
    assert np.all(np.isfinite(got))
    assert np.abs(got - quads).max() <= 2.0 * cfg.win_half
    assert not _same_bits(got, quads)
    assert np.linalg.norm(got[0].astype(np.float64) - ec.BORDER, axis=1).max() <= SLANTED_BOUND


def test_bad_config_is_refused():
    with pytest.raises(ValueError):
        ero.refine_quads(np.zeros((8, 8), np.uint8), np.zeros((1, 4, 2), np.float32), ero.config(win_half=11))


# ---- Python surface ----

def test_python_surface():
    from aruco3_amd import _lib
    from aruco3_amd.aruco import CornerRefinement

    assert (_lib.REFINE_NONE, _lib.REFINE_SUBPIX, _lib.REFINE_EDGES) == (0, 1, 2)
    r = CornerRefinement()
    assert r.method == "subpix" and r._c().method == _lib.REFINE_SUBPIX
    p = CornerRefinement(3, 0.0, 7, 0.05)   # positional construction as before
    c = p._c()
    assert (c.method, c.win_half, c.max_iterations) == (_lib.REFINE_SUBPIX, 3, 7) and c.relative_win == 0.0
    e = CornerRefinement.edges()
    c = e._c()
    assert e.method == "edges" and (c.method, c.win_half, c.max_iterations) == (_lib.REFINE_EDGES, 10, 30)
    assert abs(c.relative_win - 0.4) < 1e-7 and abs(c.min_shift - 0.01) < 1e-9
    assert CornerRefinement.edges(win_half=5, min_shift=0.0)._c().win_half == 5
    assert CornerRefinement(5, 0.4, 30, 0.01, "edges")._c().method == _lib.REFINE_EDGES
    with pytest.raises(ValueError):
        CornerRefinement(method="contour")._c()
    L = _lib.load()   # the default the library hands out is unchanged
    d = _lib.RefineConfig()
    L.a3_default_refine_config(C.byref(d))
    assert (d.method, d.win_half) == (_lib.REFINE_SUBPIX, 5)
