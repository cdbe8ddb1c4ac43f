"""The scenes of tests/contour_scenes.py are what they claim to be, checked through the CPU oracle (and, on small versions,
through tests/dart_model.py): a scene that silently degrades -- a threshold that merges strokes, a border that no longer
crosses a tile -- fails here instead of passing vacuously in tests/test_gpu_contour_paths.py.  No GPU."""
import numpy as np
import pytest

from tests import contour_scenes as S
from tests.dart_model import contours_by_darts


def _borders(oracle, frame):
    return oracle.find_contours(oracle.adaptive_threshold(frame, 7))


@pytest.mark.parametrize("name", sorted(S.STRUCTURED))
@pytest.mark.parametrize("h,w,seed", [(64, 96, 0), (65, 257, 1), (130, 300, 2), (333, 251, 3)])
def test_structured_scenes_threshold_to_their_painted_foreground(oracle, name, h, w, seed):
    f = S.STRUCTURED[name](h, w, seed)
    assert f.shape == (h, w) and f.dtype == np.uint8
    assert np.array_equal(oracle.adaptive_threshold(f, 7) > 0, S.intended(f))
    assert np.array_equal(f, S.STRUCTURED[name](h, w, seed))          # deterministic


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_every_scene_takes_any_shape(name):
    for h, w in ((1, 1), (2, 3), (3, 2), (7, 5), (63, 65)):
        f = S.SCENES[name](h, w, 5)
        assert f.shape == (h, w) and f.dtype == np.uint8


def test_long_borders(oracle):
    """one border each; the serpentine's is >= 150 000 points at 480 x 640 (about 2^17 hops over hundreds of dart tiles), and
    > 1 000 000 at 1080 x 1920"""
    for name, h, w, least in (("serpentine", 480, 640, 150_000), ("spiral", 480, 640, 150_000), ("serpentine2", 480, 640, 120_000),
                              ("serpentine", 1080, 1920, 1_000_000), ("spiral", 1080, 1920, 1_000_000)):
        cs, _, _ = _borders(oracle, S.SCENES[name](h, w, 0))
        assert len(cs) == 1 and len(cs[0]) >= least, (name, h, w, [len(c) for c in cs])


def test_spiral_border_runs_in_all_four_directions_across_tiles(oracle):
    cs, _, _ = _borders(oracle, S.spiral(480, 640, 0))
    p = cs[0].astype(np.int64)
    d = np.diff(p, axis=0)
    assert {(1, 0), (-1, 0), (0, 1), (0, -1)} <= set(map(tuple, d.tolist()))
    tiles = set(map(tuple, (p // [S.TILE_W, S.TILE_H]).tolist()))
    assert len(tiles) == 3 * 8            # every tile of the frame


def _depth(par):
    depth = np.zeros(len(par), np.int64)
    for i, p in enumerate(par):       # parents precede their children in discovery order
        depth[i] = 0 if p < 0 else depth[p] + 1
    return depth


@pytest.mark.parametrize("h,w,least", [(96, 128, 20), (480, 640, 100)])
def test_nested_rings_are_deep(oracle, h, w, least):
    cs, _, par = _borders(oracle, S.nested_rings(h, w, 0))
    assert all(p < i for i, p in enumerate(par.tolist()))
    assert _depth(par).max() >= least


@pytest.mark.parametrize("seed", [0, 1, 3])
def test_comb_borders_cross_every_tile_boundary(oracle, seed):
    h, w = 300, 700
    f = S.comb(h, w, seed)
    cs, _, _ = _borders(oracle, f)
    xs, ys = set(), set()
    for c in cs:
        p = c.astype(np.int64)
        q = np.roll(p, -1, axis=0)
        for a, b in ((p, q), (q, p)):
            xs |= {int(v) for v, u in zip(a[:, 0], b[:, 0]) if u == v + 1 and (v + 1) % S.TILE_W == 0}
            ys |= {int(v) for v, u in zip(a[:, 1], b[:, 1]) if u == v + 1 and (v + 1) % S.TILE_H == 0}
    assert xs == {255, 511} and ys == {63, 127, 191, 255}
    # teeth end on both sides of the tile row boundaries
    fg = S.intended(f)
    ends = {int(np.argmin(fg[:, x])) - 1 for x in range(seed % 4, w, 4)}
    assert {e % S.TILE_H for e in ends} >= {62, 63, 0, 1}
    # a tooth on x = 255, 256 or 257 (by phase)
    want = {3: 255, 0: 256, 1: 257}.get(seed % 4)
    assert fg[: S.TILE_H, want].all()


@pytest.mark.parametrize("h,w", [(96, 128), (480, 640), (1080, 1920)])
def test_prune_bound_scene_lands_on_both_sides_of_the_bound(oracle, dicts, h, w):
    """n^2 = 8 mel: borders just below (pruned), at and just above it (kept), and candidates that a bound twice as tight would
    lose (diamonds: n^2 = 8 x their shortest hull edge squared)"""
    d = dicts.new_from_named_dict("ARUCO_DEFAULT")
    f = S.prune_bound(h, w, 0)
    mel = S.min_edge_length(h, w)
    res = oracle.detect(f, d.code_list, d.num_bits, d._tau)
    cs, _, _ = oracle.find_contours(res["thresholded"])
    n = np.array([len(c) for c in cs], np.int64)
    assert ((n >= 5) & (n * n < 8 * mel)).any() and ((n * n >= 8 * mel) & (n * n < 16 * mel)).any()
    q = res["candidates_pre"].astype(np.int64)
    assert len(q)
    e2 = ((q - np.roll(q, 1, axis=1)) ** 2).sum(axis=2).min(axis=1)
    assert (e2 < 2 * mel).any() and (e2 >= mel).all()


def test_prune_bound_small_frames_carry_short_borders(oracle):
    """frames with mel <= 3, where the n >= 5 part of the bound decides: borders of exactly 4, 5 and 6 points"""
    for h, w in ((16, 64), (19, 48)):
        cs, _, _ = _borders(oracle, S.prune_bound(h, w, 0))
        assert {4, 5, 6} <= {len(c) for c in cs}, (h, w)


def test_specks_are_single_pixels_and_diagonal_pairs(oracle):
    cs, _, _ = _borders(oracle, S.specks(96, 128, 0))
    lens = [len(c) for c in cs]
    assert set(lens) == {1, 2} and lens.count(2) > 50 and lens.count(1) > 200


def test_checkerboards_touch_diagonally(oracle):
    for cell in (1, 2, 3):
        f = S.checkerboard(64, 96, 0, cell)
        fg = S.intended(f)
        assert (fg[1:, 1:] & fg[:-1, :-1] & ~fg[1:, :-1]).any()          # diagonal-only contacts
        assert len(_borders(oracle, f)[0]) > 100


def test_edges_and_anomaly_touch_the_frame(oracle):
    for seed in range(4):
        b = oracle.adaptive_threshold(S.edges(96, 128, seed), 7) == 0
        assert b[:, 0].any() and b[0, :].any() and (b[:, -1].any() or b[-1, :].any()), seed
        assert b[3, 1] and b[4, 0]
    b = oracle.adaptive_threshold(S.anomaly(96, 128, 0), 7)
    assert b[3, 1] == 0 and b[4, 0] == 0 and b[0, 0] == 255


def test_fields_are_nontrivial(oracle):
    for name in ("blobs", "blobs_sparse", "blobs_dense", "noise"):
        assert len(_borders(oracle, S.SCENES[name](96, 128, 0))[0]) > 30, name
    assert len(_borders(oracle, S.blank(96, 128, 0))[0]) == 0


@pytest.mark.parametrize("name", sorted(S.SCENES))
def test_small_scenes_through_the_dart_model(oracle, name):
    """the parallel formulation (tests/dart_model.py) reproduces the oracle on a small version of every scene"""
    from tests.test_dart_model import _ref

    for h, w, seed in ((20, 24, 0), (13, 31, 1)):
        img = oracle.adaptive_threshold(S.SCENES[name](h, w, seed), 7)
        got, _ = contours_by_darts(img)
        assert got == _ref(oracle, img), (name, h, w, seed)
