"""tests/yuv422_scenes.py drawn on the host and run through the CPU oracle: the frames of tests/test_gpu_yuv422_pipeline.py show markers
in every frame, and the planes reduced by 2, 3 and 4 and the rectified view still show some -- otherwise the GPU test's "4:2:2 equals
L8" would be an equality of empty lists.  No GPU."""
import numpy as np
import pytest

from tests import reduced_cases as rd
from tests import rectify_oracle as ro
from tests import yuv422_scenes as sc
from tests import yuv422_util as yu


def _ids(oracle, plane):
    d = sc.dictionary()
    return [m["id"] for m in oracle.detect(np.ascontiguousarray(plane), d.code_list, d.num_bits, d._tau, sc.oracle_config(), keep_debug=False)["markers"]]


@pytest.mark.parametrize("kind", ["grid", "charuco"])
def test_every_frame_shows_board_markers(oracle, kind):
    board = sc.grid_board() if kind == "grid" else sc.charuco_board()
    luma = sc.host_luma(kind)
    assert luma.shape == (4, sc.H, sc.W)
    for f, g in enumerate(luma):
        found = set(_ids(oracle, g)) & set(int(i) for i in board.ids)
        assert len(found) >= 3, (kind, f, found)


def test_reduced_and_rectified_views_still_show_markers(oracle):
    board_ids = set(int(i) for i in sc.grid_board().ids)
    luma = sc.host_luma("grid")
    for f in sc.FACTORS:
        per_frame = [len(set(_ids(oracle, p)) & board_ids) for p in rd.reduce(luma[..., None], f)]
        assert sum(per_frame) >= 8 and sum(1 for n in per_frame if n) >= 3, (f, per_frame)
    rect = ro.rectify(luma[..., None], sc.K, sc.LENS, sc.K, (sc.W, sc.H), None, 0)[..., 0]
    assert not np.array_equal(rect, luma)   # (the lens does something)
    per_frame = [len(set(_ids(oracle, g)) & board_ids) for g in rect]
    assert min(per_frame) >= 3, per_frame
    # the ChArUco frames: reduced by 2 and rectified
    ids = set(int(i) for i in sc.charuco_board().ids)
    luma = sc.host_luma("charuco")
    assert sum(len(set(_ids(oracle, p)) & ids) for p in rd.reduce(luma[..., None], 2)) >= 6
    rect = ro.rectify(luma[..., None], sc.K, sc.LENS, sc.K, (sc.W, sc.H), None, 0)[..., 0]
    assert min(len(set(_ids(oracle, g)) & ids) for g in rect) >= 2


def test_interleaving_keeps_the_luma_and_nothing_else():
    luma = sc.host_luma("grid")
    for fmt in yu.FORMATS:
        px = yu.interleave(luma, fmt, seed=1)
        other = yu.complement_chroma(px, fmt)
        assert px.shape == luma.shape + (2,) and np.array_equal(yu.luma_of(px, fmt), luma) and np.array_equal(yu.luma_of(other, fmt), luma)
        c = 1 - yu.LUMA_OFFSET[fmt]
        assert np.array_equal(other[..., c], 255 - px[..., c]) and len(np.unique(px[..., c])) == 256   # chroma: noise, independent of the luma
    assert not np.array_equal(yu.interleave(luma, "YUYV8", 1).reshape(-1), yu.interleave(luma, "UYVY8", 1).reshape(-1))
    p = yu.planar(luma, seed=2)
    assert p.shape == (4, sc.H * 3 // 2, sc.W) and np.array_equal(p[:, : sc.H], luma) and len(np.unique(p[:, sc.H:])) == 256
