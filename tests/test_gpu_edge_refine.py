"""Edge-fit corner refinement on the MI355X (k_refine_edges; a3_refine_config.method A3_REFINE_EDGES): bit-equal to the CPU
restatement (tests/edge_refine_oracle.c) -- the stand-alone call on the hand-made scenes of tests/edge_refine_cases.py in every frame
format and layout, and a batch through every path that reaches enqueue_back: the plain call, submit / collect on two contexts in
rotation, a reduction (the refinement samples the full-size frames from mapped corners), a rectification (it samples the rectified
plane).  Switching the method leaves SUBPIX and "off" exactly what they were."""
import functools

import numpy as np
import pytest

from tests import edge_refine_cases as ec
from tests import edge_refine_oracle as ero
from tests import rectified_cases as rc
from tests import refine_oracle as refo
from tests import yuv422_util as yu
from tests.util import marker_tuples

pytestmark = pytest.mark.gpu

W, H = 640, 480
SIZE_MM = 100.0
RECT_K = (520.0, 520.0, 320.0, 240.0)
RECT_DEG = 3.0


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


def _edges(win_half=10, relative_win=0.4, max_iterations=30, min_shift=0.01):
    from aruco3_amd import _lib

    return _lib.RefineConfig(_lib.REFINE_EDGES, win_half, relative_win, max_iterations, min_shift)


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bit_equal(got, want, what):
    got, want = np.ascontiguousarray(got, np.float32), np.ascontiguousarray(want, np.float32)
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere(_bits(got) != _bits(want))
    assert bad.size == 0, (what, bad[:4].tolist(), got[tuple(bad[0])], want[tuple(bad[0])])


# ---- the stand-alone call on the hand-made scenes ----

FORMATS = ("L8", "RGB8", "RGBA8", "BGRA8", "YUYV8", "UYVY8")


def _pixels(grey, fmt):
    """-> (the frame's pixels (H, W, C) in the format, the luma plane the library makes of them)"""
    if fmt == "L8":
        return grey[..., None], grey
    if fmt in yu.FORMATS:
        return yu.interleave(grey, fmt, seed=5), grey
    rgb = rc.tint(grey)   # (three different planes: a swapped channel order changes the luma)
    luma = rc.luma(rgb)
    if fmt == "RGB8":
        return rgb, luma
    alpha = np.full(grey.shape + (1,), 77, np.uint8)
    return np.concatenate([rgb if fmt == "RGBA8" else rgb[..., ::-1], alpha], axis=-1), luma


@functools.lru_cache(maxsize=None)
def _want(name, tinted):
    grey, quads, cfg, cell = ec.scenes()[name]
    luma = rc.luma(rc.tint(grey)) if tinted else grey
    return ero.refine_quads(luma, quads, cfg, cell)


def _fmt_value(fmt):
    from aruco3_amd import _lib

    return getattr(_lib, "FMT_" + fmt)


@pytest.mark.parametrize("fmt", FORMATS)
def test_standalone_quads_equal_the_oracle(fmt):
    from aruco3_amd import ARDictionary, _lib

    torch = _torch()
    d = ARDictionary.new_from_named_dict("ARUCO")
    ctx = _lib.Context(_lib.default_config(), d.code_list, d.num_bits, d._tau)
    moved = 0
    for name, (grey, quads, cfg, cell) in ec.scenes().items():
        px, luma = _pixels(grey, fmt)
        want = _want(name, fmt in ("RGB8", "RGBA8", "BGRA8"))
        assert np.array_equal(luma, rc.luma(rc.tint(grey)) if fmt in ("RGB8", "RGBA8", "BGRA8") else grey)
        moved += int(not np.array_equal(want, quads))
        ctx.set_corner_refinement(_lib.RefineConfig(_lib.REFINE_EDGES, cfg.win_half, cfg.relative_win, cfg.max_iterations, cfg.min_shift))
        cell_arg = None if cell is None else np.repeat(cell, 4)   # one value per corner; the quad's first is read
        if cell_arg is not None:
            cell_arg[1::4] = 1.0e6
            cell_arg[2::4] = np.nan
        h, w, c = px.shape
        for lead, pad in ((0, 0), (5, 7)):   # tightly packed; an odd offset and padded rows
            row = w * c + pad
            buf = np.full(lead + row * h + 16, 0x5A, np.uint8)
            buf[lead: lead + row * h].reshape(h, row)[:, : w * c] = px.reshape(h, w * c)
            dev = torch.from_numpy(buf).cuda()
            torch.cuda.synchronize()
            for ptr, mem in ((buf.ctypes.data + lead, _lib.MEM_HOST), (dev.data_ptr() + lead, _lib.MEM_DEVICE)):
                got = ctx.refine_corners(ptr, mem, _fmt_value(fmt), w, h, row, quads.reshape(-1, 2), cell_arg)
                _bit_equal(got.reshape(-1, 4, 2), want, (name, fmt, lead, mem))
    assert moved >= 4   # (the scenes that refine, not only those that return the start)
    ctx.close()


def test_argument_errors():
    from aruco3_amd import ARDictionary, _lib

    _torch()
    d = ARDictionary.new_from_named_dict("ARUCO")
    ctx = _lib.Context(_lib.default_config(), d.code_list, d.num_bits, d._tau)
    grey = np.ascontiguousarray(ec.slanted_frame())
    six = np.concatenate([ec.slanted_start(), ec.slanted_start()[:2]])
    args = (grey.ctypes.data, _lib.MEM_HOST, _lib.FMT_L8, ec.W, ec.H, ec.W)
    ctx.set_corner_refinement(_edges())
    with pytest.raises(_lib.A3Error) as e:
        ctx.refine_corners(*args, six)
    assert e.value.code == _lib.ERR_INVALID and "multiple of 4" in str(e.value)
    for bad in (_lib.RefineConfig(3, 5, 0.4, 30, 0.01), _edges(win_half=11), _edges(win_half=0), _edges(max_iterations=101)):
        with pytest.raises(_lib.A3Error) as e:
            ctx.set_corner_refinement(bad)
        assert e.value.code == _lib.ERR_INVALID
    # a refused setting is not kept: the context still refines quads, and SUBPIX still takes six single corners
    got = ctx.refine_corners(*args, ec.slanted_start())
    _bit_equal(got.reshape(1, 4, 2), ero.refine_quads(grey, ec.slanted_start()[None], ero.config(10, 0.4)), "after refusals")
    ctx.set_corner_refinement(_lib.default_refine_config())
    _bit_equal(ctx.refine_corners(*args, six), refo.refine_corners(grey, six), "subpix")
    ctx.close()


# ---- a batch: two config-1 frames and a 640 x 480 crop of a config-2 frame ----

@functools.lru_cache(maxsize=None)
def _frames():
    from aruco3_amd import synth

    f1, _ = synth.config_frames(1, 2)
    f2, _ = synth.config_frames(2, 1)
    out = np.concatenate([f1, f2[:, 180:180 + H, 600:600 + W]])   # (the crop holds two whole slanted markers)
    assert out.shape == (3, H, W, 3)
    out.setflags(write=False)
    return out


def _dict():
    from aruco3_amd import ARDictionary

    return ARDictionary.new_from_named_dict("ARUCO_DEFAULT")


def _cells():
    return int(np.ceil(np.sqrt(_dict().num_bits))) + 2


def _chain(oracle, detect_on, sample_on, factor=1, method="edges"):
    """the oracle chain: the detector on each plane of detect_on, the corners mapped up by factor, the refinement on the luma planes
    sample_on -> (per-frame oracle results with mapped corners, refined corners (n, 4, 2))"""
    from tests import reduced_cases as rcs

    d = _dict()
    res, ref = [], []
    for plane, luma in zip(detect_on, sample_on):
        r = oracle.detect(np.ascontiguousarray(plane), d.code_list, d.num_bits, d._tau)
        for m in r["markers"]:
            if factor > 1:
                m["corners"] = rcs.map_corners(np.asarray(m["corners"]).reshape(4, 2), factor)
        quads = [np.asarray(m["corners"]).reshape(8) for m in r["markers"]]
        if method == "edges":
            ref.append(ero.refine_markers(luma, quads, _cells(), ero.config(10, 0.4)))
        else:
            ref.append(refo.refine_markers(luma, quads, _cells()))
        res.append(r)
    return res, np.concatenate(ref)


@functools.lru_cache(maxsize=None)
def _plain_chain(method="edges"):
    from oracle import a3oracle

    a3oracle.build()
    luma = [a3oracle.to_luma8(np.ascontiguousarray(f)) for f in _frames()]
    return _chain(a3oracle, _frames(), luma, method=method)


def _ctx(refine=None):
    from aruco3_amd import _lib

    d = _dict()
    ctx = _lib.Context(_lib.default_config(), d.code_list, d.num_bits, d._tau)
    if refine is not None:
        ctx.set_corner_refinement(refine)
    return ctx


def _device_batch():
    from aruco3_amd import _lib

    torch = _torch()
    dev = torch.from_numpy(_frames().copy()).cuda()
    torch.cuda.synchronize()
    return dev, (dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, 3)


def _same_markers(m, per, res, what):
    assert [int(v) for v in per] == [len(r["markers"]) for r in res], what
    got = [(int(x["id"]), tuple(int(v) for v in np.asarray(x["corners"]).reshape(8))) for x in m]
    want = [(int(x["id"]), tuple(int(v) for v in np.asarray(x["corners"]).reshape(8))) for r in res for x in r["markers"]]
    assert got == want, what


def test_batch_refined_corners_markers_and_poses(oracle):
    res, want = _plain_chain()
    assert [len(r["markers"]) for r in res] == [4, 4, 2]
    assert np.abs(want - np.rint(want)).max() > 0.05   # (the chain refines)
    dev, args = _device_batch()
    plain = _ctx()
    m0, p0, poses0 = plain.detect_batch_pose(*args, SIZE_MM)
    ctx = _ctx(_edges())
    m, per, poses = ctx.detect_batch_pose(*args, SIZE_MM)
    # the integer corners, ids and order are those of a batch without refinement
    assert marker_tuples(m) == marker_tuples(m0) and per.tolist() == p0.tolist()
    _same_markers(m, per, res, "plain")
    got = ctx.refined_corners()
    _bit_equal(got, want, "batch")
    # the poses are those the library solves from the same float corners given stand-alone
    pts = (got / np.array([W, H], np.float32)).astype(np.float32).reshape(-1, 8)
    alone = plain.estimate_pose_normalized(pts, SIZE_MM)
    for i in range(len(m)):
        for k in range(2):
            rec = alone[2 * i + k]
            ref = np.concatenate([[rec.error], np.array(rec.rotation), np.array(rec.translation)]).astype(np.float32)
            assert np.abs(poses[i, k] - ref).max() <= 1e-4, (i, k, poses[i, k], ref)
    assert not np.array_equal(poses, poses0)
    ctx.close()
    plain.close()


def test_submit_collect_on_two_contexts_in_rotation(oracle):
    res, want = _plain_chain()
    dev, args = _device_batch()
    a, b = _ctx(_edges()), _ctx(_edges())
    for _ in range(2):
        a.submit(*args)
        b.submit(*args)
        for c in (a, b):
            m, per = c.collect()
            _same_markers(m, per, res, "rotation")
            _bit_equal(c.refined_corners(), want, "rotation")
    a.close()
    b.close()


def test_with_a_reduction_the_full_size_frames_are_sampled(oracle):
    from aruco3_amd import _lib
    from tests import reduced_cases as rcs

    luma = [oracle.to_luma8(np.ascontiguousarray(f)) for f in _frames()]
    res, want = _chain(oracle, rcs.reduce(_frames(), 2), luma, factor=2)
    assert sum(len(r["markers"]) for r in res) >= 8
    assert np.abs(want - np.rint(want)).max() > 0.05
    dev, args = _device_batch()
    ctx = _ctx(_edges())
    ctx.set_reduction(_lib.ReductionRec(2))
    m, per = ctx.detect_batch(*args)
    _same_markers(m, per, res, "reduced")
    _bit_equal(ctx.refined_corners(), want, "reduced")
    ctx.close()


def test_with_a_rectification_the_rectified_plane_is_sampled(oracle):
    import ctypes as C

    from aruco3_amd import _lib
    from tests import rectify_oracle as ro

    R = ro.rot_y(RECT_DEG)
    rect = ro.rectify(_frames(), RECT_K, None, RECT_K, (W, H), R, 0)
    grey = rc.luma(rect)
    res, want = _chain(oracle, grey, grey)
    assert sum(len(r["markers"]) for r in res) >= 6   # (the turned view loses markers at its rim; two of the rest revert)
    assert np.abs(want - np.rint(want)).max() > 0.05
    rec = _lib.RectifyRec()
    rec.src = _lib.Intrinsics(W, H, *RECT_K)
    rec.dst = _lib.Intrinsics(W, H, *RECT_K)
    rec.rotation = (C.c_float * 9)(*[float(v) for v in R.reshape(9)])
    rec.fill = 0
    dev, args = _device_batch()
    ctx = _ctx(_edges())
    ctx.set_rectification(rec)
    m, per = ctx.detect_batch(*args)
    _same_markers(m, per, res, "rectified")
    _bit_equal(ctx.refined_corners(), want, "rectified")
    ctx.close()


def test_switching_the_method_leaves_subpix_and_off_as_they_were(oracle):
    from aruco3_amd import _lib

    res, want_edges = _plain_chain()
    _, want_subpix = _plain_chain("subpix")
    dev, args = _device_batch()
    ctx = _ctx(_edges())
    m, per = ctx.detect_batch(*args)
    _bit_equal(ctx.refined_corners(), want_edges, "edges")
    ctx.set_corner_refinement(_lib.default_refine_config())
    m1, per1 = ctx.detect_batch(*args)
    _bit_equal(ctx.refined_corners(), want_subpix, "subpix after edges")
    only = _ctx(_lib.default_refine_config())   # a context that never had the method
    only.detect_batch(*args)
    assert np.array_equal(_bits(only.refined_corners()), _bits(ctx.refined_corners()))
    ctx.set_corner_refinement(None)
    m2, per2 = ctx.detect_batch(*args)
    with pytest.raises(_lib.A3Error) as e:
        ctx.refined_corners()
    assert e.value.code == _lib.ERR_INVALID
    assert marker_tuples(m) == marker_tuples(m1) == marker_tuples(m2) and per.tolist() == per1.tolist() == per2.tolist()
    ctx.close()
    only.close()
