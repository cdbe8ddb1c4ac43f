"""k_refine_corners on the MI355X on the designed inputs of tests/refine_cases.py: every window half-width 1 .. 10, every way an iteration
ends, estimates that travel the whole window toward each side of the tile, starts off the frame and at negative coordinates, frames
smaller than the tile, mixed windows in one workgroup, calls of 1, 2, 3 and 4 * 1024 + 7 corners.  Every result is bit-equal to the CPU
restatement (tests/refine_oracle.c, a3o_refine_corners); tests/test_refine_cases.py shows on the CPU what the inputs reach and that
each deliberately wrong variant of the oracle would differ here.  One context serves every setting."""
import functools

import numpy as np
import pytest

from tests import rectified_cases as rc
from tests import refine_cases as rcs
from tests import refine_oracle as refo
from tests import yuv422_util as yu
from tests.util import marker_tuples

pytestmark = pytest.mark.gpu

FORMATS = ("L8", "RGB8", "RGBA8", "BGRA8", "YUYV8", "UYVY8")
TINTED = ("RGB8", "RGBA8", "BGRA8")
LAYOUTS = ((0, 0), (5, 7))   # (bytes before the frame, bytes after each row): tightly packed; an odd offset and padded rows
FORMAT_GROUPS = ("converging", "revert", "border")   # the groups that run in every format; the others run in L8


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


def _ctx():
    from aruco3_amd import ARDictionary, _lib

    d = ARDictionary.new_from_named_dict("ARUCO")
    return _lib.Context(_lib.default_config(), d.code_list, d.num_bits, d._tau)


def _set(ctx, cfg):
    from aruco3_amd import _lib

    ctx.set_corner_refinement(_lib.RefineConfig(_lib.REFINE_SUBPIX, cfg.win_half, cfg.relative_win, cfg.max_iterations, cfg.min_shift))


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _bit_equal(got, want, what):
    assert got.shape == want.shape, (what, got.shape, want.shape)
    bad = np.argwhere((_bits(got) != _bits(want)).any(axis=1)).reshape(-1)
    assert bad.size == 0, (what, "corners", bad[:4].tolist(), got[bad[0]], want[bad[0]])


def _pixels(grey, fmt):
    """-> (the frame's pixels (H, W, C) in the format, the luma plane the library makes of them)"""
    if fmt == "L8":
        return grey[..., None], grey
    if fmt in yu.FORMATS:
        return yu.interleave(grey, fmt, seed=9), grey   # (junk chroma)
    rgb = rc.tint(grey)   # (three different planes: a swapped channel order changes the luma)
    luma = rc.luma(rgb)
    if fmt == "RGB8":
        return rgb, luma
    alpha = np.full(grey.shape + (1,), 77, np.uint8)
    return np.concatenate([rgb if fmt == "RGBA8" else rgb[..., ::-1], alpha], axis=-1), luma


@functools.lru_cache(maxsize=None)
def _want_tinted(name):
    c = rcs.by_name(name)
    return refo.refine_corners(rc.luma(rc.tint(c.grey)), c.starts, c.cfg, c.cell)


def _want(name, fmt):
    return _want_tinted(name) if fmt in TINTED else rcs.expected()[name]


class _Frames:
    """a case's frame in a format and layout, in host and in device memory; built once per distinct frame"""

    def __init__(self, torch):
        self.torch, self.made = torch, {}

    def get(self, grey, fmt, layout):
        key = (grey.shape, grey.tobytes(), fmt, layout)
        if key not in self.made:
            px, luma = _pixels(grey, fmt)
            assert np.array_equal(luma, rc.luma(rc.tint(grey)) if fmt in TINTED else grey)
            h, w, c = px.shape
            lead, pad = layout
            row = w * c + pad
            buf = np.full(lead + row * h + 16, 0x5A, np.uint8)
            buf[lead: lead + row * h].reshape(h, row)[:, : w * c] = px.reshape(h, w * c)
            dev = self.torch.from_numpy(buf).cuda()
            self.torch.cuda.synchronize()
            self.made[key] = (buf, dev, lead, row, w, h)
        return self.made[key]


def _run(ctx, frame, fmt, memory, starts, cell):
    from aruco3_amd import _lib

    buf, dev, lead, row, w, h = frame
    ptr = buf.ctypes.data + lead if memory == _lib.MEM_HOST else dev.data_ptr() + lead
    return ctx.refine_corners(ptr, memory, getattr(_lib, "FMT_" + fmt), w, h, row, starts, cell)


@pytest.mark.parametrize("fmt", FORMATS)
def test_every_case_equals_the_oracle(fmt):
    from aruco3_amd import _lib

    frames = _Frames(_torch())
    ctx = _ctx()   # one context across every setting
    ran = 0
    for c in rcs.cases():
        if c.name == "launch_long" or (fmt != "L8" and c.group not in FORMAT_GROUPS):
            continue
        want = _want(c.name, fmt)
        _set(ctx, c.cfg)
        for layout in LAYOUTS:
            frame = frames.get(c.grey, fmt, layout)
            for memory in (_lib.MEM_HOST, _lib.MEM_DEVICE):
                _bit_equal(_run(ctx, frame, fmt, memory, c.starts, c.cell), want, (c.name, fmt, layout, memory))
        ran += 1
    assert ran == (len(rcs.cases()) - 1 if fmt == "L8" else sum(c.group in FORMAT_GROUPS for c in rcs.cases()))
    ctx.close()


def test_switching_the_window_leaves_no_stale_weights():
    """w = 10, then w = 1, then w = 10 on one context and one input, and every window in turn in both directions"""
    from aruco3_amd import _lib

    frames = _Frames(_torch())
    ctx = _ctx()
    c = rcs.by_name("converging_w10_it30")
    frame = frames.get(c.grey, "L8", LAYOUTS[0])
    for w in (10, 1, 10) + rcs.WINDOWS + rcs.WINDOWS[::-1]:
        cfg = rcs.cfg(w)
        _set(ctx, cfg)
        _bit_equal(_run(ctx, frame, "L8", _lib.MEM_DEVICE, c.starts, None), refo.refine_corners(c.grey, c.starts, cfg), ("window", w))
    ctx.close()


def test_the_long_call_equals_the_oracle_and_calls_of_four():
    """4 * 1024 + 7 corners in one call: the grid-stride loop (the grid is capped at 1024 workgroups of four corners), a last workgroup
    with one idle wave, mixed windows in every workgroup.  Each corner equals the oracle and the same corner in a call of its own
    group of four"""
    from aruco3_amd import _lib

    frames = _Frames(_torch())
    ctx = _ctx()
    c = rcs.by_name("launch_long")
    assert len(c.starts) == 4 * 1024 + 7 > 4096
    frame = frames.get(c.grey, "L8", LAYOUTS[0])
    _set(ctx, c.cfg)
    got = _run(ctx, frame, "L8", _lib.MEM_DEVICE, c.starts, c.cell)
    _bit_equal(got, rcs.expected()[c.name], "long call")
    alone = np.concatenate([_run(ctx, frame, "L8", _lib.MEM_DEVICE, c.starts[k: k + 4], c.cell[k: k + 4]) for k in range(0, len(c.starts), 4)])
    _bit_equal(got, alone, "long call against calls of four")
    ctx.close()


@pytest.mark.parametrize("relative_win", [0.4, 0.0])
def test_batch_path_at_win_half_10(oracle, relative_win):
    """two config-1 frames through detect_batch with win_half 10: windows up to 10 from the quads' cell sizes, and 10 everywhere"""
    from aruco3_amd import ARDictionary, _lib, synth

    torch = _torch()
    frames, _ = synth.config_frames(1, 2)
    d = ARDictionary.new_from_named_dict("ARUCO_DEFAULT")
    cells = int(np.ceil(np.sqrt(d.num_bits))) + 2
    n, h, w, _ = frames.shape
    assert (w, h) == (640, 480)
    dev = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    args = (dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, n)
    plain = _lib.Context(_lib.default_config(), d.code_list, d.num_bits, d._tau)
    m0, p0 = plain.detect_batch(*args)
    ctx = _lib.Context(_lib.default_config(), d.code_list, d.num_bits, d._tau)
    cfg = rcs.cfg(10, relative_win)
    _set(ctx, cfg)
    m, p = ctx.detect_batch(*args)
    assert marker_tuples(m) == marker_tuples(m0) and p.tolist() == p0.tolist() and len(m) >= 6   # the markers are unchanged
    want, pos = [], 0
    for f in range(n):
        grey = oracle.to_luma8(np.ascontiguousarray(frames[f]))
        want.append(refo.refine_markers(grey, [x["corners"] for x in m[pos: pos + int(p[f])]], cells, cfg))
        pos += int(p[f])
    want = np.concatenate(want)
    got = ctx.refined_corners()
    _bit_equal(got.reshape(-1, 2), want.reshape(-1, 2), ("batch", relative_win))
    assert np.abs(want - np.rint(want)).max() > 0.05   # (the corners were refined)
    ctx.close()
    plain.close()
