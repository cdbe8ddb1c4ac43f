"""a3_reduce_frames on the MI355X (k_reduce_frames): byte for byte against the numpy restatement of the contract
(tests/reduced_cases.reduce) on uniform-noise frames, every factor x every format, at sizes chosen against the kernel's own constants,
on aligned frames (the 16-byte loads) and on unaligned ones, into strided destinations whose padding keeps a sentinel, with host and
device memory on either side -- and every input error with its message."""
import functools
import re
from pathlib import Path

import numpy as np
import pytest

from tests import reduced_cases as rd

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
CSRC = ROOT / "aruco3_amd" / "csrc"
SENTINEL = 0xA5


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


def _constant(file, name):
    """a constexpr int of a kernel file: a number, or the name of another constant of k_threshold_k1.h / a3_common.h"""
    m = re.search(r"constexpr int %s = (\w+);" % name, (CSRC / file).read_text())
    assert m, (file, name)
    v = m.group(1)
    if v.isdigit():
        return int(v)
    return _constant("k_threshold_k1.h" if v.startswith("T_") else "a3_common.h", v)


K_RUN, K_TILE_H, K_CHUNK, K_WAVES3 = (_constant("k_reduce.hip", n) for n in ("kRun", "kTileH", "kChunk", "kWaves3"))
WAVE = _constant("a3_common.h", "WAVE")
WAVE_RUN = WAVE * K_RUN   # source pixels of a wave
N = K_CHUNK + 1           # one frame more than a frame chunk: the grid's z axis is 2


def _fmts():
    from aruco3_amd import _lib

    return {"L8": (_lib.FMT_L8, 1, "rgb"), "RGB8": (_lib.FMT_RGB8, 3, "rgb"), "RGBA8": (_lib.FMT_RGBA8, 4, "rgb"), "BGRA8": (_lib.FMT_BGRA8, 4, "bgr")}


def _sizes(f):
    """(reduced width, reduced height, trailing source columns, trailing source rows).  Widths: one wave's run of reduced pixels (for
    factor 3 the workgroup's, and the 341 / 342 where its first wave's source run ends inside a block), that +- 1 (= 3, 1 mod 4), 2 mod
    4, and 1, 2, 3; heights 1 and one workgroup's rows + 1; every remainder of the source size mod f"""
    run = WAVE_RUN // f if f != 3 else WAVE_RUN
    widths = [run, run - 1, run + 1, run // 2 + 2, 1, 2, 3, 6] + ([WAVE_RUN // 3, WAVE_RUN // 3 + 1] if f == 3 else [])
    assert {w % 4 for w in widths} == {0, 1, 2, 3}
    out = []
    for k, w in enumerate(widths):
        out.append((w, 1 if k % 4 == 1 else K_TILE_H + 1, k % f, (k // 2) % f))
    assert {s[2] for s in out} == set(range(f)) and {s[3] for s in out} == set(range(f)) and {s[1] for s in out} == {1, K_TILE_H + 1}
    return out


@functools.lru_cache(maxsize=None)
def _noise(n, h, w, c, seed):
    a = np.random.default_rng(seed).integers(0, 256, (n, h, w, c), dtype=np.uint8)
    a.setflags(write=False)
    return a


def _lay_out(frames, lead, row, frame):
    n, h, w, c = frames.shape
    assert row >= w * c and frame >= row * h
    buf = np.full(lead + frame * n, 0x5A, np.uint8)
    for k in range(n):
        v = buf[lead + k * frame: lead + k * frame + row * h].reshape(h, row)
        v[:, : w * c] = frames[k].reshape(h, w * c)
    return buf


def _run(ctx, frames, fmt, f, src_layout, src_dev, dst_dev, dst_lead, dst_pad):
    """one a3_reduce_frames call -> (the planes it wrote, the destination's padding bytes)"""
    from aruco3_amd import _lib

    torch = _torch()
    n, H, W, c = frames.shape
    w, h = W // f, H // f
    lead, row, frame = src_layout
    src = _lay_out(frames, lead, row, frame)
    d_row, d_frame = w + dst_pad, (w + dst_pad) * h + 3 * dst_pad
    dst = np.full(dst_lead + d_frame * n, SENTINEL, np.uint8)
    if src_dev:
        src_keep = torch.from_numpy(src).cuda()
        src_ptr = src_keep.data_ptr() + lead
    else:
        src_keep, src_ptr = src, src.ctypes.data + lead
    if dst_dev:
        dst_keep = torch.from_numpy(dst).cuda()
        dst_ptr = dst_keep.data_ptr() + dst_lead
    else:
        dst_keep, dst_ptr = dst, dst.ctypes.data + dst_lead
    torch.cuda.synchronize()
    ctx.reduce_frames(src_ptr, _lib.MEM_DEVICE if src_dev else _lib.MEM_HOST, fmt, W, H, row, frame, n, f, dst_ptr,
                      _lib.MEM_DEVICE if dst_dev else _lib.MEM_HOST, d_row, d_frame)
    out = dst_keep.cpu().numpy() if dst_dev else dst
    mask = np.ones(out.shape, bool)
    planes = np.empty((n, h, w), np.uint8)
    for k in range(n):
        o = dst_lead + k * d_frame
        v = out[o: o + d_row * h].reshape(h, d_row)
        planes[k] = v[:, :w]
        mask[o: o + d_row * h].reshape(h, d_row)[:, :w] = False
    return planes, out[mask]


def _ctx():
    from aruco3_amd import _lib

    _torch()
    assert hasattr(_lib.load(), "a3_reduce_frames"), "the library has no a3_reduce_frames"
    return _lib.Context(_lib.default_config(), np.zeros(1, np.uint64), 64, 1)


@pytest.mark.parametrize("fmt", ["L8", "RGB8", "RGBA8", "BGRA8"])
@pytest.mark.parametrize("f", rd.FACTORS)
def test_planes_equal_numpy(f, fmt):
    code, c, order = _fmts()[fmt]
    ctx = _ctx()
    memories = [(True, True), (False, True), (True, False), (False, False)]   # (src on the device, dst on the device)
    for k, (w, h, rem_x, rem_y) in enumerate(_sizes(f)):
        W, H = w * f + rem_x, h * f + rem_y
        frames = _noise(N, H, W, c, 100 * f + c)
        want = rd.reduce(frames, f, order)
        assert want.shape == (N, h, w)
        # 16-byte aligned base and strides (the vector loads), device to device
        row16 = (W * c + 15) // 16 * 16 + 16
        got, pad = _run(ctx, frames, code, f, (0, row16, row16 * H + 32), True, True, 0, 5)
        assert np.array_equal(got, want), (f, fmt, w, h, "aligned", int((got != want).sum()))
        assert np.all(pad == SENTINEL)
        # a base 1 byte off and a row stride that is no multiple of 16 (no vector load), the memory kinds in turn; the destination's
        # rows start at every alignment (w + 7 bytes apart, from an odd base)
        src_dev, dst_dev = memories[k % 4]
        got, pad = _run(ctx, frames, code, f, (1, W * c + 7, (W * c + 7) * H + 13), src_dev, dst_dev, 1 + k % 3, 7)
        assert np.array_equal(got, want), (f, fmt, w, h, "unaligned", src_dev, dst_dev, int((got != want).sum()))
        assert np.all(pad == SENTINEL)
    ctx.close()


@pytest.mark.parametrize("f", rd.FACTORS)
def test_saturated_and_packed(f):
    """white frames stay 255 (the rounding never carries out of a byte), and a tightly packed destination is written whole"""
    from aruco3_amd import _lib

    ctx = _ctx()
    W, H = 2 * WAVE_RUN + 5, 3 * f + 1
    frames = np.full((2, H, W, 3), 255, np.uint8)
    got, pad = _run(ctx, frames, _lib.FMT_RGB8, f, (0, W * 3, W * 3 * H), True, True, 0, 0)
    assert got.shape == (2, H // f, W // f) and np.all(got == 255) and pad.size == 0
    ctx.close()


def test_python_reduce_frames():
    """aruco3_amd.reduce_frames: numpy in, numpy out; a CUDA tensor in, a CUDA tensor out; bgra=True reads B, G, R, A"""
    import aruco3_amd

    torch = _torch()
    frames = _noise(2, 45, 77, 4, 9)
    for f in rd.FACTORS:
        for bgra in (False, True):
            want = rd.reduce(frames, f, "bgr" if bgra else "rgb")
            host = aruco3_amd.reduce_frames(frames, f, bgra=bgra)
            assert isinstance(host, np.ndarray) and np.array_equal(host, want)
            dev = aruco3_amd.reduce_frames(torch.from_numpy(frames.copy()).cuda(), f, bgra=bgra)
            assert isinstance(dev, torch.Tensor) and dev.is_cuda and np.array_equal(dev.cpu().numpy(), want)
    one = aruco3_amd.reduce_frames(frames[0, :, :, 0], 2)   # a single grey frame
    assert np.array_equal(one, rd.reduce(frames[:1, :, :, :1], 2))


def test_argument_errors():
    """every input error is A3_ERR_INVALID with its message; nothing is written"""
    from aruco3_amd import _lib

    torch = _torch()
    ctx = _ctx()
    W, H, n, f = 33, 17, 2, 2
    src = torch.zeros(W * 3 * H * n + 64, dtype=torch.uint8, device="cuda")
    dst = torch.full((4096,), SENTINEL, dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    D = _lib.MEM_DEVICE
    good = dict(src=src.data_ptr(), src_memory=D, fmt=_lib.FMT_RGB8, width=W, height=H, src_row=W * 3, src_frame=W * 3 * H, n=n, factor=f,
                dst=dst.data_ptr(), dst_memory=D, dst_row=W // f, dst_frame=(W // f) * (H // f))

    def call(**kw):
        a = dict(good, **kw)
        ctx.reduce_frames(a["src"], a["src_memory"], a["fmt"], a["width"], a["height"], a["src_row"], a["src_frame"], a["n"], a["factor"],
                          a["dst"], a["dst_memory"], a["dst_row"], a["dst_frame"])

    def refused(needle, **kw):
        with pytest.raises(_lib.A3Error) as e:
            call(**kw)
        assert e.value.code == _lib.ERR_INVALID and needle in str(e.value), str(e.value)

    refused("a3_reduce_frames: null argument", src=0)
    refused("a3_reduce_frames: null argument", dst=0)
    refused("a3_reduce_frames: n_frames must be in 1..65535", n=0)
    refused("a3_reduce_frames: n_frames must be in 1..65535", n=65536)
    refused("a3_reduce_frames: unknown pixel format", fmt=7)
    refused("a3_reduce_frames: memory must be A3_MEM_HOST or A3_MEM_DEVICE", src_memory=5)
    refused("a3_reduce_frames: memory must be A3_MEM_HOST or A3_MEM_DEVICE", dst_memory=5)
    for bad in (0, 1, 5):
        refused("a3_reduce_frames: factor must be 2, 3 or 4", factor=bad)
    refused("a3_reduce_frames: a reduced width or height of 0", width=1)
    refused("a3_reduce_frames: a reduced width or height of 0", height=0)
    refused("a3_reduce_frames: a reduced size above 65535 or of 2^30 pixels and more", width=2 * 65536, src_row=1 << 24, src_frame=1 << 40,
            dst_row=1 << 20, dst_frame=1 << 30, n=1)
    refused("a3_reduce_frames: row stride smaller than a row", src_row=W * 3 - 1)
    refused("a3_reduce_frames: row stride smaller than a row", dst_row=W // f - 1)
    refused("a3_reduce_frames: frame stride smaller than a frame", src_frame=W * 3 * H - 1)
    refused("a3_reduce_frames: frame stride smaller than a frame", dst_frame=(W // f) * (H // f) - 1)
    refused("a3_reduce_frames: src and dst overlap", dst=src.data_ptr() + 100)
    refused("a3_reduce_frames: src and dst overlap", dst=src.data_ptr())
    torch.cuda.synchronize()
    assert bool((dst == SENTINEL).all())
    call()   # (and the call every case above departs from goes through)
    torch.cuda.synchronize()
    assert bool((dst[: n * (W // f) * (H // f)] == 0).all()) and bool((dst[n * (W // f) * (H // f):] == SENTINEL).all())
    # not while a submitted batch is in flight
    ctx.submit(src.data_ptr(), D, _lib.FMT_RGB8, W, H, W * 3, W * 3 * H, n)
    refused("a3_reduce_frames: a submitted batch has not been collected")
    ctx.collect()
    call()
    ctx.close()
