"""The threshold stage on packed 4:2:2 frames (A3_FMT_YUYV8, A3_FMT_UYVY8) against tests/threshold_util.py's numpy reference on the luma
plane, bit for bit: every radius class (1..7 the register-resident kernel, 8..26 and 27..31 the ring kernel with its two splits, 32..128
separable, beyond: brute force), the FAST form (16-byte aligned base and strides, W % 16 == 0) and the careful one (base off by 1, 2, 3
bytes, an odd row pad, frames with a gap), widths below one lane's 16 pixels, no multiple of 16 and across one wave's 992 output columns,
one and two rows.  The frames sit on the comparison's boundary (threshold_util.knife) and every run is repeated with every chroma byte
complemented.  GPU only."""
import functools

import numpy as np
import pytest

from tests import sampler_util as su
from tests import threshold_util as tu
from tests import yuv422_util as yu

pytestmark = pytest.mark.gpu

# radii of every launch path and on both sides of every edge between two: 7 | 8 (K1 | ring), 16 (two apron lanes), 18 | 19 is inside
# 16..26 (the ring's LDS part stays at 19 rows), 27 | 28 (ring_reg_rows: the last radius of 4:2:2 with two waves per SIMD | the first with
# one; 26 is RGB8's last), 31 | 32 (ring | separable), 128 | 129 (separable | brute force)
RADII = (1, 4, 7, 8, 16, 26, 27, 28, 31, 32, 128, 129)
# (h, w): below one lane's 16 pixels; no multiple of 16; across a wave's 992 columns (FAST: W % 16 == 0); one row; two rows
SHAPES = ((9, 6), (33, 40), (20, 1008), (1, 64), (2, 1010))
# name -> (offset of the first byte from a 16-byte aligned address, row pad, frame gap): pads that keep the strides multiples of 16 are
# added per shape ("aligned"); the others leave the row stride at 2 W + pad
LAYOUTS = {"aligned": (0, None, 0), "base+1": (1, 0, 0), "base+2": (2, 0, 0), "base+3": (3, 0, 0), "rows+5": (0, 5, 0), "frames+7": (0, 0, 7)}
CONTENTS = {"noise": tu.noise, "knife100": tu.knife(100), "knife253": tu.knife(253, 1)}   # three frames; the last is behind the gap


@functools.lru_cache(maxsize=None)
def _luma(h, w):
    g = np.stack([fn(np.random.default_rng([h, w, i]), h, w) for i, fn in enumerate(CONTENTS.values())])
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _want(h, w, radius):
    """the reference on the luma planes: computed once per shape and radius, shared by both formats and every layout, never written to"""
    t = tu.reference(_luma(h, w), radius)[0]
    t.setflags(write=False)
    return t


def _same(got, want, what):
    bad = np.argwhere(got != want)
    assert bad.size == 0, f"{what}: {len(bad)} px differ, first (y, x) {bad[:5].tolist()}"


@pytest.mark.parametrize("fmt", yu.FORMATS)
@pytest.mark.parametrize("radius", RADII)
def test_threshold_on_the_luma_byte(dicts, radius, fmt):
    import torch

    from aruco3_amd import _lib
    from aruco3_amd.aruco import Detector, DetectorConfig

    det = Detector(DetectorConfig(threshold_window=radius), dicts.new_from_named_dict("ARUCO"))
    ctx = det._context()
    for h, w in SHAPES:
        luma, want = _luma(h, w), _want(h, w, radius)
        n = len(luma)
        px = yu.interleave(luma, fmt, seed=h * w)
        for layout, (lead, pad, gap) in LAYOUTS.items():
            if pad is None:
                pad = (-2 * w) % 16
            for chroma, frames in (("drawn", px), ("complemented", yu.complement_chroma(px, fmt))):
                buf, rs, fs = su.lay(frames, lead, pad, gap, seed=lead + pad + gap)
                assert np.array_equal(yu.luma_of(su.laid(buf, lead, rs, fs, n, h, w, 2), fmt), luma)
                dev = torch.from_numpy(buf).cuda()
                assert dev.data_ptr() % 16 == 0
                if layout == "aligned":
                    assert rs % 16 == 0 and fs % 16 == 0
                for taps in (True, False):
                    ctx.set_debug_taps(taps)
                    ctx.detect_batch(dev.data_ptr() + lead, _lib.MEM_DEVICE, yu.fmt_value(_lib, fmt), w, h, rs, fs, n)
                    for f in range(n):
                        what = f"{fmt} r{radius} {h}x{w} {layout} chroma {chroma} taps {taps} frame {f}"
                        _same(ctx.download_grey(f, w, h, thresholded=True), want[f], what)
                        if taps or radius > 31:   # (the fused kernels write a grey plane for the debug taps only)
                            _same(ctx.download_grey(f, w, h), luma[f], what + " grey")
                del dev
        # from host memory too, packed: the staging copy is sized with two bytes per pixel
        host = np.ascontiguousarray(px)
        ctx.set_debug_taps(True)
        ctx.detect_batch(host.ctypes.data, _lib.MEM_HOST, yu.fmt_value(_lib, fmt), w, h, 0, 0, n)
        for f in range(n):
            _same(ctx.download_grey(f, w, h, thresholded=True), want[f], f"{fmt} r{radius} {h}x{w} host frame {f}")
            _same(ctx.download_grey(f, w, h), luma[f], f"{fmt} r{radius} {h}x{w} host frame {f} grey")
    ctx.set_debug_taps(False)


@pytest.mark.parametrize("fmt", yu.FORMATS)
def test_refusals(dicts, fmt):
    """an odd width has a message of its own; a row stride of 2 W - 1 is refused, 2 W accepted; 4 stays refused"""
    from aruco3_amd import _lib
    from aruco3_amd.aruco import Detector, DetectorConfig

    ctx = Detector(DetectorConfig(), dicts.new_from_named_dict("ARUCO"))._context()
    buf = np.zeros(64 * 64, np.uint8)
    v = yu.fmt_value(_lib, fmt)
    with pytest.raises(_lib.A3Error, match="4:2:2 frames have an even width") as e:
        ctx.detect_batch(buf.ctypes.data, _lib.MEM_HOST, v, 17, 8, 0, 0, 1)
    assert e.value.code == _lib.ERR_INVALID
    with pytest.raises(_lib.A3Error, match="row_stride smaller than a row"):
        ctx.detect_batch(buf.ctypes.data, _lib.MEM_HOST, v, 16, 8, 31, 0, 1)
    with pytest.raises(_lib.A3Error, match="frame_stride smaller than a frame"):
        ctx.detect_batch(buf.ctypes.data, _lib.MEM_HOST, v, 16, 8, 32, 32 * 8 - 1, 2)
    ctx.detect_batch(buf.ctypes.data, _lib.MEM_HOST, v, 16, 8, 32, 32 * 8, 2)
    with pytest.raises(_lib.A3Error, match="unknown pixel format"):
        ctx.detect_batch(buf.ctypes.data, _lib.MEM_HOST, 4, 16, 8, 0, 0, 1)
