"""Packed 4:2:2 test buffers in numpy: a luma plane interleaved with chroma bytes drawn as independent uniform noise (YUYV: Y0 U Y1 V,
UYVY: U Y0 V Y1), the same buffer with every chroma byte complemented, and planar luma-first buffers (NV12 / I420: H rows of luma, then
H / 2 rows of chroma noise).  A result may depend on the luma bytes only, so every test runs a frame twice -- as drawn and with the
chroma complemented -- and a kernel that reads the wrong byte of a pair fails even where luma and chroma happen to agree."""
import numpy as np

FORMATS = ("YUYV8", "UYVY8")
LUMA_OFFSET = {"YUYV8": 0, "UYVY8": 1}
PIXEL_FORMAT = {"YUYV8": "yuyv", "UYVY8": "uyvy"}


def fmt_value(lib, name):
    return {"YUYV8": lib.FMT_YUYV8, "UYVY8": lib.FMT_UYVY8}[name]


def interleave(luma, fmt, seed=0):
    """luma [..., h, w] uint8 -> [..., h, w, 2]: the luma byte at LUMA_OFFSET, noise in the chroma byte"""
    luma = np.asarray(luma, dtype=np.uint8)
    out = np.random.default_rng(2000 + seed).integers(0, 256, luma.shape + (2,), dtype=np.uint8)
    out[..., LUMA_OFFSET[fmt]] = luma
    return out


def complement_chroma(px, fmt):
    """a copy with every chroma byte complemented (the luma bytes as they are)"""
    out = px.copy()
    c = 1 - LUMA_OFFSET[fmt]
    out[..., c] = ~out[..., c]
    return out


def luma_of(px, fmt):
    return np.ascontiguousarray(px[..., LUMA_OFFSET[fmt]])


def planar(luma, seed=0):
    """luma [n, h, w] (h, w even) -> [n, 3h/2, w]: the luma rows followed by h / 2 rows of chroma noise (NV12's interleaved plane or
    I420's two quarter planes: the same bytes as far as the detector is concerned -- it never reads them)"""
    luma = np.asarray(luma, dtype=np.uint8)
    n, h, w = luma.shape
    assert h % 2 == 0 and w % 2 == 0
    out = np.random.default_rng(3000 + seed).integers(0, 256, (n, h * 3 // 2, w), dtype=np.uint8)
    out[:, :h] = luma
    return out
