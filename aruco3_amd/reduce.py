"""The reduced grey plane on the device (a3_reduce_frames): frames of any format -> their luma, box-filtered over factor x factor blocks,
one byte per block.  It is the plane a `Detector(reduction=Reduction(factor))` detects on.

Not part of the reference: an extension whose arithmetic include/aruco3_hip.h fixes to the bit.  For a CUDA tensor the output stays on
the device."""
import threading

import numpy as np

from . import _lib
from .aruco import _as_frames, _pixel_format

_ctxs = {}   # one context per device
_ctx_lock = threading.Lock()


def reduction_rec(factor: int) -> "_lib.ReductionRec":
    """the a3_reduction of this factor: what a3_set_reduction takes, and whose factor a3_reduce_frames takes"""
    if int(factor) != factor or not 2 <= int(factor) <= 4:
        raise ValueError("factor must be 2, 3 or 4")
    r = _lib.ReductionRec()
    r.factor = int(factor)
    return r


def reduce_frames(frames, factor: int, bgra: bool = False, pixel_format=None):
    """frames: H x W, H x W x C or N x H x W x C uint8 (C 1, 3 or 4), a numpy array or a torch tensor; factor 2, 3 or 4; bgra: 4-channel
    frames are in the byte order B, G, R, A; pixel_format: as in `Detector.detect_batch` ("yuyv" / "uyvy": N x H x W x 2, "nv12" ...:
    N x 3H/2 x W; their luma is what is reduced).
    -> N x (H // factor) x (W // factor) uint8: a CUDA tensor for a CUDA tensor (no host copy), else a numpy array."""
    ptr, mem, fmt, w, h, row, frame, n, keep = _as_frames(frames, _pixel_format(pixel_format, bgra))
    f =reduction_rec(factor).factor
    ow, oh = w // f, h // f
    device = keep.device.index or 0 if mem == _lib.MEM_DEVICE else 0
    with _ctx_lock:
        ctx = _ctxs.get(device)
        if ctx is None:
            ctx = _ctxs[device] = _lib.Context(_lib.default_config(), np.zeros(1, np.uint64), 64, 1, device)
        if mem == _lib.MEM_DEVICE:
            import torch

            out = torch.empty((n, oh, ow), dtype=torch.uint8, device=keep.device)
            with torch.cuda.device(keep.device):
                torch.cuda.current_stream().synchronize()   # (the frames may still be in the making on torch's stream)
                ctx.reduce_frames(ptr, mem, fmt, w, h, row, frame, n, f, out.data_ptr(), _lib.MEM_DEVICE, ow, oh * ow)
            return out
        out = np.empty((n, oh, ow), dtype=np.uint8)
        ctx.reduce_frames(ptr, mem, fmt, w, h, row, frame, n, f, out.ctypes.data, _lib.MEM_HOST, ow, oh * ow)
        return out
