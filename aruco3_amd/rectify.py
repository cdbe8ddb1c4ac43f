"""Frame rectification on the device (a3_rectify_frames): whole frames seen through a calibrated lens -> the frames an ideal pinhole
camera would have seen, optionally rotated (the R of cv::initUndistortRectifyMap, for row-aligned frames of a calibrated rig).

Not part of the reference: an extension whose map and blend include/aruco3_hip.h fixes to the bit (OpenCV's rational model forwards,
bilinear interpolation of every byte).  The output keeps the input's format and, for a CUDA tensor, stays on the device: it feeds
`Detector.detect_batch*` as it is, with the plain intrinsics of the rectified view."""
import threading

import numpy as np

from . import _lib
from .aruco import _as_frames
from .pinhole import CameraIntrinsics

_ctxs = {}   # one context per device
_ctx_lock = threading.Lock()


def rectify_rec(intrinsics: CameraIntrinsics, new_intrinsics: CameraIntrinsics = None, rotation=None, fill: int = 0) -> "_lib.RectifyRec":
    """the a3_rectify of these arguments (rectify_frames states them): what a3_rectify_frames and a3_set_rectification take"""
    new = new_intrinsics if new_intrinsics is not None else intrinsics
    r = _lib.RectifyRec()
    r.src = intrinsics._c()
    if intrinsics.distortion is not None:
        r.distortion = intrinsics.distortion._c()
    r.dst = new._c()
    R = np.eye(3) if rotation is None else np.asarray(rotation, dtype=np.float64).reshape(3, 3)
    r.rotation = (_lib.C.c_float * 9)(*[float(v) for v in R.reshape(9)])
    if not 0 <= int(fill) <= 255:
        raise ValueError("fill must be in 0..255")
    r.fill = int(fill)
    return r


def rectify_frames(frames, intrinsics: CameraIntrinsics, new_intrinsics: CameraIntrinsics = None, rotation=None, fill: int = 0,
                   pixel_format=None):
    """frames: H x W, H x W x C or N x H x W x C uint8 (C 1, 3 or 4), a numpy array or a torch tensor, of `intrinsics`' size.
    intrinsics: the camera (its `distortion` may be None); new_intrinsics: the rectified view and the output size (default: the same
    focal lengths, principal point and size, no lens); rotation: 3 x 3, camera -> rectified view (default: the identity); fill: the
    value of every byte of a pixel that sees nothing; pixel_format: as in `Detector.detect_batch`.
    -> N x H' x W' x C uint8: a CUDA tensor for a CUDA tensor (no host copy), else a numpy array.  Packed 4:2:2 ("yuyv" / "uyvy") and
    planar ("nv12" ...) frames give their rectified LUMA view, C = 1: the plane a rectifying detector detects on."""
    ptr, mem, fmt, w, h, row, frame, n, keep = _as_frames(frames, pixel_format)
    if (w, h) != (int(intrinsics.image_width), int(intrinsics.image_height)):
        raise ValueError(f"frames are {w} x {h}, the intrinsics say {intrinsics.image_width} x {intrinsics.image_height}")
    new = new_intrinsics if new_intrinsics is not None else intrinsics
    r = rectify_rec(intrinsics, new_intrinsics, rotation, fill)
    c = 1 if fmt in (_lib.FMT_YUYV8, _lib.FMT_UYVY8) else row // w
    ow, oh = int(new.image_width), int(new.image_height)
    device = keep.device.index or 0 if mem == _lib.MEM_DEVICE else 0
    with _ctx_lock:
        ctx = _ctxs.get(device)
        if ctx is None:
            ctx = _ctxs[device] = _lib.Context(_lib.default_config(), np.zeros(1, np.uint64), 64, 1, device)
        if mem == _lib.MEM_DEVICE:
            import torch

            out = torch.empty((n, oh, ow, c), dtype=torch.uint8, device=keep.device)
            with torch.cuda.device(keep.device):
                torch.cuda.current_stream().synchronize()   # (the frames may still be in the making on torch's stream)
                ctx.rectify_frames(ptr, mem, fmt, row, frame, n, r, out.data_ptr(), _lib.MEM_DEVICE, ow * c, oh * ow * c)
            return out
        out = np.empty((n, oh, ow, c), dtype=np.uint8)
        ctx.rectify_frames(ptr, mem, fmt, row, frame, n, r, out.ctypes.data, _lib.MEM_HOST, ow * c, oh * ow * c)
        return out
