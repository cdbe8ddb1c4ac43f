"""Frame rectification (a3_rectify_frames, an extension beyond the reference): what it costs on one GPU.  Rectifies 256 x 1920 x 1080
frames of noise, L8 and RGB8, device to device, to a 1920 x 1080 view with fx = fy = 1400 every pixel of which sees the source:
through the WEBCAM lens of a camera with the view's own fx fy cx cy (--model rational), or through a cv::fisheye lens of a camera with
fx = fy = 1460 whose frame the view just fits into (--model fisheye).  Prints the bytes a call moves (frames in + frames out) and the
time per synchronous call.  The kernel's own time comes from a trace: run it under `rocprofv3 --kernel-trace --stats -- python
tools/rectify_bench.py` and read k_rectify<1, M> (L8) and k_rectify<3, M> (RGB8), M = 1 rational / 3 fisheye, one launch per call.
Parity with the CPU restatement is tests/test_gpu_rectify.py's and tests/test_gpu_fisheye.py's business.

    python tools/rectify_bench.py [--model rational|fisheye] [--device 0] [--frames 256] [--regions 3] [--steps 5] [--out rectify.json]

Prints one JSON object (DESIGN.md sections 4.12 and 4.13 quote it)."""
import argparse
import ctypes as C
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

WEBCAM = (-0.28, 0.09, 1e-3, -5e-4, 0.0, 0.0, 0.0, 0.0)
W, H = 1920, 1080
K = (1400.0, 1400.0, 960.0, 540.0)
# the fisheye camera: the `mild` set of tests/fisheye_oracle.py (k1 k2 k3 k4, in a3_distortion's slots) at K_FISHEYE, seen by the view K
FISHEYE = (-0.02, 0.005, 0.0, 0.0, -0.003, 0.0005, 0.0, 0.0)
K_FISHEYE = (1460.0, 1460.0, 960.0, 540.0)
HBM_PEAK_TBS = 8.0


def _time(fn, steps):
    fn()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    return (time.perf_counter() - t0) / steps * 1e3


def rectify_bench(device=0, frames=256, regions=3, steps=5, model="rational"):
    import torch

    from aruco3_amd import _lib

    ctx = _lib.Context(_lib.default_config(), np.zeros(1, np.uint64), 64, 1, device)
    if model == "fisheye":
        rec = _lib.default_rectify(_lib.Intrinsics(W, H, *K_FISHEYE), _lib.DistortionRec(_lib.DIST_FISHEYE, 20, *FISHEYE, 0.1))
        rec.dst = _lib.Intrinsics(W, H, *K)
    else:
        rec = _lib.default_rectify(_lib.Intrinsics(W, H, *K), _lib.DistortionRec(_lib.DIST_RATIONAL, 20, *WEBCAM, 0.1))
    work = {}
    for name, fmt, c in (("L8", _lib.FMT_L8, 1), ("RGB8", _lib.FMT_RGB8, 3)):
        src = torch.randint(0, 256, (frames, H, W, c), dtype=torch.uint8, device=f"cuda:{device}")
        dst = torch.empty_like(src)
        work[name] = (fmt, c, src, dst)
    torch.cuda.synchronize()
    ms = {name: [] for name in work}
    info = None
    for _ in range(regions):   # (the two workloads alternate, so that a drift of the machine shows in both)
        for name, (fmt, c, src, dst) in work.items():
            def call():
                return ctx.rectify_frames(src.data_ptr(), _lib.MEM_DEVICE, fmt, W * c, H * W * c, frames, rec, dst.data_ptr(), _lib.MEM_DEVICE,
                                          W * c, H * W * c)
            info = call()
            ms[name].append(_time(call, steps))
    res = {"model": model, "frames": frames, "width": W, "height": H, "tiles": int(info.tiles),
           "path_tiles": [int(v) for v in info.path_tiles]}
    for name, (fmt, c, src, dst) in work.items():
        moved = 2 * frames * H * W * c
        call_ms = float(np.median(ms[name]))
        res[name] = {"bytes_moved": moved, "call_ms": call_ms, "call_ms_all": [round(v, 4) for v in ms[name]],
                     "call_tb_per_s": moved / (call_ms * 1e-3) / 1e12, "call_share_of_hbm_peak": moved / (call_ms * 1e-3) / 1e12 / HBM_PEAK_TBS}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--model", choices=("rational", "fisheye"), default="rational")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = rectify_bench(a.device, a.frames, a.regions, a.steps, a.model)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
