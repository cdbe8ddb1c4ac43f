"""Frame rectification (a3_rectify_frames, an extension beyond the reference): what it costs on one GPU.  Rectifies 256 x 1920 x 1080
frames of noise, L8 and RGB8, device to device, to a 1920 x 1080 view with fx = fy = 1400 every pixel of which sees the source:
through the WEBCAM lens of a camera with the view's own fx fy cx cy (--model rational), or through a cv::fisheye lens of a camera with
fx = fy = 1460 whose frame the view just fits into (--model fisheye).  Prints the bytes a call moves (frames in + frames out) and the
time per synchronous call.  The kernel's own time comes from a trace: run it under `rocprofv3 --kernel-trace --stats -- python
tools/rectify_bench.py` and read k_rectify<1, M> (L8) and k_rectify<3, M> (RGB8), M = 1 rational / 3 fisheye, one launch per call.
Parity with the CPU restatement is tests/test_gpu_rectify.py's and tests/test_gpu_fisheye.py's business.

    python tools/rectify_bench.py [--model rational|fisheye] [--device 0] [--frames 256] [--regions 3] [--steps 5] [--out rectify.json]

--detect times rectification INSIDE the detect call (a3_set_rectification) against the two calls it replaces: 256 frames of BASELINE
config 2 (1920 x 1080 RGB8, 4-8 markers each, rendered on the device) taken as the frames of the lens camera, device-resident and
host-resident (pageable memory).  "two_calls" is a3_rectify_frames into a buffer of the frames' memory kind followed by a3_detect_batch
on it; "one_call" is a3_detect_batch on the source frames of a context with the setting; both synchronous, on contexts of their own,
alternating region by region.  Per form and memory kind: the median over the regions of the mean time of a region's calls (`steps`
of them, or as many as fill 0.3 s), every region's figure, and spread = (max - min) / median of the regions.

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
MIN_REGION_S = 0.3   # --detect: the least a timed region lasts


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
    rec = _rec(model)
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


def _rec(model):
    from aruco3_amd import _lib

    if model == "fisheye":
        rec = _lib.default_rectify(_lib.Intrinsics(W, H, *K_FISHEYE), _lib.DistortionRec(_lib.DIST_FISHEYE, 20, *FISHEYE, 0.1))
        rec.dst = _lib.Intrinsics(W, H, *K)
        return rec
    return _lib.default_rectify(_lib.Intrinsics(W, H, *K), _lib.DistortionRec(_lib.DIST_RATIONAL, 20, *WEBCAM, 0.1))


def detect_bench(device=0, frames=256, regions=5, steps=3, model="rational"):
    """two calls (a3_rectify_frames, a3_detect_batch) against one (a3_detect_batch with a3_set_rectification)"""
    import torch

    from aruco3_amd import ARDictionary, _lib, synth

    spec, name = synth.config_spec(2)
    assert (spec.width, spec.height) == (W, H)
    d = ARDictionary.new_from_named_dict(name)
    dev, _ = synth.render_frames_device(spec, d.code_list, d.num_bits, [synth.frame_seed(2, i) for i in range(frames)], device=device)
    torch.cuda.synchronize()
    host = dev.cpu().numpy()
    rec = _rec(model)
    row, frame = W * 3, W * H * 3
    two = _lib.Context(_lib.default_config(), d.code_list, d.num_bits, d._tau, device)
    one = _lib.Context(_lib.default_config(), d.code_list, d.num_bits, d._tau, device)
    one.set_rectification(rec)
    flat_dev, flat_host = torch.empty_like(dev), np.empty_like(host)
    cap = 64 * frames
    forms = {}
    for kind, src, flat, mem in (("device", dev.data_ptr(), flat_dev.data_ptr(), _lib.MEM_DEVICE),
                                 ("host", host.ctypes.data, flat_host.ctypes.data, _lib.MEM_HOST)):
        def two_calls(src=src, flat=flat, mem=mem):
            two.rectify_frames(src, mem, _lib.FMT_RGB8, row, frame, frames, rec, flat, mem, row, frame)
            return two.detect_batch(flat, mem, _lib.FMT_RGB8, W, H, row, frame, frames, cap)

        def one_call(src=src, mem=mem):
            return one.detect_batch(src, mem, _lib.FMT_RGB8, W, H, row, frame, frames, cap)

        forms[kind] = {"two_calls": two_calls, "one_call": one_call}
    res = {"mode": "detect", "model": model, "frames": frames, "width": W, "height": H, "fmt": "RGB8", "regions": regions, "steps": steps}
    for kind, pair in forms.items():
        (ma, pa), (mb, pb) = pair["two_calls"](), pair["one_call"]()   # warm-up: pools, plans -- and the same markers from both forms
        same = bool(np.array_equal(pa, pb)) and len(ma) == len(mb) and all(
            np.array_equal(ma[f], mb[f]) for f in ("frame", "id", "code", "corners", "hamming_distance", "rotation"))
        # a region is at least `steps` calls and at least MIN_REGION_S of work: a window of a few milliseconds measures the clock
        n_steps = max(steps, int(MIN_REGION_S / (_time(pair["one_call"], 1) * 1e-3)) + 1)
        ms = {k: [] for k in pair}
        for _ in range(regions):
            for k, fn in pair.items():
                ms[k].append(_time(fn, n_steps))
        res[kind] = {"markers": int(len(ma)), "same_markers": same, "steps_per_region": n_steps}
        for k, v in ms.items():
            med = float(np.median(v))
            res[kind][k] = {"ms": med, "ms_all": [round(x, 3) for x in v], "spread": (max(v) - min(v)) / med}
        res[kind]["one_over_two"] = res[kind]["one_call"]["ms"] / res[kind]["two_calls"]["ms"]
    two.close()
    one.close()
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--regions", type=int, default=3)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--model", choices=("rational", "fisheye"), default="rational")
    ap.add_argument("--detect", action="store_true", help="time a3_rectify_frames + a3_detect_batch against a3_detect_batch with a3_set_rectification")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = (detect_bench if a.detect else rectify_bench)(a.device, a.frames, a.regions, a.steps, a.model)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
