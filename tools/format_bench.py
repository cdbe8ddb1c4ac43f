"""What a frame's pixel format costs the threshold stage and a whole detect call on one GPU: L8, YUYV8, UYVY8, RGB8 and RGBA8 in one run
on `--frames` x 1920 x 1080 device-resident frames of BASELINE config 2's scene (the same markers in every format: the RGB render, its
luma plane as L8, that plane interleaved with noise chroma as YUYV8 / UYVY8, and the render with a noise alpha byte as RGBA8).  One JSON
object is printed and written to profiles/format_bench.json (DESIGN.md section 4.18 quotes it); per format:

  threshold_ms   the threshold launch alone, timed by the library's own events (a3_set_profiling(A3_PROFILE_THRESHOLD_ONLY)): what must
                 move per pixel is bpp bytes in and 1/8 byte out, `bytes_moved`, and `tb_per_s` is that over the time
  detect_ms      a synchronous a3_detect_batch on the frames, `frames_per_s` = frames over it; `markers` found (the same in every format:
                 every format's grey levels are the render's luma)

The formats alternate region by region in one process; per figure: the median over the regions, every region's value and
spread = (max - min) / median.  The claim the run is there to check: YUYV8 and UYVY8 take no longer than RGB8 in the threshold stage
(2.125 B/px against 3.125 and no luma arithmetic); `yuv422_no_slower_than_rgb8` says whether it held.

    python tools/format_bench.py [--device 0] [--frames 256] [--regions 7] [--out profiles/format_bench.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

W, H = 1920, 1080
HBM_PEAK_TBS = 8.0
FORMATS = ("L8", "YUYV8", "UYVY8", "RGB8", "RGBA8")
BPP = {"L8": 1, "YUYV8": 2, "UYVY8": 2, "RGB8": 3, "RGBA8": 4}


def _frames(device, frames):
    """-> {format: CUDA tensor (N, H, W, C)} of one scene"""
    import torch

    from aruco3_amd import ARDictionary, synth

    spec, name = synth.config_spec(2)
    assert (spec.width, spec.height) == (W, H)
    d = ARDictionary.new_from_named_dict(name)
    distinct = min(frames, 32)   # (rendered once, repeated: the detector does not know)
    rgb, _ = synth.render_frames_device(spec, d.code_list, d.num_bits, [synth.frame_seed(2, i) for i in range(distinct)], device=device)
    rgb = rgb.repeat((frames + distinct - 1) // distinct, 1, 1, 1)[:frames].contiguous()
    p = rgb.to(torch.int64)
    luma = ((2126 * p[..., 0] + 7152 * p[..., 1] + 722 * p[..., 2]) // 10000).to(torch.uint8)
    del p
    g = torch.Generator(device=rgb.device).manual_seed(1)
    noise = lambda: torch.randint(0, 256, (frames, H, W), dtype=torch.uint8, device=rgb.device, generator=g)
    out = {"L8": luma[..., None].contiguous(), "YUYV8": torch.stack([luma, noise()], dim=-1), "UYVY8": torch.stack([noise(), luma], dim=-1),
           "RGB8": rgb, "RGBA8": torch.cat([rgb, noise()[..., None]], dim=-1)}
    torch.cuda.synchronize()
    return d, out


def _stat(v):
    med = float(np.median(v))
    return {"median": med, "all": [round(x, 4) for x in v], "spread": (max(v) - min(v)) / med}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--regions", type=int, default=7)
    ap.add_argument("--steps", type=int, default=5, help="calls per region and format")
    ap.add_argument("--out", default=str(ROOT / "profiles" / "format_bench.json"))
    a = ap.parse_args()

    import torch

    from aruco3_amd import _lib

    d, frames = _frames(a.device, a.frames)
    n = a.frames
    fmt_of = {"L8": _lib.FMT_L8, "YUYV8": _lib.FMT_YUYV8, "UYVY8": _lib.FMT_UYVY8, "RGB8": _lib.FMT_RGB8, "RGBA8": _lib.FMT_RGBA8}
    ctx = _lib.Context(_lib.default_config(), d.code_list, d.num_bits, d._tau, a.device)
    markers = {}

    def call(f):
        t = frames[f]
        m, per = ctx.detect_batch(t.data_ptr(), _lib.MEM_DEVICE, fmt_of[f], W, H, W * BPP[f], W * H * BPP[f], n, 64 * n)
        markers[f] = int(len(m))

    thr = {f: [] for f in FORMATS}
    det = {f: [] for f in FORMATS}
    for region in range(a.regions + 1):   # (the first region is the warm-up: pools, plans, the first batch of a shape runs twice)
        for f in FORMATS:
            ctx.set_profiling(_lib.PROFILE_THRESHOLD_ONLY)
            ctx.profile(_lib.STAGE_THRESHOLD, reset=True)
            for _ in range(a.steps):
                call(f)
            ms, cnt = ctx.profile(_lib.STAGE_THRESHOLD, reset=True)
            ctx.set_profiling(_lib.PROFILE_OFF)
            call(f)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.steps):
                call(f)
            dt = (time.perf_counter() - t0) / a.steps * 1e3
            if region:
                thr[f].append(ms / max(cnt, 1))
                det[f].append(dt)
    ctx.close()

    res = {"frames": n, "width": W, "height": H, "regions": a.regions, "steps_per_region": a.steps, "scene": "BASELINE config 2", "formats": {}}
    for f in FORMATS:
        t, e = _stat(thr[f]), _stat(det[f])
        moved = (BPP[f] + 0.125) * W * H * n
        res["formats"][f] = {"bytes_per_pixel_moved": BPP[f] + 0.125, "bytes_moved": moved, "threshold_ms": t,
                             "tb_per_s": moved / (t["median"] * 1e-3) / 1e12, "share_of_hbm_peak": moved / (t["median"] * 1e-3) / 1e12 / HBM_PEAK_TBS,
                             "detect_ms": e, "frames_per_s": n / (e["median"] * 1e-3), "markers": markers[f]}
    rgb8 = res["formats"]["RGB8"]["threshold_ms"]["median"]
    res["threshold_ms_relative_to_rgb8"] = {f: res["formats"][f]["threshold_ms"]["median"] / rgb8 for f in FORMATS}
    res["yuv422_no_slower_than_rgb8"] = all(res["formats"][f]["threshold_ms"]["median"] <= rgb8 for f in ("YUYV8", "UYVY8"))
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).parent.mkdir(parents=True, exist_ok=True)
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
