"""Lens distortion (a3_set_distortion, an extension beyond the reference): what it costs on one GPU.  Times a synchronous
a3_detect_batch_pose of the BASELINE config-2 batch (256 x 1080p, with intrinsics) with and without distortion in alternating regions
on two contexts of their own, a one-frame call the same way, and the stand-alone a3_undistort_points of 10^5 points.  The kernel's own
time comes from a trace: run it under `rocprofv3 --kernel-trace --stats -- python tools/lens_bench.py` and read k_undistort_corners
(one launch per pose batch with distortion).  Accuracy is measured by tests/test_gpu_distortion.py::test_accuracy_through_a_lens.

    python tools/lens_bench.py [--model rational|fisheye] [--device 0] [--regions 6] [--steps 10] [--out lens.json]

Prints one JSON object (DESIGN.md section 4.7 quotes it)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

WEBCAM = (-0.28, 0.09, 1e-3, -5e-4, 0.0, 0.0, 0.0, 0.0)
FISHEYE = (-0.02, 0.005, 0.0, 0.0, -0.003, 0.0005, 0.0, 0.0)   # cv::fisheye's k1 k2 k3 k4 in a3_distortion's slots (--model fisheye)


def _time(fn, steps):
    fn()
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    return (time.perf_counter() - t0) / steps * 1e3


def lens_bench(device=0, regions=6, steps=10, model="rational"):
    import torch

    from aruco3_amd import _lib, synth
    from aruco3_amd.dictionaries import ARDictionary

    spec, name = synth.config_spec(2)
    d = ARDictionary.new_from_named_dict(name)
    dev, _ = synth.render_frames_device(spec, d.code_list, d.num_bits, [synth.frame_seed(2, i) for i in range(256)], device=device)
    torch.cuda.synchronize()
    w, h = spec.width, spec.height
    intr = _lib.Intrinsics(w, h, 1400.0, 1400.0, w / 2, h / 2)
    dist = _lib.DistortionRec(_lib.DIST_RATIONAL, 20, *WEBCAM, 0.1)
    if model == "fisheye":
        dist = _lib.DistortionRec(_lib.DIST_FISHEYE, 20, *FISHEYE, 0.1)
    ctxs = {}
    for on in (False, True):
        c = _lib.Context(_lib.default_config(), d.code_list, d.num_bits, d._tau, device)
        if on:
            c.set_distortion(dist)
        ctxs[on] = c
    args = lambda n: (dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, n, 100.0, intr)
    out = {"batch_ms": {False: [], True: []}, "frame_ms": {False: [], True: []}}
    for _ in range(regions):
        for on in (False, True):
            out["batch_ms"][on].append(_time(lambda: ctxs[on].detect_batch_pose(*args(256), out_cap=256 * 64), steps))
            out["frame_ms"][on].append(_time(lambda: ctxs[on].detect_batch_pose(*args(1)), steps * 10))
    markers = ctxs[True].stats()["markers"]
    pts = np.random.default_rng(0).uniform([0, 0], [w, h], size=(100000, 2)).astype(np.float32)
    stand_ms = _time(lambda: ctxs[True].undistort_points(pts, intr, dist), steps)
    med = lambda v: float(np.median(v))
    res = {
        "model": model, "config": 2, "frames": 256, "markers_per_batch": int(markers),
        "batch_ms_off": med(out["batch_ms"][False]), "batch_ms_on": med(out["batch_ms"][True]),
        "frame_ms_off": med(out["frame_ms"][False]), "frame_ms_on": med(out["frame_ms"][True]),
        "undistort_points_1e5_ms": stand_ms,
    }
    res["batch_added_ms"] = res["batch_ms_on"] - res["batch_ms_off"]
    res["frame_added_us"] = (res["frame_ms_on"] - res["frame_ms_off"]) * 1e3
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--regions", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--model", choices=("rational", "fisheye"), default="rational")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = lens_bench(a.device, a.regions, a.steps, a.model)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
