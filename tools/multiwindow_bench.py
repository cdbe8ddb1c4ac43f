"""Detection with several threshold windows (a3_set_threshold_windows, an extension beyond the reference): what it costs and what it
finds on one GPU.  Four parts, each a key of the one JSON object printed and written to profiles/multiwindow_bench.json (DESIGN.md
section 4.20 quotes it):

  end_to_end  BASELINE config 2 (1920 x 1080, 4 to 8 markers, batches of `--frames`, synchronous a3_detect_batch on device-resident
              frames) with the windows off, (7), (3, 7, 15) and (7, 15): frames/s.
  threshold   the threshold stage alone (a3_set_profiling(A3_PROFILE_THRESHOLD_ONLY), the library's own events) on the same frames for
              K = 1, 2, 3 windows.  The K launches read the frames K times: K x 3.125 B/px.  A kernel that read them once would move
              3 + K x 0.125 B/px; the measured K-launch time stands beside the time that bound would take at the rate the single launch
              reaches -- the case for a follow-up.
  kernels     k_merge_candidates against k_frame_candidates on the same batch: a child of this tool run under
              `rocprofv3 --kernel-trace --stats` alternates batches with the windows off and (3, 7, 15); the kernels' average times come
              from its stats table.
  found       markers found per window set against the renderer's truth, on config 1 and config 4 frames with added Gaussian blur and
              noise (the blur and noise are applied on the host; seeds fixed).

The variants of a part alternate region by region in one process; per variant: the median over the regions, every region's figure and
spread = (max - min) / median.

    python tools/multiwindow_bench.py [--part end_to_end|threshold|kernels|found|all] [--device 0] [--frames 64] [--regions 5] [--out PATH]"""
import argparse
import csv
import json
import shutil
import subprocess
import sys
import tempfile
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

MIN_REGION_S = 0.3
SETS = {"off": (), "w7": (7,), "w3_7_15": (3, 7, 15), "w7_15": (7, 15)}


def _time(fn, steps):
    t0 = time.perf_counter()
    for _ in range(steps):
        fn()
    return (time.perf_counter() - t0) / steps * 1e3


def _alternate(variants, regions, min_steps=3):
    """variants: name -> callable.  -> name -> {"ms": median, "ms_all": [...], "spread": ...}"""
    steps = {}
    for name, fn in variants.items():
        fn()   # warm-up: pools, plans
        fn()
        steps[name] = max(min_steps, int(MIN_REGION_S / max(_time(fn, 1) * 1e-3, 1e-6)) + 1)
    ms = {name: [] for name in variants}
    for _ in range(regions):
        for name, fn in variants.items():
            ms[name].append(_time(fn, steps[name]))
    out = {}
    for name, v in ms.items():
        med = float(np.median(v))
        out[name] = {"ms": med, "ms_all": [round(x, 4) for x in v], "spread": (max(v) - min(v)) / med, "steps_per_region": steps[name]}
    return out


def _config2(device, frames):
    import torch

    from aruco3_amd import ARDictionary, synth

    spec, name = synth.config_spec(2)
    d = ARDictionary.new_from_named_dict(name)
    dev, truths = synth.render_frames_device(spec, d.code_list, d.num_bits, [synth.frame_seed(2, i) for i in range(frames)], device=device)
    torch.cuda.synchronize()
    return spec, d, dev, truths


def _ctx_for(d, device, windows, cfg=None):
    from aruco3_amd import _lib

    ctx = _lib.Context(cfg or _lib.default_config(), d.code_list, d.num_bits, d._tau, device)
    if windows:
        ctx.set_threshold_windows(windows)
    return ctx


def end_to_end_bench(device, frames, regions):
    from aruco3_amd import _lib

    spec, d, dev, truths = _config2(device, frames)
    W, H = spec.width, spec.height
    ctxs = {name: _ctx_for(d, device, w) for name, w in SETS.items()}
    counts = {}

    def run(name):
        m, per = ctxs[name].detect_batch(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, frames, 64 * frames)
        counts[name] = int(len(m))

    res = _alternate({name: (lambda name=name: run(name)) for name in ctxs}, regions)
    for name, r in res.items():
        r["windows"] = list(SETS[name])
        r["frames_per_s"] = frames / (r["ms"] * 1e-3)
        r["markers"] = counts[name]
        r["candidates_pre"] = ctxs[name].stats()["candidates_pre"]
        r["candidates"] = ctxs[name].stats()["candidates"]
    for name, r in res.items():
        r["relative_to_off"] = r["frames_per_s"] / res["off"]["frames_per_s"]
    for c in ctxs.values():
        c.close()
    return {"config": 2, "frames": frames, "width": W, "height": H, "call": "detect_batch", "true_markers": sum(len(t) for t in truths), **res}


def threshold_bench(device, frames, regions):
    from aruco3_amd import _lib

    spec, d, dev, _ = _config2(device, frames)
    W, H = spec.width, spec.height
    sets = {"K1": (7,), "K2": (7, 15), "K3": (3, 7, 15)}
    ctxs = {name: _ctx_for(d, device, w) for name, w in sets.items()}
    ms = {name: [] for name in sets}
    for c in ctxs.values():
        c.set_profiling(_lib.PROFILE_THRESHOLD_ONLY)
    for region in range(regions + 1):
        for name, ctx in ctxs.items():
            ctx.profile(_lib.STAGE_THRESHOLD, reset=True)
            for _ in range(5):
                ctx.detect_batch(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, frames, 64 * frames)
            t, n = ctx.profile(_lib.STAGE_THRESHOLD, reset=True)
            if region:   # (the first region holds the warm-up)
                ms[name].append(t / max(n, 1))
    out = {"frames": frames, "width": W, "height": H, "fmt": "RGB8"}
    px = float(W) * H * frames
    for name, v in ms.items():
        K = len(sets[name])
        med = float(np.median(v))
        out[name] = {"windows": list(sets[name]), "ms": med, "ms_all": [round(x, 4) for x in v], "spread": (max(v) - min(v)) / med,
                     "bytes_per_px_moved": K * 3.125, "tb_per_s": K * 3.125 * px / (med * 1e-3) / 1e12,
                     "bytes_per_px_read_once": 3.0 + K * 0.125}
    rate = out["K1"]["tb_per_s"] * 1e12   # what the single launch reaches
    for name in sets:
        r = out[name]
        r["ms_read_once_bound"] = r["bytes_per_px_read_once"] * px / rate * 1e3
        r["ms_over_bound"] = r["ms"] / r["ms_read_once_bound"]
        r["ms_over_K1"] = r["ms"] / out["K1"]["ms"]
    for c in ctxs.values():
        c.close()
    return out


def kernels_child(device, frames):
    """what the trace is taken of: batches with the windows off and (3, 7, 15), alternating"""
    from aruco3_amd import _lib

    spec, d, dev, _ = _config2(device, frames)
    W, H = spec.width, spec.height
    ctxs = [_ctx_for(d, device, ()), _ctx_for(d, device, (3, 7, 15))]
    for _ in range(12):
        for ctx in ctxs:
            ctx.detect_batch(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, frames, 64 * frames)
    print(json.dumps({"candidates_pre": [c.stats()["candidates_pre"] for c in ctxs], "candidates": [c.stats()["candidates"] for c in ctxs]}))
    for c in ctxs:
        c.close()


def kernels_bench(device, frames):
    prof = shutil.which("rocprofv3")
    if not prof:
        return {"skipped": "rocprofv3 is not on the PATH"}
    with tempfile.TemporaryDirectory() as tmp:
        p = subprocess.run([prof, "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "mw", "--", sys.executable, str(Path(__file__).resolve()),
                            "--part", "kernels_child", "--device", str(device), "--frames", str(frames)], capture_output=True, text=True,
                           stdin=subprocess.DEVNULL, timeout=600)
        if p.returncode != 0:
            return {"failed": p.returncode, "stderr": p.stderr[-2000:]}
        tables = sorted(Path(tmp).rglob("*kernel_stats.csv"))
        if not tables:
            return {"failed": "no kernel stats table written", "stderr": p.stderr[-2000:]}
        rows = list(csv.DictReader(tables[0].open()))
    out = {"frames": frames, "windows": [3, 7, 15], "kernels": {}}
    for ln in p.stdout.splitlines():
        if ln.startswith("{"):
            out["lists"] = json.loads(ln)
    for r in rows:
        for k in ("k_merge_candidates", "k_frame_candidates", "k_decode", "k_compact_markers", "k_contour_quads"):
            if k in r["Name"]:
                out["kernels"].setdefault(k, []).append({"name": r["Name"][:80], "calls": int(r["Calls"]), "avg_us": float(r["AverageNs"]) / 1e3,
                                                         "min_us": float(r.get("MinNs", 0) or 0) / 1e3, "max_us": float(r.get("MaxNs", 0) or 0) / 1e3})
    return out


def _blur(frames, sigma):
    if not sigma:
        return frames
    r = int(np.ceil(3 * sigma))
    k = np.exp(-0.5 * (np.arange(-r, r + 1) / sigma) ** 2)
    k /= k.sum()
    a = frames.astype(np.float32)
    for axis in (1, 2):
        pad = [(0, 0)] * a.ndim
        pad[axis] = (r, r)
        p = np.pad(a, pad, mode="edge")
        a = sum(k[i] * np.take(p, range(i, i + frames.shape[axis]), axis=axis) for i in range(2 * r + 1))
    return a


def found_bench(device, frames):
    from aruco3_amd import ARDictionary, _lib, synth

    cases = (("config1_blur2.3_noise10", 1, 2.3, 10.0), ("config1_blur4.3", 1, 4.3, 0.0), ("config4_noise25", 4, 0.0, 25.0), ("config1_clean", 1, 0.0, 0.0))
    sets = ((3,), (7,), (11,), (15,), (23,), (3, 7, 15), (7, 15), (3, 7, 11, 15), (7, 11, 15))
    out = {}
    for name, config, sigma, noise in cases:
        rgb, truths = synth.config_frames(config, frames)
        d = ARDictionary.new_from_named_dict(synth.config_spec(config)[1])
        a = _blur(rgb, sigma).astype(np.float32)
        if noise:
            a = a + np.random.default_rng(20 + config).normal(0.0, noise, a.shape).astype(np.float32)
        a = np.ascontiguousarray(np.clip(np.rint(a), 0, 255).astype(np.uint8))
        n, h, w, _ = a.shape
        row = {"frames": n, "true_markers": sum(len(t) for t in truths)}
        for ws in sets:
            ctx = _ctx_for(d, device, ws)
            m, per = ctx.detect_batch(a.ctypes.data, _lib.MEM_HOST, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, n, 64 * n)
            found = false = 0
            pos = 0
            for f, t in enumerate(truths):
                ids = [int(x["id"]) for x in m[pos: pos + int(per[f])]]
                true_ids = [tm.id for tm in t]
                hit = sum(1 for i in set(true_ids) if i in ids)
                found += hit
                false += len(ids) - sum(1 for i in ids if i in true_ids)
                pos += int(per[f])
            row["r" + "_".join(str(v) for v in ws)] = {"found": found, "not_in_truth": false, "detected": int(len(m))}
            ctx.close()
        out[name] = row
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("end_to_end", "threshold", "kernels", "kernels_child", "found", "all"), default="all")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--found-frames", type=int, default=12)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "multiwindow_bench.json"))
    a = ap.parse_args()
    if a.part == "kernels_child":
        kernels_child(a.device, a.frames)
        return
    res = {}
    if a.part in ("kernels", "all"):   # (first: the child is started before this process opens the GPU)
        res["kernels"] = kernels_bench(a.device, a.frames)
    if a.part in ("end_to_end", "all"):
        res["end_to_end"] = end_to_end_bench(a.device, a.frames, a.regions)
    if a.part in ("threshold", "all"):
        res["threshold"] = threshold_bench(a.device, a.frames, a.regions)
    if a.part in ("found", "all"):
        res["found"] = found_bench(a.device, a.found_frames)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
