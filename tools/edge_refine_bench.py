"""Edge-fit corner refinement (a3_refine_config.method A3_REFINE_EDGES, an extension beyond the reference): what it costs and what it
buys on one GPU, beside A3_REFINE_SUBPIX.

  * the refinement kernel alone, by device events (a3_debug_kernel_time, kernel 6: the kernel re-run on the marker list of the batch
    before it): k_refine_corners and k_refine_edges at win_half 5 and 10, per BASELINE config 2 batch (256 frames of 1920x1080
    rendered on the device) and per config 1 frame;
  * a 256-frame synchronous step (one a3_detect_batch per step) with refinement off / SUBPIX / EDGES, on three contexts in
    alternating regions of one process;
  * the corner error against the renderer's true corners and the share of corners left at their start, on the device, for config 2
    unreduced and detected at factors 2, 3 and 4 (a3_set_reduction), win_half 5 and 10, both methods.

    python tools/edge_refine_bench.py [--device 0] [--regions 6] [--steps 10] [--frames 256] [--out profiles/edge_refine_bench.json]

Prints one JSON object (DESIGN.md section 4.19 quotes it)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

PROBE_REFINE = 6


def _pct(a, q):
    return round(float(np.percentile(a, q)), 4)


def _corner_errors(markers, per, refined, truths, factor):
    """errors of the start and of the refined corners against the nearest true corner (matched within 3 px x factor), and the share of
    matched corners that sit at their start"""
    e_int, e_ref, stayed, pos = [], [], 0, 0
    for f in range(len(per)):
        cnt = int(per[f])
        if cnt and truths[f]:
            allt = np.concatenate([np.asarray(t.corners) for t in truths[f]])
            ic = markers["corners"][pos: pos + cnt].reshape(-1, 2).astype(np.float64)
            rc = refined[pos: pos + cnt].reshape(-1, 2).astype(np.float64)
            dist = np.linalg.norm(ic[:, None, :] - allt[None, :, :], axis=2)
            j = dist.argmin(axis=1)
            ok = dist[np.arange(len(ic)), j] <= 3.0 * factor
            e_int += list(dist[np.arange(len(ic)), j][ok])
            e_ref += list(np.linalg.norm(rc - allt[j], axis=1)[ok])
            stayed += int(np.all(rc == ic, axis=1)[ok].sum())
        pos += cnt
    return {"corners": len(e_ref), "start_median_px": _pct(e_int, 50), "median_px": _pct(e_ref, 50), "p90_px": _pct(e_ref, 90),
            "p99_px": _pct(e_ref, 99), "at_start_share": round(stayed / max(len(e_ref), 1), 4)}


def edge_refine_cost(device, regions=6, steps=10, frames=256):
    import torch

    from aruco3_amd import _lib, synth
    from aruco3_amd.dictionaries import ARDictionary

    spec, name = synth.config_spec(2)
    d = ARDictionary.new_from_named_dict(name)
    dev, truths = synth.render_frames_device(spec, d.code_list, d.num_bits, [synth.frame_seed(2, i) for i in range(frames)], device=device)
    torch.cuda.synchronize(device)
    w, h = spec.width, spec.height
    a = (dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, frames)
    methods = {"subpix": _lib.REFINE_SUBPIX, "edges": _lib.REFINE_EDGES}

    def cfg(method, win_half):
        return _lib.RefineConfig(methods[method], win_half, 0.4, 30, 0.01)

    def ctx_for(dic, refine=None, factor=None):
        c = _lib.Context(_lib.default_config(), dic.code_list, dic.num_bits, dic._tau, device)
        if refine is not None:
            c.set_corner_refinement(refine)
        if factor is not None:
            c.set_reduction(_lib.ReductionRec(factor))
        return c

    out = {"workload": f"BASELINE config 2, {frames} frames of 1920x1080 rendered on the device", "regions": regions, "steps_per_region": steps}

    # ---- the kernels alone, by device events ----
    kernel = {}
    f1, _ = synth.config_frames(1, 1)
    d1 = ARDictionary.new_from_named_dict("ARUCO_DEFAULT")
    a1 = (f1.ctypes.data, _lib.MEM_HOST, _lib.FMT_RGB8, 640, 480, 640 * 3, 640 * 480 * 3, 1)
    for label, dic, args, cap in (("config2_batch", d, a, frames * 64), ("config1_frame", d1, a1, 64)):
        for win_half in (5, 10):
            c = ctx_for(dic, cfg("edges", win_half))
            m, _ = c.detect_batch(*args, out_cap=cap)
            rec = {"markers": int(len(m))}
            for method, value in methods.items():
                try:
                    c.debug_kernel_time(PROBE_REFINE, value, reps=3)
                    rec[method + "_us"] = round(c.debug_kernel_time(PROBE_REFINE, value, reps=20) * 1e3, 2)
                except _lib.A3Error as e:   # (the probe takes single-chunk batches only)
                    if e.code != _lib.ERR_INVALID:
                        raise
                    rec[method + "_us"] = None
                    rec["probe_error"] = str(e)
            kernel[f"{label}_win_half_{win_half}"] = rec
            c.close()
    out["kernel_us_by_device_events"] = kernel

    # ---- a synchronous step: off / SUBPIX / EDGES in alternating regions ----
    modes = {"off": None, "subpix": _lib.default_refine_config(), "edges_win_half_5": cfg("edges", 5), "edges_win_half_10": cfg("edges", 10)}
    ctxs = {k: ctx_for(d, v) for k, v in modes.items()}
    times = {k: [] for k in modes}
    for k in modes:
        for _ in range(2):
            ctxs[k].detect_batch(*a, out_cap=frames * 64)
    order = list(modes)
    for r in range(regions):
        for k in (order if r % 2 == 0 else order[::-1]):
            t0 = time.perf_counter()
            for _ in range(steps):
                ctxs[k].detect_batch(*a, out_cap=frames * 64)
            times[k].append((time.perf_counter() - t0) * 1e3 / steps)
    med = {k: float(np.median(v)) for k, v in times.items()}
    out["step_ms"] = {k: {"median": round(med[k], 4), "regions": [round(x, 4) for x in times[k]],
                          "added_us": round((med[k] - med["off"]) * 1e3, 1), "added_frac": round((med[k] - med["off"]) / med["off"], 5)} for k in modes}
    for c in ctxs.values():
        c.close()

    # ---- corner error and the share of corners left at their start ----
    acc = {}
    for factor in (1, 2, 3, 4):
        for win_half in (5, 10):
            for method in methods:
                c = ctx_for(d, cfg(method, win_half), None if factor == 1 else factor)
                m, per = c.detect_batch(*a, out_cap=frames * 64)
                acc[f"factor_{factor}_win_half_{win_half}_{method}"] = dict(markers=int(len(m)), **_corner_errors(m, per, c.refined_corners(), truths, factor))
                c.close()
    out["corner_error"] = acc
    return out


def main():
    ap = argparse.ArgumentParser(description="time edge-fit corner refinement beside SUBPIX and measure its corner error")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--regions", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--out", default="", help="also write the result to this JSON file")
    args = ap.parse_args()
    res = edge_refine_cost(args.device, regions=args.regions, steps=args.steps, frames=args.frames)
    text = json.dumps(res, indent=1)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
