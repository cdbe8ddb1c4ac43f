"""Sub-pixel corner refinement (a3_set_corner_refinement, an extension beyond the reference): what it costs and what it buys on
one GPU.  Times BASELINE config 2 (256 frames of 1920x1080 rendered on the device, one synchronous a3_detect_batch per step) with
refinement off and on in alternating regions on two contexts of their own, and a one-frame config 1 call from host memory the same
way, and measures the corner error of the refined and of the integer corners against the renderer's true corners.

    python tools/refine_bench.py [--device 0] [--regions 6] [--steps 10] [--out refine.json]

Prints one JSON object (DESIGN.md section 4.5 quotes it)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def refine_cost(device, regions=6, steps=10, frames=256):
    """Sub-pixel corner refinement (an extension beyond the reference): what it adds to a synchronous config 2 step (256 1080p frames
    rendered on the device, one a3_detect_batch per step) and to a one-frame config 1 call from host memory -- refinement off and on
    in alternating regions on two contexts of their own -- and the corner error of the refined and of the integer corners against the
    renderer's true corners."""
    import torch

    from aruco3_amd import _lib, synth
    from aruco3_amd.dictionaries import ARDictionary

    spec, name = synth.config_spec(2)
    d = ARDictionary.new_from_named_dict(name)
    dev, truths = synth.render_frames_device(spec, d.code_list, d.num_bits, [synth.frame_seed(2, i) for i in range(frames)], device=device)
    torch.cuda.synchronize(device)
    w, h = spec.width, spec.height
    ctxs = {}
    for mode in ("off", "on"):
        ctxs[mode] = _lib.Context(_lib.default_config(), d.code_list, d.num_bits, d._tau, device)
        if mode == "on":
            ctxs[mode].set_corner_refinement(_lib.default_refine_config())
    a = (dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, frames)
    times = {"off": [], "on": []}
    for mode in ("off", "on"):
        for _ in range(2):
            ctxs[mode].detect_batch(*a, out_cap=frames * 64)
    for r in range(regions):
        for mode in (("off", "on") if r % 2 == 0 else ("on", "off")):
            t0 = time.perf_counter()
            for _ in range(steps):
                res = ctxs[mode].detect_batch(*a, out_cap=frames * 64)
            times[mode].append((time.perf_counter() - t0) * 1e3 / steps)
    markers, per = res if mode == "on" else ctxs["on"].detect_batch(*a, out_cap=frames * 64)
    refined = ctxs["on"].refined_corners()
    e_int, e_ref, pos = [], [], 0
    for f in range(frames):
        allt = np.concatenate([np.asarray(t.corners) for t in truths[f]]) if truths[f] else np.zeros((0, 2))
        for i in range(pos, pos + int(per[f])):
            ic = np.asarray(markers[i]["corners"], np.float64).reshape(4, 2)
            for k in range(4):
                if not len(allt):
                    continue
                j = int(np.argmin(np.linalg.norm(allt - ic[k], axis=1)))
                if np.linalg.norm(allt[j] - ic[k]) <= 3.0:
                    e_int.append(float(np.linalg.norm(ic[k] - allt[j]))); e_ref.append(float(np.linalg.norm(refined[i, k] - allt[j])))
        pos += int(per[f])
    med = {m: float(np.median(v)) for m, v in times.items()}
    out = {"workload": f"BASELINE config 2, {frames} frames of 1920x1080 rendered on the device, one synchronous a3_detect_batch per step",
           "regions": regions, "steps_per_region": steps,
           "ms_per_step_off": round(med["off"], 4), "ms_per_step_on": round(med["on"], 4),
           "added_ms_per_step": round(med["on"] - med["off"], 4), "added_frac": round((med["on"] - med["off"]) / med["off"], 5),
           "region_ms_off": [round(x, 4) for x in times["off"]], "region_ms_on": [round(x, 4) for x in times["on"]],
           "markers": int(len(markers)),
           "corner_error_px": {"corners": len(e_ref), "matched_within_px": 3.0,
                               "integer_median": round(float(np.median(e_int)), 4), "integer_p99": round(float(np.percentile(e_int, 99)), 4),
                               "refined_median": round(float(np.median(e_ref)), 4), "refined_p99": round(float(np.percentile(e_ref, 99)), 4)}}
    for c in ctxs.values():
        c.close()
    # one config 1 frame per call from host memory (the caller_latency call) with and without refinement, alternating
    f1, _ = synth.config_frames(1, 1)
    d1 = ARDictionary.new_from_named_dict("ARUCO_DEFAULT")
    one = {m: _lib.Context(_lib.default_config(), d1.code_list, d1.num_bits, d1._tau, device) for m in ("off", "on")}
    one["on"].set_corner_refinement(_lib.default_refine_config())
    a1 = (f1.ctypes.data, _lib.MEM_HOST, _lib.FMT_RGB8, 640, 480, 640 * 3, 640 * 480 * 3, 1)
    lat = {"off": [], "on": []}
    for m in ("off", "on"):
        for _ in range(5):
            one[m].detect_batch(*a1, out_cap=64)
    for r in range(2 * regions):
        for m in (("off", "on") if r % 2 == 0 else ("on", "off")):
            for _ in range(25):
                t0 = time.perf_counter(); one[m].detect_batch(*a1, out_cap=64); lat[m].append((time.perf_counter() - t0) * 1e3)
    lm = {m: float(np.median(v)) for m, v in lat.items()}
    out["C1_one_frame_call"] = {"median_ms_off": round(lm["off"], 4), "median_ms_on": round(lm["on"], 4),
                                "added_us": round((lm["on"] - lm["off"]) * 1e3, 2), "calls_per_mode": len(lat["off"])}
    for c in one.values():
        c.close()
    return out


def main():
    ap = argparse.ArgumentParser(description="time sub-pixel corner refinement off / on and measure its corner error")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--regions", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--out", default="", help="also write the result to this JSON file")
    args = ap.parse_args()
    res = refine_cost(args.device, regions=args.regions, steps=args.steps, frames=args.frames)
    text = json.dumps(res)
    print(text)
    if args.out:
        Path(args.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
