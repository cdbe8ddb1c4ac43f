"""Inverted markers (a3_set_marker_polarity, an extension beyond the reference): what mode A3_POLARITY_BOTH costs beside
A3_POLARITY_DARK on one GPU, and whether mode DARK moved against another build of the library.

BASELINE config 2 (256 frames of 1920x1080 rendered on the device), synchronous: one a3_detect_batch per step, on the frames as
rendered and on their complement (255 - frame), in modes DARK and BOTH:
  * frames/s: a host clock around `steps` calls (each ends in the library's wait for its read-back), profiling off, in alternating
    regions;
  * the decode stage's device time per batch through a3_get_profile (A3_PROFILE_STAGES), in regions of their own: the event records
    cost device time, so these regions give no frames/s;
  * markers found, and how many of them are flagged inverted.
Every measurement runs in a child process that loads one library: this build's, or with --parent-lib another build's (the parent
commit's libaruco3_hip.so; it has mode DARK only).  The children alternate, `rounds` times each; the spread of one library's
per-round medians is the run-to-run noise a difference between the libraries has to be read against.

    python tools/polarity_bench.py [--device 0] [--rounds 3] [--regions 4] [--steps 10] [--frames 256] [--parent-lib PATH]
                                   [--out profiles/polarity_bench.json]

Prints one JSON object (DESIGN.md section 4.22 quotes it)."""
import argparse
import json
import os
import subprocess
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def measure(device, regions, steps, frames):
    """one library (whichever A3_HIP_LIB names), in this process -> dict"""
    import torch

    from aruco3_amd import _lib, synth
    from aruco3_amd.dictionaries import ARDictionary

    spec, name = synth.config_spec(2)
    d = ARDictionary.new_from_named_dict(name)
    dev, _ = synth.render_frames_device(spec, d.code_list, d.num_bits, [synth.frame_seed(2, i) for i in range(frames)], device=device)
    inv = 255 - dev
    torch.cuda.synchronize(device)
    w, h = spec.width, spec.height
    inputs = {"as_rendered": dev, "complemented": inv}
    has_both = hasattr(_lib.load(), "a3_set_marker_polarity")
    modes = ("dark", "both") if has_both else ("dark",)
    cases = [(m, i) for m in modes for i in inputs]

    def args(t):
        return (t.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, frames)

    ctxs = {}
    for m in modes:
        c = _lib.Context(_lib.default_config(), d.code_list, d.num_bits, d._tau, device)
        if m == "both":
            c.set_marker_polarity(_lib.POLARITY_BOTH)
        ctxs[m] = c
    out = {"has_mode_both": has_both, "cases": {}}
    cap = frames * 64
    for m, i in cases:   # warm-up, and what is found
        for _ in range(2):
            mk, _ = ctxs[m].detect_batch(*args(inputs[i]), out_cap=cap)
        rec = {"markers": int(len(mk))}
        if m == "both":
            rec["inverted"] = int(ctxs[m].marker_flags().sum())
        out["cases"][f"{m}/{i}"] = rec
    # frames/s, profiling off
    times = {k: [] for k in cases}
    for r in range(regions):
        for k in (cases if r % 2 == 0 else cases[::-1]):
            a = args(inputs[k[1]])
            t0 = time.perf_counter()
            for _ in range(steps):
                ctxs[k[0]].detect_batch(*a, out_cap=cap)
            times[k].append((time.perf_counter() - t0) / steps)
    # the decode stage by device events
    stage = {k: [] for k in cases}
    for c in ctxs.values():
        c.set_profiling(1)
    for r in range(regions):
        for k in (cases if r % 2 == 0 else cases[::-1]):
            c, a = ctxs[k[0]], args(inputs[k[1]])
            c.detect_batch(*a, out_cap=cap)
            c.profile(_lib.STAGE_DECODE, reset=True)
            for _ in range(steps):
                c.detect_batch(*a, out_cap=cap)
            ms, n = c.profile(_lib.STAGE_DECODE, reset=True)
            stage[k].append(ms / max(n, 1))
    for m, i in cases:
        rec = out["cases"][f"{m}/{i}"]
        rec["frames_per_s"] = round(frames / float(np.median(times[(m, i)])), 1)
        rec["frames_per_s_regions"] = [round(frames / t, 1) for t in times[(m, i)]]
        rec["decode_stage_ms"] = round(float(np.median(stage[(m, i)])), 5)
        rec["decode_stage_ms_regions"] = [round(x, 5) for x in stage[(m, i)]]
    for c in ctxs.values():
        c.close()
    return out


def _child(lib, a):
    env = dict(os.environ)
    if lib:
        env["A3_HIP_LIB"] = str(lib)
    else:
        env.pop("A3_HIP_LIB", None)
    p = subprocess.run([sys.executable, str(Path(__file__).resolve()), "--child", "--device", str(a.device), "--regions", str(a.regions),
                        "--steps", str(a.steps), "--frames", str(a.frames)], env=env, stdout=subprocess.PIPE, text=True, stdin=subprocess.DEVNULL)
    if p.returncode != 0:
        raise RuntimeError(f"the measuring child for {lib or 'this build'} ended with status {p.returncode}")
    return json.loads(p.stdout.strip().splitlines()[-1])


def _summary(runs, key, field):
    v = [r["cases"][key][field] for r in runs if key in r["cases"]]
    return {"per_round": v, "median": round(float(np.median(v)), 5), "spread": round(float(max(v) - min(v)), 5)} if v else None


def main():
    ap = argparse.ArgumentParser(description="time marker polarity modes DARK and BOTH, and mode DARK against another build")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--regions", type=int, default=4)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--parent-lib", default="", help="another build's libaruco3_hip.so to measure mode DARK of, alternating with this one")
    ap.add_argument("--out", default="", help="also write the result to this JSON file")
    ap.add_argument("--child", action="store_true", help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.child:
        print(json.dumps(measure(a.device, a.regions, a.steps, a.frames)))
        return
    libs = {"this_build": ""}
    if a.parent_lib:
        libs["parent"] = a.parent_lib
    runs = {k: [] for k in libs}
    order = list(libs)
    for r in range(a.rounds):
        for k in (order if r % 2 == 0 else order[::-1]):
            runs[k].append(_child(libs[k], a))
    res = {"workload": f"BASELINE config 2, {a.frames} frames of 1920x1080 rendered on the device, synchronous a3_detect_batch",
           "rounds": a.rounds, "regions_per_round": a.regions, "steps_per_region": a.steps, "parent_measured": bool(a.parent_lib), "libraries": {}}
    for k in libs:
        keys = list(runs[k][0]["cases"])
        res["libraries"][k] = {key: {"markers": runs[k][0]["cases"][key]["markers"], "inverted": runs[k][0]["cases"][key].get("inverted"),
                                     "frames_per_s": _summary(runs[k], key, "frames_per_s"),
                                     "decode_stage_ms": _summary(runs[k], key, "decode_stage_ms")} for key in keys}
    if a.parent_lib:   # mode DARK of the two builds: the difference of the medians beside the larger of the two run-to-run spreads
        cmp = {}
        for key in ("dark/as_rendered", "dark/complemented"):
            for field in ("frames_per_s", "decode_stage_ms"):
                t, p = res["libraries"]["this_build"][key][field], res["libraries"]["parent"][key][field]
                margin = max(t["spread"], p["spread"])
                cmp[f"{key}:{field}"] = {"this_build": t["median"], "parent": p["median"], "difference": round(t["median"] - p["median"], 5),
                                         "run_to_run_spread": margin, "within_spread": bool(abs(t["median"] - p["median"]) <= margin)}
        res["dark_against_parent"] = cmp
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        Path(a.out).write_text(text + "\n")


if __name__ == "__main__":
    main()
