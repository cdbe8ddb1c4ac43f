"""Detection on reduced frames (a3_reduce_frames / a3_set_reduction, an extension beyond the reference): what it costs and what it
buys on one GPU.  Three parts, each a key of the one JSON object printed (DESIGN.md section 4.17 quotes it):

  kernel      k_reduce_frames alone on `--frames` x 3840 x 2160 RGB8 device frames of noise, per factor: the time of a synchronous
              device-to-device a3_reduce_frames call, the same minus the time of a call on one 8 x 8 frame (launch + wait, no work to
              speak of), the bytes the contract moves ((3 + 1/f^2) W H N) over that time and that rate as a share of the 8 TB/s peak;
              beside it the threshold stage on the same frames (a3_set_profiling(A3_PROFILE_THRESHOLD_ONLY)), 3.125 B/px.  The kernel's
              own time comes from a trace: `rocprofv3 --kernel-trace --stats -- python tools/reduce_bench.py --part kernel`.
  end_to_end  BASELINE config 5 (3840 x 2160, 16 markers, detect + pose, batches of `--frames`) at factor off, 2, 3, 4, and the
              reference's noise recipe (1920 x 1080 uniform noise, batches of 32, detect) at off and 2: frames/s of synchronous calls on
              device-resident frames.
  results     on config 5's frames, whose true corners are known: markers found per factor, and with corner refinement on the RMS
              distance of the refined corners from the truth; then a sweep over marker sizes (1920 x 1080, 8 markers per frame of one
              side length each) for the cell size, in full-size pixels, below which a factor starts to lose markers.

The variants of a part alternate region by region in one process; per variant: the median over the regions, every region's figure and
spread = (max - min) / median.

    python tools/reduce_bench.py [--part kernel|end_to_end|results|all] [--device 0] [--frames 64] [--regions 5] [--out reduce.json]"""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))

HBM_PEAK_TBS = 8.0
MIN_REGION_S = 0.3
FACTORS = (2, 3, 4)
SIZE_MM = 100.0


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


def kernel_bench(device, frames, regions):
    import torch

    from aruco3_amd import ARDictionary, _lib

    W, H = 3840, 2160
    d = ARDictionary.new_from_named_dict("ARUCO")
    ctx = _lib.Context(_lib.default_config(), d.code_list, d.num_bits, d._tau, device)
    src = torch.randint(0, 256, (frames, H, W, 3), dtype=torch.uint8, device=f"cuda:{device}")
    dst = torch.empty((frames, H // 2, W // 2), dtype=torch.uint8, device=f"cuda:{device}")
    tiny = torch.zeros((8, 8, 3), dtype=torch.uint8, device=f"cuda:{device}")
    torch.cuda.synchronize()
    D = _lib.MEM_DEVICE
    variants = {}
    for f in FACTORS:
        variants[f"factor_{f}"] = lambda f=f: ctx.reduce_frames(src.data_ptr(), D, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, frames, f, dst.data_ptr(), D,
                                                                W // f, (W // f) * (H // f))
    variants["empty_call"] = lambda: ctx.reduce_frames(tiny.data_ptr(), D, _lib.FMT_RGB8, 8, 8, 24, 192, 1, 2, dst.data_ptr(), D, 4, 16)
    res = {"frames": frames, "width": W, "height": H, "fmt": "RGB8", "regions": regions, **_alternate(variants, regions, 10)}
    empty = res["empty_call"]["ms"]
    for f in FACTORS:
        r = res[f"factor_{f}"]
        moved = (3.0 + 1.0 / (f * f)) * W * H * frames
        r["bytes_moved"] = moved
        r["ms_less_empty_call"] = r["ms"] - empty
        r["tb_per_s"] = moved / (r["ms_less_empty_call"] * 1e-3) / 1e12
        r["share_of_hbm_peak"] = r["tb_per_s"] / HBM_PEAK_TBS
    # the threshold stage on the same frames, timed by the library's own events
    ctx.set_profiling(_lib.PROFILE_THRESHOLD_ONLY)
    thr = []
    for _ in range(regions + 1):
        ctx.profile(_lib.STAGE_THRESHOLD, reset=True)
        for _ in range(3):
            ctx.detect_batch(src.data_ptr(), D, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, frames, 64 * frames)
        ms, n = ctx.profile(_lib.STAGE_THRESHOLD, reset=True)
        thr.append(ms / max(n, 1))
    thr = thr[1:]   # (the first region holds the warm-up)
    med = float(np.median(thr))
    moved = 3.125 * W * H * frames
    res["threshold_stage"] = {"ms": med, "ms_all": [round(x, 4) for x in thr], "spread": (max(thr) - min(thr)) / med, "bytes_moved": moved,
                              "tb_per_s": moved / (med * 1e-3) / 1e12, "share_of_hbm_peak": moved / (med * 1e-3) / 1e12 / HBM_PEAK_TBS}
    ctx.close()
    return res


def _config5(device, frames):
    import torch

    from aruco3_amd import ARDictionary, synth

    spec, name = synth.config_spec(5)
    d = ARDictionary.new_from_named_dict(name)
    dev, truths = synth.render_frames_device(spec, d.code_list, d.num_bits, [synth.frame_seed(5, i) for i in range(frames)], device=device)
    torch.cuda.synchronize()
    return spec, d, dev, truths


def _ctx_for(d, device, factor, refine=False, cfg=None):
    from aruco3_amd import _lib

    ctx = _lib.Context(cfg or _lib.default_config(), d.code_list, d.num_bits, d._tau, device)
    if factor:
        ctx.set_reduction(_lib.ReductionRec(factor))
    if refine:
        ctx.set_corner_refinement(_lib.default_refine_config())
    return ctx


def end_to_end_bench(device, frames, regions):
    import torch

    from aruco3_amd import ARDictionary, _lib

    D = _lib.MEM_DEVICE
    spec, d, dev, _ = _config5(device, frames)
    W, H = spec.width, spec.height
    ctxs = {f: _ctx_for(d, device, f) for f in (0,) + FACTORS}
    counts = {}

    def run5(f):
        m, per, _ = ctxs[f].detect_batch_pose(dev.data_ptr(), D, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, frames, SIZE_MM, None, 64 * frames)
        counts[f] = int(len(m))

    t5 = _alternate({("off" if f == 0 else f"factor_{f}"): (lambda f=f: run5(f)) for f in ctxs}, regions)
    for name, r in t5.items():
        r["frames_per_s"] = frames / (r["ms"] * 1e-3)
        r["markers"] = counts[0 if name == "off" else int(name[-1])]
    for name, r in t5.items():
        r["speedup"] = r["frames_per_s"] / t5["off"]["frames_per_s"]
    for c in ctxs.values():
        c.close()
    del dev
    # the reference's noise recipe
    NW, NH, NN = 1920, 1080, 32
    noise = torch.randint(0, 256, (NN, NH, NW, 3), dtype=torch.uint8, device=f"cuda:{device}")
    torch.cuda.synchronize()
    dn = ARDictionary.new_from_named_dict("ARUCO")
    nctx = {f: _ctx_for(dn, device, f) for f in (0, 2)}
    tn = _alternate({("off" if f == 0 else f"factor_{f}"): (lambda f=f: nctx[f].detect_batch(noise.data_ptr(), D, _lib.FMT_RGB8, NW, NH, NW * 3, NW * NH * 3, NN,
                                                                                          64 * NN)) for f in nctx}, regions)
    for name, r in tn.items():
        r["frames_per_s"] = NN / (r["ms"] * 1e-3)
    for name, r in tn.items():
        r["speedup"] = r["frames_per_s"] / tn["off"]["frames_per_s"]
    for c in nctx.values():
        c.close()
    return {"config5": {"frames": frames, "width": W, "height": H, "call": "detect_batch_pose", **t5},
            "noise_1080p": {"frames": NN, "width": NW, "height": NH, "call": "detect_batch", **tn}}


def _score(m, per, refined, truths):
    """-> (true markers found, squared distances of the found markers' corners -- integer and refined -- from the nearest corner of the
    true marker of that id whose centre is nearest: an id can occur twice in a frame)"""
    found, d_int, d_ref = 0, [], []
    pos = 0
    for k, truth in enumerate(truths):
        by_id = {}
        for j, t in enumerate(truth):
            by_id.setdefault(t.id, []).append((j, np.asarray(t.corners, np.float64)))
        seen = set()
        for i in range(pos, pos + int(per[k])):
            mid = int(m[i]["id"])
            c = m[i]["corners"].reshape(4, 2).astype(np.float64)
            cands = [(float(((q.mean(axis=0) - c.mean(axis=0)) ** 2).sum()), j, q) for j, q in by_id.get(mid, ())]
            if not cands:
                continue
            _, j, q = min(cands, key=lambda x: x[0])
            if j in seen:
                continue
            seen.add(j)
            d_int += [float(((q - p) ** 2).sum(axis=1).min()) for p in c]
            if refined is not None:
                d_ref += [float(((q - p) ** 2).sum(axis=1).min()) for p in refined[i].astype(np.float64)]
        found += len(seen)
        pos += int(per[k])
    return found, d_int, d_ref


def results_bench(device, frames):
    import torch

    from aruco3_amd import ARDictionary, _lib, synth

    D = _lib.MEM_DEVICE
    spec, d, dev, truths = _config5(device, frames)
    W, H = spec.width, spec.height
    total = sum(len(tr) for tr in truths)
    out = {"config5": {"frames": frames, "true_markers": total, "cell_px": [round(s / 7.0, 1) for s in spec.side]}}
    def stats(d2):
        e = np.sqrt(np.asarray(d2, np.float64))
        return {"rms_px": float(np.sqrt(np.mean(e ** 2))), "median_px": float(np.median(e)), "p90_px": float(np.percentile(e, 90)),
                "within_1px": float(np.mean(e <= 1.0))} if e.size else None

    for f in (0,) + FACTORS:
        ctx = _ctx_for(d, device, f, refine=True)
        m, per = ctx.detect_batch(dev.data_ptr(), D, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, frames, 64 * frames)
        found, d_int, d_ref = _score(m, per, ctx.refined_corners(), truths)
        wide = _lib.default_refine_config()   # the widest window the contract takes
        wide.win_half = 10
        ctx.set_corner_refinement(wide)
        m, per = ctx.detect_batch(dev.data_ptr(), D, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, frames, 64 * frames)
        _, _, d_wide = _score(m, per, ctx.refined_corners(), truths)
        out["config5"]["off" if f == 0 else f"factor_{f}"] = {"found": found, "detected": int(len(m)), "integer": stats(d_int),
                                                             "refined_default": stats(d_ref), "refined_win_half_10": stats(d_wide)}
        ctx.close()
    del dev
    # the size sweep: 16 frames of 8 markers of one side length, 1920 x 1080, ARUCO (7 cells across a marker)
    d = ARDictionary.new_from_named_dict("ARUCO")
    sweep = []
    n = 16
    for side in (168.0, 140.0, 112.0, 98.0, 84.0, 70.0, 56.0, 49.0, 42.0, 35.0, 28.0):
        sp = synth.SynthSpec(1920, 1080, n_markers=(8, 8), side=(side, side), min_center_sep=max(1.6 * side, 120.0))
        dev, truths = synth.render_frames_device(sp, d.code_list, d.num_bits, [synth.frame_seed(2, 1000 + i) for i in range(n)], device=device)
        torch.cuda.synchronize()
        row = {"side_px": side, "cell_px": side / 7.0, "true_markers": sum(len(tr) for tr in truths)}
        for f in (0,) + FACTORS:
            ctx = _ctx_for(d, device, f)
            m, per = ctx.detect_batch(dev.data_ptr(), D, _lib.FMT_RGB8, 1920, 1080, 1920 * 3, 1920 * 1080 * 3, n, 64 * n)
            row["off" if f == 0 else f"factor_{f}"] = _score(m, per, None, truths)[0]
            ctx.close()
        sweep.append(row)
    out["size_sweep"] = sweep
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--part", choices=("kernel", "end_to_end", "results", "all"), default="all")
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--regions", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {}
    if a.part in ("kernel", "all"):
        res["kernel"] = kernel_bench(a.device, a.frames, a.regions)
    if a.part in ("end_to_end", "all"):
        res["end_to_end"] = end_to_end_bench(a.device, a.frames, a.regions)
    if a.part in ("results", "all"):
        res["results"] = results_bench(a.device, a.frames)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
