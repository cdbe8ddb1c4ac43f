"""Board-aided marker recovery (a3_set_board_recovery, an extension beyond the reference): what it costs and what it buys on one GPU.
Renders a 5 x 7 grid board (ARUCO dictionary, 35 markers) at 1080p tilted 15 .. 50 degrees on the device, every fifth marker drawn with
three or four of its cells flipped (the decoder refuses it: tau is 3), and times a synchronous a3_detect_batch of `--frames` frames with
and without recovery in alternating regions on two contexts of their own, and a one-frame call the same way, plus the stand-alone
a3_recover_markers on one frame's lists; then how many of the damaged markers come back, and how far the recovered corners lie from
the renderer's truth.  The kernels' own time comes from a trace: run it under
`rocprofv3 --kernel-trace --stats -- python tools/recover_bench.py` and read k_recover_frames and k_recover_merge.

    python tools/recover_bench.py [--device 0] [--frames 256] [--regions 6] [--steps 10] [--out recover.json]

Prints one JSON object (DESIGN.md section 4.16 quotes it)."""
import argparse
import json
import sys
import time
from pathlib import Path
from types import SimpleNamespace

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def recover_bench(device=0, frames=256, regions=6, steps=10):
    import torch

    from aruco3_amd import _lib
    from aruco3_amd.board import GridBoard
    from aruco3_amd.dictionaries import ARDictionary
    from tests import board_util as bu   # (the board scenes and their detector configuration)

    d = ARDictionary.new_from_named_dict("ARUCO")
    board = GridBoard(5, 7, 30.0, 6.0, first_id=10)
    rng = np.random.default_rng(1)
    drawn = d.code_list.copy()   # the codes the renderer paints: every fifth board marker damaged
    damaged = [int(i) for i in board.ids[::5]]
    for i in damaged:
        for b in rng.choice(d.num_bits, size=int(rng.integers(3, 5)), replace=False).tolist():
            drawn[i] ^= np.uint64(1 << b)
    scenes = []
    for k in range(frames):
        R, t = bu.board_pose_facing(board, rng.uniform(15, 50), rng.uniform(0, 360), rng.uniform(-30, 30), rng.uniform(480, 560),
                                    (rng.uniform(-60, 60), rng.uniform(-30, 30)))
        scenes.append(bu.board_scene(board, R, t))
    dev = bu.render(scenes, SimpleNamespace(code_list=drawn, num_bits=d.num_bits), device=device)
    torch.cuda.synchronize(device)
    W, H = bu.W1080, bu.H1080
    ctxs = {}
    for mode in ("off", "on"):
        ctxs[mode] = _lib.Context(bu.config(), d.code_list, d.num_bits, d._tau, device)
        ctxs[mode].set_board(board.ids, board.corners)
        if mode == "on":
            ctxs[mode].set_board_recovery(ctxs[mode].default_recover_config())

    def step(mode, n):
        return ctxs[mode].detect_batch(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, n)

    timing = {}
    for n in (frames, 1):
        t = {"off": [], "on": []}
        for mode in ("off", "on"):
            for _ in range(3):
                step(mode, n)
        for r in range(regions):
            for mode in (("off", "on") if r % 2 == 0 else ("on", "off")):
                t0 = time.perf_counter()
                for _ in range(steps):
                    step(mode, n)
                t[mode].append((time.perf_counter() - t0) / steps * 1e6)
        timing[f"{n}_frames_us"] = {m: float(np.median(v)) for m, v in t.items()}
        timing[f"{n}_frames_us"]["added"] = timing[f"{n}_frames_us"]["on"] - timing[f"{n}_frames_us"]["off"]
    # what it buys: the damaged markers that come back, and where
    m_off, p_off = step("off", frames)
    m_on, p_on = step("on", frames)
    rec = ctxs["on"].recovered_counts(frames)
    truth = {int(board.ids[s]): s for s in range(len(board))}
    err, wrong, pos = [], 0, 0
    for f, sc in enumerate(scenes):
        quads = {mid: q for q, mid in sc.quads}
        for i in range(pos + int(p_on[f]) - int(rec[f]), pos + int(p_on[f])):
            mid = int(m_on[i]["id"])
            if mid not in damaged or mid not in truth:
                wrong += 1
                continue
            err.append(float(np.abs(m_on[i]["corners"].reshape(4, 2) - quads[mid]).max()))
        pos += int(p_on[f])
    # stand-alone call on frame 0's lists (the taps give the rejected quads and their codes)
    ctx = ctxs["on"]
    ctx.set_board_recovery(None)
    ctx.set_debug_taps(True)
    m1, p1 = step("on", 1)
    cands = ctx.candidates(0)
    _, ok, codes, dec = ctx.homographies(0, with_patches=False)
    ctx.set_debug_taps(False)
    rejected = np.setdiff1d(np.arange(len(cands)), m1["candidate_index"])
    has = (ok.astype(bool) & (dec != 0)).astype(np.uint8)
    cfg = ctx.default_recover_config()
    args = (m1["id"], m1["corners"], cands[rejected], codes[rejected], has[rejected], cfg)
    for _ in range(5):
        alone = ctx.recover_markers(*args)
    t0 = time.perf_counter()
    for _ in range(50):
        ctx.recover_markers(*args)
    timing["standalone_us"] = (time.perf_counter() - t0) / 50 * 1e6
    return {"frames": frames, "timing": timing, "board_markers": len(board), "damaged_per_frame": len(damaged),
            "markers_per_frame_off": float(np.mean(p_off)), "markers_per_frame_on": float(np.mean(p_on)), "recovered_per_frame": float(np.mean(rec)), "recovered_frame0": int(rec[0]),
            "recovered_wrong": wrong, "recovered_corner_error_px_median": float(np.median(err)) if err else None,
            "recovered_corner_error_px_max": float(np.max(err)) if err else None, "standalone_frame0": {"rejected": int(len(rejected)),
                                                                                                    "recovered": int(len(alone))}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--regions", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = recover_bench(a.device, a.frames, a.regions, a.steps)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
