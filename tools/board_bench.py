"""Board pose (a3_set_board, an extension beyond the reference): what it costs and what it buys on one GPU.  Renders a 5 x 7 grid
board (ARUCO dictionary, 35 markers) at 1080p tilted 15 .. 50 degrees on the device and times a synchronous a3_detect_batch_pose of
`--frames` frames with and without the board in alternating regions on two contexts of their own, and a one-frame call the same
way, plus the stand-alone a3_estimate_board_pose; then the median rotation / translation error of the board pose and of the best
single-marker IPPE pose of each frame against the renderer's truth, with integer and with refined corners.  The kernel's own time
comes from a trace: run it under `rocprofv3 --kernel-trace --stats -- python tools/board_bench.py` and read k_board_pose.

    python tools/board_bench.py [--device 0] [--frames 256] [--regions 6] [--steps 10] [--out board.json]

Prints one JSON object (DESIGN.md section 4.6 quotes it)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def board_bench(device=0, frames=256, regions=6, steps=10):
    import torch

    from aruco3_amd import _lib
    from aruco3_amd.board import GridBoard
    from aruco3_amd.dictionaries import ARDictionary
    from tests import board_util as bu   # (the board scenes and their detector configuration)

    d = ARDictionary.new_from_named_dict("ARUCO")
    board = GridBoard(5, 7, 30.0, 6.0, first_id=10)
    rng = np.random.default_rng(1)
    scenes = []
    for k in range(frames):
        R, t = bu.board_pose_facing(board, rng.uniform(15, 50), rng.uniform(0, 360), rng.uniform(-30, 30), rng.uniform(480, 560),
                                    (rng.uniform(-60, 60), rng.uniform(-30, 30)))
        scenes.append(bu.board_scene(board, R, t))
    dev = bu.render(scenes, d, device=device)
    torch.cuda.synchronize(device)
    W, H = bu.W1080, bu.H1080
    intr = _lib.Intrinsics(W, H, *bu.K1080)
    ctxs = {}
    for mode in ("off", "on"):
        ctxs[mode] = _lib.Context(bu.config(), d.code_list, d.num_bits, d._tau, device)
        if mode == "on":
            ctxs[mode].set_board(board.ids, board.corners)

    def step(mode, n):
        return ctxs[mode].detect_batch_pose(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, n, 30.0, intr)

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
    # stand-alone call (one frame's markers)
    m, p, _ = step("on", 1)
    ids, px = m["id"], m["corners"].reshape(-1, 4, 2).astype(np.float32)
    for _ in range(5):
        ctxs["on"].estimate_board_pose(ids, px, intrinsics=intr)
    t0 = time.perf_counter()
    for _ in range(50):
        ctxs["on"].estimate_board_pose(ids, px, intrinsics=intr)
    timing["standalone_us"] = (time.perf_counter() - t0) / 50 * 1e6
    # accuracy
    acc = {}
    for refine in (False, True):
        ctx = ctxs["on"]
        ctx.set_corner_refinement(_lib.default_refine_config() if refine else None)
        m, p, poses = step("on", frames)
        recs = ctx.board_poses()
        rb, tb, rs, ts, it, used = [], [], [], [], [], []
        pos = 0
        for f, sc in enumerate(scenes):
            if recs[f]["status"]:
                assert np.all(np.isfinite(recs[f]["rotation"])) and np.all(np.isfinite(recs[f]["translation"]))
                rb.append(bu.rotation_error_deg(recs[f]["rotation"].reshape(3, 3), sc.R))
                tb.append(float(np.linalg.norm(recs[f]["translation"] - sc.t) / np.linalg.norm(sc.t)))
                it.append(int(recs[f]["iterations"]))
                used.append(int(recs[f]["markers_used"]))
            best_r, best_t = [], []
            for i in range(pos, pos + int(p[f])):
                if m[i]["id"] not in board.ids:   # (a foreign read, if any)
                    continue
                slot = int(np.nonzero(board.ids == m[i]["id"])[0][0])
                c = board.corners[slot].mean(axis=0)
                Rm = poses[i, 0, 1:10].reshape(3, 3)
                if not np.all(np.isfinite(poses[i, 0])):   # (IPPE has no pose for some near-degenerate quads)
                    continue
                best_r.append(bu.rotation_error_deg(Rm, sc.R))
                best_t.append(float(np.linalg.norm(poses[i, 0, 10:13] - Rm @ np.array([c[0], c[1], 0.0]) - sc.t) / np.linalg.norm(sc.t)))
            pos += int(p[f])
            if best_r:
                rs.append((min(best_r), float(np.median(best_r))))
                ts.append((min(best_t), float(np.median(best_t))))
        ctx.set_corner_refinement(None)
        acc["refined" if refine else "integer"] = {
            "board_rot_deg_median": float(np.median(rb)), "board_trans_rel_median": float(np.median(tb)),
            "best_marker_rot_deg_median": float(np.median([r[0] for r in rs])), "typical_marker_rot_deg_median": float(np.median([r[1] for r in rs])),
            "best_marker_trans_rel_median": float(np.median([r[0] for r in ts])),
            "typical_marker_trans_rel_median": float(np.median([r[1] for r in ts])),
            "iterations_median": float(np.median(it)), "markers_used_median": float(np.median(used)), "frames_solved": len(rb)}
    return {"frames": frames, "timing": timing, "accuracy": acc}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--regions", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = board_bench(a.device, a.frames, a.regions, a.steps)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
