"""ChArUco boards (a3_set_charuco, an extension beyond the reference): what they cost and what they buy on one GPU.  Renders a 5 x 7
ChArUco board (ARUCO_DEFAULT, 17 markers, 24 chessboard corners) at 1080p tilted 15 .. 50 degrees on the device and times a
synchronous a3_detect_batch_pose of `--frames` frames (marker refinement on, intrinsics) with and without ChArUco in alternating
regions on two contexts of their own, and a one-frame call the same way, plus the stand-alone a3_interpolate_charuco; then the median
chessboard-corner error and the median rotation / translation error of the ChArUco pose and of the marker board pose against the
renderer's truth.  The kernels' own time comes from a trace: run it under `rocprofv3 --kernel-trace --stats -- python
tools/charuco_bench.py` and read k_charuco_interp, k_charuco_refine and k_charuco_pose.

    python tools/charuco_bench.py [--device 0] [--frames 256] [--regions 6] [--steps 10] [--out charuco.json]

Prints one JSON object (DESIGN.md section 4.8 quotes it)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def charuco_bench(device=0, frames=256, regions=6, steps=10):
    import torch

    from aruco3_amd import _lib
    from aruco3_amd.board import CharucoBoard
    from aruco3_amd.dictionaries import ARDictionary
    from tests import board_util as bu     # (the pose helpers and the 1080p camera)
    from tests import charuco_util as cu   # (the ChArUco scenes and their detector configuration)

    d = ARDictionary.new_from_named_dict("ARUCO_DEFAULT")
    board = CharucoBoard(5, 7, 40.0, 28.0, first_id=5)
    poses = cu.tilted_poses(board, frames, seed=1)
    scenes = [cu.Scene(board, R, t) for R, t in poses]
    dev = cu.render(scenes, d, device=device)
    torch.cuda.synchronize(device)
    W, H = bu.W1080, bu.H1080
    intr = _lib.Intrinsics(W, H, *bu.K1080)
    ctxs = {}
    for mode in ("off", "on"):
        c = _lib.Context(cu.config(), d.code_list, d.num_bits, d._tau, device)
        c.set_corner_refinement(_lib.default_refine_config())
        c.set_board(board.ids, board.corners)
        if mode == "on":
            c.set_charuco(board.chessboard_corners, board.adjacent_ids)
        ctxs[mode] = c

    def step(mode, n):
        return ctxs[mode].detect_batch_pose(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, n, 28.0, intr)

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
    ctx = ctxs["on"]
    ids, px = m["id"], ctx.refined_corners()
    args = (dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, ids, px)
    for _ in range(5):
        ctx.interpolate_charuco(*args)
    t0 = time.perf_counter()
    for _ in range(50):
        ctx.interpolate_charuco(*args)
    timing["standalone_us"] = (time.perf_counter() - t0) / 50 * 1e6
    # accuracy
    step("on", frames)
    cp, bp, recs = ctx.charuco_poses(), ctx.board_poses(), ctx.charuco_corners()
    err, ec, eb, tc, tb = [], [], [], [], []
    for f, sc in enumerate(scenes):
        r = recs[recs["frame"] == f]
        truth = cu.true_corners(board, sc.R, sc.t)[r["id"]]
        err.extend(np.hypot(r["x"] - truth[:, 0], r["y"] - truth[:, 1]).tolist())
        if cp[f]["status"]:
            ec.append(bu.rotation_error_deg(cp[f]["rotation"].reshape(3, 3), sc.R))
            tc.append(float(np.linalg.norm(cp[f]["translation"] - sc.t) / np.linalg.norm(sc.t)))
        if bp[f]["status"]:
            eb.append(bu.rotation_error_deg(bp[f]["rotation"].reshape(3, 3), sc.R))
            tb.append(float(np.linalg.norm(bp[f]["translation"] - sc.t) / np.linalg.norm(sc.t)))
    acc = {"corners": len(recs), "corner_err_px_median": float(np.median(err)), "corner_err_px_p95": float(np.percentile(err, 95)),
           "charuco_rot_deg_median": float(np.median(ec)), "board_rot_deg_median": float(np.median(eb)),
           "charuco_trans_rel_median": float(np.median(tc)), "board_trans_rel_median": float(np.median(tb)),
           "frames_solved": [len(ec), len(eb)]}
    return {"frames": frames, "timing": timing, "accuracy": acc}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--regions", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = charuco_bench(a.device, a.frames, a.regions, a.steps)
    line = json.dumps(res)
    print(line)
    if a.out:
        Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
