"""3-D boards (a3_set_board3d, an extension beyond the reference): what the pose costs and what it buys on one GPU.

Cost: renders `--frames` 1080p frames of a cube (ARUCO dictionary, one marker per face, one to three faces towards the camera) on the
device and times a synchronous a3_detect_batch_pose of them with and without the cube set as the board, in alternating regions on two
contexts of their own; beside it the same for a flat board (a 3 x 1 grid) of which each frame shows as many markers as the cube frame
of the same index shows faces, with a3_set_board.  `added` is what the board costs a batch: k_board3d_pose (or k_board_pose) and the
read-back of its records.  The kernels' own times come from a trace: run the tool under `rocprofv3 --kernel-trace --stats -- python
tools/board3d_bench.py` and read k_board3d_pose and k_board_pose.

Accuracy: the median rotation / translation error of the cube's pose against the renderer's truth in the frames that show one, two
and three faces, beside the best single-marker IPPE pose of each frame (the better of the frame's markers, picked knowing the truth,
carried into the cube's frame), with the detector's integer corners and with refined corners.

    python tools/board3d_bench.py [--device 0] [--frames 256] [--regions 6] [--steps 10] [--out profiles/board3d_bench.json]

Prints one JSON object and writes it to --out (DESIGN.md section 4.21 and the README quote it)."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
if str(ROOT) not in sys.path:
    sys.path.insert(0, str(ROOT))


def cube_scenes(cube, frames, seed=1):
    """`frames` random cube poses, a third each showing one, two and three faces (every marker the scene draws faces the camera by
    tests/board3d_util.FACE_COS_LIMIT)"""
    from tests import board3d_util as b3

    rng = np.random.default_rng(seed)
    want = {1: frames - 2 * (frames // 3), 2: frames // 3, 3: frames // 3}
    out = []
    while len(out) < frames:
        R, t = b3.view_pose(rng.standard_normal(3), rng.uniform(-30, 30), rng.uniform(480, 560), (rng.uniform(-60, 60), rng.uniform(-30, 30)))
        v = len(b3.visible(cube, R, t))
        if v and want[v]:
            want[v] -= 1
            out.append(b3.board_scene(cube, R, t))
    return out


def board3d_bench(device=0, frames=256, regions=6, steps=10):
    import torch

    from aruco3_amd import _lib
    from aruco3_amd.board import GridBoard
    from aruco3_amd.dictionaries import ARDictionary
    from tests import board3d_util as b3   # (the cube scenes)
    from tests import board_util as bu     # (the planar scenes, the renderer and the detector configuration)

    d = ARDictionary.new_from_named_dict("ARUCO")
    cube = b3.cube()
    flat = GridBoard(3, 1, b3.CUBE_MARKER, 12.0, first_id=40)
    scenes = cube_scenes(cube, frames)
    rng = np.random.default_rng(2)
    flat_scenes = []
    for sc in scenes:
        R, t = bu.board_pose_facing(flat, rng.uniform(15, 50), rng.uniform(0, 360), rng.uniform(-30, 30), rng.uniform(480, 560),
                                    (rng.uniform(-60, 60), rng.uniform(-30, 30)))
        flat_scenes.append(bu.board_scene(flat, R, t, keep=range(len(sc.quads))))
    W, H = bu.W1080, bu.H1080
    intr = _lib.Intrinsics(W, H, *bu.K1080)
    devs = {"cube": bu.render(scenes, d, device=device), "flat": bu.render(flat_scenes, d, device=device)}
    torch.cuda.synchronize(device)
    ctxs = {}
    for mode in ("off", "cube", "flat"):
        ctxs[mode] = _lib.Context(bu.config(), d.code_list, d.num_bits, d._tau, device)
    ctxs["cube"].set_board3d(cube.ids, cube.corners)
    ctxs["flat"].set_board(flat.ids, flat.corners)

    def step(mode, what, n):
        return ctxs[mode].detect_batch_pose(devs[what].data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, W, H, W * 3, W * H * 3, n, b3.CUBE_MARKER, intr)

    timing = {}
    for what in ("cube", "flat"):
        for n in (frames, 1):
            t = {"off": [], what: []}
            for mode in t:
                for _ in range(3):
                    step(mode, what, n)
            for r in range(regions):
                for mode in (("off", what) if r % 2 == 0 else (what, "off")):
                    t0 = time.perf_counter()
                    for _ in range(steps):
                        step(mode, what, n)
                    t[mode].append((time.perf_counter() - t0) / steps * 1e6)
            off, on = float(np.median(t["off"])), float(np.median(t[what]))
            timing[f"{what}_{n}_frames_us"] = {"off": off, "on": on, "added": on - off}
    # the stand-alone call (one frame's markers: three faces)
    three = next(f for f, sc in enumerate(scenes) if len(sc.quads) == 3)
    px = b3.project(cube, scenes[three].R, scenes[three].t)[b3.visible(cube, scenes[three].R, scenes[three].t)].astype(np.float32)
    ids = np.array([mid for _, mid in scenes[three].quads], np.uint32)
    for _ in range(5):
        ctxs["cube"].estimate_board_pose(ids, px, intrinsics=intr)
    t0 = time.perf_counter()
    for _ in range(50):
        ctxs["cube"].estimate_board_pose(ids, px, intrinsics=intr)
    timing["standalone_us"] = (time.perf_counter() - t0) / 50 * 1e6
    # accuracy, by the number of faces drawn
    c = cube.corners.astype(np.float64)
    ex, ey = c[:, 1] - c[:, 0], c[:, 0] - c[:, 3]
    ex, ey = ex / np.linalg.norm(ex, axis=1, keepdims=True), ey / np.linalg.norm(ey, axis=1, keepdims=True)
    frame = np.stack([ex, ey, np.cross(ex, ey)], axis=2)   # (slot, 3, 3): marker -> cube
    centre = c.mean(axis=1)
    acc = {}
    ctx = ctxs["cube"]
    for refine in (False, True):
        ctx.set_corner_refinement(_lib.default_refine_config() if refine else None)
        m, p, poses = step("cube", "cube", frames)
        recs = ctx.board_poses()
        rows = {1: [], 2: [], 3: []}
        found_all = 0
        pos = 0
        for f, sc in enumerate(scenes):
            n = int(p[f])
            best_r, best_t = [], []
            for i in range(pos, pos + n):
                if m[i]["id"] not in cube.ids or not np.all(np.isfinite(poses[i, 0])):
                    continue
                slot = int(np.nonzero(cube.ids == m[i]["id"])[0][0])
                Rb = poses[i, 0, 1:10].reshape(3, 3).astype(np.float64) @ frame[slot].T
                best_r.append(bu.rotation_error_deg(Rb, sc.R))
                best_t.append(float(np.linalg.norm(poses[i, 0, 10:13] - Rb @ centre[slot] - sc.t) / np.linalg.norm(sc.t)))
            pos += n
            found_all += int(recs[f]["markers_used"]) == len(sc.quads)
            if recs[f]["status"] and best_r:
                rows[len(sc.quads)].append((bu.rotation_error_deg(recs[f]["rotation"].reshape(3, 3), sc.R),
                                            float(np.linalg.norm(recs[f]["translation"] - sc.t) / np.linalg.norm(sc.t)), min(best_r), min(best_t),
                                            int(recs[f]["iterations"]), int(recs[f]["markers_used"])))
        ctx.set_corner_refinement(None)
        by = {}
        for faces, r in rows.items():
            a = np.array(r, np.float64).reshape(-1, 6)
            by[f"{faces}_faces"] = {"frames_solved": int(a.shape[0]), "board_rot_deg_median": float(np.median(a[:, 0])),
                                    "board_trans_rel_median": float(np.median(a[:, 1])), "best_marker_rot_deg_median": float(np.median(a[:, 2])),
                                    "best_marker_trans_rel_median": float(np.median(a[:, 3])), "iterations_median": float(np.median(a[:, 4])),
                                    "markers_used_median": float(np.median(a[:, 5]))}
        by["frames_with_every_drawn_marker_used"] = found_all
        acc["refined" if refine else "integer"] = by
    return {"frames": frames, "cube": {"side": b3.CUBE_SIDE, "marker_length": b3.CUBE_MARKER, "face_cos_limit": b3.FACE_COS_LIMIT},
            "timing": timing, "accuracy": acc}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--device", type=int, default=0)
    ap.add_argument("--frames", type=int, default=256)
    ap.add_argument("--regions", type=int, default=6)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--out", default=str(ROOT / "profiles" / "board3d_bench.json"))
    a = ap.parse_args()
    res = board3d_bench(a.device, a.frames, a.regions, a.steps)
    line = json.dumps(res, indent=1)
    print(line)
    Path(a.out).write_text(line + "\n")


if __name__ == "__main__":
    main()
