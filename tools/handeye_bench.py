"""Hand-eye calibration cost (a3_calibrate_hand_eyes / k_handeye): end-to-end call time per shape on the MI355X against the CPU oracle
(tests/handeye_oracle.c, one thread).  Kernel times come from running this under
`rocprofv3 --kernel-trace --stats -- python tools/handeye_bench.py` (k_handeye's rows of the kernel trace, in launch order: the
warm-up and `--reps` calls of every shape).

    python tools/handeye_bench.py [--reps 3] [--shapes 1x12x24,1x25x140,1x256x140,16x12x24] [--fix]

A shape is problems x frames x points per frame (24: the inner corners of a 5 x 7 ChArUco board, 140: the marker corners of a 5 x 7
GridBoard).  One JSON line per shape: device ms per call (median), oracle ms, iterations, the worst error of X and Y against the truth
and the rms of the solve.  The frames are synthetic: board points projected through a known camera, mount and board placement by the
contract's own model, with 0.2 px of Gaussian noise.  --fix runs the same shapes with the true mount fixed (Y alone).  Accuracy on
rendered and detected frames is measured by tests/test_gpu_handeye.py, which prints it; DESIGN.md section 4.15 reports it."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from aruco3_amd import _lib  # noqa: E402
from tests import handeye_oracle as ho  # noqa: E402
from tests import handeye_util as hu  # noqa: E402

SHAPES = "1x12x24,1x25x140,1x256x140,16x12x24"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--fix", action="store_true")
    ap.add_argument("--no-oracle", action="store_true")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("handeye_bench needs the MI355X")
    ctx = _lib.Context(_lib.default_config(), np.zeros(1, np.uint64), 64, 1)
    if not args.no_oracle:
        ho.lib()                                        # (compiled on first use: not part of the first shape's oracle time)
    mounts = list(hu.MOUNTS)
    for shape in args.shapes.split(","):
        n_probs, n_frames, n_pts = (int(v) for v in shape.split("x"))
        ps = [hu.make_problem(F=n_frames, seed=k, kind="charuco" if n_pts == 24 else "grid", noise=0.2, mount=mounts[k % len(mounts)])
              for k in range(n_probs)]
        packed = hu.pack(ps, flags=_lib.HANDEYE_FIX_X if args.fix else 0, guess=[(p["X"], None) for p in ps])
        ctx.calibrate_hand_eyes(*packed)                # warm-up: code object load, scratch growth
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            res, fres = ctx.calibrate_hand_eyes(*packed)
            times.append((time.perf_counter() - t0) * 1e3)
        errs = [hu.errors(res, p, k) for k, p in enumerate(ps)]
        line = dict(problems=n_probs, frames=n_frames, points=n_pts, fix=bool(args.fix), device_ms=float(np.median(times)),
                    device_ms_all=[round(t, 3) for t in times], iterations=[int(r.iterations) for r in res][:4],
                    pairs=[int(r.pairs_used) for r in res][:4], status=sorted({int(r.status) for r in res}),
                    rotation_err_deg_max=max(e[0] for e in errs), translation_err_max=max(e[1] for e in errs), rms_px=float(res[0].rms_px))
        if not args.no_oracle:
            t0 = time.perf_counter()
            ora = ho.calibrate_hand_eyes(*packed)
            line["oracle_ms"] = (time.perf_counter() - t0) * 1e3
            line["bit_equal"] = all(bytes(a) == bytes(b) for a, b in zip(res, ora[0])) and all(bytes(a) == bytes(b) for a, b in zip(fres, ora[1]))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
