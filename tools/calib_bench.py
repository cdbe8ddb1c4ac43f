"""Camera calibration cost and accuracy (a3_calibrate_cameras / k_calibrate): end-to-end call time per shape on the MI355X against the CPU
oracle (tests/calib_oracle.c, one thread), and the recovered camera on noisy synthetic views.  Kernel times come from running this
under `rocprofv3 --kernel-trace --stats -- python tools/calib_bench.py` (k_calibrate's row of the stats file).

    python tools/calib_bench.py [--reps 3] [--shapes 1x25x24,1x256x140,16x25x24] [--model rational|fisheye]

--model fisheye measures a3_calibrate_fisheye_cameras / k_calibrate_fisheye the same way, against tests/fisheye_calib_oracle.c, on
views of tests/fisheye_calib_util.py (board centres up to 72 degrees off the axis, the MILD lens).

One JSON line per shape: cameras, views per camera, points per view, device ms per call (median), oracle ms, iterations, and the
largest relative focal-length error and rms of the solve.  The views are synthetic: board points projected through a known camera by
the contract's own model, with 0.2 px of Gaussian noise.  Accuracy on rendered and detected frames (a GridBoard through a lens, a
ChArUco board through a pinhole camera) is measured by tests/test_gpu_calibration.py, which prints it; DESIGN.md section 4.9 reports it."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from aruco3_amd import _lib  # noqa: E402
from tests import calib_oracle as co  # noqa: E402
from tests import calib_util as cu  # noqa: E402
from tests import fisheye_calib_oracle as fco  # noqa: E402
from tests import fisheye_calib_util as fu  # noqa: E402

SHAPES = "1x25x24,1x25x140,1x256x24,1x256x140,1x1024x24,1x1024x140,16x25x24"


def build(n_cams, n_views, n_pts, seed=0, fisheye=False):
    kind = "charuco" if n_pts == 24 else "grid"
    if fisheye:
        ps = [fu.problem(kind, n_views, seed=seed + k, coeffs=fu.MILD, noise=0.2) for k in range(n_cams)]
    else:
        ps = [cu.problem(kind, n_views, seed=seed + k, coeffs=cu.WEBCAM5, noise=0.2) for k in range(n_cams)]
    obj = np.concatenate([p["obj"] for p in ps])
    img = np.concatenate([p["img"] for p in ps])
    offs = [0]
    for p in ps:
        offs += list(p["offsets"][1:] + offs[-1])
    cams = cu.cameras([dict(size=p["size"], first_view=n_views * k, n_views=n_views) for k, p in enumerate(ps)])
    return ps, cams, np.array(offs, np.uint32), obj, img


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--no-oracle", action="store_true")
    ap.add_argument("--model", choices=("rational", "fisheye"), default="rational")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("calib_bench needs the MI355X")
    ctx = _lib.Context(_lib.default_config(), np.zeros(1, np.uint64), 64, 1)
    fisheye = args.model == "fisheye"
    solve = ctx.calibrate_fisheye_cameras if fisheye else ctx.calibrate_cameras
    oracle, params = (fco, fu.params) if fisheye else (co, cu.params)
    for shape in args.shapes.split(","):
        n_cams, n_views, n_pts = (int(v) for v in shape.split("x"))
        ps, cams, offs, obj, img = build(n_cams, n_views, n_pts, fisheye=fisheye)
        solve(cams, offs, obj, img)                                     # warm-up: code object load, scratch growth
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            res, _ = solve(cams, offs, obj, img, with_views=False)
            times.append((time.perf_counter() - t0) * 1e3)
        line = dict(model=args.model, cameras=n_cams, views=n_views, points=n_pts, device_ms=float(np.median(times)), device_ms_all=[round(t, 3) for t in times],
                    iterations=[int(r.iterations) for r in res][:4], status=sorted({int(r.status) for r in res}))
        errs = [float(np.max(np.abs(params(r)[:2] - p["truth"][:2]) / p["truth"][:2])) for r, p in zip(res, ps)]
        line["focal_rel_err_max"] = max(errs)
        line["rms_px"] = float(res[0].rms_px)
        if not args.no_oracle:
            t0 = time.perf_counter()
            ores, _ = oracle.calibrate(cams, offs, obj, img)
            line["oracle_ms"] = (time.perf_counter() - t0) * 1e3
            line["bit_equal"] = all(bytes(a) == bytes(b) for a, b in zip(res, ores))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
