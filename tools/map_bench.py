"""Marker map cost (a3_build_marker_maps / k_map): end-to-end call time per shape on the MI355X against the CPU oracle
(tests/map_oracle.c, one thread).  Kernel times come from running this under
`rocprofv3 --kernel-trace --stats -- python tools/map_bench.py` (k_map's rows of the kernel trace, in launch order: the warm-up
and `--reps` calls of every shape).

    python tools/map_bench.py [--reps 3] [--shapes 1x8x25xmissing,1x32x200xmissing,1x128x63xwindow,16x8x25xmissing] [--fix]

A shape is maps x markers x frames x visibility pattern (tests/map_util.visibility: 'full', 'missing' drops a third of the
observations, 'window' shows four consecutive markers per frame).  One JSON line per shape: device ms per call (median), oracle ms,
iterations, the worst marker error against the truth and the rms of the solve.  The observations are synthetic: marker corners on the
three planes of a room corner projected through a known camera at known poses by the contract's own model, with 0.2 px of Gaussian
noise.  --fix runs the same shapes with the true map fixed (one camera pose per frame: localisation).  Accuracy on rendered and
detected frames is measured by tests/test_gpu_map.py, which prints it; DESIGN.md section 4.11 reports it."""
import argparse
import json
import sys
import time
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))

from aruco3_amd import _lib  # noqa: E402
from tests import map_oracle as mo  # noqa: E402
from tests import map_util as mu  # noqa: E402

SHAPES = "1x8x25xmissing,1x32x200xmissing,1x128x63xwindow,16x8x25xmissing"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--shapes", default=SHAPES)
    ap.add_argument("--fix", action="store_true")
    ap.add_argument("--no-oracle", action="store_true")
    args = ap.parse_args()
    import torch

    if not torch.cuda.is_available():
        sys.exit("map_bench needs the MI355X")
    ctx = _lib.Context(_lib.default_config(), np.zeros(1, np.uint64), 64, 1)
    if not args.no_oracle:
        mo.lib()                                        # (compiled on first use: not part of the first shape's oracle time)
    for shape in args.shapes.split(","):
        n_maps, n_markers, n_frames, pattern = shape.split("x")
        n_maps, n_markers, n_frames = int(n_maps), int(n_markers), int(n_frames)
        ps = [mu.make_map(n_markers, n_frames, seed=k, noise=0.2, pattern=pattern) for k in range(n_maps)]
        packed = mu.pack(ps, flags=_lib.MAP_FIX_MAP if args.fix else 0, guess=[p["Mw"] for p in ps])
        ctx.build_marker_maps(*packed)                  # warm-up: code object load, scratch growth
        times = []
        for _ in range(args.reps):
            t0 = time.perf_counter()
            res, mres, frames, ores = ctx.build_marker_maps(*packed)
            times.append((time.perf_counter() - t0) * 1e3)
        errs = [mu.marker_errors(mres, p["Mw"], m0=n_markers * k) for k, p in enumerate(ps)]
        line = dict(maps=n_maps, markers=n_markers, frames=n_frames, pattern=pattern, observations=len(packed[2]), fix=bool(args.fix),
                    device_ms=float(np.median(times)), device_ms_all=[round(t, 3) for t in times],
                    iterations=[int(r.iterations) for r in res][:4], status=sorted({int(r.status) for r in res}),
                    rotation_err_deg_max=max(e[0] for e in errs), translation_err_lengths_max=max(e[1] for e in errs), rms_px=float(res[0].rms_px))
        if not args.no_oracle:
            t0 = time.perf_counter()
            ora = mo.build_marker_maps(*packed)
            line["oracle_ms"] = (time.perf_counter() - t0) * 1e3
            line["bit_equal"] = all(bytes(a) == bytes(b) for a, b in zip(res, ora[0])) and all(bytes(a) == bytes(b) for a, b in zip(mres, ora[1]))
        print(json.dumps(line), flush=True)


if __name__ == "__main__":
    main()
