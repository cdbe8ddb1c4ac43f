"""Sub-pixel corner refinement on its CPU restatement (tests/refine_oracle.c, an extension beyond the reference): accuracy against the
synthetic renderer's true corners, the degenerate cases of the contract, and the layout of a3_refine_config in C, ctypes and Rust.

Accuracy thresholds are the oracle's measured numbers with a margin.  They sit above the 0.08 px first guessed for clean frames:
the renderer's box-filtered edges are one pixel wide, and the gradient-weighted (cornerSubPix) estimate of such an edge is pulled
toward the pixel grid (an analytic, 16x supersampled square corner 0.3 px off the grid comes out 0.15-0.25 px off as well), so the
median error of clean frames is 0.17-0.20 px.  The integer corners' own error is reported beside it and must be worse."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import refine_cases as rcs
from tests import refine_oracle as refo

ROOT = Path(__file__).resolve().parent.parent


def _cells(d):
    return int(np.ceil(np.sqrt(d.num_bits))) + 2


def _errors(oracle, config, n_frames, start):
    from aruco3_amd import ARDictionary, synth

    frames, truths = synth.config_frames(config, n_frames)
    _, name = synth.config_spec(config)
    d = ARDictionary.new_from_named_dict(name)
    cells = _cells(d)
    e_int, e_ref = [], []
    rng = np.random.default_rng(7 + config)
    for f in range(n_frames):
        res = oracle.detect(frames[f], d.code_list, d.num_bits, d._tau)
        grey = res["grey"]
        if start == "detection":
            quads = [m["corners"] for m in res["markers"]]
            ref = refo.refine_markers(grey, quads, cells)
            for q, r in zip(quads, ref):
                ic = np.asarray(q, dtype=np.float64).reshape(4, 2)
                allt = np.concatenate([np.asarray(t.corners) for t in truths[f]])
                for k in range(4):
                    j = int(np.argmin(np.linalg.norm(allt - ic[k], axis=1)))
                    if np.linalg.norm(allt[j] - ic[k]) > 3.0:
                        continue   # (a corner that belongs to no true marker corner)
                    e_int.append(np.linalg.norm(ic[k] - allt[j]))
                    e_ref.append(np.linalg.norm(r[k] - allt[j]))
        else:   # truth + uniform offsets in +-1.5 px, window from the true quad's cell size
            for t in truths[f]:
                tc = np.asarray(t.corners, dtype=np.float64)
                st = (tc + rng.uniform(-1.5, 1.5, size=tc.shape)).astype(np.float32)
                cell = refo.quad_cell_px(np.clip(np.rint(tc), 0, None).astype(np.uint32), cells)
                r = refo.refine_corners(grey, st, cell_px=np.full(4, cell, np.float32))
                e_ref += list(np.linalg.norm(r - tc, axis=1))
                e_int += list(np.linalg.norm(np.rint(st) - tc, axis=1))
    return np.array(e_int), np.array(e_ref)


@pytest.mark.parametrize("config,start,med,p99", [
    (1, "detection", 0.22, 0.40), (2, "detection", 0.22, 0.40),
    (1, "truth", 0.22, 0.40), (2, "truth", 0.22, 0.40),
])
def test_refined_corners_clean_frames(oracle, config, start, med, p99):
    e_int, e_ref = _errors(oracle, config, 3, start)
    assert len(e_ref) >= 40
    print(f"config {config} start {start}: {len(e_ref)} corners, integer median {np.median(e_int):.3f} p99 {np.percentile(e_int, 99):.3f}, "
          f"refined median {np.median(e_ref):.3f} p99 {np.percentile(e_ref, 99):.3f}")
    assert np.median(e_ref) <= med and np.percentile(e_ref, 99) <= p99
    assert np.median(e_int) > np.median(e_ref) and np.percentile(e_int, 99) > np.percentile(e_ref, 99)


@pytest.mark.parametrize("start", ["detection", "truth"])
def test_refined_corners_noisy_frames(oracle, start):
    e_int, e_ref = _errors(oracle, 4, 3, start)   # BASELINE config 4: sigma = 8 grey levels of noise
    assert len(e_ref) >= 30
    print(f"config 4 start {start}: {len(e_ref)} corners, integer median {np.median(e_int):.3f}, refined median {np.median(e_ref):.3f}")
    assert np.median(e_ref) <= 0.25
    assert np.median(e_int) > np.median(e_ref)


def test_weights_are_the_stated_expression():
    import math

    for w in range(1, 11):
        g = refo.refine_weights(w)
        want = np.array([math.exp(-(i * i) / (w * w)) for i in range(-w, w + 1)], dtype=np.float32)
        assert np.array_equal(g, want)


def test_flat_window_keeps_the_start():
    grey = np.full((40, 50), 117, np.uint8)   # no gradient anywhere: det == 0 at once
    start = np.array([[20.25, 13.5], [3.0, 4.0]], np.float32)
    assert np.array_equal(refo.refine_corners(grey, start), start)


@pytest.mark.parametrize("d", [0, 1, 2])
def test_corner_near_the_frame_border(d):
    """border replicate: a corner 0-2 px from the frame edge refines without reading outside and stays in the window (the frame of
    tests/refine_cases.py that the kernel runs as well: a dark rectangle of 20 x 14 from pixel (d, d))"""
    img, _ = rcs.border_frames(d)["corners"]
    assert img[d, d] == 30 and img[d + 13, d + 19] == 30 and img[d + 14, d + 19] == 220 and img[d + 13, d + 20] == 220
    cfg = refo.RefineConfig(1, 5, 0.0, 30, 0.01)
    start = np.array([[d, d], [d + 19, d + 13]], np.float32)
    r = refo.refine_corners(img, start, cfg)
    assert np.all(np.isfinite(r))
    assert np.all(np.abs(r - start) <= 5.0)
    assert np.linalg.norm(r[1] - np.array([d + 19.5, d + 13.5])) < 0.3   # the free corner finds the edge crossing (between two pixels)


def test_start_that_drifts_past_the_window_reverts():
    """the corner of a dark square sits at (29.5, 29.5) (tests/refine_cases.py, box_frame); started at (27, 27) with w = 2, the window's
    last column and row (pixels 29) already see both edges (det != 0), the first step lands about 2.5 px away -- past w -- and the
    corner reverts to q0"""
    img = rcs.box_frame()
    assert rcs.BOX[:2] == (29.5, 29.5)
    start = np.array([[27.0, 27.0]], np.float32)
    free = refo.refine_corners(img, start, refo.RefineConfig(1, 5, 0.0, 30, 0.0))
    assert np.linalg.norm(free[0] - np.array([29.5, 29.5])) < 0.1, free   # with room it finds the corner, 2.5 px away
    for it in (1, 30):
        assert np.array_equal(refo.refine_corners(img, start, refo.RefineConfig(1, 2, 0.0, it, 0.0)), start)
    moved = refo.refine_corners(img, start, refo.RefineConfig(1, 3, 0.0, 1, 0.0))   # w = 3 allows the same first step
    assert np.abs(moved - start).max() > 2.0, moved


def test_bad_config_is_refused():
    with pytest.raises(ValueError):
        refo.refine_corners(np.zeros((8, 8), np.uint8), [[3.0, 3.0]], refo.RefineConfig(1, 11, 0.4, 30, 0.01))


# ---- a3_refine_config layout: C (a program of its own), ctypes, the oracle's mirror and the Rust shim ----

_LAYOUT_C = r"""
#include <stddef.h>
#include <stdio.h>
#include "aruco3_hip.h"
int main(void) {
    printf("size %zu align %zu\n", sizeof(a3_refine_config), _Alignof(a3_refine_config));
#define F(f) printf("%s %zu %zu\n", #f, offsetof(a3_refine_config, f), sizeof(((a3_refine_config *)0)->f));
    F(method) F(win_half) F(relative_win) F(max_iterations) F(min_shift)
    printf("consts %d %d\n", A3_REFINE_NONE, A3_REFINE_SUBPIX);
    return 0;
}
"""


def test_refine_config_layout(tmp_path):
    cc = shutil.which("cc") or shutil.which("gcc")
    if cc is None:
        pytest.skip("no C compiler")
    src = tmp_path / "layout.c"
    src.write_text(_LAYOUT_C)
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c11", "-Wall", "-I", str(ROOT / "include"), str(src), "-o", str(exe)])
    lines = subprocess.check_output([str(exe)], text=True).split("\n")
    size, align = map(int, re.match(r"size (\d+) align (\d+)", lines[0]).groups())
    fields = [(ln.split()[0], int(ln.split()[1]), int(ln.split()[2])) for ln in lines[1:6]]
    assert lines[6].split()[1:] == ["0", "1"]

    from aruco3_amd import _lib

    for S in (_lib.RefineConfig, refo.RefineConfig):
        assert C.sizeof(S) == size and C.alignment(S) == align
        assert [(n, getattr(S, n).offset, getattr(S, n).size) for n, _ in S._fields_] == fields
    text = re.sub(r"//[^\n]*", "", (ROOT / "integration" / "aruco3_hip.rs").read_text())
    m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^\]]*\)\]\s*)?pub struct A3RefineConfig \{(.*?)\}", text, flags=re.S)
    assert m
    rust = re.findall(r"pub\s+([a-z0-9_]+)\s*:\s*([a-z0-9]+)", m.group(1))
    assert [n for n, _ in rust] == [f[0] for f in fields]
    assert [4 if t in ("u32", "f32", "i32") else None for _, t in rust] == [f[2] for f in fields]
    assert "pub fn detect_refined(&self, image: DynamicImage, refine: &RefineConfig) -> (Detection, Vec<[(f32, f32); 4]>)" in text


def test_python_surface_defaults():
    from aruco3_amd import _lib
    from aruco3_amd.aruco import CornerRefinement, Marker

    r = CornerRefinement()
    c = r._c()
    assert (c.method, c.win_half, c.max_iterations) == (_lib.REFINE_SUBPIX, 5, 30)
    assert abs(c.relative_win - 0.4) < 1e-7 and abs(c.min_shift - 0.01) < 1e-9
    m = Marker(3, 0x55, [(1, 2), (3, 4), (5, 6), (7, 8)], 0)   # positional construction as before; the new field defaults to None
    assert m.corners_refined is None
    L = _lib.load()
    d = _lib.RefineConfig()
    L.a3_default_refine_config(C.byref(d))
    assert [getattr(d, n) for n, _ in d._fields_] == [getattr(c, n) for n, _ in c._fields_]
