"""Detection on reduced frames (a3_reduce_frames, a3_set_reduction), the part that needs no GPU: the three entry points are declared on
every side of the boundary, `Reduction` builds the record `reduce_frames` builds, a reduction together with a rectification is refused,
the shared argument checks give their messages first failing check first -- and the CPU expectations of
tests/test_gpu_reduced_detection.py are not empty: a case whose oracle finds nothing would prove nothing."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import rectified_cases as rc
from tests import reduced_cases as rd

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("a3_reduce_frames", "a3_set_reduction", "a3_get_reduction")


def _strip_c(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def _flat(text):
    return re.sub(r"\s+", " ", text)


def test_the_three_entry_points_are_declared_everywhere():
    from aruco3_amd import _lib

    header = _flat(_strip_c((ROOT / "include" / "aruco3_hip.h").read_text()))
    assert "typedef struct a3_reduction { uint32_t factor; uint32_t reserved[3]; } a3_reduction;" in header
    assert ("int a3_reduce_frames(a3_ctx *ctx, const void *src, int src_memory, int fmt, uint32_t width, uint32_t height, size_t src_row_stride, "
            "size_t src_frame_stride, uint32_t n_frames, uint32_t factor, void *dst, int dst_memory, size_t dst_row_stride, "
            "size_t dst_frame_stride);") in header
    assert "int a3_set_reduction(a3_ctx *ctx, const a3_reduction *r);" in header
    assert "int a3_get_reduction(const a3_ctx *ctx, a3_reduction *r, int *enabled);" in header
    assert re.search(r"#define\s+A3_ABI_VERSION\s+5\b", header)   # additive: the ABI version stays
    rust = re.sub(r"//[^\n]*", "", (ROOT / "integration" / "aruco3_hip.rs").read_text())
    for n in NAMES:
        assert n in _lib.SYMBOLS
        assert re.search(r"pub\s+fn\s+%s\s*\(" % n, rust), n
        assert hasattr(_lib.load(), n), n
    assert _lib.load().a3_abi_version() == 5
    assert "pub fn detect_reduced(&self, image: DynamicImage, factor: u32) -> Detection" in rust
    launch = (ROOT / "aruco3_amd" / "csrc" / "a3_launch.h").read_text()
    assert "struct ReduceLaunch" in launch and "hipError_t launch_reduce_frames(hipStream_t st, const ReduceLaunch& r);" in launch
    assert "struct ScaleMarkersLaunch" in launch and "hipError_t launch_scale_markers(hipStream_t st, const ScaleMarkersLaunch& s);" in launch
    assert "k_reduce.hip" in (ROOT / "aruco3_amd" / "csrc" / "Makefile").read_text()


def test_reduction_builds_the_record_of_reduce_frames(monkeypatch):
    """what reduce_frames hands to a3_reduce_frames, caught at the call, against Reduction._c() for the same factor"""
    import aruco3_amd
    from aruco3_amd import Reduction, _lib, reduce

    seen = []

    class _Ctx:
        def reduce_frames(self, *args):
            seen.append(args)

    monkeypatch.setattr(reduce, "_ctxs", {0: _Ctx()})
    frames = np.zeros((2, 17, 33, 4), np.uint8)
    for f in rd.FACTORS:
        out = aruco3_amd.reduce_frames(frames, f, bgra=True)
        r = Reduction(f)._c()
        assert isinstance(r, _lib.ReductionRec) and bytes(r) == bytes(_lib.ReductionRec(f))
        ptr, mem, fmt, w, h, row, frame, n, factor, dst, dst_mem, dst_row, dst_frame = seen[-1]
        assert factor == r.factor == f and (mem, fmt, w, h, row, frame, n) == (_lib.MEM_HOST, _lib.FMT_BGRA8, 33, 17, 132, 132 * 17, 2)
        assert out.shape == (2, 17 // f, 33 // f) and out.dtype == np.uint8 and (dst_mem, dst_row, dst_frame) == (_lib.MEM_HOST, 33 // f, (33 // f) * (17 // f))
    for bad in (0, 1, 5, 2.5):
        with pytest.raises(ValueError):
            Reduction(bad)._c()
        with pytest.raises(ValueError):
            aruco3_amd.reduce_frames(frames, bad)
    with pytest.raises(ValueError):
        aruco3_amd.reduce_frames(frames[..., :3], 2, bgra=True)


def test_reduction_and_rectification_together_are_refused():
    from aruco3_amd import CameraIntrinsics, Detector, Rectification, Reduction
    from aruco3_amd.aruco import BatchQueue

    cam = CameraIntrinsics(64, 48, 50.0, 50.0, 32.0, 24.0)
    with pytest.raises(ValueError):
        Detector(reduction=Reduction(2), rectification=Rectification(cam))
    det = Detector(reduction=Reduction(2))
    det.rectification = Rectification(cam)   # (set afterwards: refused where the detector is used)
    with pytest.raises(ValueError):
        det.detect_batch(np.zeros((1, 48, 64, 3), np.uint8))
    with pytest.raises(ValueError):
        BatchQueue(det, depth=1)


def test_shared_check_function(tmp_path):
    """tests/reduce_checks.cpp: a3_reduce_check.h alone, under the address and undefined-behaviour sanitizers -- every input error of
    a3_reduce_frames, the first failing check reported, and every boundary that passes"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "tests/reduce_checks.cpp needs a C++ compiler (g++ or c++)"
    exe = tmp_path / "reduce_checks"
    # the sanitizers' runtimes are linked into the program, so it does not depend on the order in which the loader brings libraries in
    clang = "clang" in subprocess.run([cxx, "--version"], stdout=subprocess.PIPE, text=True).stdout
    subprocess.check_call([cxx, "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           *(["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]), "-o", str(exe),
                           str(ROOT / "tests" / "reduce_checks.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert out.returncode == 0, out.stdout + out.stderr
    assert re.search(r"^ok: \d+ checks$", out.stdout.strip().splitlines()[-1])


def test_the_messages_are_in_the_library_as_they_read():
    """the GPU tests match on them: each is one whole literal of the library's read-only data"""
    blob = (ROOT / "aruco3_amd" / "libaruco3_hip.so").read_bytes()
    text = (ROOT / "aruco3_amd" / "csrc" / "a3_reduce_check.h").read_text()
    msgs = re.findall(r'"(a3_(?:reduce_frames|set_reduction|detect_batch): [^"]+)"', text)
    assert len(msgs) >= 12
    for m in msgs + ["a3_reduce_frames: null argument", "a3_reduce_frames: a submitted batch has not been collected",
                     "a3_set_reduction: a submitted batch has not been collected",
                     "a3_set_reduction: a rectification is set (a3_set_rectification): set one or the other",
                     "a3_set_rectification: a reduction is set (a3_set_reduction): set one or the other"]:
        assert m.encode() + b"\0" in blob, m


@pytest.mark.parametrize("f", rd.FACTORS)
def test_expectations_are_not_empty(f):
    """for every (case, factor) used on the GPU the oracle finds at least 3 markers on the reduced plane, every id is the board's, and
    at least one case of the factor has a mapped corner within 8 f px of the full frame's edge"""
    W, H = rd.SIZE
    frames = rd.frames(f)
    assert frames.shape == (len(rd.names(f)), H, W, 3) and len(frames) >= 3
    assert not np.array_equal(frames[..., 0], frames[..., 2])   # R and B differ
    assert W % f or H % f   # trailing columns or rows that belong to no block
    planes, res, refined = rd.expectation(f)
    assert planes.shape == (len(frames), H // f, W // f)
    near = []
    for r, ref in zip(res, refined):
        assert len(r["markers"]) >= 3
        c = np.array([m["corners"] for m in r["markers"]]).reshape(-1, 2)
        small = np.array([m["corners_reduced"] for m in r["markers"]]).reshape(-1, 2)
        assert np.array_equal(c, f * small + f // 2)
        near.append(min(c[:, 0].min(), c[:, 1].min(), W - 1 - c[:, 0].max(), H - 1 - c[:, 1].max()))
        assert ref.shape == (len(r["markers"]), 4, 2) and np.isfinite(ref).all()
        assert np.abs(ref - c.reshape(-1, 4, 2)).max() > 0.25   # (the refinement moves the mapped corners: not an empty comparison)
    assert min(near) <= rd.EDGE_BLOCKS * f, near
    ids = {m["id"] for r in res for m in r["markers"]}
    assert ids <= set(int(i) for i in rd.board().ids)


def test_every_case_is_used_and_the_table_is_the_stated_one():
    assert {n: fs for n, (_, fs) in rd.CASES.items()} == {"frontal": (2, 3, 4), "tilted": (2, 3, 4), "near_corner": (2, 3, 4), "milder_tilt": (2, 3)}
    assert rd.SIZE == (963, 725) and rd.K == (680.0, 680.0, 481.0, 362.0)


def _loop_reduce(frame, f, order):
    """the contract once more, pixel by pixel in plain Python"""
    H, W, C = frame.shape
    h, w = H // f, W // f
    out = np.zeros((h, w), np.uint8)
    for i in range(h):
        for j in range(w):
            s = 0
            for b in range(f):
                for a in range(f):
                    px = [int(v) for v in frame[f * i + b, f * j + a]]
                    if C == 1:
                        s += px[0]
                    else:
                        r, g, bl = (px[0], px[1], px[2]) if order == "rgb" else (px[2], px[1], px[0])
                        s += (2126 * r + 7152 * g + 722 * bl) // 10000
            out[i, j] = (s + (f * f) // 2) // (f * f)
    return out


@pytest.mark.parametrize("f", rd.FACTORS)
def test_numpy_reduce_equals_a_plain_loop(f):
    rng = np.random.default_rng(40 + f)
    for c, order in ((1, "rgb"), (3, "rgb"), (4, "rgb"), (4, "bgr")):
        frame = rng.integers(0, 256, (14, 19, c), dtype=np.uint8)
        frame[:4, :4] = 255   # (a saturated block: the rounding never overflows a byte)
        frame[4:8, :4] = 0
        got = rd.reduce(frame, f, order)
        assert got.shape == (14 // f, 19 // f) and np.array_equal(got, _loop_reduce(frame, f, order)), (f, c, order)
        assert got[0, 0] == 255
    batch = rng.integers(0, 256, (3, 9, 11, 3), dtype=np.uint8)
    assert np.array_equal(rd.reduce(batch, f), np.stack([_loop_reduce(b, f, "rgb") for b in batch]))
    assert np.array_equal(rc.luma(batch[..., :1]), batch[..., 0])
