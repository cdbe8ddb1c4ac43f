"""Rectification inside the detect calls (a3_set_rectification), the part that needs no GPU: the two entry points are declared on every
side of the boundary, `Rectification` builds the a3_rectify `rectify_frames` builds, a lens on a pose call is refused, the shared
argument check gives a3_rectify_frames' messages as they always read and the setter's behind its own name -- and the CPU expectations
of tests/test_gpu_rectified_detection.py are not empty: a case whose oracle finds nothing would prove nothing."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import rectified_cases as rc

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("a3_set_rectification", "a3_get_rectification")


def _strip_c(text):
    return re.sub(r"/\*.*?\*/", "", text, flags=re.S)


def test_the_two_entry_points_are_declared_everywhere():
    from aruco3_amd import _lib

    header = _strip_c((ROOT / "include" / "aruco3_hip.h").read_text())
    assert re.search(r"int\s+a3_set_rectification\(a3_ctx \*ctx, const a3_rectify \*r\);", header)
    assert re.search(r"int\s+a3_get_rectification\(const a3_ctx \*ctx, a3_rectify \*r, int \*enabled\);", header)
    assert re.search(r"#define\s+A3_ABI_VERSION\s+5\b", header)   # additive: the ABI version stays
    rust = re.sub(r"//[^\n]*", "", (ROOT / "integration" / "aruco3_hip.rs").read_text())
    for n in NAMES:
        assert n in _lib.SYMBOLS
        assert re.search(r"pub\s+fn\s+%s\s*\(" % n, rust), n
        assert hasattr(_lib.load(), n), n
    assert "pub fn detect_rectified(&self, image: DynamicImage, rect: &A3Rectify) -> Detection" in rust
    launch = (ROOT / "aruco3_amd" / "csrc" / "a3_launch.h").read_text()
    assert "struct RectifyGreyLaunch" in launch and "hipError_t launch_rectify_grey(hipStream_t st, const RectifyGreyLaunch& r);" in launch


def test_rectification_builds_the_a3_rectify_of_rectify_frames(monkeypatch):
    """the record rectify_frames hands to a3_rectify_frames, caught at the call, against Rectification._c() for the same arguments"""
    from aruco3_amd import CameraIntrinsics, Distortion, Rectification, _lib, rectify

    seen = []

    class _Ctx:
        def rectify_frames(self, *args):
            seen.append(bytes(args[6]))

    monkeypatch.setattr(rectify, "_ctxs", {0: _Ctx()})
    R = np.array([[0.0, -1.0, 0.0], [1.0, 0.0, 0.0], [0.0, 0.0, 1.0]])
    cam = CameraIntrinsics(24, 16, 30.0, 31.0, 12.5, 7.5, distortion=Distortion(-0.2, 0.05, 1e-3, -2e-3, 0.01, 0.1, 0.02, 0.003))
    fish = CameraIntrinsics(24, 16, 30.0, 31.0, 12.5, 7.5, distortion=Distortion.fisheye(-0.02, 0.005, -0.003, 0.0005))
    plain = CameraIntrinsics(24, 16, 30.0, 31.0, 12.5, 7.5)
    view = CameraIntrinsics(20, 12, 25.0, 26.0, 10.0, 6.0)
    frames = np.zeros((2, 16, 24, 3), np.uint8)
    cases = [(cam, None, None, 0), (cam, view, R, 200), (fish, view, None, 7), (plain, view, R, 255), (plain, None, None, 0)]
    for args in cases:
        rectify.rectify_frames(frames, *args)
        r = Rectification(*args)._c()
        assert bytes(r) == seen[-1], args
        assert isinstance(r, _lib.RectifyRec) and r.fill == args[3] and (r.dst.image_width, r.dst.image_height) == Rectification(*args).view_size
    assert len(set(seen)) == len(cases)
    with pytest.raises(ValueError):
        Rectification(cam, fill=256)._c()


def test_a_lens_on_a_pose_call_is_refused():
    from aruco3_amd import CameraIntrinsics, Detector, Distortion, Rectification
    from aruco3_amd.board import CharucoBoard, GridBoard

    cam = CameraIntrinsics(64, 48, 50.0, 50.0, 32.0, 24.0, distortion=Distortion(-0.1, 0.01))
    frames = np.zeros((1, 48, 64, 3), np.uint8)
    for board, call in ((None, lambda d: d.detect_batch_with_pose(frames, 30.0, cam)),
                        (GridBoard(2, 2, 30.0, 6.0), lambda d: d.detect_batch_with_board_pose(frames, cam)),
                        (CharucoBoard(4, 3, 40.0, 28.0), lambda d: d.detect_batch_with_charuco_pose(frames, cam))):
        with pytest.raises(ValueError) as e:
            call(Detector(rectification=Rectification(cam), board=board))
        assert "the view's plain intrinsics" in str(e.value)


def test_shared_check_function(tmp_path):
    """tests/rectify_checks.cpp: a3_rectify_check.h alone, under the address and undefined-behaviour sanitizers -- a3_rectify_frames'
    messages byte for byte, the setter's the same text behind its name, the first failing check reported"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "tests/rectify_checks.cpp needs a C++ compiler (g++ or c++)"
    exe = tmp_path / "rectify_checks"
    # the sanitizers' runtimes are linked into the program, so it does not depend on the order in which the loader brings libraries in
    clang = "clang" in subprocess.run([cxx, "--version"], stdout=subprocess.PIPE, text=True).stdout
    subprocess.check_call([cxx, "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           *(["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]), "-o", str(exe),
                           str(ROOT / "tests" / "rectify_checks.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert out.returncode == 0, out.stdout + out.stderr
    assert re.search(r"^ok: \d+ checks$", out.stdout.strip().splitlines()[-1])


def test_the_messages_of_rectify_frames_are_in_the_library_as_they_read():
    """existing tests match on them: each is one whole literal of the library's read-only data"""
    blob = (ROOT / "aruco3_amd" / "libaruco3_hip.so").read_bytes()
    for m in ("a3_rectify_frames: an image size of 0, above 65535 or of 2^30 pixels and more", "a3_rectify_frames: row stride smaller than a row",
              "a3_rectify_frames: frame stride smaller than a frame", "a3_rectify_frames: an intrinsic is not finite",
              "a3_rectify_frames: focal lengths must be > 0", "a3_rectify.reserved must be 0", "a3_rectify.distortion.model: unknown model",
              "a3_rectify.distortion: a coefficient is not finite", "a3_rectify.rotation: an entry is not finite",
              "a3_rectify.distortion: model A3_DIST_FISHEYE reads k1 k2 k3 k4; p1 p2 k5 k6 must be 0",
              "a3_set_rectification: a3_rectify.reserved must be 0", "a3_set_rectification: focal lengths must be > 0",
              "a3_set_rectification: a submitted batch has not been collected"):
        assert m.encode() + b"\0" in blob, m


@pytest.mark.parametrize("name", list(rc.CASES))
def test_expectations_are_not_empty(name):
    """every frame of the case holds at least 3 markers in the oracle's eyes, and in at least one frame a marker lies within 8 px of
    the view's edge"""
    case = rc.CASES[name]
    frames = rc.source_frames(name)
    assert frames.shape == (len(case.poses), rc.SRC_SIZE[1], rc.SRC_SIZE[0], 3)
    assert not np.array_equal(frames[..., 0], frames[..., 2])   # R and B differ
    rect, grey, res = rc.expectation(name)
    dw, dh = case.view_size
    assert rect.shape == (len(frames), dh, dw, 3) and grey.shape == (len(frames), dh, dw)
    near = []
    for r in res:
        assert len(r["markers"]) >= 3
        c = np.array([m["corners"] for m in r["markers"]]).reshape(-1, 2)
        near.append(min(c[:, 0].min(), c[:, 1].min(), dw - 1 - c[:, 0].max(), dh - 1 - c[:, 1].max()))
    assert min(near) <= rc.EDGE_PX, near
    ids = {m["id"] for r in res for m in r["markers"]}
    assert ids <= set(int(i) for i in rc.board().ids)


def test_luma_is_the_librarys():
    """tests/rectified_cases.luma against the oracle's into_luma8, in both channel orders"""
    from oracle import a3oracle

    rgb = np.random.default_rng(5).integers(0, 256, (9, 31, 3), dtype=np.uint8)
    assert np.array_equal(rc.luma(rgb), a3oracle.to_luma8(rgb))
    assert np.array_equal(rc.luma(rgb[..., ::-1], "bgr"), a3oracle.to_luma8(rgb))
    rgba = np.concatenate([rgb, np.full((9, 31, 1), 9, np.uint8)], axis=-1)
    assert np.array_equal(rc.luma(rgba), a3oracle.to_luma8(rgb))
    assert np.array_equal(rc.luma(rgb[..., :1]), rgb[..., 0])
