"""Packed 4:2:2 (YUYV, UYVY) and planar luma-first frames on the host side: the header's values against the Python and the Rust bindings,
aruco3_amd/csrc/a3_format.h and the argument checks built on it (tests/format_checks.cpp), and what `_as_frames` hands the library for
every `pixel_format` and shape.  No GPU: nothing here loads the library."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.fixture(scope="module")
def header_values(tmp_path_factory):
    """tests/format_checks.cpp: a3_format.h and the checks that use it, under the address and undefined-behaviour sanitizers -> the
    header's constants as the program printed them"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "tests/format_checks.cpp needs a C++ compiler (g++ or c++)"
    exe = tmp_path_factory.mktemp("format_checks") / "format_checks"
    # the sanitizers' runtimes are linked into the program, so it does not depend on the order in which the loader brings libraries in
    clang = "clang" in subprocess.run([cxx, "--version"], stdout=subprocess.PIPE, text=True).stdout
    subprocess.check_call([cxx, "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           *(["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]), "-o", str(exe),
                           str(ROOT / "tests" / "format_checks.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert re.search(r"^ok: \d+ checks$", lines[-1]), out.stdout
    return {m.group(1): int(m.group(2)) for m in (re.match(r"value (\w+) (-?\d+)$", l) for l in lines) if m}


def test_format_header_and_checks(header_values):
    """every format of the enum through a3_format.h; 4, 7 and -1 invalid; odd width, row stride 2W - 1, the frame-stride minimum"""
    assert header_values == {"A3_ABI_VERSION": 5, "A3_FMT_RGB8": 0, "A3_FMT_RGBA8": 1, "A3_FMT_L8": 2, "A3_FMT_BGRA8": 3,
                             "A3_FMT_YUYV8": 5, "A3_FMT_UYVY8": 6}


def test_bindings_carry_the_headers_values(header_values):
    from aruco3_amd import _lib

    rust = (ROOT / "integration" / "aruco3_hip.rs").read_text()
    rs = {m.group(1): int(m.group(2)) for m in re.finditer(r"pub const (A3_(?:FMT_\w+|ABI_VERSION)): c_int = (-?\d+);", rust)}
    assert rs == header_values
    py = {"A3_" + k: getattr(_lib, k) for k in ("FMT_RGB8", "FMT_RGBA8", "FMT_L8", "FMT_BGRA8", "FMT_YUYV8", "FMT_UYVY8")}
    assert py == {k: v for k, v in header_values.items() if k.startswith("A3_FMT_")}
    assert re.search(r"pub fn detect_raw\(&self, bytes: &\[u8\], fmt: c_int, width: u32, height: u32, row_stride: usize\) -> Detection", rust)


def test_the_checks_use_the_one_description():
    """no entry point spells the formats out any more"""
    api = (ROOT / "aruco3_amd" / "csrc" / "a3_api.hip").read_text()
    assert "fmt == A3_FMT_RGB8 ? 3" not in api and "fmt != A3_FMT_RGB8 &&" not in api
    for name in ("a3_reduce_check.h", "a3_rectify_check.h"):
        assert '#include "a3_format.h"' in (ROOT / "aruco3_amd" / "csrc" / name).read_text()
    assert "4:2:2 frames have an even width" in api or "format_width_error" in api


# ---- _as_frames ----------------------------------------------------------------------------------------------------------------
def _tuple(image, pixel_format=None):
    from aruco3_amd.aruco import _as_frames

    ptr, mem, fmt, w, h, rs, fs, n, keep = _as_frames(image, pixel_format)
    return ptr, (mem, fmt, w, h, rs, fs, n), keep


def _both(shape):
    """a numpy array and a host torch tensor of this shape"""
    import torch

    a = np.arange(int(np.prod(shape)), dtype=np.uint8).reshape(shape)
    return a, torch.from_numpy(a.copy())


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_as_frames_inferred_formats_are_unchanged(kind):
    from aruco3_amd import _lib

    H, L8, RGB, RGBA = _lib.MEM_HOST, _lib.FMT_L8, _lib.FMT_RGB8, _lib.FMT_RGBA8
    pick = 0 if kind == "numpy" else 1
    for shape, want in [((6, 8), (H, L8, 8, 6, 8, 48, 1)), ((6, 8, 1), (H, L8, 8, 6, 8, 48, 1)), ((6, 8, 3), (H, RGB, 8, 6, 24, 144, 1)),
                        ((6, 8, 4), (H, RGBA, 8, 6, 32, 192, 1)), ((3, 6, 8, 3), (H, RGB, 8, 6, 24, 144, 3)), ((3, 6, 8, 1), (H, L8, 8, 6, 8, 48, 3)),
                        ((3, 6, 8), (H, L8, 8, 6, 8, 48, 3))]:
        img = _both(shape)[pick]
        ptr, got, keep = _tuple(img)
        assert got == want, shape
        assert ptr == (keep.ctypes.data if kind == "numpy" else keep.data_ptr())
        assert _tuple(img, None)[1] == want


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_as_frames_named_formats(kind):
    from aruco3_amd import _lib

    H = _lib.MEM_HOST
    pick = 0 if kind == "numpy" else 1
    # packed 4:2:2: two bytes per pixel in both strides
    for name, fmt in (("yuyv", _lib.FMT_YUYV8), ("uyvy", _lib.FMT_UYVY8), ("YUYV", _lib.FMT_YUYV8)):
        assert _tuple(_both((6, 8, 2))[pick], name)[1] == (H, fmt, 8, 6, 16, 96, 1)
        assert _tuple(_both((3, 6, 8, 2))[pick], name)[1] == (H, fmt, 8, 6, 16, 96, 3)
    # bgra: what bgra=True means
    assert _tuple(_both((6, 8, 4))[pick], "bgra")[1] == (H, _lib.FMT_BGRA8, 8, 6, 32, 192, 1)
    assert _tuple(_both((2, 6, 8, 4))[pick], "bgra")[1] == (H, _lib.FMT_BGRA8, 8, 6, 32, 192, 2)
    # planar, luma first: the luma plane in place -- L8, H = rows * 2 / 3, row stride W, frame stride rows * W
    for name in ("nv12", "nv21", "i420", "yv12"):
        img = _both((9, 8))[pick]
        ptr, got, keep = _tuple(img, name)
        assert got == (H, _lib.FMT_L8, 8, 6, 8, 72, 1), name
        assert ptr == (keep.ctypes.data if kind == "numpy" else keep.data_ptr())
        assert _tuple(_both((5, 9, 8))[pick], name)[1] == (H, _lib.FMT_L8, 8, 6, 8, 72, 5)
        assert _tuple(_both((2, 360, 320))[pick], name)[1] == (H, _lib.FMT_L8, 320, 240, 320, 360 * 320, 2)


def test_as_frames_reads_in_place():
    """a contiguous buffer is handed over as it is: no copy"""
    import torch

    a = np.zeros((2, 6, 8, 2), np.uint8)
    assert _tuple(a, "yuyv")[0] == a.ctypes.data
    p = np.zeros((2, 9, 8), np.uint8)
    assert _tuple(p, "nv12")[0] == p.ctypes.data
    t = torch.zeros((2, 9, 8), dtype=torch.uint8)
    assert _tuple(t, "i420")[0] == t.data_ptr()
    # a non-contiguous view is made contiguous (the one copy there is)
    v = np.zeros((2, 6, 16, 2), np.uint8)[:, :, ::2]
    ptr, got, keep = _tuple(v, "uyvy")
    assert got[2:6] == (8, 6, 16, 96) and keep.flags["C_CONTIGUOUS"] and ptr == keep.ctypes.data


@pytest.mark.parametrize("kind", ["numpy", "torch"])
def test_as_frames_refusals(kind):
    pick = 0 if kind == "numpy" else 1
    bad = [
        ((3, 6, 8, 2), None),        # two channels without a format: the byte order is ambiguous
        ((6, 8, 3), "rgb"), ((6, 8, 2), "yuy2"),                              # an unknown name
        ((6, 8, 3), "yuyv"), ((6, 8), "yuyv"), ((3, 6, 8, 4), "uyvy"),      # not two channels
        ((6, 7, 2), "yuyv"), ((2, 6, 7, 2), "uyvy"),                          # an odd width
        ((6, 8, 3), "bgra"), ((6, 8), "bgra"),                                # not four channels
        # rows not divisible by 3 (3H/2 rows with H odd is no whole number of rows: 3 * 5 / 2)
        ((10, 8), "nv12"), ((2, 8, 8), "i420"), ((7, 8), "yv12"),
        ((9, 7), "nv21"),                                                     # an odd width
        ((2, 2, 9, 8), "nv12"), ((9,), "nv12"),                               # one axis too many, one too few
    ]
    for shape, name in bad:
        with pytest.raises(ValueError):
            _tuple(_both(shape)[pick], name)
    with pytest.raises(ValueError, match="C in 1,3,4"):
        _tuple(_both((3, 6, 8, 2))[pick])
    with pytest.raises(ValueError, match="even width"):
        _tuple(_both((6, 7, 2))[pick], "yuyv")
    with pytest.raises(TypeError):
        _tuple(np.zeros((6, 8, 2), np.float32) if kind == "numpy" else __import__("torch").zeros((6, 8, 2)), "yuyv")


def test_every_frame_call_takes_pixel_format():
    import inspect

    import aruco3_amd
    from aruco3_amd.aruco import BatchQueue, Detector

    for fn in (Detector.detect, Detector.detect_batch, Detector.detect_batch_with_pose, Detector.detect_batch_with_board_pose,
               Detector.detect_batch_with_charuco_pose, Detector.detect_batch_raw, Detector.interpolate_charuco, Detector.refine_corners,
               BatchQueue.submit, aruco3_amd.reduce_frames, aruco3_amd.rectify_frames):
        p = inspect.signature(fn).parameters
        assert "pixel_format" in p and p["pixel_format"].default is None, fn.__qualname__
    assert inspect.signature(Detector.detect_batch).parameters["bgra"].default is False   # bgra=True keeps working where it was
    assert inspect.signature(aruco3_amd.reduce_frames).parameters["bgra"].default is False


def test_bgra_flag_and_pixel_format_agree():
    from aruco3_amd.aruco import _pixel_format

    assert _pixel_format(None, False) is None and _pixel_format(None, True) == "bgra" and _pixel_format("bgra", True) == "bgra"
    assert _pixel_format("yuyv", False) == "yuyv"
    with pytest.raises(ValueError):
        _pixel_format("yuyv", True)
