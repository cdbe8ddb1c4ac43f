"""Detection with several threshold windows (a3_set_threshold_windows), the part that needs no GPU: the two entry points are declared on
every side of the boundary, the argument checks and the index arithmetic give their answers (tests/windows_checks.cpp over
a3_windows_check.h), the Python front end hands the setting on -- and the expectation tests/test_gpu_multiwindow.py compares against
exercises the merge: a case whose restated discard never met a rotated or an equal-perimeter pair would prove nothing."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import numpy as np
import pytest

from tests import multiwindow_util as mw

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("a3_set_threshold_windows", "a3_get_threshold_windows")


def _flat(text):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_the_two_entry_points_are_declared_everywhere():
    from aruco3_amd import _lib

    header = _flat((ROOT / "include" / "aruco3_hip.h").read_text())
    assert "#define A3_MAX_THRESHOLD_WINDOWS 4" in header
    assert "int a3_set_threshold_windows(a3_ctx *ctx, const uint32_t *radii, size_t n);" in header
    assert "int a3_get_threshold_windows(const a3_ctx *ctx, uint32_t *radii, size_t cap, size_t *n);" in header
    assert re.search(r"#define\s+A3_ABI_VERSION\s+5\b", header)   # additive: the ABI version stays
    rust = re.sub(r"//[^\n]*", "", (ROOT / "integration" / "aruco3_hip.rs").read_text())
    for n in NAMES:
        assert n in _lib.SYMBOLS
        assert re.search(r"pub\s+fn\s+%s\s*\(" % n, rust), n
        assert hasattr(_lib.load(), n), n
    assert _lib.load().a3_abi_version() == 5
    assert _lib.MAX_THRESHOLD_WINDOWS == 4
    assert "pub fn detect_windows(&self, image: DynamicImage, windows: &[u32]) -> Detection" in rust
    launch = (ROOT / "aruco3_amd" / "csrc" / "a3_launch.h").read_text()
    assert "hipError_t launch_merge_candidates(hipStream_t st, const DecodeStage& d);" in launch
    assert "a3_windows_check.h" in (ROOT / "aruco3_amd" / "csrc" / "Makefile").read_text()


def test_shared_check_function(tmp_path):
    """tests/windows_checks.cpp: a3_windows_check.h alone, under the address and undefined-behaviour sanitizers -- every refusal of the
    setter, the plane index and the capacity rule"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "tests/windows_checks.cpp needs a C++ compiler (g++ or c++)"
    exe = tmp_path / "windows_checks"
    # the sanitizers' runtimes are linked into the program, so it does not depend on the order in which the loader brings libraries in
    clang = "clang" in subprocess.run([cxx, "--version"], stdout=subprocess.PIPE, text=True).stdout
    subprocess.check_call([cxx, "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           *(["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]), "-o", str(exe),
                           str(ROOT / "tests" / "windows_checks.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert out.returncode == 0, out.stdout + out.stderr
    assert re.search(r"^ok: \d+ checks$", out.stdout.strip().splitlines()[-1])


def test_the_messages_are_in_the_library_as_they_read():
    """the GPU tests match on them: each is one whole literal of the library's read-only data"""
    blob = (ROOT / "aruco3_amd" / "libaruco3_hip.so").read_bytes()
    text = (ROOT / "aruco3_amd" / "csrc" / "a3_windows_check.h").read_text()
    msgs = re.findall(r'"(a3_(?:set_threshold_windows|detect_batch): [^"]+)"', text)
    assert len(msgs) == 7
    for m in msgs:
        assert m.encode() + b"\0" in blob, m


def test_the_front_end_hands_the_setting_on():
    """Detector(threshold_windows=...) reaches the context through _apply_threshold_windows, once per change; BatchQueue carries it"""
    from aruco3_amd import aruco
    from aruco3_amd.aruco import Detector

    class _Ctx:
        def __init__(self):
            self.calls = []

        def set_threshold_windows(self, radii):
            self.calls.append(tuple(radii))

    c = _Ctx()
    aruco._apply_threshold_windows(c, None)            # off on a fresh context: nothing to say
    assert c.calls == []
    aruco._apply_threshold_windows(c, (3, 7, 15))
    aruco._apply_threshold_windows(c, [3, 7, 15])      # the same set: not handed over again
    assert c.calls == [(3, 7, 15)]
    aruco._apply_threshold_windows(c, None)
    aruco._apply_threshold_windows(c, ())
    assert c.calls == [(3, 7, 15), ()]
    assert Detector(threshold_windows=(3, 7, 15)).threshold_windows == (3, 7, 15) and Detector().threshold_windows is None
    src = (ROOT / "aruco3_amd" / "aruco.py").read_text()
    assert "self._threshold_windows = detector.threshold_windows" in src and "_apply_threshold_windows(ctx, self._threshold_windows)" in src
    assert "threshold_windows" not in {f for f in aruco.DetectorConfig.__dataclass_fields__}   # the config stays the crate's mirror


@pytest.mark.parametrize("factor", mw.FACTORS)
def test_the_expectation_exercises_the_merge(oracle, dicts, factor):
    """BASELINE config 1, frames 0-2, windows (3, 7, 15).  The survivors of the restated discard, handed to the oracle as its candidate
    list, all come back as its final candidates (the second, unrotated discard kills none); and the walk met what it is there for: a
    cross-window pair decided only through a rotation, a cross-window pair with equal perimeters, a survivor from a later window.
    (Measured: per-plane counts [16, 9, 10], [13, 7, 6], [12, 6, 6]; at factor 0.1 the survivors per window are [6, 0, 1], [5, 2, 0],
    [4, 1, 0]; frames 1 and 2 hold rotation-only pairs, every frame 14 to 21 close pairs of equal perimeter.)"""
    d = dicts.new_from_named_dict("ARUCO_DEFAULT")
    frames = mw.config1_frames(3)
    exp = mw.expectation(oracle, d, frames, mw.WINDOWS, factor, key="config1")
    assert [[len(p["candidates_pre"]) for p in e["planes"]] for e in exp] == [[16, 9, 10], [13, 7, 6], [12, 6, 6]]
    by_window = [[int(np.count_nonzero(e["win"][e["kept"]] == k)) for k in range(3)] for e in exp]
    if factor == 0.1:
        assert by_window == [[6, 0, 1], [5, 2, 0], [4, 1, 0]]
    for e in exp:
        assert e["final"] is not None and e["final"]["candidates"].tolist() == e["fin"].tolist()
        assert len(e["final"]["markers"]) >= max(len(p["markers"]) for p in e["planes"][1:])
        # concatenation: each plane's list in its own (ascending start key) order
        off = 0
        for p in e["planes"]:
            assert np.all(np.diff(p["candidates_pre_start"].astype(np.int64)) > 0)
            assert e["pre"][off: off + len(p["candidates_pre"])].tolist() == p["candidates_pre"].tolist()
            off += len(p["candidates_pre"])
    assert sum(e["census"]["rotation_only_kills"] for e in exp) >= 1
    assert sum(e["census"]["cross_equal_perimeter_pairs"] for e in exp) >= 1
    assert sum(w[1] + w[2] for w in by_window) >= 1
    assert sum(e["census"]["i_dies"] for e in exp) >= 1   # the later quad wins at least once: the order of the walk matters


def test_rotation_is_for_pairs_across_windows_only():
    """one quad and its copy rotated left by one corner, 2 px off: from one window both survive (the reference's behaviour stays),
    from two windows the later one dies; at equal perimeters the earlier one wins"""
    a = np.array([(100, 100), (180, 100), (180, 180), (100, 180)])
    b = np.roll(a, -1, axis=0) + 2
    _, _, kept, census = mw.merged_model([np.stack([a, b])], 10.0)
    assert kept.tolist() == [0, 1] and census["rotation_only_kills"] == 0
    _, win, kept, census = mw.merged_model([a[None], b[None]], 10.0)
    assert kept.tolist() == [0] and win.tolist() == [0, 1] and census == dict(rotation_only_kills=1, cross_equal_perimeter_pairs=1, cross_kills=1, i_dies=0)
    bigger = np.array([(98, 98), (184, 98), (184, 184), (98, 184)])
    _, _, kept, census = mw.merged_model([a[None], np.roll(bigger, -3, axis=0)[None]], 10.0)
    assert kept.tolist() == [1] and census["i_dies"] == 1 and census["rotation_only_kills"] == 1
    _, _, kept, _ = mw.merged_model([np.zeros((0, 4, 2)), a[None], np.zeros((0, 4, 2))], 10.0)
    assert kept.tolist() == [0]
