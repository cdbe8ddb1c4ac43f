"""Inverted markers (a3_set_marker_polarity), the part that needs no GPU: the three entry points and the constants are declared on every
side of the boundary, the ABI version and every struct of the header are what they were, the argument checks that need no device give
their answers, the read-back layout without flags is what it was and with flags carries one word per marker behind everything else,
and the Python front end hands the setting on."""
import ctypes as C
import re
import shutil
import subprocess
from pathlib import Path

import pytest

ROOT = Path(__file__).resolve().parent.parent
NAMES = ("a3_set_marker_polarity", "a3_get_marker_polarity", "a3_get_marker_flags")
# sizeof of every struct tests/c_abi/caller.c prints, written out so that a change shows here as a number; the test below also holds the
# header to tests/test_c_abi.py's own expectations: the Rust shim's #[repr(C)] structs (untouched by this feature) and the ctypes mirror
SIZES = {"a3_config": 32, "a3_marker": 56, "a3_pose": 52, "a3_intrinsics": 24, "a3_stats": 64, "a3_synth_marker": 80, "a3_synth_frame": 32}


def _flat(text):
    return re.sub(r"\s+", " ", re.sub(r"/\*.*?\*/", "", text, flags=re.S))


def test_the_entry_points_are_declared_everywhere():
    from aruco3_amd import _lib

    raw = (ROOT / "include" / "aruco3_hip.h").read_text()
    header = _flat(raw)
    assert "enum { A3_POLARITY_DARK = 0 , A3_POLARITY_BOTH = 1 };" in header
    assert "#define A3_MARKER_INVERTED 1u" in header
    assert "int a3_set_marker_polarity(a3_ctx *ctx, int mode);" in header
    assert "int a3_get_marker_polarity(const a3_ctx *ctx, int *mode);" in header
    assert "int a3_get_marker_flags(a3_ctx *ctx, uint32_t *dst, size_t cap_markers, size_t *n);" in header
    assert re.search(r"#define\s+A3_ABI_VERSION\s+5\b", header)   # additive: the ABI version stays
    assert "Out of scope: inverted (bright-inside) markers" not in raw
    assert "0 = no codes" in raw and "2 = read inverted" in raw     # a3_download_homographies' decode_ok
    rust = re.sub(r"//[^\n]*", "", (ROOT / "integration" / "aruco3_hip.rs").read_text())
    for n in NAMES:
        assert n in _lib.SYMBOLS
        assert re.search(r"pub\s+fn\s+%s\s*\(" % n, rust), n
        assert hasattr(_lib.load(), n), n
    for const, value in (("A3_POLARITY_DARK: c_int", 0), ("A3_POLARITY_BOTH: c_int", 1), ("A3_MARKER_INVERTED: u32", 1)):
        assert re.search(r"pub\s+const\s+%s\s*=\s*%d\s*;" % (re.escape(const), value), rust), const
    assert _lib.load().a3_abi_version() == 5
    assert (_lib.POLARITY_DARK, _lib.POLARITY_BOTH, _lib.MARKER_INVERTED) == (0, 1, 1)
    launch = (ROOT / "aruco3_amd" / "csrc" / "a3_launch.h").read_text()
    assert "hipError_t launch_marker_flags(hipStream_t st, const MarkerFlagsLaunch& m);" in launch
    assert "const uint32_t* flags = nullptr;" in launch


def test_no_struct_of_the_header_changed(tmp_path):
    exe = tmp_path / "caller"
    lib_dir = ROOT / "aruco3_amd"
    assert (lib_dir / "libaruco3_hip.so").exists(), "build the library first (__graft_entry__.build())"
    subprocess.check_call(["gcc", "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", str(ROOT / "include"), str(ROOT / "tests" / "c_abi" / "caller.c"),
                           "-o", str(exe), "-L", str(lib_dir), "-laruco3_hip", f"-Wl,-rpath,{lib_dir}", "-Wl,-rpath-link,/opt/rocm/lib"])
    out = subprocess.run([str(exe), "layout"], capture_output=True, text=True, timeout=60, stdin=subprocess.DEVNULL)
    assert out.returncode == 0, out.stderr
    sizes = {ln.split()[0]: int(ln.split()[2]) for ln in out.stdout.splitlines() if " - " in ln}
    assert sizes.pop("A3_ABI_VERSION") == 5
    assert sizes == SIZES
    from aruco3_amd import _lib
    from tests import test_c_abi as abi

    assert set(abi._RUST_OF_C) == set(SIZES)      # every struct tests/c_abi knows, and no other
    for c_name, rust_name in abi._RUST_OF_C.items():
        assert abi._rust_layout(rust_name)[1] == sizes[c_name], c_name
    for c_name, cls in (("a3_config", _lib.Config), ("a3_marker", _lib.MarkerRec), ("a3_pose", _lib.PoseRec), ("a3_intrinsics", _lib.Intrinsics),
                        ("a3_stats", _lib.Stats)):
        assert C.sizeof(cls) == sizes[c_name], c_name


def test_argument_checks_that_need_no_device():
    from aruco3_amd import _lib

    L = _lib.load()
    mode, n = C.c_int(7), C.c_size_t(9)
    buf = (C.c_uint32 * 4)()
    assert L.a3_set_marker_polarity(None, _lib.POLARITY_BOTH) == _lib.ERR_INVALID
    assert L.a3_get_marker_polarity(None, C.byref(mode)) == _lib.ERR_INVALID and mode.value == 7
    assert L.a3_get_marker_flags(None, buf, 4, C.byref(n)) == _lib.ERR_INVALID and n.value == 9


def test_readback_layout_with_and_without_flags(tmp_path):
    """a3_readback.h in a plain C++ program, under the address and undefined-behaviour sanitizers: with the switch off (its default)
    every span and the end are what they are without it; with it on the flags lie behind everything else, one word per marker of the
    guess, and in the re-fetch one per marker of the list; tests/readback_layout.cpp (untouched) holds every existing combination"""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "needs a C++ compiler (g++ or c++)"
    src = ROOT / "tests" / "readback_flags_layout.cpp"
    exe = tmp_path / "flags_layout"
    clang = "clang" in subprocess.run([cxx, "--version"], stdout=subprocess.PIPE, text=True).stdout
    subprocess.check_call([cxx, "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           *(["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]), "-o", str(exe), str(src)])
    out = subprocess.run([str(exe)], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert out.returncode == 0, out.stdout + out.stderr
    assert re.search(r"^ok: \d+ checks$", out.stdout.strip().splitlines()[-1])


def test_the_front_end_hands_the_setting_on():
    from aruco3_amd import _lib, aruco
    from aruco3_amd.aruco import Detector, Marker

    class _Ctx:
        def __init__(self):
            self.calls = []

        def set_marker_polarity(self, mode):
            self.calls.append(mode)

    c = _Ctx()
    aruco._apply_polarity(c, False)            # DARK on a fresh context: nothing to say
    assert c.calls == []
    aruco._apply_polarity(c, True)
    aruco._apply_polarity(c, True)             # the same mode: not handed over again
    aruco._apply_polarity(c, False)
    assert c.calls == [_lib.POLARITY_BOTH, _lib.POLARITY_DARK]
    assert Detector(inverted_markers=True).inverted_markers is True and Detector().inverted_markers is False
    assert Marker(1, 2, [(0, 0)] * 4, 0).inverted is False
    assert aruco._inverted_at(None, 0) is False
    assert aruco._inverted_at([0, 1], 1) is True and aruco._inverted_at([0, 1], 0) is False
    src = (ROOT / "aruco3_amd" / "aruco.py").read_text()
    assert "self._inverted = bool(detector.inverted_markers)" in src and "_apply_polarity(ctx, self._inverted)" in src
    assert "inverted_markers" not in {f for f in aruco.DetectorConfig.__dataclass_fields__}   # the config stays the crate's mirror


@pytest.mark.parametrize("path", ("README.md", "INTEGRATION.md", "DESIGN.md"))
def test_the_documents_speak_of_it(path):
    assert "a3_set_marker_polarity" in (ROOT / path).read_text()
