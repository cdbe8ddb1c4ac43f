"""The argument checks of 3-D boards (aruco3_amd/csrc/a3_board3d_check.h) without a GPU: tests/board3d_checks.cpp runs every refusal
and every accepted boundary case under the address and undefined-behaviour sanitizers, and each message is one whole literal of the
library, which the GPU tests match on."""
import os
import re
import shutil
import subprocess
from pathlib import Path

ROOT = Path(__file__).resolve().parent.parent


def test_shared_check_functions(tmp_path):
    """tests/board3d_checks.cpp: a3_board3d_check.h alone, as a stand-alone program with the sanitizers' runtimes linked in"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "tests/board3d_checks.cpp needs a C++ compiler (g++ or c++)"
    exe = tmp_path / "board3d_checks"
    clang = "clang" in subprocess.run([cxx, "--version"], stdout=subprocess.PIPE, text=True).stdout
    subprocess.check_call([cxx, "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           *(["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]), "-o", str(exe),
                           str(ROOT / "tests" / "board3d_checks.cpp")])
    out = subprocess.run([str(exe)], capture_output=True, text=True, stdin=subprocess.DEVNULL)
    assert out.returncode == 0, out.stdout + out.stderr
    assert re.search(r"^ok: \d+ checks$", out.stdout.strip().splitlines()[-1])


def test_the_messages_are_in_the_library_as_they_read():
    blob = (ROOT / "aruco3_amd" / "libaruco3_hip.so").read_bytes()
    text = (ROOT / "aruco3_amd" / "csrc" / "a3_board3d_check.h").read_text()
    msgs = re.findall(r'"(a3_(?:set_board3d|set_charuco|set_board_recovery|recover_markers): [^"]+)"', text)
    assert len(msgs) == 11
    for m in msgs:
        assert m.encode() + b"\0" in blob, m
    api = (ROOT / "aruco3_amd" / "csrc" / "a3_api.hip").read_text()
    for call in ("check_board3d_call(", "check_board3d_marker(", "check_charuco_board_kind(", "check_recovery_board_kind(",
                 "check_recover_markers_board_kind("):
        assert call in api, call
