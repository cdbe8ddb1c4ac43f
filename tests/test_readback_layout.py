"""The staging layout of a batch's read-back (aruco3_amd/csrc/a3_readback.h) without a GPU: tests/readback_layout.cpp compares every
span with the byte-offset sums a3_api.hip wrote out by hand before the header existed -- 64 feature combinations x frame counts x marker
guesses x ChArUco guesses x head sizes, the re-fetch of a short guess included -- and copies patterned arrays through a heap buffer of
exactly the layout's end with the writer's offsets in and the reader's out.  Compiled with the address and undefined-behaviour
sanitizers and run as an ordinary child process: a span past the end, or a mismatch (the program names it), fails here."""
import os
import re
import shutil
import subprocess
from pathlib import Path

HERE = Path(__file__).resolve().parent


def test_layout_equals_the_hand_written_sums(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "tests/readback_layout.cpp needs a C++ compiler (g++ or c++)"
    exe = tmp_path / "readback_layout"
    # the sanitizers' runtimes are linked into the program, so it does not depend on the order in which the loader brings libraries in
    clang = "clang" in subprocess.run([cxx, "--version"], stdout=subprocess.PIPE, text=True).stdout
    subprocess.check_call([cxx, "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           *(["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]), "-o", str(exe),
                           str(HERE / "readback_layout.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, stdin=subprocess.DEVNULL)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    m = re.fullmatch(r"readback layout: (\d+) staged cases, (\d+) re-fetch cases, (\d+) checks\n", run.stdout)
    assert m, run.stdout[-2000:]
    # 64 feature sets x 3 frame counts x 5 guesses x 4 ChArUco guesses x 3 head sizes, two totals each for the re-fetch
    assert int(m.group(1)) == 64 * 3 * 5 * 4 * 3 and int(m.group(2)) == 2 * int(m.group(1)) and int(m.group(3)) > 20 * int(m.group(1))
