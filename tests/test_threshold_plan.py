"""The threshold stage's launch plans (aruco3_amd/csrc/a3_threshold_plan.h) without a GPU: tests/threshold_plan_checks.cpp runs the path
choice at every class boundary and the ring kernel's LDS invariants under the address and undefined-behaviour sanitizers, and answers the
planner's result for every shape tests/test_gpu_threshold_paths.py relies on; those answers are held against tests/threshold_util.py's
Python mirrors, and the strips the GPU tests' docstrings promise are asserted on the compiled planner's word."""
import os
import re
import shutil
import subprocess
from pathlib import Path

import pytest

from tests import threshold_util as tu

ROOT = Path(__file__).resolve().parent.parent
FMT = {k: int(v) for k, v in re.findall(r"A3_FMT_(\w+) = (\d+)", (ROOT / "include" / "aruco3_hip.h").read_text())}

# (n, w, h, radius) the strip assertions below name beyond the tables' own shapes
EXTRA_K1 = [(1, 640, 100), (10, 1008, 100), (10, 1985, 100), (10, 993, 100), (10, 992, 100), (256, 1920, 1080)]


def _rows():
    """every (n, w, h, radius, format) the GPU module's tables launch a fused kernel with, and fast as their packed batches get it
    (w % 16 == 0; the unaligned layouts of tu.LAYOUTS run radii 1..7 only, whose plan does not depend on it)"""
    rows = []
    for R in tu.K1_RADII:
        cases = tu.k1_cases(R) + tu.layout_cases(R) + tu.flush_cases(R)
        rows += [(len(c.contents), c.w, c.h, R, c.fmt, c.w % 16 == 0) for c in cases]
        rows += [(n, w, h, R, "RGB8", w % 16 == 0) for n, w, h in EXTRA_K1]
    for R in tu.RING_RADII:
        cases = tu.ring_cases(R) + (tu.ring_flush_cases(R) if R in tu.RING_FLUSH_RADII else [])
        rows += [(len(c.contents), c.w, c.h, R, c.fmt, c.w % 16 == 0) for c in cases]
    return list(dict.fromkeys(rows))


@pytest.fixture(scope="module")
def planned(tmp_path_factory):
    """tests/threshold_plan_checks.cpp with the sanitizers' runtimes linked in, run once on _rows():
    {(n, w, h, radius, format, fast): (strips_x, strips_y, rows_per_wave, flush_rows, lds_bytes)}"""
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "tests/threshold_plan_checks.cpp needs a C++ compiler (g++ or c++)"
    exe = tmp_path_factory.mktemp("threshold_plan") / "threshold_plan_checks"
    clang = "clang" in subprocess.run([cxx, "--version"], stdout=subprocess.PIPE, text=True).stdout
    subprocess.check_call([cxx, "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           *(["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]), "-o", str(exe),
                           str(ROOT / "tests" / "threshold_plan_checks.cpp")])
    rows = _rows()
    table = "".join(f"{n} {w} {h} {R} {FMT[fmt]} {int(fast)}\n" for n, w, h, R, fmt, fast in rows)
    out = subprocess.run([str(exe)], input=table, capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    lines = out.stdout.strip().splitlines()
    assert re.search(r"^ok: \d+ checks$", lines[-1]), lines[-1]
    name = {v: k for k, v in FMT.items()}
    got = {}
    for line in lines[:-1]:
        v = [int(x) for x in line.split()[1:]]
        got[(v[0], v[1], v[2], v[3], name[v[4]], bool(v[5]))] = tuple(v[6:])
    assert list(got) == rows
    return got


def test_path_checks_and_ring_invariants(planned):
    """the program's own checks passed (its exit status and last line, asserted by the fixture) and it answered every row"""
    assert len(planned) == len(_rows()) > 100


def test_python_mirrors_equal_the_compiled_planner(planned):
    """tu.k1_geometry and tu.ring_geometry on every row against plan_k1 and plan_ring"""
    for (n, w, h, R, fmt, fast), (sx, sy, rows, flush, lds) in planned.items():
        if R <= 7:
            assert tu.k1_geometry(n, w, h, R) == (sx, sy, rows), (n, w, h, R)
            assert flush == min(tu.K1_FLUSH_ROWS, rows) and lds == (flush + 3 * -(-(2 * R + 1) // 3)) * 128, (n, w, h, R)
        else:
            assert tu.ring_geometry(n, w, h, R, fmt, fast) == (sx, sy, rows, flush), (n, w, h, R, fmt, fast)


def test_k1_geometry(planned):
    """the strips tests/test_gpu_threshold_paths.py relies on for radii 1..7, from the compiled planner"""
    def plan(n, w, h, R):
        return planned[(n, w, h, R, "RGB8", w % 16 == 0)][:3]

    for R in tu.K1_RADII:
        assert plan(1, 640, 100, R) == (1, 6, 17) and plan(10, 1008, 100, R) == (2, 6, 17)
        assert plan(10, 1985, 100, R) == (3, 6, 17)
        assert plan(10, 993, 100, R)[0] == 2 and plan(10, 992, 100, R)[0] == 1
        flush = tu.flush_cases(R)
        assert [(len(c.contents), c.h, c.w) for c in flush] == [(2048, 300, 16), (1024, 260, 16)]
        got = [planned[(len(c.contents), c.w, c.h, R, c.fmt, True)] for c in flush]
        assert got[0][:3] == (1, 1, 300)      # 300 rows: bursts of 128, 128 and a remainder
        assert got[1][:3] == (1, 2, 130)      # 130 rows: a burst and a remainder of 2, the second strip upwards
        assert all(rows > flush_rows == tu.K1_FLUSH_ROWS for _, _, rows, flush_rows, _ in got)
    assert planned[(256, 1920, 1080, 7, "RGB8", True)][:4] == (2, 4, 270, 128)   # 2048 waves: one round of two per SIMD


def test_ring_flush_geometry(planned):
    """the strips and bursts tu.ring_flush_cases' docstring states, from the compiled planner: every strip is taller than a burst"""
    want = {8: [(2048, 300, (1, 1, 300, 84)), (1024, 260, (1, 2, 130, 84))], 31: [(1024, 200, (1, 1, 200, 60)), (512, 260, (1, 2, 130, 60))]}
    assert set(want) == set(tu.RING_FLUSH_RADII)
    for R, shapes in want.items():
        cases = tu.ring_flush_cases(R)
        assert [(len(c.contents), c.h, c.w, c.fmt) for c in cases] == [(n, h, 16, "L8") for n, h, _ in shapes]
        for c, (n, h, plan) in zip(cases, shapes):
            got = planned[(n, 16, h, R, "L8", True)]
            assert got[:4] == plan, (R, n, h, got)
            assert got[2] > got[3]   # rows_per_wave > flush_rows
