"""The batch head, the device's verdict on a batch and the plan arithmetic (aruco3_amd/csrc/a3_batch_head.h) without a GPU:
tests/batch_verdict.cpp walks one designed head-and-counters input per branch of batch_verdict and per precedence pair, sends 200 000
seeded random heads through the header and through finish_batch's decision sequence as it stood before the header existed (transcribed
literally, reading the scratch words by number) -- action, code, message, hints and stats equal on every one, every branch reached --
and compares the chunk split, the frame bases, the doubling rounds, zero_layout, pool_darts_of and device_plan_capacity with the loops
and sums enqueue_chain held.  Compiled with the address and undefined-behaviour sanitizers and run as an ordinary child process: a
mismatch (the program names it) or a write past the chunk or base arrays fails here."""
import os
import re
import shutil
import subprocess
from pathlib import Path

HERE = Path(__file__).resolve().parent


def test_verdict_and_plan_equal_the_transcribed_parent(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "tests/batch_verdict.cpp needs a C++ compiler (g++ or c++)"
    exe = tmp_path / "batch_verdict"
    # the sanitizers' runtimes are linked into the program, so it does not depend on the order in which the loader brings libraries in
    clang = "clang" in subprocess.run([cxx, "--version"], stdout=subprocess.PIPE, text=True).stdout
    subprocess.check_call([cxx, "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           *(["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]), "-o", str(exe),
                           str(HERE / "batch_verdict.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, stdin=subprocess.DEVNULL)
    assert run.returncode == 0, (run.stdout[-2000:], run.stderr[-4000:])
    m = re.fullmatch(r"batch verdict: (\d+) designed cases, (\d+) random heads over (\d+) branches \(fewest (\d+)\), (\d+) plan cases, (\d+) checks\n",
                     run.stdout)
    assert m, run.stdout[-2000:]
    designed, heads, branches, fewest, plans, checks = map(int, m.groups())
    # three ways to deliver, nine re-runs (a hint or a pool each) and seven messages, in 15 places of the sequence
    assert designed >= 14 and heads >= 100_000 and branches == 15 and fewest >= 20 and plans > 20_000 and checks > 10 * heads
