"""The one way the C oracles under tests/ are compiled.  TEST INFRASTRUCTURE ONLY.

Each library is compiled once per process into a temporary directory of its own (gcc / cc, -ffp-contract=off as the kernels), so the
repository tree is not written to."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile
from pathlib import Path

HERE = Path(__file__).resolve().parent
_libs = {}


def build(name, sources=None) -> C.CDLL:
    """lib<name>.so from sources (default: tests/<name>.c), loaded"""
    if name not in _libs:
        cc = os.environ.get("CC") or shutil.which("gcc") or shutil.which("cc")
        if cc is None:
            raise RuntimeError(f"tests/{name}.c needs a C compiler (gcc or cc)")
        d = tempfile.mkdtemp(prefix=f"a3_{name}_")
        atexit.register(shutil.rmtree, d, True)
        so = Path(d) / f"lib{name}.so"
        subprocess.check_call([cc, "-O2", "-std=c11", "-fPIC", "-Wall", "-Wextra", "-ffp-contract=off", "-fno-fast-math",
                               "-fno-unsafe-math-optimizations", "-shared", "-o", str(so),
                               *map(str, sources or [HERE / f"{name}.c"]), "-lm"])
        _libs[name] = C.CDLL(str(so))
    return _libs[name]
