"""The lens undistortion's CPU restatement (tests/lens_oracle.c) against an independent float64 model, and the a3_distortion layout
of the header, the ctypes binding and the Rust shim.  No GPU needed."""
import ctypes as C
import shutil
import subprocess

import numpy as np
import pytest

from tests import lens_oracle as lo

W, H = 1920, 1080
INTR = (1400.0, 1380.0, 955.5, 542.25)
ROUND_TRIP = ("barrel", "pincushion", "tangential", "rational8")


def _grid(step=16, margin=0):
    ys, xs = np.mgrid[-margin: H + margin: step, -margin: W + margin: step]
    return np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1).astype(np.float32)


def _forward64(points, intr, k):
    from aruco3_amd.pinhole import Distortion

    fx, fy, cx, cy = intr
    p = np.asarray(points, np.float64)
    n = np.stack([(p[:, 0] - cx) / fx, (p[:, 1] - cy) / fy], axis=1)
    d = Distortion(*k).distort_normalized(n)
    return np.stack([d[:, 0] * fx + cx, d[:, 1] * fy + cy], axis=1)


@pytest.mark.parametrize("name", ROUND_TRIP)
def test_round_trip_against_float64_model(name):
    """undistort (oracle, f32) then distort (float64 numpy): back within 1e-3 px of every point of a 1080p grid"""
    k = lo.COEFFS[name]
    pts = _grid()
    und, res = lo.undistort(pts, INTR, k)
    assert np.isfinite(res).all() and res.max() <= 0.1
    back = _forward64(und, INTR, k)
    err = np.linalg.norm(back - pts, axis=1)
    assert err.max() <= 1e-3, (name, float(err.max()))
    # the residual the contract reports is that of its own f32 check: small where the float64 error is small
    assert np.abs(res - err).max() <= 1e-3
    moved = np.linalg.norm(und - pts, axis=1).max()
    assert moved > (0.5 if name == "tangential" else 20.0), moved   # (these lenses really move the corners)


def test_webcam5_round_trip_and_forward_f32():
    k = lo.COEFFS["webcam5"]
    pts = _grid(24)
    und, res = lo.undistort(pts, INTR, k)
    ok = np.isfinite(res)
    assert ok.mean() > 0.99
    assert np.linalg.norm(_forward64(und[ok], INTR, k) - pts[ok], axis=1).max() <= 1e-3
    f32 = lo.distort(und[ok], INTR, k)
    assert np.linalg.norm(f32 - _forward64(und[ok], INTR, k), axis=1).max() <= 1e-3


def test_points_past_the_valid_field_fail():
    """k1 = -0.5: r (1 - 0.5 r^2) never exceeds 0.544, so a distorted point farther out has no preimage -- returned as it came, +inf"""
    k = (-0.5, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0)
    intr = (500.0, 500.0, 960.0, 540.0)
    pts = _grid(32, margin=64)
    und, res = lo.undistort(pts, intr, k)
    r = np.hypot((pts[:, 0] - 960.0) / 500.0, (pts[:, 1] - 540.0) / 500.0)
    bad = ~np.isfinite(res)
    assert bad[r > 0.56].all() and not bad[r < 0.4].any()
    assert np.array_equal(und[bad], pts[bad])
    assert (res[~bad] <= 0.1).all()


def test_zero_coefficients_are_the_identity_of_the_contract():
    pts = _grid(7)
    und, res = lo.undistort(pts, INTR, (0.0,) * 8)
    f = np.float32
    fx, fy, cx, cy = (f(v) for v in INTR)
    x0, y0 = (pts[:, 0] - cx) / fx, (pts[:, 1] - cy) / fy
    assert np.array_equal(und[:, 0].view(np.uint32), (x0 * fx + cx).view(np.uint32))
    assert np.array_equal(und[:, 1].view(np.uint32), (y0 * fy + cy).view(np.uint32))
    assert not res.any()


def test_iterations_and_threshold():
    k = lo.COEFFS["barrel"]
    pts = _grid(40)
    _, res1 = lo.undistort(pts, INTR, k, iterations=1, max_residual_px=1e9)
    _, res20 = lo.undistort(pts, INTR, k, iterations=20, max_residual_px=1e9)
    assert res20.max() < res1.max()
    _, strict = lo.undistort(pts, INTR, k, iterations=1, max_residual_px=0.0)
    assert np.isinf(strict[res1 > 0]).all()


def test_distortion_layouts_match_the_header(tmp_path):
    from aruco3_amd import _lib
    from tests.test_rust_shim import _c_struct_fields, _rust_struct_fields

    fields = [f for f, _ in _lib.DistortionRec._fields_]
    assert fields == _c_struct_fields("a3_distortion") == _rust_struct_fields("A3Distortion")
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.skip("needs a C compiler")
    from pathlib import Path

    inc = Path(__file__).resolve().parent.parent / "include"
    src = tmp_path / "layout.c"
    src.write_text("#include <stdio.h>\n#include <stddef.h>\n#include \"aruco3_hip.h\"\nint main(void) {\n"
                   + "".join(f'    printf("%zu ", offsetof(a3_distortion, {f}));\n' for f in fields)
                   + '    printf("%zu\\n", sizeof(a3_distortion));\n'
                   + "    return A3_DIST_NONE + A3_DIST_RATIONAL - 1;\n}\n")
    exe = tmp_path / "layout"
    subprocess.check_call([cc, "-std=c11", "-pedantic", "-Wall", "-Wextra", "-Werror", "-I", str(inc), str(src), "-o", str(exe)])
    got = [int(v) for v in subprocess.check_output([str(exe)]).split()]
    assert got == [getattr(_lib.DistortionRec, f).offset for f in fields] + [C.sizeof(_lib.DistortionRec)]
    assert _lib.DIST_NONE == 0 and _lib.DIST_RATIONAL == 1


def test_python_distortion_record():
    from aruco3_amd import _lib
    from aruco3_amd.pinhole import CameraIntrinsics, Distortion

    d = Distortion.from_opencv([-0.28, 0.09, 1e-3, -5e-4, -0.012])
    assert (d.k3, d.k4, d.k6, d.iterations, d.max_residual_px) == (-0.012, 0.0, 0.0, 20, 0.1)
    rec = d._c()
    assert rec.model == _lib.DIST_RATIONAL and rec.iterations == 20 and abs(rec.k1 + 0.28) < 1e-7
    with pytest.raises(ValueError):
        Distortion.from_opencv([0.1, 0.2, 0.3])
    ci = CameraIntrinsics(640, 480, 500.0, 500.0)
    assert ci.distortion is None and ci.principal_x == 320.0
    assert CameraIntrinsics(640, 480, 500.0, 500.0, 300.0, 200.0, d).distortion is d
    # the host forward model equals the C restatement's (float64 against f32)
    pts = np.array([[100.0, 200.0], [1500.0, 900.0]])
    f32 = lo.distort(pts, INTR, lo.COEFFS["rational8"])
    assert np.abs(_forward64(pts, INTR, lo.COEFFS["rational8"]) - f32).max() < 1e-3


def test_symbols_are_listed():
    from aruco3_amd import _lib

    for s in ("a3_default_distortion", "a3_set_distortion", "a3_get_undistorted_corners", "a3_undistort_points"):
        assert s in _lib.SYMBOLS
