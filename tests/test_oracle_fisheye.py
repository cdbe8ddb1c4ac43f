"""The fisheye lens model's CPU restatement (tests/fisheye_oracle.c) against independent float64 models -- its fixed-arithmetic
arctangent against numpy.arctan, the forward model against Distortion.distort_normalized, the inverse against a bracketed root solve
per point -- and the model's constants and Python surface.  No GPU needed."""
import re
from pathlib import Path

import numpy as np
import pytest

from tests import fisheye_oracle as fo

ROOT = Path(__file__).resolve().parent.parent
W, H = fo.SRC_SIZE
NO_FAILURES = ("equidistant", "mild", "strong")


def _grid(step=1, margin=0):
    ys, xs = np.mgrid[-margin: H + margin: step, -margin: W + margin: step]
    return np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1).astype(np.float32)


def _theta_d(theta, k):
    t2 = theta * theta
    return theta * (1 + (((k[3] * t2 + k[2]) * t2 + k[1]) * t2 + k[0]) * t2)


def _largest_theta_d(k):
    """the largest theta_d the model reaches on theta in [0, pi / 2): a distorted radius beyond it has no root"""
    return float(_theta_d(np.linspace(0.0, np.pi / 2, 200001), k).max())


# ---- the arctangent ----

def _atan_samples():
    t = np.concatenate([np.linspace(0.0, 8.0, 1_500_001), np.logspace(-8.0, 6.0, 1_500_001)]).astype(np.float32)
    t.sort()
    return t


def test_atan_against_float64():
    """A against numpy.arctan in float64: at most 2e-7 rad off (2.8 ulp of pi / 2 measured), and never decreasing"""
    t = _atan_samples()
    a = fo.atan(t)
    err = np.abs(a.astype(np.float64) - np.arctan(t.astype(np.float64)))
    print(f"A: largest error {err.max():.3e} rad at t = {t[err.argmax()]!r}")
    assert err.max() <= 2e-7
    assert (np.diff(a) >= 0).all()


def test_atan_ends():
    a = fo.atan([0.0, np.inf])
    assert a[0] == 0.0 and a[0].view(np.uint32) == 0
    assert a[1] == np.float32(np.pi / 2)


# ---- the forward model ----

@pytest.mark.parametrize("name", list(fo.COEFFS))
def test_forward_against_float64_model(name):
    """ideal pixels out to r = 6.7 (theta = 1.42) through the f32 oracle and through Distortion.distort_normalized: within 2e-4 px.
    The distorted positions stay below 300 px from the principal point and below 512 px.  Per coordinate, worst case: A is 1.4e-7
    rad * 150 px = 2.1e-5 px off; five roundings of 6e-8 relative on the way (the normalised input, th * poly, its inner sum, thd / r,
    x * s) are 5 * 6e-8 * 250 px = 7.5e-5 px; the product with fx and the sum with cx round by half an ulp of 512 at most, 1.5e-5 px
    each: 1.3e-4 px, times sqrt 2 for the distance"""
    from aruco3_amd.pinhole import Distortion

    k = fo.COEFFS[name]
    fx, fy, cx, cy = fo.K
    ys, xs = np.mgrid[-600: 851: 25, -600: 933: 25]
    pts = np.stack([xs.reshape(-1), ys.reshape(-1)], axis=1).astype(np.float32)
    n = np.stack([(pts[:, 0].astype(np.float64) - cx) / fx, (pts[:, 1].astype(np.float64) - cy) / fy], axis=1)
    d = Distortion.fisheye(*k).distort_normalized(n)
    want = np.stack([d[:, 0] * fx + cx, d[:, 1] * fy + cy], axis=1)
    got = fo.distort(pts, fo.K, k)
    err = np.linalg.norm(got - want, axis=1)
    print(f"{name}: forward f32 against float64, largest {err.max():.3e} px")
    assert err.max() < 2e-4
    # the principal point itself: r = 0 takes the scale 1
    assert np.array_equal(fo.distort([[cx, cy]], fo.K, k), np.array([[cx, cy]], np.float32))
    assert np.array_equal(Distortion.fisheye(*k).distort_normalized([[0.0, 0.0]]), np.zeros((1, 2)))


# ---- the inverse ----

@pytest.mark.parametrize("name", list(fo.COEFFS))
def test_inverse_against_bracketed_float64_solve(name):
    """a few hundred distorted pixels: theta from scipy's brentq on theta_d(theta) = rd in float64, r = tan(theta).  The oracle's
    theta is off by A's error (<= 2e-7 rad) and by the f32 rounding of theta_d and rd (a few ulp of 1.4: <= 5e-7 rad) over the slope
    d theta_d / d theta >= 0.5 on these sets, together <= 1.2e-6 rad; a pixel moves by fx (1 + r^2) per radian; plus 2 ulp of the
    output"""
    from scipy.optimize import brentq

    k = fo.COEFFS[name]
    fx, fy, cx, cy = fo.K
    pts = _grid(step=17)
    assert 200 <= len(pts) <= 400
    rd = np.hypot((pts[:, 0].astype(np.float64) - cx) / fx, (pts[:, 1].astype(np.float64) - cy) / fy)
    top = _largest_theta_d(k)
    und, res = fo.undistort(pts, fo.K, k)
    checked, worst = 0, 0.0
    for p, r_d, u, r_px in zip(pts.astype(np.float64), rd, und.astype(np.float64), res):
        if r_d >= 0.98 * top:   # (no root, or one too close to the end of the field for the bracket)
            continue
        theta = brentq(lambda t: _theta_d(t, k) - r_d, 0.0, np.pi / 2, xtol=1e-15, rtol=1e-15) if r_d > 0 else 0.0
        r = np.tan(theta)
        s = r / r_d if r_d > 0 else 1.0
        want = np.array([(p[0] - cx) / fx * s * fx + cx, (p[1] - cy) / fy * s * fy + cy])
        tol = fx * (1 + r * r) * 1.2e-6 + 2 * np.spacing(np.float32(np.abs(want).max()))
        assert np.isfinite(r_px), (name, p)
        e = float(np.linalg.norm(u - want))
        assert e <= tol, (name, p, e, tol)
        worst = max(worst, e / tol)
        checked += 1
    print(f"{name}: {checked} points checked, largest error / tolerance {worst:.3f}")
    assert checked >= (200 if name in NO_FAILURES else 100)


@pytest.mark.parametrize("name", NO_FAILURES)
def test_whole_grid_inverts_at_20_iterations(name):
    """K = (150, 150, 166, 125): every pixel of the 333 x 251 frame has a root, none fails, every residual < 1e-3 px"""
    und, res = fo.undistort(_grid(), fo.K, fo.COEFFS[name], iterations=20)
    print(f"{name}: largest residual {res.max():.3e} px")
    assert np.isfinite(res).all() and np.isfinite(und).all()
    assert res.max() < 1e-3


@pytest.mark.parametrize("name", list(fo.COEFFS))
def test_points_without_a_root_report_inf(name):
    """K = (100, 100, 166, 125): the frame's corners lie past the largest theta_d the model reaches; those points keep (u, v) and
    report +inf (8 % .. 44 % of the grid, depending on the set)"""
    k = fo.COEFFS[name]
    fx, fy, cx, cy = fo.K_WIDE
    pts = _grid()
    und, res = fo.undistort(pts, fo.K_WIDE, k)
    rd = np.hypot((pts[:, 0].astype(np.float64) - cx) / fx, (pts[:, 1].astype(np.float64) - cy) / fy)
    rootless = rd > _largest_theta_d(k) + 1e-5
    print(f"{name}: {rootless.mean() * 100:.1f} % of the grid has no root, {np.isinf(res).mean() * 100:.1f} % reports +inf")
    assert 0.05 < rootless.mean() < 0.5
    assert np.isinf(res[rootless]).all() and (res[rootless] > 0).all()
    bad = ~np.isfinite(res)
    assert np.array_equal(und[bad], pts[bad])
    assert not bad[rd < 0.9].any() and (res[~bad] <= 0.1).all()


def test_iterations_and_threshold():
    pts = _grid(step=9)
    _, res1 = fo.undistort(pts, fo.K, fo.COEFFS["strong"], iterations=1, max_residual_px=1e9)
    _, res20 = fo.undistort(pts, fo.K, fo.COEFFS["strong"], iterations=20, max_residual_px=1e9)
    assert res20.max() < res1.max()
    _, strict = fo.undistort(pts, fo.K, fo.COEFFS["strong"], iterations=1, max_residual_px=0.0)
    assert np.isinf(strict[res1 > 0]).all()


def test_rectify_oracle_agrees_with_the_forward_oracle():
    """a3o_fisheye_rectify's map is the forward model: a view equal to the camera without its lens samples the source where
    a3o_fisheye_distort puts the view's pixel (nearest pixel of a ramp image, within the blend's rounding)"""
    k = fo.COEFFS["mild"]
    ramp = np.tile((np.arange(W) % 251).astype(np.uint8)[None, :], (H, 1))
    out, inside = fo.rectify(ramp, fo.K, k, fill=0, with_inside=True)
    assert inside.all()
    src = fo.distort(_grid(), fo.K, k).reshape(H, W, 2)
    x0 = np.floor(src[..., 0]).astype(int)
    wrap = (x0 % 251) == 250   # (the ramp's jump: the blend there is not between neighbours of the ramp)
    want = (src[..., 0] - x0) + (x0 % 251)
    assert np.abs(out[0, :, :, 0].astype(np.float64) - want)[~wrap].max() <= 0.5 + 1e-3


# ---- constants and the Python surface ----

def test_constants_in_header_ctypes_and_rust():
    from aruco3_amd import _lib

    header = (ROOT / "include" / "aruco3_hip.h").read_text()
    assert re.search(r"\bA3_DIST_FISHEYE\s*=\s*3\b", header)
    assert _lib.DIST_FISHEYE == 3 and _lib.DIST_NONE == 0 and _lib.DIST_RATIONAL == 1
    rust = (ROOT / "integration" / "aruco3_hip.rs").read_text()
    assert re.search(r"pub const A3_DIST_FISHEYE:\s*u32\s*=\s*3;", rust)
    assert re.search(r"pub fn fisheye\(k1: f32, k2: f32, k3: f32, k4: f32\)\s*->\s*Self", rust)
    assert re.search(r"pub struct Distortion \{\s*pub model: u32", rust)
    assert "model: self.model" in rust


def test_python_fisheye_record():
    from aruco3_amd import _lib
    from aruco3_amd.pinhole import Distortion

    d = Distortion.fisheye(-0.02, 0.005, -0.003, 0.0005)
    assert d.model == "fisheye" and (d.k1, d.k2, d.k3, d.k4) == (-0.02, 0.005, -0.003, 0.0005) and (d.p1, d.p2, d.k5, d.k6) == (0, 0, 0, 0)
    rec = d._c()
    assert rec.model == 3 == _lib.DIST_FISHEYE and rec.iterations == 20 and abs(rec.max_residual_px - 0.1) < 1e-7
    assert (rec.k1, rec.k2, rec.k3, rec.k4) == tuple(np.float32(v) for v in (-0.02, 0.005, -0.003, 0.0005))
    assert (rec.p1, rec.p2, rec.k5, rec.k6) == (0.0, 0.0, 0.0, 0.0)
    e = Distortion.from_opencv_fisheye(np.array([[0.08], [-0.03], [0.01], [-0.002]]), iterations=7)
    assert e.model == "fisheye" and e.iterations == 7 and (e.k1, e.k2, e.k3, e.k4) == (0.08, -0.03, 0.01, -0.002)
    for n in (3, 5, 8):
        with pytest.raises(ValueError):
            Distortion.from_opencv_fisheye([0.0] * n)
    # the rational record is what it was
    r = Distortion(0.1, 0.2, 0.3, 0.4, 0.5)
    assert r.model == "rational" and r._c().model == _lib.DIST_RATIONAL
    assert Distortion.from_opencv([0.1, 0.2, 0.3, 0.4]).model == "rational"


@pytest.mark.parametrize("field", ["p1", "p2", "k5", "k6"])
def test_fisheye_with_a_rational_coefficient_is_refused(field):
    from aruco3_amd.pinhole import Distortion

    with pytest.raises(ValueError):
        Distortion(k1=0.1, model="fisheye", **{field: 1e-3})
    d = Distortion.fisheye(0.1)
    setattr(d, field, 1e-3)   # (set after construction)
    with pytest.raises(ValueError):
        d._c()
    with pytest.raises(ValueError):
        d.distort_normalized([[0.1, 0.2]])
    with pytest.raises(ValueError):
        Distortion(model="equidistant")


def test_flattening_a_fisheye_lens_to_rational_numbers_is_refused():
    """the rig and map solves and the calibration's guess know the rational model only: a fisheye lens is refused with the route"""
    from aruco3_amd import calibration, markermap, rig
    from aruco3_amd.pinhole import CameraIntrinsics, Distortion

    cam = CameraIntrinsics(640, 480, 300.0, 300.0, distortion=Distortion.fisheye(*fo.COEFFS["mild"]))
    for fn in (rig.camera_params, markermap.camera_params):
        with pytest.raises(ValueError, match="rectify"):
            fn(cam)
    obj = [np.array([[0, 0], [1, 0], [1, 1], [0, 1], [2, 0], [2, 1]], np.float32)]
    img = [np.array([[10, 10], [50, 10], [50, 50], [10, 50], [90, 10], [90, 50]], np.float32)]
    with pytest.raises(ValueError, match="rectify"):
        calibration.calibrate_camera(obj, img, (640, 480), guess=cam)
    # a rational lens still flattens as before
    rat = CameraIntrinsics(640, 480, 300.0, 300.0, distortion=Distortion(0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8))
    assert rig.camera_params(rat).tolist() == [300.0, 300.0, 320.0, 240.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]
    assert rig.camera_params(CameraIntrinsics(640, 480, 300.0, 300.0)).tolist() == [300.0, 300.0, 320.0, 240.0] + [0.0] * 8
