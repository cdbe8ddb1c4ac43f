"""Camera calibration on the CPU (tests/calib_oracle.c, the restatement k_calibrate is held to): recovery of known cameras, the flags,
the covariance against the spread of noisy solves, an independent least-squares cross-check, degenerate input, and the struct layouts
across the C header, ctypes and the Rust mirror."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

from aruco3_amd import _lib as A
from tests import calib_oracle as co
from tests import calib_util as cu

ROOT = Path(__file__).resolve().parent.parent


def _solve(p, flags=0, guess=None, max_iterations=0):
    res, views = co.calibrate(cu.one_camera(p, flags, guess, max_iterations), p["offsets"], p["obj"], p["img"])
    return res[0], [views[i] for i in range(len(p["offsets"]) - 1)]


def _distortion_profile(a, size):
    """the lens of intrinsics a (12) as the pixel displacement it causes over a grid of the image (for coefficient sets that are not
    unique, as the rational model's are)"""
    fx, fy, cx, cy = a[:4]
    u, v = np.meshgrid(np.linspace(0, size[0] - 1, 17), np.linspace(0, size[1] - 1, 11))
    x, y = ((u - cx) / fx).ravel(), ((v - cy) / fy).ravel()
    k1, k2, p1, p2, k3, k4, k5, k6 = a[4:]
    r2 = x * x + y * y
    rad = (1 + ((k3 * r2 + k2) * r2 + k1) * r2) / (1 + ((k6 * r2 + k5) * r2 + k4) * r2)
    xd = x * rad + (2 * p1 * x * y + p2 * (r2 + 2 * x * x))
    yd = y * rad + (p1 * (r2 + 2 * y * y) + 2 * p2 * x * y)
    return np.stack([(xd - x) * fx, (yd - y) * fy], axis=1)


@pytest.mark.parametrize("kind", ["charuco", "grid"])
def test_noise_free_recovery_webcam_lens(kind):
    p = cu.problem(kind, 25, seed=3, coeffs=cu.WEBCAM5)
    r, views = _solve(p)
    assert r.status == A.CALIB_OK and r.views_used == 25 and r.points_used == p["offsets"][-1]
    got = cu.params(r)
    assert np.all(np.abs(got[:4] - p["truth"][:4]) <= 1e-6 * np.abs(p["truth"][:4])), got[:4] - p["truth"][:4]
    assert np.all(np.abs(got[4:9] - p["truth"][4:9]) <= 1e-5), got[4:9] - p["truth"][4:9]
    assert np.all(got[9:] == 0.0)                       # no RATIONAL_MODEL: k4 .. k6 fixed at 0
    assert r.rms_px < 1e-3
    for v, (R, t) in zip(views, p["poses"]):
        assert v.status == A.CALIB_VIEW_USED and v.rms_px < 1e-3
        assert cu.rotation_error_deg(np.array(v.rotation).reshape(3, 3), R) < 0.05   # (float32 records; acos near 1)
    # the result is what the pose calls and a3_set_distortion take, in float
    assert r.intrinsics.focal_x == np.float32(r.fx) and r.distortion.model == A.DIST_RATIONAL and r.distortion.k1 == np.float32(r.dist[0])


@pytest.mark.parametrize("kind", ["charuco", "grid"])
def test_noise_free_recovery_rational_lens(kind):
    """k1 .. k6 of the rational model trade off against each other (numerator against denominator), so the coefficients are not unique
    from a few hundred points: the intrinsics and the lens's displacement field are what is recovered"""
    p = cu.problem(kind, 25, seed=4, coeffs=cu.RATIONAL)
    r, _ = _solve(p, A.CALIB_RATIONAL_MODEL)
    assert r.status == A.CALIB_OK
    got = cu.params(r)
    assert np.all(np.abs(got[:4] - p["truth"][:4]) <= 1e-6 * np.abs(p["truth"][:4])), got[:4] - p["truth"][:4]
    # (measured: at most 0.008 px, at the image corners, outside every view's points)
    assert np.max(np.abs(_distortion_profile(got, p["size"]) - _distortion_profile(p["truth"], p["size"]))) < 0.02
    assert np.all(np.abs(got[6:8] - p["truth"][6:8]) <= 1e-5)
    assert r.rms_px < 1e-3


def test_flags():
    p = cu.problem("charuco", 25, seed=5, coeffs=cu.WEBCAM)
    W, H = p["size"]
    r, _ = _solve(p, A.CALIB_ZERO_TANGENT_DIST)
    assert r.dist[2] == 0.0 and r.dist[3] == 0.0 and r.std_dev[6] == 0.0 and r.std_dev[7] == 0.0
    r, _ = _solve(p, A.CALIB_FIX_K3)
    assert r.dist[4] == 0.0 and r.std_dev[8] == 0.0
    r, _ = _solve(p, A.CALIB_FIX_PRINCIPAL_POINT)
    assert r.cx == (W - 1) * 0.5 and r.cy == (H - 1) * 0.5 and r.std_dev[2] == 0.0
    guess = list(p["truth"])
    guess[4] = -0.25
    r, _ = _solve(p, A.CALIB_FIX_PRINCIPAL_POINT | A.CALIB_FIX_K3 | A.CALIB_USE_INTRINSIC_GUESS, guess=[g * 1.0 for g in guess])
    assert r.cx == np.float32(guess[2]) and r.cy == np.float32(guess[3]) and r.dist[4] == np.float32(guess[8])
    # a guess 20 % off reaches the optimum of the free start
    free, _ = _solve(p)
    off = [v * 1.2 for v in p["truth"][:4]] + [0.0] * 8
    r, _ = _solve(p, A.CALIB_USE_INTRINSIC_GUESS, guess=off)
    assert r.status == A.CALIB_OK
    np.testing.assert_allclose(cu.params(r)[:4], cu.params(free)[:4], rtol=1e-7)
    np.testing.assert_allclose(cu.params(r)[4:], cu.params(free)[4:], atol=1e-6)
    # a run cut short stops at max_iterations
    r, _ = _solve(p, max_iterations=2)
    assert r.iterations == 2 and r.converged == 0


def test_std_dev_covers_the_truth_under_noise():
    hits, total = 0, 0
    for seed in range(6):
        p = cu.problem("grid", 40, seed=100 + seed, coeffs=cu.WEBCAM, noise=0.2)
        r, _ = _solve(p, A.CALIB_FIX_K3)
        assert r.status == A.CALIB_OK and 0.25 < r.rms_px < 0.31   # (sqrt(2) sigma: rms_px sums both coordinates)
        got, sd = cu.params(r), np.array(r.std_dev)
        free = sd > 0
        assert np.all(np.isfinite(sd[free]))
        ok = np.abs(got - p["truth"])[free] <= 4 * sd[free]
        hits += int(ok.sum())
        total += int(free.sum())
        assert ok.all(), (seed, (got - p["truth"])[free] / sd[free])
    assert total == 6 * 8 and hits == total


def test_independent_least_squares_reaches_the_same_optimum():
    """scipy.optimize.least_squares on the same residuals, poses as Rodrigues vectors, started from the oracle's answer perturbed"""
    opt = pytest.importorskip("scipy.optimize")
    from scipy.spatial.transform import Rotation

    p = cu.problem("grid", 12, seed=7, coeffs=cu.WEBCAM, noise=0.2)
    r, views = _solve(p)
    a0 = cu.params(r)
    n_v = len(views)
    obj = p["obj"].astype(np.float64)
    img = p["img"].astype(np.float64)
    off = p["offsets"]
    free = [0, 1, 2, 3, 4, 5, 6, 7, 8]

    def residuals(x):
        a = np.zeros(12)
        a[free] = x[:9]
        out = []
        for j in range(n_v):
            rv, t = x[9 + 6 * j: 12 + 6 * j], x[12 + 6 * j: 15 + 6 * j]
            uv = co.project(a, Rotation.from_rotvec(rv).as_matrix(), t, obj[off[j]:off[j + 1]])
            out.append((uv - img[off[j]:off[j + 1]]).ravel())
        return np.concatenate(out)

    x0 = [a0[free] * (1 + 1e-3)]
    for v in views:
        R = np.array(v.rotation, np.float64).reshape(3, 3)
        x0 += [Rotation.from_matrix(R).as_rotvec() + 1e-3, np.array(v.translation, np.float64) * (1 + 1e-3)]
    sol = opt.least_squares(residuals, np.concatenate(x0), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=20000)
    got = sol.x[:9]
    np.testing.assert_allclose(a0[:4], got[:4], rtol=1e-6)
    np.testing.assert_allclose(a0[4:9], got[4:], atol=1e-5)
    rms = math.sqrt(float(np.sum(sol.fun ** 2)) / off[-1])
    assert abs(rms - r.rms_px) <= 1e-9 * r.rms_px


def test_degenerate_input_gives_statuses_and_no_nan():
    p = cu.problem("grid", 6, seed=8, coeffs=cu.WEBCAM)
    obj, img, offs = list(np.split(p["obj"], p["offsets"][1:-1])), list(np.split(p["img"], p["offsets"][1:-1])), None
    obj[1], img[1] = obj[1][:3], img[1][:3]                          # 3 points
    line = np.array([[x, 0.0] for x in range(8)], np.float32)        # 8 collinear points
    obj[2], img[2] = line, np.stack([100.0 + 10 * line[:, 0], 200.0 + 3 * line[:, 0]], 1).astype(np.float32)
    offs = np.concatenate([[0], np.cumsum([len(o) for o in obj])]).astype(np.uint32)
    res, views = co.calibrate(cu.cameras([dict(size=p["size"], first_view=0, n_views=6)]), offs, np.concatenate(obj), np.concatenate(img))
    st = [views[i].status for i in range(6)]
    assert st == [A.CALIB_VIEW_USED, A.CALIB_VIEW_TOO_FEW_POINTS, A.CALIB_VIEW_DEGENERATE] + [A.CALIB_VIEW_USED] * 3
    assert res[0].status == A.CALIB_OK and res[0].views_used == 4
    assert views[1].rms_px == 0.0 and views[2].rotation[0] == 0.0
    # fronto-parallel views only: the orthogonality equations say nothing about the focal lengths
    pts = cu.target_points("grid")
    a = list(cu.K720) + [0.0] * 8
    obj, img = [], []
    for k in range(5):
        t = np.array([-60.0 + 10 * k, 50.0 - 5 * k, 500.0 + 30 * k])
        obj.append(pts.astype(np.float32))
        img.append(co.project(a, np.diag([1.0, -1.0, -1.0]), t, pts).astype(np.float32))
    offs = np.concatenate([[0], np.cumsum([len(o) for o in obj])]).astype(np.uint32)
    res, views = co.calibrate(cu.cameras([dict(size=(1280, 720), first_view=0, n_views=5)]), offs, np.concatenate(obj), np.concatenate(img))
    assert res[0].status == A.CALIB_NO_INIT and res[0].fx == 0.0 and res[0].rms_px == 0.0
    # too few observations for the free parameters
    res, views = co.calibrate(cu.cameras([dict(size=(1280, 720), first_view=0, n_views=1)]), [0, 4], obj[0][:4], img[0][:4])
    assert res[0].status == A.CALIB_TOO_FEW and views[0].status == A.CALIB_VIEW_USED
    for r in (res[0],):
        vals = [r.fx, r.fy, r.cx, r.cy, r.rms_px] + list(r.dist) + list(r.std_dev)
        assert not any(math.isnan(v) for v in vals)


def test_several_cameras_equal_each_alone():
    ps = [cu.problem("charuco", 9, seed=20 + k, coeffs=cu.WEBCAM) for k in range(3)]
    obj = np.concatenate([p["obj"] for p in ps])
    img = np.concatenate([p["img"] for p in ps])
    offs = np.concatenate([[0]] + [p["offsets"][1:] + sum(q["offsets"][-1] for q in ps[:k]) for k, p in enumerate(ps)]).astype(np.uint32)
    specs = [dict(size=p["size"], first_view=9 * k, n_views=9, flags=[0, A.CALIB_FIX_K3, A.CALIB_ZERO_TANGENT_DIST][k]) for k, p in enumerate(ps)]
    res, views = co.calibrate(cu.cameras(specs), offs, obj, img)
    for k, p in enumerate(ps):
        alone, _ = _solve(p, specs[k]["flags"])
        assert bytes(res[k]) == bytes(alone)


def test_host_reprojection_matches_the_contract_model():
    """calibration.reproject (the outlier passes' forward model, numpy) against the oracle's"""
    from aruco3_amd.calibration import reproject

    pts = cu.target_points("grid")
    rng = np.random.default_rng(3)
    for coeffs in (cu.WEBCAM5, cu.RATIONAL):
        a = list(cu.K720) + list(coeffs)
        for R, t in cu.random_poses(pts, 4, rng, coeffs=coeffs):
            np.testing.assert_allclose(reproject(a, R, t, pts), co.project(a, R, t, pts), rtol=0, atol=1e-9)


def test_layouts_match_across_c_ctypes_and_rust():
    import ctypes as C

    lay = co.layout()
    py = [C.sizeof(A.CalibCamera), A.CalibCamera.guess.offset, A.CalibCamera.guess_distortion.offset, C.sizeof(A.CalibResult),
          A.CalibResult.fx.offset, A.CalibResult.dist.offset, A.CalibResult.std_dev.offset, A.CalibResult.rms_px.offset,
          A.CalibResult.intrinsics.offset, A.CalibResult.distortion.offset, C.sizeof(A.CalibView), A.CalibView.rms_px.offset,
          A.CalibView.rotation.offset, A.CalibView.translation.offset]
    assert lay == py == [92, 24, 48, 296, 24, 56, 120, 216, 224, 248, 60, 8, 12, 48]
    text = re.sub(r"//[^\n]*", "", (ROOT / "integration" / "aruco3_hip.rs").read_text())
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "aruco3_hip.h").read_text(), flags=re.S)
    for c_name, r_name in (("a3_calib_camera", "A3CalibCamera"), ("a3_calib_result", "A3CalibResult"), ("a3_calib_view", "A3CalibView")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (c_name, c_name), header, flags=re.S).group(1)
        c_fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                for n in decl.split(None, 1)[1].split(","):
                    c_fields.append(re.sub(r"\[.*?\]", "", n).split()[-1])
        m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^\]]*\)\]\s*)?pub struct %s \{(.*?)\}" % r_name, text, flags=re.S)
        assert m and re.findall(r"pub\s+([a-z0-9_]+)\s*:", m.group(1)) == c_fields, c_name
