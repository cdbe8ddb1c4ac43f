"""Fisheye camera calibration on the CPU (tests/fisheye_calib_oracle.c, the restatement k_calibrate_fisheye is held to): the contract's
arctangent, the Jacobian, recovery of known cameras, the covariance against noisy solves, an independent least-squares cross-check, the
flags, the start's kept-point rule and the statuses, the struct layouts, and the Python surface (its device call replaced by the
oracle, which computes the same bytes)."""
import ctypes as C
import math
import re
from pathlib import Path

import numpy as np
import pytest

from aruco3_amd import _lib as A
from tests import calib_oracle as co
from tests import fisheye_calib_oracle as fco
from tests import fisheye_calib_util as fu

ROOT = Path(__file__).resolve().parent.parent
START_720 = [1280 / 3.141592653589793] * 2 + [639.5, 359.5, 0.0, 0.0, 0.0, 0.0]   # the start without a guess at 1280 x 720


def _solve(p, flags=0, guess=None, max_iterations=0):
    res, views = fco.calibrate(fu.one_camera(p, flags, guess, max_iterations), p["offsets"], p["obj"], p["img"])
    return res[0], [views[i] for i in range(len(p["offsets"]) - 1)]


def test_a64_against_the_library_arctangent():
    """the issue's comparison: 200 000 uniform values on [0, 5] and 200 000 log-uniform ones on [1e-8, 1e6]; measured 1.0 ulp at worst,
    asserted 2 (one more for another libm)"""
    rng = np.random.default_rng(0)
    xs = np.concatenate([rng.uniform(0.0, 5.0, 200000), np.exp(rng.uniform(math.log(1e-8), math.log(1e6), 200000))])
    f = fco.lib().a3o_a64
    worst = max(abs(f(x) - math.atan(x)) / math.ulp(math.atan(x)) for x in xs.tolist())
    print(f"A64 against math.atan: {worst} ulp at worst")
    assert worst <= 2.0
    assert fco.a64(0.0) == 0.0 and fco.a64(0.66) == math.atan(0.66) and abs(fco.a64(1e300) - math.pi / 2) <= math.ulp(math.pi / 2)


def test_jacobian_columns_against_central_differences():
    """every analytic column against central differences of the oracle's own residual, at points from the axis out to 70 degrees"""
    def cay(w):   # the contract's Cayley map: I + 2 / (1 + w.w) ([w]x + w w^T - w.w I)
        W = np.array([[0.0, -w[2], w[1]], [w[2], 0.0, -w[0]], [-w[1], w[0], 0.0]])
        return np.eye(3) + 2.0 / (1.0 + w @ w) * (W + np.outer(w, w) - (w @ w) * np.eye(3))

    rng = np.random.default_rng(1)
    pts = fu.target_points("charuco")
    worst = 0.0
    for coeffs in (fu.MILD, fu.STRONG):
        a = np.array(list(fu.K420) + list(coeffs))
        for R, t in fu.random_poses(pts, 6, rng, coeffs=coeffs):
            for X, Y in pts[::5]:
                au, av = fco.row(a, R, t, X, Y)
                res = lambda a_, R_, t_: np.array([r[14] for r in fco.row(a_, R_, t_, X, Y)])   # noqa: E731
                for c in range(14):
                    if c < 8:
                        h = 1e-6 * max(1.0, abs(a[c])) if c < 4 else 1e-6
                        d = np.zeros(8)
                        d[c] = h
                        num = (res(a + d, R, t) - res(a - d, R, t)) / (2 * h)
                    elif c < 11:   # w of R <- cay(w) R
                        h = 1e-6
                        w = np.zeros(3)
                        w[c - 8] = h
                        num = (res(a, cay(w) @ R, t) - res(a, cay(-w) @ R, t)) / (2 * h)
                    else:
                        h = 1e-5 * np.linalg.norm(t)
                        d = np.zeros(3)
                        d[c - 11] = h
                        num = (res(a, R, t + d) - res(a, R, t - d)) / (2 * h)
                    ana = np.array([au[c], av[c]])
                    scale = max(1.0, float(np.max(np.abs(ana))))
                    worst = max(worst, float(np.max(np.abs(num - ana))) / scale)
    print(f"analytic against central differences: {worst:.2e} relative at worst")
    assert worst < 1e-5   # (central differences of step h: truncation h^2 ~ 1e-12 and rounding eps / h ~ 1e-10 on values of order 1e2 .. 1e3)


@pytest.mark.parametrize("kind", ["charuco", "grid"])
@pytest.mark.parametrize("lens", ["MILD", "STRONG"])
def test_noise_free_recovery(kind, lens):
    """tests/test_oracle_calib.py's bounds.  Measured with these four problems: focal lengths and principal point within 1.9e-7
    relative, coefficients within 7.0e-7, rms 1.9e-5 px (the f32 rounding of the image points) -- each 3 x inside its bound and more"""
    p = fu.problem(kind, 25, seed=3, coeffs=getattr(fu, lens))
    r, views = _solve(p)
    assert r.status == A.CALIB_OK and r.views_used == 25 and r.points_used == p["offsets"][-1]
    got = fu.params(r)
    print(f"{kind} {lens}: {got - p['truth']} rms {r.rms_px:.2e} field {fu.field_difference_px(got, p['truth']):.2e} px")
    assert np.all(np.abs(got[:4] - p["truth"][:4]) <= 1e-6 * np.abs(p["truth"][:4])), got[:4] - p["truth"][:4]
    assert np.all(np.abs(got[4:] - p["truth"][4:]) <= 1e-5), got[4:] - p["truth"][4:]
    assert fu.field_difference_px(got, p["truth"]) < 0.02
    assert r.rms_px < 1e-3
    for v, (R, t) in zip(views, p["poses"]):
        assert v.status == A.CALIB_VIEW_USED and v.rms_px < 1e-3
        assert fu.rotation_error_deg(np.array(v.rotation).reshape(3, 3), R) < 0.05   # (float32 records; acos near 1)
    # the record: a3_distortion's field order, and what a3_set_distortion / a3_rectify_frames take, in float
    assert r.dist[2] == r.dist[3] == r.dist[6] == r.dist[7] == 0.0 and all(r.std_dev[i] == 0.0 for i in (6, 7, 10, 11))
    d = r.distortion
    assert r.intrinsics.focal_x == np.float32(r.fx) and (r.intrinsics.image_width, r.intrinsics.image_height) == p["size"]
    assert d.model == A.DIST_FISHEYE and d.iterations == 20 and d.max_residual_px == np.float32(0.1)
    assert (d.k1, d.k2, d.k3, d.k4) == tuple(np.float32(r.dist[i]) for i in (0, 1, 4, 5)) and d.p1 == d.p2 == d.k5 == d.k6 == 0.0


@pytest.mark.parametrize("focal", [300.0, 600.0, 900.0])
def test_recovery_from_the_fixed_start_at_other_focal_lengths(focal):
    """the start is max(W, H) / pi = 407 px whatever the lens: cameras far from it are still reached"""
    p = fu.problem("grid", 25, seed=1, K=(focal, focal + 2.0, 640.0, 360.0))
    r, _ = _solve(p)
    assert r.status == A.CALIB_OK and r.views_used >= 24
    got = fu.params(r)
    assert np.all(np.abs(got[:4] - p["truth"][:4]) <= 1e-6 * np.abs(p["truth"][:4])), got[:4] - p["truth"][:4]
    assert fu.field_difference_px(got, p["truth"]) < 0.02 and r.rms_px < 1e-3


@pytest.mark.parametrize("lens", ["MILD", "STRONG"])
def test_std_dev_covers_the_truth_under_noise(lens):
    for seed in range(6):
        p = fu.problem("grid", 40, seed=100 + seed, coeffs=getattr(fu, lens), noise=0.2)
        r, _ = _solve(p)
        assert r.status == A.CALIB_OK and 0.25 < r.rms_px < 0.31   # (sqrt(2) sigma: rms_px sums both coordinates)
        got, sd = fu.params(r), fu.std_devs(r)
        assert np.all(np.isfinite(sd)) and np.all(sd > 0)
        assert np.all(np.abs(got - p["truth"]) <= 4 * sd), (seed, (got - p["truth"]) / sd)   # (measured: 2.4 at most)


def test_independent_least_squares_reaches_the_same_optimum():
    """scipy.optimize.least_squares on the same residuals, poses as Rodrigues vectors, started from the oracle's answer perturbed"""
    opt = pytest.importorskip("scipy.optimize")
    from scipy.spatial.transform import Rotation

    p = fu.problem("grid", 12, seed=7, noise=0.2)
    r, views = _solve(p)
    a0 = fu.params(r)
    obj, img, off = p["obj"].astype(np.float64), p["img"].astype(np.float64), p["offsets"]

    def residuals(x):
        out = []
        for j in range(len(views)):
            rv, t = x[8 + 6 * j: 11 + 6 * j], x[11 + 6 * j: 14 + 6 * j]
            uv = fco.project(x[:8], Rotation.from_rotvec(rv).as_matrix(), t, obj[off[j]:off[j + 1]])
            out.append((uv - img[off[j]:off[j + 1]]).ravel())
        return np.concatenate(out)

    x0 = [a0 * (1 + 1e-3)]
    for v in views:
        R = np.array(v.rotation, np.float64).reshape(3, 3)
        x0 += [Rotation.from_matrix(R).as_rotvec() + 1e-3, np.array(v.translation, np.float64) * (1 + 1e-3)]
    sol = opt.least_squares(residuals, np.concatenate(x0), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=20000)
    # The joint LM stops at a relative cost decrease below A3_CALIB_REL_TOL = 1e-10.  Near the optimum the cost is c (1 + z.z / (2 dof))
    # for a parameter offset of z deviations (sigma2 = c / dof), so a step that lowers it by less than 1e-10 c may leave
    # |z| ~ sqrt(2e-10 dof) = 8e-4 here (dof = 2 * 1680 - 8 - 72); k2 .. k4, barely told apart by 12 views, have deviations of 1e-3 and
    # more, so a fixed 1e-5 on them would ask for more than the stopping rule gives.  Asserted: 1e-2 deviations on every parameter.
    z = np.abs(a0 - sol.x[:8]) / fu.std_devs(r)
    print(f"oracle against scipy, in deviations: {z}")
    assert np.all(z <= 1e-2), z
    np.testing.assert_allclose(a0[:4], sol.x[:4], rtol=1e-6)
    rms = math.sqrt(float(np.sum(sol.fun ** 2)) / off[-1])
    assert abs(rms - r.rms_px) <= 1e-9 * r.rms_px


def test_flags_guess_and_iteration_cap():
    p = fu.problem("charuco", 25, seed=5, coeffs=fu.STRONG)
    W, H = p["size"]
    free, _ = _solve(p)
    for bit, k in ((A.FISHEYE_FIX_K1, 4), (A.FISHEYE_FIX_K2, 5), (A.FISHEYE_FIX_K3, 8), (A.FISHEYE_FIX_K4, 9)):
        r, _ = _solve(p, bit)
        assert r.status == A.CALIB_OK and r.dist[k - 4] == 0.0 and r.std_dev[k] == 0.0
        assert sum(1 for s in r.std_dev if s > 0) == 7
    r, _ = _solve(p, A.FISHEYE_FIX_PRINCIPAL_POINT)
    assert r.cx == (W - 1) * 0.5 and r.cy == (H - 1) * 0.5 and r.std_dev[2] == 0.0 and r.std_dev[3] == 0.0
    # fixed parameters stay at the guess's values
    guess = list(p["truth"])
    fixed = A.FISHEYE_FIX_PRINCIPAL_POINT | A.FISHEYE_FIX_K3 | A.FISHEYE_FIX_K4 | A.FISHEYE_USE_INTRINSIC_GUESS
    r, _ = _solve(p, fixed, guess=guess)
    assert r.cx == np.float32(guess[2]) and r.cy == np.float32(guess[3]) and r.dist[4] == np.float32(guess[6]) and r.dist[5] == np.float32(guess[7])
    assert r.status == A.CALIB_OK and abs(r.fx - guess[0]) < 1e-3 and abs(r.dist[0] - guess[4]) < 1e-5
    # a guess 20 % off reaches the optimum of the free start
    off = [v * 1.2 for v in p["truth"][:4]] + [0.0] * 4
    r, _ = _solve(p, A.FISHEYE_USE_INTRINSIC_GUESS, guess=off)
    assert r.status == A.CALIB_OK
    np.testing.assert_allclose(fu.params(r)[:4], fu.params(free)[:4], rtol=1e-7)
    np.testing.assert_allclose(fu.params(r)[4:], fu.params(free)[4:], atol=1e-6)
    # a run cut short stops at max_iterations
    r, _ = _solve(p, max_iterations=2)
    assert r.iterations == 2 and r.converged == 0


def _far_views(n, off_axis, seed, want):
    """n ChArUco views whose centre lies `off_axis` degrees off the axis and of whose 24 points the start keeps `want(kept)`"""
    rng = np.random.default_rng(seed)
    pts = fu.target_points("charuco")
    a = list(fu.K420) + list(fu.MILD)
    out = []
    while len(out) < n:
        (R, t), = fu.random_poses(pts, 1, rng, off_axis=off_axis, extent_deg=(5.0, 7.0))
        uv = fco.project(a, R, t, pts).astype(np.float32)
        kept, _ = fco.start_points(START_720, uv)
        if want(int(kept.sum())):
            out.append((pts.astype(np.float32), uv))
    return out


def bad_view_mix():
    """six good views with, in their midst: a 3-point view, a collinear one, a view the start keeps fewer than 4 points of (beyond
    A3_FISHEYE_START_MAX_R), and one it keeps most but not all points of -> (obj list, img list, expected view statuses)"""
    p = fu.problem("grid", 6, seed=8)
    obj, img = list(np.split(p["obj"], p["offsets"][1:-1])), list(np.split(p["img"], p["offsets"][1:-1]))
    obj[1], img[1] = obj[1][:3], img[1][:3]
    line = np.array([[x, 0.0] for x in range(8)], np.float32)
    obj[2], img[2] = line, np.stack([600.0 + 10 * line[:, 0], 300.0 + 3 * line[:, 0]], 1).astype(np.float32)
    obj[3], img[3] = _far_views(1, (80.0, 84.0), 5, lambda k: k < 4)[0]
    obj[4], img[4] = _far_views(1, (72.0, 76.0), 6, lambda k: 4 <= k < 24)[0]
    st = [A.CALIB_VIEW_USED, A.CALIB_VIEW_TOO_FEW_POINTS, A.CALIB_VIEW_DEGENERATE, A.CALIB_VIEW_DEGENERATE, A.CALIB_VIEW_USED, A.CALIB_VIEW_USED]
    return obj, img, st, p["size"]


def test_statuses_and_no_nan():
    obj, img, want, size = bad_view_mix()
    offs = np.concatenate([[0], np.cumsum([len(o) for o in obj])]).astype(np.uint32)
    res, views = fco.calibrate(fu.cameras([dict(size=size, first_view=0, n_views=6)]), offs, np.concatenate(obj), np.concatenate(img))
    assert [views[i].status for i in range(6)] == want
    r = res[0]
    # the view with a few points past START_MAX_R is USED with all its points counted; the one mostly past it is left out, harmlessly
    assert r.status == A.CALIB_OK and r.views_used == 3 and r.points_used == 140 + 24 + 140 and views[4].points == 24
    assert views[1].rms_px == 0.0 and views[2].rotation[0] == 0.0 and views[3].rotation[0] == 0.0 and views[3].points == 24
    assert r.rms_px < 1e-3 and views[4].rms_px < 1e-3
    assert abs(r.fx - fu.K420[0]) < 1e-2 and abs(r.cy - fu.K420[3]) < 1e-2
    # too few observations for the free parameters; no view at all
    res1, views1 = fco.calibrate(fu.cameras([dict(size=size, first_view=0, n_views=1)]), [0, 4], obj[0][:4], img[0][:4])
    assert res1[0].status == A.CALIB_TOO_FEW and views1[0].status == A.CALIB_VIEW_USED
    res2, views2 = fco.calibrate(fu.cameras([dict(size=size, first_view=0, n_views=1)]), [0, 24], obj[3], img[3])
    assert res2[0].status == A.CALIB_TOO_FEW and views2[0].status == A.CALIB_VIEW_DEGENERATE and res2[0].views_used == 0
    for r in (res[0], res1[0], res2[0]):
        vals = [r.fx, r.fy, r.cx, r.cy, r.rms_px] + list(r.dist) + list(r.std_dev)
        assert not any(math.isnan(v) for v in vals)
    for r in (res1[0], res2[0]):
        assert bytes(r)[12:] == bytes(len(bytes(r)) - 12)   # status, views_used, points_used; zeros elsewhere
    for v in list(views)[:6] + [views1[0], views2[0]]:
        assert not any(math.isnan(x) for x in [v.rms_px] + list(v.rotation) + list(v.translation))


def test_several_cameras_equal_each_alone():
    ps = [fu.problem("charuco", 9, seed=20 + k, coeffs=[fu.MILD, fu.STRONG, fu.MILD][k]) for k in range(3)]
    obj = np.concatenate([p["obj"] for p in ps])
    img = np.concatenate([p["img"] for p in ps])
    offs = np.concatenate([[0]] + [p["offsets"][1:] + sum(q["offsets"][-1] for q in ps[:k]) for k, p in enumerate(ps)]).astype(np.uint32)
    flags = [0, A.FISHEYE_FIX_K4, A.FISHEYE_FIX_PRINCIPAL_POINT | A.FISHEYE_FIX_K3]
    specs = [dict(size=p["size"], first_view=9 * k, n_views=9, flags=flags[k]) for k, p in enumerate(ps)]
    res, views = fco.calibrate(fu.cameras(specs), offs, obj, img)
    for k, p in enumerate(ps):
        alone, aviews = _solve(p, flags[k])
        assert alone.status == A.CALIB_OK and bytes(res[k]) == bytes(alone)
        assert all(bytes(views[9 * k + j]) == bytes(aviews[j]) for j in range(9))


def test_layouts_match_across_c_ctypes_and_rust():
    lay = fco.layout()
    py = [C.sizeof(A.CalibCamera), A.CalibCamera.guess.offset, A.CalibCamera.guess_distortion.offset, C.sizeof(A.CalibResult),
          A.CalibResult.fx.offset, A.CalibResult.dist.offset, A.CalibResult.std_dev.offset, A.CalibResult.rms_px.offset,
          A.CalibResult.intrinsics.offset, A.CalibResult.distortion.offset, C.sizeof(A.CalibView), A.CalibView.rms_px.offset,
          A.CalibView.rotation.offset, A.CalibView.translation.offset]
    assert lay == py == [92, 24, 48, 296, 24, 56, 120, 216, 224, 248, 60, 8, 12, 48]
    text = re.sub(r"//[^\n]*", "", (ROOT / "integration" / "aruco3_hip.rs").read_text())
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "aruco3_hip.h").read_text(), flags=re.S)
    assert re.search(r"#define A3_ABI_VERSION 5\b", header)
    # the flags, by name and value, in the header, the ctypes binding and the Rust mirror
    enum = dict(re.findall(r"(A3_FISHEYE_[A-Z0-9_]+) = (\d+)", header))
    assert enum == {"A3_FISHEYE_FIX_PRINCIPAL_POINT": "1", "A3_FISHEYE_FIX_K1": "2", "A3_FISHEYE_FIX_K2": "4", "A3_FISHEYE_FIX_K3": "8",
                    "A3_FISHEYE_FIX_K4": "16", "A3_FISHEYE_USE_INTRINSIC_GUESS": "32"}
    for name, value in enum.items():
        assert getattr(A, name[3:]) == int(value)
        assert re.search(r"pub const %s: u32 = %s;" % (name, value), text), name
    assert re.search(r"#define A3_FISHEYE_START_MAX_R 4\.0\b", header) and A.FISHEYE_START_MAX_R == 4.0
    m = re.search(r"pub fn a3_calibrate_fisheye_cameras\((.*?)\)\s*->\s*c_int;", text, flags=re.S)
    ref = re.search(r"pub fn a3_calibrate_cameras\((.*?)\)\s*->\s*c_int;", text, flags=re.S)
    assert m and re.sub(r"\s+", " ", m.group(1)) == re.sub(r"\s+", " ", ref.group(1))   # the same records, the same arguments
    assert "a3_calibrate_fisheye_cameras" in A.SYMBOLS


# ---- the Python surface, its device call replaced by the oracles (which compute the device's bytes) ----

@pytest.fixture
def on_oracle(monkeypatch):
    from aruco3_amd import calibration

    calls = []

    def fake(cams, offsets, obj, img, fisheye=False):
        calls.append("fisheye" if fisheye else "rational")
        return (fco if fisheye else co).calibrate(cams, offsets, obj, img)

    monkeypatch.setattr(calibration, "_calibrate", fake)
    return calls


def _views_of(p):
    return list(np.split(p["obj"], p["offsets"][1:-1])), list(np.split(p["img"], p["offsets"][1:-1]))


def test_python_fisheye_calibration(on_oracle):
    import aruco3_amd
    from aruco3_amd import CameraIntrinsics, Distortion
    from aruco3_amd.calibration import Calibration, calibrate_camera_fisheye, calibrate_cameras_fisheye, reproject

    assert aruco3_amd.calibrate_camera_fisheye is calibrate_camera_fisheye and aruco3_amd.calibrate_cameras_fisheye is calibrate_cameras_fisheye
    p = fu.problem("grid", 12, seed=30, coeffs=fu.STRONG)
    obj, img = _views_of(p)
    cal = calibrate_camera_fisheye(obj, img, p["size"])
    assert isinstance(cal, Calibration) and cal.ok and cal.model == "fisheye" and on_oracle == ["fisheye"]
    np.testing.assert_allclose(cal.distortion_coeffs, fu.STRONG, atol=1e-5)
    assert cal.distortion_coeffs.shape == (4,) and cal.params.shape == (12,) and np.all(cal.params[[6, 7, 10, 11]] == 0.0)
    np.testing.assert_allclose(cal.params[:4], fu.K420, rtol=1e-6)
    d = cal.intrinsics.distortion
    assert isinstance(d, Distortion) and d.model == "fisheye" and d.iterations == 20 and d._c().model == A.DIST_FISHEYE
    assert (d.k1, d.k2, d.k3, d.k4) == tuple(np.float32(c) for c in cal.distortion_coeffs) and d.p1 == d.p2 == d.k5 == d.k6 == 0.0
    # the host reprojection of the outlier passes is the contract's forward model
    R, t = p["poses"][0]
    np.testing.assert_allclose(reproject(cal.params, R, t, obj[0], "fisheye"), fco.project(fu.params_of(cal.params), R, t, obj[0]), rtol=0, atol=1e-9)
    # flags and a guess: fixed coefficients stay at the guess's
    guess = CameraIntrinsics(p["size"][0], p["size"][1], 500.0, 500.0, 640.0, 360.0, distortion=Distortion.fisheye(0.05, 0.0, 0.01, -0.002))
    g = calibrate_camera_fisheye(obj, img, p["size"], guess=guess, fix_k3=True, fix_k4=True, fix_principal_point=True, max_iterations=40)
    assert g.ok and g.params[2] == 640.0 and g.params[3] == 360.0 and tuple(g.distortion_coeffs[2:]) == (np.float32(0.01), np.float32(-0.002))
    assert g.std_devs[2] == g.std_devs[3] == g.std_devs[8] == g.std_devs[9] == 0.0 and g.std_devs[0] > 0
    plain = calibrate_camera_fisheye(obj, img, p["size"], guess=CameraIntrinsics(p["size"][0], p["size"][1], 500.0, 500.0, 640.0, 360.0))
    np.testing.assert_allclose(plain.params, cal.params, rtol=1e-6, atol=1e-6)
    with pytest.raises(ValueError, match="fisheye"):
        calibrate_camera_fisheye(obj, img, p["size"], guess=CameraIntrinsics(p["size"][0], p["size"][1], 500.0, 500.0, distortion=Distortion(0.1)))
    # several cameras in one call
    two = calibrate_cameras_fisheye([dict(object_points=obj, image_points=img, image_size=p["size"]),
                                     dict(object_points=obj[:8], image_points=img[:8], image_size=p["size"], fix_k4=True)])
    assert np.array_equal(two[0].params, cal.params) and two[1].ok and two[1].params[9] == 0.0 and len(two[1].views) == 8


def test_python_outlier_passes_reproject_through_the_fisheye_model(on_oracle):
    from aruco3_amd.calibration import calibrate_camera_fisheye

    p = fu.problem("grid", 12, seed=31, noise=0.1)
    obj, img = _views_of(p)
    img[2] = img[2].copy()
    img[2][5] += (6.0, -4.0)
    img[7] = img[7].copy()
    img[7][100] += (-5.0, 5.0)
    plain = calibrate_camera_fisheye(obj, img, p["size"])
    cal = calibrate_camera_fisheye(obj, img, p["size"], outlier_passes=2)
    assert cal.ok and on_oracle == ["fisheye"] * 4
    assert not cal.inliers[2][5] and not cal.inliers[7][100] and sum(int(k.sum()) for k in cal.inliers) == cal.points_used
    assert cal.points_used >= 12 * 140 - 12 and cal.rms_px < 0.16 < plain.rms_px


def test_python_model_dispatch_and_refusals(on_oracle):
    from aruco3_amd import CameraIntrinsics, Distortion
    from aruco3_amd.board import CharucoBoard
    from aruco3_amd.calibration import calibrate_camera, calibrate_camera_board, calibrate_camera_charuco

    class Marker:
        def __init__(self, i, c):
            self.id, self.corners, self.corners_refined = i, np.rint(c), c

    class Det:
        def __init__(self, markers):
            self.markers = markers

    from aruco3_amd.board import GridBoard

    board = GridBoard(5, 7, 30.0, 6.0)
    p = fu.problem("grid", 10, seed=32)
    dets = [Det([Marker(int(board.ids[k]), i.reshape(-1, 4, 2)[k]) for k in range(35)]) for i in _views_of(p)[1]]
    cal = calibrate_camera_board(board, dets, p["size"], model="fisheye", fix_k3=True, fix_k4=True)
    assert cal.ok and cal.model == "fisheye" and on_oracle == ["fisheye"] and cal.params[8] == 0.0 and cal.params[9] == 0.0
    assert abs(cal.params[0] - fu.K420[0]) < 0.5
    rat = calibrate_camera_board(board, dets, p["size"])
    assert rat.model == "rational" and on_oracle == ["fisheye", "rational"]
    cb = CharucoBoard(5, 7, 40.0, 30.0)
    q = fu.problem("charuco", 10, seed=33)
    views = [(np.arange(24), i) for i in _views_of(q)[1]]
    ch = calibrate_camera_charuco(cb, views, q["size"], model="fisheye")
    assert ch.ok and ch.model == "fisheye" and on_oracle[-1] == "fisheye"
    np.testing.assert_allclose(ch.params[:4], fu.K420, rtol=1e-5)
    with pytest.raises(ValueError, match="model"):
        calibrate_camera_board(board, dets, p["size"], model="pinhole")
    with pytest.raises(TypeError):
        calibrate_camera_board(board, dets, p["size"], model="fisheye", rational=True)   # (a rational-only keyword)
    # calibrate_camera itself stays rational and keeps refusing a fisheye guess
    obj, img = _views_of(p)
    fish = CameraIntrinsics(1280, 720, 420.0, 420.0, distortion=Distortion.fisheye(*fu.MILD))
    with pytest.raises(ValueError, match="rectify"):
        calibrate_camera(obj, img, p["size"], guess=fish)


def test_python_result_feeds_rectification_and_distortion(on_oracle):
    """the fisheye result's lens, as it is, is what the rectification record and the undistortion take"""
    from aruco3_amd.calibration import calibrate_camera_fisheye
    from tests import fisheye_oracle as fo

    p = fu.problem("grid", 12, seed=34)
    obj, img = _views_of(p)
    cal = calibrate_camera_fisheye(obj, img, p["size"])
    intr = cal.intrinsics
    rec = intr.distortion._c()
    assert rec.model == A.DIST_FISHEYE and (rec.p1, rec.p2, rec.k5, rec.k6) == (0.0, 0.0, 0.0, 0.0)
    # the f32 undistortion contract (tests/fisheye_oracle.c) with the solved camera takes the image points back to the ideal pinhole ones
    K = (intr.focal_x, intr.focal_y, intr.principal_x, intr.principal_y)
    D = tuple(float(c) for c in cal.distortion_coeffs)
    R, t = p["poses"][0]
    und, res = fo.undistort(img[0], K, D)
    P = obj[0].astype(np.float64) @ R[:, :2].T + t
    ideal = P[:, :2] / P[:, 2:3] * np.array(fu.K420[:2]) + np.array(fu.K420[2:])
    # (the f32 contract's arctangent is within 1.5e-7 rad; an angle error grows by dr / dtheta = 1 + r^2 <= 10.5 at 72 degrees and by
    # the focal length: 7e-4 px, beside the f32 rounding of coordinates near 1000 px, 6e-5.  Measured over the 12 views: 6e-4 at most)
    assert np.all(np.isfinite(res)) and np.max(np.abs(und - ideal)) < 5e-3
