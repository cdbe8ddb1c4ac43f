"""Hand-eye calibration on the CPU (tests/handeye_oracle.c, the restatement k_handeye is held to): recovery of known mounts in both
set-ups and at every orientation the four charts exist for, an independent least-squares cross-check, the deviations against noisy
solves, guesses and a fixed mount, degenerate input, several problems in one call, the Python front end, and the struct layouts across
the C header, ctypes and the Rust mirror."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

from aruco3_amd import _lib as A
from tests import calib_oracle as co
from tests import handeye_oracle as ho
from tests import handeye_util as hu

ROOT = Path(__file__).resolve().parent.parent

# Noise-free recovery, measured with this oracle on the 30 problems below (gcc 13, x86-64; 24 points per frame at 340 .. 530 board
# units): worst rotation error of X or Y 4.78e-6 degrees, worst translation error 3.23e-5 board units (both at 3 frames); rms_px
# 1.3e-5 .. 2.1e-5, the rounding of the image points to f32.  The bounds are ten times the worst value seen: the f32 image points set
# the floor, the factor covers other compilers.  The smallest pivot ratio of the start over the 30 problems is 0.16 (axes of the
# relative rotations 65 .. 90 degrees apart).
RECOVERY_ROT_DEG = 10 * 4.78e-6
RECOVERY_T = 10 * 3.23e-5
RECOVERY = [(F, s, m) for F in (3, 4, 25) for s in ("eye_in_hand", "eye_to_hand") for m in hu.MOUNTS]


def _seed(F, setup, mount):
    return 100 * F + 10 * ("eye_in_hand", "eye_to_hand").index(setup) + list(hu.MOUNTS).index(mount)


def _solve(p, **kw):
    res, fres = ho.calibrate_hand_eyes(*hu.pack([p], **kw))
    return res[0], fres


def _values(r, fres, F):
    out = [r.rms_px] + list(r.x_rotation) + list(r.x_translation) + list(r.y_rotation) + list(r.y_translation) + list(r.std_dev)
    for f in range(F):
        out += list(fres[f].rotation) + list(fres[f].translation) + [fres[f].rms_px]
    return out


@pytest.mark.parametrize("F,setup,mount", RECOVERY)
def test_noise_free_recovery(F, setup, mount):
    """3, 4 and 25 frames, both set-ups, and the mounts at which a single chart of the rotation would be singular: 180 degrees about z
    and about x have w = 0, so the chart pinned at w cannot hold them"""
    p = hu.make_problem(F=F, seed=_seed(F, setup, mount), setup=setup, mount=mount)
    assert hu.axis_spread_deg(p) >= 20.0
    r, fres = _solve(p)
    assert r.status == A.HANDEYE_OK and r.frames_used == F and r.pairs_used == F * (F - 1) // 2 and r.points_used == 24 * F
    rot, tr = hu.errors([r], p)
    piv = ho.pivots()
    print(f"F {F} {setup} {mount}: rotation {rot:.3e} deg, translation {tr:.3e} units, rms {r.rms_px:.3e} px, {r.iterations} iterations, "
          f"pivot ratios {piv[0]:.3f} {piv[1]:.3f}")
    assert rot <= RECOVERY_ROT_DEG and tr <= RECOVERY_T
    assert r.rms_px < 1e-3
    assert min(piv) >= 100 * A.HANDEYE_MIN_PIVOT_RATIO
    for f in range(F):
        assert fres[f].status == A.HANDEYE_FRAME_USED and fres[f].points == 24 and fres[f].rms_px < 1e-3
        assert hu.rotation_error_deg(np.array(fres[f].rotation).reshape(3, 3), p["P"][f][0]) < 1e-3
        assert np.linalg.norm(np.array(fres[f].translation) - p["P"][f][1]) < 1e-2
    # the float copies are the doubles rounded
    assert r.x_translation_f[0] == np.float32(r.x_translation[0]) and r.y_rotation_f[4] == np.float32(r.y_rotation[4])
    assert fres[0].rotation_f[1] == np.float32(fres[0].rotation[1])


def test_independent_least_squares_reaches_the_same_optimum():
    """scipy.optimize.least_squares on the same residuals, X and Y a Rodrigues vector and a translation each, started from the oracle's
    answer perturbed; the comparison and its tolerances are test_oracle_rig.py's"""
    opt = pytest.importorskip("scipy.optimize")
    from scipy.spatial.transform import Rotation

    p = hu.make_problem(F=10, seed=7, kind="grid", noise=0.3, mount="y90")
    r, _ = _solve(p)
    assert r.status == A.HANDEYE_OK and r.converged
    obs = [(o.astype(np.float64), i.astype(np.float64)) for o, i in p["obs"]]

    def residuals(x):
        X = (Rotation.from_rotvec(x[0:3]).as_matrix(), x[3:6])
        Y = (Rotation.from_rotvec(x[6:9]).as_matrix(), x[9:12])
        return np.concatenate([(co.project(p["a"], *hu.mul(X, hu.mul(p["M"][f], Y)), o) - i).ravel() for f, (o, i) in enumerate(obs)])

    (RX, tX), (RY, tY) = hu.solved([r])
    x0 = np.concatenate([Rotation.from_matrix(RX).as_rotvec() + 1e-3, tX * (1 + 1e-3), Rotation.from_matrix(RY).as_rotvec() + 1e-3, tY * (1 + 1e-3)])
    sol = opt.least_squares(residuals, x0, method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=20000)
    rms = math.sqrt(float(np.sum(sol.fun ** 2)) / r.points_used)
    assert abs(rms - r.rms_px) <= 1e-9 * r.rms_px
    for k, (R, t) in enumerate(((RX, tX), (RY, tY))):
        assert math.radians(hu.rotation_error_deg(Rotation.from_rotvec(sol.x[6 * k: 6 * k + 3]).as_matrix(), R)) <= 1e-6
        np.testing.assert_allclose(t, sol.x[6 * k + 3: 6 * k + 6], rtol=0, atol=1e-6 * np.linalg.norm(t))


def test_std_dev_covers_the_truth_under_noise():
    """test_oracle_rig.py's rule: sigma = 0.2 px on every image coordinate, six seeds, every one of the 12 unknowns within 4 of its
    deviations of the truth.  A rotation's deviations are those of the Cayley increment at the solution: compared is the w of
    R_true R_solved^T.  Beside it the share within 3 deviations: 99.7 % for a Gaussian, so of 72 values at most a few may miss; fewer
    than 95 % would mean deviations that are too small."""
    hits = hits3 = total = 0
    for seed in range(6):
        p = hu.make_problem(F=30, seed=100 + seed, kind="grid", noise=0.2, mount=list(hu.MOUNTS)[seed % 5])
        r, _ = _solve(p)
        assert r.status == A.HANDEYE_OK and 0.25 < r.rms_px < 0.31   # (sqrt(2) sigma: rms_px sums both coordinates)
        sd = np.array(r.std_dev)
        assert np.all(np.isfinite(sd)) and np.all(sd > 0)
        X, Y = hu.solved([r])
        err = np.concatenate([hu.cayley_w(p["X"][0] @ X[0].T), p["X"][1] - X[1], hu.cayley_w(p["Y"][0] @ Y[0].T), p["Y"][1] - Y[1]])
        ok = np.abs(err) <= 4 * sd
        hits += int(ok.sum())
        hits3 += int((np.abs(err) < 3 * sd).sum())
        total += 12
        assert ok.all(), (seed, err / sd)
    print(f"within 4 deviations {hits} / {total}, within 3 deviations {hits3} / {total}")
    assert total == 72 and hits == total and hits3 >= 0.95 * total


def test_guess_and_fixed_mount():
    p = hu.make_problem(F=8, seed=31, noise=0.2, mount="d120")
    free, _ = _solve(p)
    assert free.status == A.HANDEYE_OK and free.converged
    # a near guess reaches the same optimum
    near = ((hu.bu.rot_xyz(0.5, -0.4, 0.3) @ p["X"][0], p["X"][1] + [1.0, -2.0, 1.5]), (hu.bu.rot_xyz(-0.3, 0.6, 0.2) @ p["Y"][0], p["Y"][1] + [3.0, 1.0, -2.0]))
    g, _ = _solve(p, flags=A.HANDEYE_USE_GUESS, guess=[near])
    assert g.status == A.HANDEYE_OK and g.converged and g.pairs_used == 0
    assert abs(g.rms_px - free.rms_px) <= 1e-7 * free.rms_px
    assert hu.rotation_error_deg(np.array(g.x_rotation).reshape(3, 3), np.array(free.x_rotation).reshape(3, 3)) < 1e-4
    assert np.linalg.norm(np.array(g.x_translation) - np.array(free.x_translation)) < 1e-3
    assert np.linalg.norm(np.array(g.y_translation) - np.array(free.y_translation)) < 1e-3
    # the true mount, fixed: Y alone, X untouched and without deviations
    q = hu.make_problem(F=6, seed=32, mount="z180")
    fx, _ = _solve(q, flags=A.HANDEYE_FIX_X, guess=[(q["X"], None)])
    assert fx.status == A.HANDEYE_OK and fx.pairs_used == 0
    assert np.array_equal(np.array(fx.x_rotation).reshape(3, 3), q["X"][0]) and list(fx.x_translation) == list(q["X"][1])
    assert list(fx.std_dev[:6]) == [0.0] * 6 and all(0 < v < math.inf for v in fx.std_dev[6:])
    Y = hu.solved([fx])[1]
    assert hu.rotation_error_deg(Y[0], q["Y"][0]) <= RECOVERY_ROT_DEG and np.linalg.norm(Y[1] - q["Y"][1]) <= RECOVERY_T
    # the board moved to a second place: the same mount finds it
    moved = (hu.bu.rot_xyz(175.0, -20.0, 40.0), np.array([300.0, -250.0, 60.0]))
    q2 = hu.make_problem(F=6, seed=33, mount="z180", board_y=moved)
    fx2, _ = _solve(q2, flags=A.HANDEYE_FIX_X, guess=[(q2["X"], None)])
    Y2 = hu.solved([fx2])[1]
    assert fx2.status == A.HANDEYE_OK
    assert hu.rotation_error_deg(Y2[0], moved[0]) <= RECOVERY_ROT_DEG and np.linalg.norm(Y2[1] - moved[1]) <= RECOVERY_T


def test_degenerate_input_gives_statuses_and_no_nan():
    # two USED frames
    p = hu.make_problem(F=4, seed=41, few=(1, 3))
    r, fres = _solve(p)
    assert r.status == A.HANDEYE_TOO_FEW_FRAMES and r.frames_used == 2 and r.points_used == 48 and r.iterations == 0 and r.pairs_used == 0
    assert fres[1].status == A.HANDEYE_FRAME_TOO_FEW_POINTS and fres[1].points == 3 and fres[0].status == A.HANDEYE_FRAME_USED
    assert all(v == 0.0 for v in _values(r, fres, 0)) and list(fres[1].rotation) == [0.0] * 9 and fres[0].rms_px == 0.0
    assert hu.rotation_error_deg(np.array(fres[0].rotation).reshape(3, 3), p["P"][0][0]) < 1e-3    # a USED frame still reports P_f
    # a frame of 3 points and a frame of collinear points are left out, the rest solves
    p = hu.make_problem(F=6, seed=42, few=(1,), collinear=(4,))
    r, fres = _solve(p)
    assert r.status == A.HANDEYE_OK and r.frames_used == 4 and r.pairs_used == 6 and r.points_used == 96
    assert fres[1].status == A.HANDEYE_FRAME_TOO_FEW_POINTS and fres[4].status == A.HANDEYE_FRAME_DEGENERATE and fres[4].points == 6
    assert fres[4].rms_px == 0.0 and list(fres[4].translation) == [0.0] * 3
    rot, tr = hu.errors([r], p)
    assert rot <= RECOVERY_ROT_DEG and tr <= RECOVERY_T
    assert not any(math.isnan(v) for v in _values(r, fres, 6))
    # a robot that only translates: every pair is below A3_HANDEYE_MIN_PAIR_ANGLE
    p = hu.make_problem(F=8, seed=43, motion="translate")
    r, fres = _solve(p)
    assert r.status == A.HANDEYE_NO_MOTION and r.frames_used == 8 and r.pairs_used == 0
    assert all(v == 0.0 for v in _values(r, fres, 0)) and not any(math.isnan(v) for v in _values(r, fres, 8))
    # a robot that turns about one axis only: pairs there are, the pivots are not
    p = hu.make_problem(F=8, seed=44, motion="one_axis")
    assert hu.axis_spread_deg(p) < 1e-3
    r, fres = _solve(p)
    assert r.status == A.HANDEYE_NO_MOTION and r.frames_used == 8 and r.pairs_used == 28
    assert all(v == 0.0 for v in _values(r, fres, 0)) and not any(math.isnan(v) for v in _values(r, fres, 8))
    # given the mount, the same frames locate the board
    r, _ = _solve(p, flags=A.HANDEYE_FIX_X, guess=[(p["X"], None)])
    assert r.status == A.HANDEYE_OK and r.rms_px < 1e-3


def test_several_problems_equal_each_alone():
    ps = [hu.make_problem(F=[5, 3, 9, 6][k], seed=50 + k, noise=0.1 * k, mount=list(hu.MOUNTS)[k], setup=["eye_in_hand", "eye_to_hand"][k % 2],
                          motion="one_axis" if k == 3 else "general") for k in range(4)]
    flags = [0, A.HANDEYE_USE_GUESS, A.HANDEYE_FIX_X, 0]
    guess = [(p["X"], p["Y"]) for p in ps]
    packed = hu.pack(ps, flags=flags, guess=guess)
    res, fres = ho.calibrate_hand_eyes(*packed)
    assert [r.status for r in res] == [A.HANDEYE_OK] * 3 + [A.HANDEYE_NO_MOTION]
    for k, p in enumerate(ps):
        alone = ho.calibrate_hand_eyes(*hu.pack([p], flags=flags[k], guess=[guess[k]]))
        R = packed[0][k]
        assert bytes(alone[0][0]) == bytes(res[k])
        assert all(bytes(alone[1][j]) == bytes(fres[R.first_frame + j]) for j in range(R.n_frames))


class _Oracle:
    """aruco3_amd.handeye with the oracle in the device's place; `calls` keeps what the front end built"""

    def __enter__(self):
        from aruco3_amd import handeye as he

        self.he, self.old, self.calls = he, he._solve, []

        def solve(*args):
            self.calls.append(args)
            return ho.calibrate_hand_eyes(*args)

        he._solve = solve
        return self

    def __exit__(self, *exc):
        self.he._solve = self.old


@pytest.mark.parametrize("setup", ["eye_in_hand", "eye_to_hand"])
def test_python_front_end_builds_the_call(setup):
    p = hu.make_problem(F=6, seed=61, setup=setup, mount="x180")
    want = ho.calibrate_hand_eyes(*hu.pack([p]))
    T4 = [np.block([[R, t.reshape(3, 1)], [np.zeros((1, 3)), np.ones((1, 1))]]) for R, t in p["robot"]]
    with _Oracle() as o:
        out = o.he.calibrate_hand_eye(p["a"], p["robot"], p["obs"], setup=setup)
        out4 = o.he.calibrate_hand_eye(p["a"], T4, p["obs"], setup=setup)
        both = o.he.calibrate_hand_eyes([dict(camera=p["a"], robot_poses=p["robot"], observations=p["obs"], setup=setup)] * 2)
    # the set-up maps the robot poses onto M_f
    frames = o.calls[0][1]
    for f in range(6):
        np.testing.assert_allclose(np.array(frames[f].rotation).reshape(3, 3), p["M"][f][0], rtol=0, atol=1e-15)
        np.testing.assert_allclose(np.array(frames[f].translation), p["M"][f][1], rtol=0, atol=1e-12)
    assert out.ok and out.setup == setup and out.frames_used == 6 and out.pairs_used == 15 and len(out.frames) == 6 and out.inliers is None
    assert abs(out.rms_px - want[0][0].rms_px) < 1e-6 and np.array_equal(out4.X[0], out.X[0]) and np.array_equal(both[1].Y[1], out.Y[1])
    assert out.std_devs.shape == (12,) and out.frames[2].used and out.frames[2].points == 24
    # the accessors
    X, Y = out.X, out.Y
    assert hu.rotation_error_deg(X[0], p["X"][0]) <= RECOVERY_ROT_DEG and np.linalg.norm(Y[1] - p["Y"][1]) <= RECOVERY_T
    if setup == "eye_in_hand":
        R, t = out.camera_to_gripper()
        np.testing.assert_allclose(R @ X[0], np.eye(3), atol=1e-12)
        np.testing.assert_allclose(R @ X[1] + t, 0.0, atol=1e-9)
        assert out.board_to_base() is Y
        with pytest.raises(ValueError):
            out.camera_to_base()
        # camera -> base at a robot pose: base <- gripper <- camera
        Rb, tb = out.camera_pose_in_base(p["robot"][3])
        np.testing.assert_allclose(Rb, p["robot"][3][0] @ R, atol=1e-12)
        np.testing.assert_allclose(tb, p["robot"][3][0] @ t + p["robot"][3][1], atol=1e-9)
        with pytest.raises(ValueError):
            out.camera_pose_in_base()
        # cv::calibrateHandEye's unknown composed with the inputs reproduces every frame's own pose within the solve's rms, under noise
        # (noise-free both sit at the rounding floor): board -> camera = (camera -> gripper)^-1 . (gripper -> base)^-1 . (board -> base)
        n = hu.make_problem(F=8, seed=63, setup=setup, noise=0.2, mount="x180")
        with _Oracle() as o2:
            noisy = o2.he.calibrate_hand_eye(n["a"], n["robot"], n["obs"])
        assert noisy.ok and 0.2 < noisy.rms_px < 0.35
        for f in range(8):
            G = hu.mul(hu.inv(noisy.camera_to_gripper()), hu.mul(hu.inv(n["robot"][f]), noisy.board_to_base()))
            pts = n["obs"][f][0].astype(np.float64)
            own = co.project(n["a"], noisy.frames[f].rotation, noisy.frames[f].translation, pts)
            diff = math.sqrt(float(np.mean(np.sum((co.project(n["a"], G[0], G[1], pts) - own) ** 2, axis=1))))
            print(f"frame {f}: chain against the frame's own pose {diff:.4f} px, solve rms {noisy.rms_px:.4f} px")
            assert diff <= noisy.rms_px
    else:
        R, t = out.camera_to_base()
        np.testing.assert_allclose(R @ X[0], np.eye(3), atol=1e-12)
        assert out.board_to_gripper() is Y
        with pytest.raises(ValueError):
            out.camera_to_gripper()
        Rb, tb = out.camera_pose_in_base()
        assert np.array_equal(Rb, R) and np.array_equal(tb, t)
    G = out.board_pose_in_camera(p["robot"][1])
    assert hu.rotation_error_deg(G[0], p["P"][1][0]) < 1e-4 and np.linalg.norm(G[1] - p["P"][1][1]) < 1e-2


def test_front_end_fixed_mount_and_outliers():
    p = hu.make_problem(F=8, seed=62, kind="grid", noise=0.1)
    rng = np.random.default_rng(5)
    obs = [(o.copy(), i.copy()) for o, i in p["obs"]]
    planted = {}
    for f in (1, 4, 6):
        idx = rng.choice(len(obs[f][0]), 5, replace=False)
        obs[f][1][idx] += rng.choice([-1.0, 1.0], (5, 2)).astype(np.float32) * rng.uniform(6.0, 12.0, (5, 2)).astype(np.float32)
        planted[f] = set(int(v) for v in idx)
    with _Oracle() as o:
        dirty = o.he.calibrate_hand_eye(p["a"], p["robot"], obs)
        clean = o.he.calibrate_hand_eye(p["a"], p["robot"], obs, outlier_passes=2)
        fixed = o.he.calibrate_hand_eye(p["a"], p["robot"], p["obs"], guess=p["X"], fix_mount=True)
        guessed = o.he.calibrate_hand_eye(p["a"], p["robot"], p["obs"], guess=(p["X"], p["Y"]), max_iterations=3)
    assert dirty.ok and clean.ok and dirty.rms_px > 0.5 and clean.rms_px < 0.2
    for f in range(8):
        dropped = set(int(v) for v in np.nonzero(~clean.inliers[f])[0])
        assert planted.get(f, set()) <= dropped and len(dropped) <= len(planted.get(f, ())) + 3
    assert len(o.calls) == 1 + 3 + 1 + 1
    assert o.calls[4][0][0].flags == A.HANDEYE_FIX_X and o.calls[5][0][0].flags == A.HANDEYE_USE_GUESS and o.calls[5][0][0].max_iterations == 3
    assert fixed.ok and np.array_equal(fixed.X[0], p["X"][0]) and guessed.ok and guessed.iterations <= 3


def test_front_end_refuses_what_the_library_would():
    """counts, limits, non-finite poses, a fixed mount without a mount, a fisheye camera: refused on the host, before a context is
    needed (the library's own refusals need one: tests/test_gpu_handeye.py)"""
    from aruco3_amd import handeye as he
    from aruco3_amd.pinhole import CameraIntrinsics, Distortion

    p = hu.make_problem(F=3, seed=1)
    with pytest.raises(ValueError):
        he.calibrate_hand_eye(p["a"], p["robot"], p["obs"][:2])
    with pytest.raises(ValueError):
        he.calibrate_hand_eye(p["a"], p["robot"], p["obs"], setup="eye_on_stalk")
    with pytest.raises(ValueError):
        he.calibrate_hand_eye(p["a"], [], [])
    with pytest.raises(ValueError):
        he.calibrate_hand_eye(p["a"], p["robot"] * 86, p["obs"] * 86)          # 258 frames
    with pytest.raises(ValueError):
        he.calibrate_hand_eyes([])
    bad = [(p["robot"][0][0], np.array([0.0, math.nan, 0.0]))] + p["robot"][1:]
    with pytest.raises(ValueError):
        he.calibrate_hand_eye(p["a"], bad, p["obs"])
    with pytest.raises(ValueError):
        he.calibrate_hand_eye(p["a"], p["robot"], p["obs"], fix_mount=True)
    with pytest.raises(ValueError):
        he.calibrate_hand_eye(p["a"], p["robot"], p["obs"], guess=p["X"])         # X alone, not fixed
    with pytest.raises(ValueError):
        he.calibrate_hand_eye(p["a"], p["robot"], p["obs"], guess=((p["X"][0], np.array([math.inf, 0, 0])), p["Y"]))
    big = (np.zeros((A.CALIB_MAX_POINTS + 1, 2), np.float32), np.zeros((A.CALIB_MAX_POINTS + 1, 2), np.float32))
    with pytest.raises(ValueError):
        he.calibrate_hand_eye(p["a"], p["robot"], [big] + p["obs"][1:])
    a = p["a"].copy()
    a[0] = 0.0
    with pytest.raises(ValueError):
        he.calibrate_hand_eye(a, p["robot"], p["obs"])
    cam = CameraIntrinsics(1280, 720, 900.0, 900.0, distortion=Distortion.fisheye(0.01, 0.002, 0.0, 0.0))
    with pytest.raises(ValueError, match="rectify"):
        he.calibrate_hand_eye(cam, p["robot"], p["obs"])
    import aruco3_amd

    assert aruco3_amd.calibrate_hand_eye is he.calibrate_hand_eye and aruco3_amd.HandEyeCalibration is he.HandEyeCalibration
    assert aruco3_amd.calibrate_hand_eye_board is he.calibrate_hand_eye_board and aruco3_amd.calibrate_hand_eye_charuco is he.calibrate_hand_eye_charuco


def test_layouts_match_across_c_ctypes_and_rust():
    import ctypes as C

    lay = ho.layout()
    P, Fr, Rs, FR = A.HandEyeProblem, A.HandEyeFrame, A.HandEyeResult, A.HandEyeFrameResult
    py = [C.sizeof(P), P.flags.offset, P.a.offset, P.guess_x_rotation.offset, P.guess_y_translation.offset,
          C.sizeof(Fr), Fr.translation.offset, Fr.first_point.offset,
          C.sizeof(Rs), Rs.pairs_used.offset, Rs.rms_px.offset, Rs.x_rotation.offset, Rs.y_translation.offset, Rs.std_dev.offset,
          Rs.x_rotation_f.offset, Rs.y_translation_f.offset, C.sizeof(FR), FR.rms_px.offset, FR.rotation.offset, FR.rotation_f.offset]
    assert lay == py == [304, 8, 16, 112, 280, 104, 72, 96, 416, 12, 24, 32, 200, 224, 320, 404, 160, 8, 16, 112]
    text = re.sub(r"//[^\n]*", "", (ROOT / "integration" / "aruco3_hip.rs").read_text())
    raw = (ROOT / "include" / "aruco3_hip.h").read_text()
    header = re.sub(r"/\*.*?\*/", "", raw, flags=re.S)
    assert re.search(r"#define\s+A3_ABI_VERSION\s+5\b", raw) and "a3_calibrate_hand_eyes" in A.SYMBOLS
    for name, value in (("MAX_FRAMES", "256"), ("MAX_PROBLEMS", "1024"), ("MAX_CALL_FRAMES", "65536"), ("MIN_PIVOT_RATIO", "1e-4"),
                        ("MAX_PAIR_ANGLE", "170.0"), ("MIN_PAIR_ANGLE", "2.0")):
        assert re.search(r"#define\s+A3_HANDEYE_%s\s+%s\b" % (name, re.escape(value)), raw), name
    # the literal cosines are those of half the pair angles
    lo = float(re.search(r"#define\s+A3_HANDEYE_COS_HALF_MAX_PAIR_ANGLE\s+([0-9.e-]+)", raw).group(1))
    hi = float(re.search(r"#define\s+A3_HANDEYE_COS_HALF_MIN_PAIR_ANGLE\s+([0-9.e-]+)", raw).group(1))
    assert abs(lo - math.cos(math.radians(85.0))) < 1e-15 and abs(hi - math.cos(math.radians(1.0))) < 1e-15
    for c_name, r_name in (("a3_handeye_problem", "A3HandEyeProblem"), ("a3_handeye_frame", "A3HandEyeFrame"),
                           ("a3_handeye_result", "A3HandEyeResult"), ("a3_handeye_frame_result", "A3HandEyeFrameResult")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (c_name, c_name), header, flags=re.S).group(1)
        c_fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                for n in decl.split(None, 1)[1].split(","):
                    c_fields.append(re.sub(r"\[.*?\]", "", n).split()[-1])
        m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^\]]*\)\]\s*)?pub struct %s \{(.*?)\}" % r_name, text, flags=re.S)
        assert m and re.findall(r"pub\s+([a-z0-9_]+)\s*:", m.group(1)) == c_fields, c_name
