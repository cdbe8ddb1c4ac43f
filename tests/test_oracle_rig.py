"""Camera rig calibration on the CPU (tests/rig_oracle.c, the restatement k_rig is held to): recovery of known rigs, an independent
least-squares cross-check, the deviations against noisy solves, fixed extrinsics frame by frame, degenerate input, several rigs in one
call, and the struct layouts across the C header, ctypes and the Rust mirror."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

from aruco3_amd import _lib as A
from tests import calib_oracle as co
from tests import rig_oracle as ro
from tests import rig_util as ru

ROOT = Path(__file__).resolve().parent.parent

# Noise-free recovery, measured with this oracle on the six problems below (gcc 13, x86-64): worst rotation error 1.60e-6 degrees
# (the chain rig), worst translation error 2.32e-7 of the baseline length (2 cameras, 12 frames); rms_px 1.7e-5 .. 1.9e-5, the rounding
# of the image points to f32.  The bounds are ten times the worst value seen: the f32 image points set the floor, the factor covers
# other seeds and compilers.
RECOVERY_ROT_DEG = 10 * 1.6e-6
RECOVERY_T_REL = 10 * 2.32e-7
RECOVERY = [(2, 12, "full", 11), (2, 25, "missing", 12), (3, 15, "chain", 13), (3, 25, "missing", 14), (8, 25, "missing", 15), (8, 16, "full", 16)]


def _solve(p, **kw):
    res, cres, frames, ores = ro.calibrate_rigs(*ru.pack([p], **kw))
    return res[0], cres, frames, ores


@pytest.mark.parametrize("C_,F,pattern,seed", RECOVERY)
def test_noise_free_recovery(C_, F, pattern, seed):
    """cameras with different intrinsics and lenses, a different subset of the board's points in every observation, frames missing in
    some cameras, and a chain rig in which camera 2 never shares a frame with camera 0"""
    p = ru.make_rig(C_, F, seed=seed, pattern=pattern)
    if pattern == "chain":
        seen = {(c, f) for c, f, _, _ in p["obs"]}
        assert not any((0, f) in seen and (2, f) in seen for f in range(F))
    if pattern == "missing":
        assert len(p["obs"]) < C_ * F
    assert len({len(o) for _, _, o, _ in p["obs"]}) > 1
    r, cres, frames, ores = _solve(p)
    assert r.status == A.RIG_OK and r.frames_used == F and r.obs_used == len(p["obs"])
    assert r.points_used == sum(len(o) for _, _, o, _ in p["obs"])
    rot, tr = ru.extrinsic_errors(cres, p["E"])
    print(f"C {C_} F {F} {pattern}: rotation {rot:.3e} deg, translation {tr:.3e} of the baseline, rms {r.rms_px:.3e} px, {r.iterations} iterations")
    assert rot <= RECOVERY_ROT_DEG and tr <= RECOVERY_T_REL
    assert r.rms_px < 1e-3 and all(cres[c].rms_px < 1e-3 for c in range(C_))
    assert list(cres[0].rotation) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(cres[0].translation) == [0, 0, 0] and list(cres[0].std_dev) == [0] * 6
    for f in range(F):
        assert frames[f].status == A.RIG_FRAME_USED
        assert ru.rotation_error_deg(np.array(frames[f].rotation).reshape(3, 3), p["T"][f][0]) < 1e-3
        assert np.linalg.norm(np.array(frames[f].translation) - p["T"][f][1]) < 1e-3
    # the float copies are the doubles rounded
    assert cres[1].translation_f[0] == np.float32(cres[1].translation[0]) and frames[0].rotation_f[4] == np.float32(frames[0].rotation[4])


def test_independent_least_squares_reaches_the_same_optimum():
    """scipy.optimize.least_squares on the same residuals, every pose a Rodrigues vector and a translation, started from the oracle's
    answer perturbed"""
    opt = pytest.importorskip("scipy.optimize")
    from scipy.spatial.transform import Rotation

    p = ru.make_rig(3, 10, seed=7, kind="grid", noise=0.2, pattern="missing")
    r, cres, frames, _ = _solve(p)
    assert r.status == A.RIG_OK and r.converged
    C_, F = p["C"], p["F"]
    obs = [(c, f, o.astype(np.float64), i.astype(np.float64)) for c, f, o, i in p["obs"]]

    def residuals(x):
        E = [(np.eye(3), np.zeros(3))] + [(Rotation.from_rotvec(x[6 * k: 6 * k + 3]).as_matrix(), x[6 * k + 3: 6 * k + 6]) for k in range(C_ - 1)]
        base = 6 * (C_ - 1)
        T = [(Rotation.from_rotvec(x[base + 6 * f: base + 6 * f + 3]).as_matrix(), x[base + 6 * f + 3: base + 6 * f + 6]) for f in range(F)]
        return np.concatenate([(co.project(p["a"][c], *ru.mul(E[c], T[f]), o) - i).ravel() for c, f, o, i in obs])

    x0 = []
    for c in range(1, C_):
        x0 += [Rotation.from_matrix(np.array(cres[c].rotation).reshape(3, 3)).as_rotvec() + 1e-3, np.array(cres[c].translation) * (1 + 1e-3)]
    for f in range(F):
        x0 += [Rotation.from_matrix(np.array(frames[f].rotation).reshape(3, 3)).as_rotvec() + 1e-3, np.array(frames[f].translation) * (1 + 1e-3)]
    sol = opt.least_squares(residuals, np.concatenate(x0), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=20000)
    rms = math.sqrt(float(np.sum(sol.fun ** 2)) / r.points_used)
    assert abs(rms - r.rms_px) <= 1e-9 * r.rms_px
    for c in range(1, C_):
        R = Rotation.from_rotvec(sol.x[6 * (c - 1): 6 * (c - 1) + 3]).as_matrix()
        t = sol.x[6 * (c - 1) + 3: 6 * (c - 1) + 6]
        assert math.radians(ru.rotation_error_deg(R, np.array(cres[c].rotation).reshape(3, 3))) <= 1e-6
        np.testing.assert_allclose(np.array(cres[c].translation), t, rtol=0, atol=1e-6 * np.linalg.norm(t))


def test_std_dev_covers_the_truth_under_noise():
    """sigma = 0.2 px on every image coordinate, six seeds: every extrinsic parameter within 4 of its deviations of the truth.  A
    rotation's deviations are those of the Cayley increment at the solution: compared is the w of R_true R_solved^T."""
    hits = total = 0
    for seed in range(6):
        p = ru.make_rig(3, 30, seed=100 + seed, kind="grid", noise=0.2, pattern="missing")
        r, cres, _, _ = _solve(p)
        assert r.status == A.RIG_OK and 0.25 < r.rms_px < 0.31   # (sqrt(2) sigma: rms_px sums both coordinates)
        for c in range(1, 3):
            sd = np.array(cres[c].std_dev)
            assert np.all(np.isfinite(sd)) and np.all(sd > 0)
            w = ru.cayley_w(p["E"][c][0] @ np.array(cres[c].rotation).reshape(3, 3).T)
            err = np.concatenate([w, p["E"][c][1] - np.array(cres[c].translation)])
            ok = np.abs(err) <= 4 * sd
            hits += int(ok.sum())
            total += 6
            assert ok.all(), (seed, c, err / sd)
    assert total == 6 * 12 and hits == total


def test_fixed_extrinsics_solve_every_frame_alone_bit_for_bit():
    p = ru.make_rig(3, 9, seed=5, kind="grid", noise=0.2, pattern="missing")
    r, cres, frames, ores = _solve(p, flags=A.RIG_FIX_EXTRINSICS, guess=[p["E"]])
    assert r.status == A.RIG_OK and r.frames_used == 9
    for c in range(3):
        assert np.array_equal(np.array(cres[c].rotation).reshape(3, 3), p["E"][c][0]) and list(cres[c].std_dev) == [0] * 6
    its = []
    for f in range(9):
        one = dict(p, F=1, obs=[(c, 0, o, i) for c, g, o, i in p["obs"] if g == f])
        r1, _, f1, _ = _solve(one, flags=A.RIG_FIX_EXTRINSICS, guess=[p["E"]])
        assert bytes(f1[0]) == bytes(frames[f]), f
        its.append((r1.iterations, r1.converged))
        assert ru.rotation_error_deg(np.array(frames[f].rotation).reshape(3, 3), p["T"][f][0]) < 0.2
    assert r.iterations == max(i for i, _ in its) and r.converged == min(c for _, c in its)   # the largest count; converged when all have


def _values(res, cres, frames, ores, n):
    out = [res.rms_px]
    for c in range(n[0]):
        out += list(cres[c].rotation) + list(cres[c].translation) + list(cres[c].std_dev) + [cres[c].rms_px]
    for f in range(n[1]):
        out += list(frames[f].rotation) + list(frames[f].translation) + [frames[f].rms_px]
    return out + [ores[o].rms_px for o in range(n[2])]


def test_degenerate_input_gives_statuses_and_no_nan():
    # cameras 0 and 1 never share a frame
    p = ru.make_rig(2, 6, seed=81)
    p["obs"] = [o for o in p["obs"] if o[1] % 2 == o[0]]
    r, cres, frames, ores = _solve(p)
    assert r.status == A.RIG_NOT_CONNECTED and r.frames_used == 6 and r.obs_used == 6 and r.rms_px == 0.0 and r.iterations == 0
    assert all(frames[f].status == A.RIG_FRAME_USED and frames[f].obs_used == 1 for f in range(6))
    assert all(v == 0.0 for v in _values(r, cres, frames, ores, (2, 6, 6)))
    assert cres[0].obs_used == 3 and cres[1].points_used == sum(len(o[2]) for o in p["obs"] if o[0] == 1)
    # with the extrinsics given and fixed, the same observations are one board pose per frame
    r, _, frames, _ = _solve(p, flags=A.RIG_FIX_EXTRINSICS, guess=[p["E"]])
    assert r.status == A.RIG_OK and r.rms_px < 1e-3
    # an observation with 3 points, one with collinear points, a frame nobody sees
    p = ru.make_rig(3, 8, seed=80, kind="grid")
    obs = [o for o in p["obs"] if o[1] != 5]
    c, f, o, i = obs[1]
    obs[1] = (c, f, o[:3], i[:3])
    line = np.array([[x, 0.0] for x in range(8)], np.float32)
    c, f, _, _ = obs[3]
    obs[3] = (c, f, line, np.stack([100.0 + 10 * line[:, 0], 200.0 + 3 * line[:, 0]], 1).astype(np.float32))
    p["obs"] = obs
    r, cres, frames, ores = _solve(p)
    assert r.status == A.RIG_OK and r.frames_used == 7 and r.obs_used == len(obs) - 2
    assert ores[1].status == A.RIG_OBS_TOO_FEW_POINTS and ores[3].status == A.RIG_OBS_DEGENERATE and ores[1].rms_px == 0.0 and ores[1].points == 3
    assert frames[5].status == A.RIG_FRAME_UNUSED and frames[5].obs_used == 0 and list(frames[5].rotation) == [0.0] * 9
    assert frames[0].obs_used == 2 and frames[1].obs_used == 2
    rot, tr = ru.extrinsic_errors(cres, p["E"])
    assert rot < 1e-4 and tr < 1e-5
    assert not any(math.isnan(v) for v in _values(r, cres, frames, ores, (3, 8, len(obs))))
    # nothing usable at all
    p = ru.make_rig(2, 2, seed=3)
    p["obs"] = [(c, f, o[:3], i[:3]) for c, f, o, i in p["obs"]]
    r, cres, frames, ores = _solve(p)
    assert r.status == A.RIG_NOT_CONNECTED and r.frames_used == 0 and frames[0].status == A.RIG_FRAME_UNUSED


def test_several_rigs_equal_each_alone():
    ps = [ru.make_rig([2, 3, 4][k], 9, seed=20 + k, noise=0.1 * k, pattern=["full", "chain", "missing"][k]) for k in range(3)]
    flags = [0, A.RIG_USE_EXTRINSIC_GUESS, A.RIG_FIX_EXTRINSICS]
    guess = [p["E"] for p in ps]
    packed = ru.pack(ps, flags=flags, guess=guess)
    res, cres, frames, ores = ro.calibrate_rigs(*packed)
    for k, p in enumerate(ps):
        alone = ro.calibrate_rigs(*ru.pack([p], flags=flags[k], guess=[guess[k]]))
        R = packed[0][k]
        assert bytes(alone[0][0]) == bytes(res[k])
        assert all(bytes(alone[1][j]) == bytes(cres[R.first_camera + j]) for j in range(R.n_cameras))
        assert all(bytes(alone[2][j]) == bytes(frames[R.first_frame + j]) for j in range(R.n_frames))
        assert all(bytes(alone[3][j]) == bytes(ores[R.first_obs + j]) for j in range(R.n_obs))


def test_front_end_refuses_what_the_library_would():
    """C = 1 or 9, a duplicate (camera, frame), an index outside the rig: refused on the host, before a context is needed (the
    library's own refusals need one: tests/test_gpu_rig.py)"""
    from aruco3_amd import rig as rg

    p = ru.make_rig(2, 3, seed=1)
    for cams in (p["a"][:1], [p["a"][0]] * 9):
        with pytest.raises(ValueError):
            rg.calibrate_rig(cams, [o for o in p["obs"] if o[0] == 0])
    with pytest.raises(ValueError):
        rg.calibrate_rig(p["a"], p["obs"] + [p["obs"][0]])
    with pytest.raises(ValueError):
        rg.calibrate_rig(p["a"], [(2,) + p["obs"][0][1:]] + p["obs"][1:])
    with pytest.raises(ValueError):
        rg.calibrate_rig(p["a"], p["obs"], n_frames=2)
    with pytest.raises(ValueError):
        rg.calibrate_rig(p["a"], p["obs"], fix_extrinsics=True)


def test_python_front_end_builds_the_call():
    """rig.calibrate_rigs' arrays through the oracle instead of the device: the same answer as the packed problem"""
    from aruco3_amd import rig as rg

    p = ru.make_rig(3, 6, seed=9, pattern="missing")
    want = ro.calibrate_rigs(*ru.pack([p]))
    got = {}

    def solve(*args):
        got["r"] = ro.calibrate_rigs(*args)
        return got["r"]

    old, rg._solve = rg._solve, solve
    try:
        out = rg.calibrate_rig(p["a"], p["obs"])
        st = rg.stereo_calibrate([o for c, _, o, _ in p["obs"] if c == 0], [i for c, _, _, i in p["obs"] if c == 0],
                                 [i for c, _, _, i in p["obs"] if c == 0], p["a"][0], p["a"][0])
    finally:
        rg._solve = old
    assert out.ok and out.rms_px == want[0][0].rms_px and out.iterations == want[0][0].iterations
    assert np.array_equal(out.rotations[2].ravel(), np.array(want[1][2].rotation)) and np.array_equal(out.std_devs[1], np.array(want[1][1].std_dev))
    assert len(out.frames) == 6 and np.array_equal(out.frames[3].translation, np.array(want[2][3].translation))
    assert [(o.camera, o.frame) for o in out.observations] == [(c, f) for c, f, _, _ in p["obs"]]
    R, t = out.camera_pose(1, 2)
    np.testing.assert_allclose(R, ru.mul(p["E"][1], p["T"][2])[0], atol=1e-6)
    # two identical cameras seeing the same pixels: R = I, T = 0, E = F = 0 up to the f32 floor
    assert st.rig.ok and ru.rotation_error_deg(st.R, np.eye(3)) < 1e-4 and np.linalg.norm(st.T) < 1e-3 and st.E.shape == (3, 3) and st.F.shape == (3, 3)


def test_stereo_matrices_satisfy_the_epipolar_constraint():
    from aruco3_amd import rig as rg

    p = ru.make_rig(2, 10, seed=12, subsets=False)
    old, rg._solve = rg._solve, lambda *a: ro.calibrate_rigs(*a)
    try:
        st = rg.stereo_calibrate([o for c, _, o, _ in p["obs"] if c == 0], [i for c, _, _, i in p["obs"] if c == 0],
                                 [i for c, _, _, i in p["obs"] if c == 1], p["a"][0], p["a"][1])
    finally:
        rg._solve = old
    assert st.rig.ok
    np.testing.assert_allclose(st.T, p["E"][1][1], rtol=0, atol=1e-5 * np.linalg.norm(p["E"][1][1]))
    # x2^T F x1 = 0 for the pinhole projections of the same 3-D points
    pts = ru.cu.target_points("charuco")
    X = np.concatenate([pts, np.zeros((len(pts), 1))], 1) @ p["T"][0][0].T + p["T"][0][1]
    K = [np.array([[a[0], 0, a[2]], [0, a[1], a[3]], [0, 0, 1.0]]) for a in p["a"]]
    x1 = (X / X[:, 2:]) @ K[0].T
    X2 = X @ p["E"][1][0].T + p["E"][1][1]
    x2 = (X2 / X2[:, 2:]) @ K[1].T
    assert np.max(np.abs(np.einsum("ni,ij,nj->n", x2, st.F, x1))) < 1e-6 * np.linalg.norm(st.F) * 1280 * 1280


def test_layouts_match_across_c_ctypes_and_rust():
    import ctypes as C

    lay = ro.layout()
    py = [C.sizeof(A.Rig), A.Rig.flags.offset, C.sizeof(A.RigCamera), A.RigCamera.guess_rotation.offset, A.RigCamera.guess_translation.offset,
          C.sizeof(A.RigObservation), A.RigObservation.first_point.offset, C.sizeof(A.RigResult), A.RigResult.rms_px.offset,
          C.sizeof(A.RigCameraResult), A.RigCameraResult.std_dev.offset, A.RigCameraResult.rms_px.offset, A.RigCameraResult.rotation_f.offset,
          A.RigCameraResult.obs_used.offset, C.sizeof(A.RigFrame), A.RigFrame.rms_px.offset, A.RigFrame.rotation.offset,
          A.RigFrame.rotation_f.offset, C.sizeof(A.RigObservationResult), A.RigObservationResult.rms_px.offset]
    assert lay == py == [32, 24, 192, 96, 168, 16, 8, 32, 24, 208, 96, 144, 152, 200, 160, 12, 16, 112, 16, 8]
    text = re.sub(r"//[^\n]*", "", (ROOT / "integration" / "aruco3_hip.rs").read_text())
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "aruco3_hip.h").read_text(), flags=re.S)
    for c_name, r_name in (("a3_rig", "A3Rig"), ("a3_rig_camera", "A3RigCamera"), ("a3_rig_observation", "A3RigObservation"),
                           ("a3_rig_result", "A3RigResult"), ("a3_rig_camera_result", "A3RigCameraResult"), ("a3_rig_frame", "A3RigFrame"),
                           ("a3_rig_observation_result", "A3RigObservationResult")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (c_name, c_name), header, flags=re.S).group(1)
        c_fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                for n in decl.split(None, 1)[1].split(","):
                    c_fields.append(re.sub(r"\[.*?\]", "", n).split()[-1])
        m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^\]]*\)\]\s*)?pub struct %s \{(.*?)\}" % r_name, text, flags=re.S)
        assert m and re.findall(r"pub\s+([a-z0-9_]+)\s*:", m.group(1)) == c_fields, c_name
