"""Camera rig calibration on the MI355X (k_rig; a3_calibrate_rigs): every output bit-equal to the CPU restatement (tests/rig_oracle.c)
across camera, frame and point counts, both flags, noise, an iteration cap, bad observations and a rig that is not connected; several
rigs in one launch equal to each alone; the ABI's refusals; detection unchanged around a call; and two simulated cameras looking at one
board, each calibrated from its own detections, then the rig, then fused board poses."""
import ctypes as C

import numpy as np
import pytest

from tests import rig_oracle as ro
from tests import rig_util as ru

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


_ctx_cache = {}


def _ctx():
    from aruco3_amd import _lib

    _torch()
    if "c" not in _ctx_cache:
        _ctx_cache["c"] = _lib.Context(_lib.default_config(), np.zeros(1, np.uint64), 64, 1)
    return _ctx_cache["c"]


def _check(packed):
    """the device against the oracle, raw bits of every record -> the device's (results, camera results, frames, observation results)"""
    dev = _ctx().calibrate_rigs(*packed)
    ora = ro.calibrate_rigs(*packed)
    rigs, cams, obs = packed[:3]
    n_frames = max(int(r.first_frame) + int(r.n_frames) for r in rigs)
    for k in range(len(rigs)):
        assert bytes(dev[0][k]) == bytes(ora[0][k]), (k, dev[0][k].status, ora[0][k].status, dev[0][k].iterations, ora[0][k].iterations,
                                                      dev[0][k].rms_px, ora[0][k].rms_px)
    for k in range(len(cams)):
        assert bytes(dev[1][k]) == bytes(ora[1][k]), ("camera", k, list(dev[1][k].translation), list(ora[1][k].translation))
    for k in range(n_frames):
        assert bytes(dev[2][k]) == bytes(ora[2][k]), ("frame", k)
    for k in range(len(obs)):
        assert bytes(dev[3][k]) == bytes(ora[3][k]), ("observation", k)
    return dev


@pytest.mark.parametrize("C_,F,pattern", [(2, 1, "full"), (2, 3, "full"), (2, 25, "missing"), (3, 25, "chain"), (8, 25, "missing"), (3, 3, "full"),
                                          (8, 1, "full"), (2, 500, "missing"), (8, 500, "missing")])
def test_bit_equal_cameras_and_frames(C_, F, pattern):
    from aruco3_amd import _lib

    p = ru.make_rig(C_, F, seed=100 + C_ + F, pattern=pattern)
    res = _check(ru.pack([p]))[0]
    assert res[0].status == _lib.RIG_OK and res[0].frames_used == F


def test_bit_equal_four_and_max_points():
    from aruco3_amd import _lib

    p = ru.make_rig(3, 25, seed=31, kind="grid", subsets=False)
    p["obs"] = [(c, f, o[4 * ((c + f) % 35):][:4], i[4 * ((c + f) % 35):][:4]) for c, f, o, i in p["obs"]]   # one marker's 4 corners each
    res = _check(ru.pack([p]))[0]
    assert res[0].obs_used == 75 and res[0].points_used == 300
    d = ru.make_rig(2, 3, seed=32, kind="dense", subsets=False)
    assert len(d["obs"][0][2]) == _lib.CALIB_MAX_POINTS
    res = _check(ru.pack([d]))[0]
    assert res[0].status == _lib.RIG_OK


@pytest.mark.parametrize("C_", [2, 3, 8])
def test_bit_equal_flags_noise_and_iteration_cap(C_):
    from aruco3_amd import _lib

    p = ru.make_rig(C_, 25, seed=40 + C_, kind="grid", noise=0.2, pattern="missing")
    near = [(ru.bu.rot_xyz(0.5, -0.4, 0.3) @ R, t + np.array([2.0, -1.0, 1.5])) for R, t in p["E"]]
    _check(ru.pack([p]))
    _check(ru.pack([p], flags=_lib.RIG_USE_EXTRINSIC_GUESS, guess=[near]))
    _check(ru.pack([p], flags=_lib.RIG_FIX_EXTRINSICS, guess=[p["E"]]))
    _check(ru.pack([p], flags=_lib.RIG_FIX_EXTRINSICS | _lib.RIG_USE_EXTRINSIC_GUESS, guess=[near], max_iterations=2))
    res = _check(ru.pack([p], max_iterations=1))[0]
    assert res[0].iterations == 1 and res[0].converged == 0


def _bad_and_disconnected():
    """rig 0: good but for an observation of 3 points, one of collinear points and a frame nobody sees; rig 1: cameras 0 and 1 never
    share a frame; rig 2: good"""
    a = ru.make_rig(3, 8, seed=80, kind="grid")
    obs = [o for o in a["obs"] if o[1] != 5]
    c, f, o, i = obs[1]
    obs[1] = (c, f, o[:3], i[:3])
    line = np.array([[x, 0.0] for x in range(8)], np.float32)
    c, f, _, _ = obs[3]
    obs[3] = (c, f, line, np.stack([100.0 + 10 * line[:, 0], 200.0 + 3 * line[:, 0]], 1).astype(np.float32))
    a["obs"] = obs
    b = ru.make_rig(2, 6, seed=81)
    b["obs"] = [o for o in b["obs"] if o[1] % 2 == o[0]]
    return [a, b, ru.make_rig(2, 6, seed=82, noise=0.1)]


def test_bit_equal_bad_observations_and_a_rig_that_is_not_connected():
    from aruco3_amd import _lib

    res, cres, frames, ores = _check(ru.pack(_bad_and_disconnected()))
    assert [r.status for r in res] == [_lib.RIG_OK, _lib.RIG_NOT_CONNECTED, _lib.RIG_OK]
    assert ores[1].status == _lib.RIG_OBS_TOO_FEW_POINTS and ores[3].status == _lib.RIG_OBS_DEGENERATE
    assert frames[5].status == _lib.RIG_FRAME_UNUSED and res[0].frames_used == 7
    assert bytes(cres[3])[:-8] == bytes(len(bytes(cres[3])) - 8) and res[1].rms_px == 0.0


def test_sixteen_rigs_in_one_launch_equal_each_alone():
    from aruco3_amd import _lib

    ps = [ru.make_rig([2, 3, 4][k % 3], 25, seed=90 + k, kind=["charuco", "grid"][k % 2], noise=0.1 * (k % 3),
                      pattern=["full", "missing", "chain"][k % 3 if k % 3 != 2 or [2, 3, 4][k % 3] > 2 else 0]) for k in range(16)]
    flags = [0, 0, 2, 0, 1, 0, 2, 0, 0, 3, 0, 0, 1, 0, 2, 0]
    guess = [p["E"] for p in ps]
    packed = ru.pack(ps, flags=flags, guess=guess)
    res, cres, frames, ores = _check(packed)
    assert all(r.status == _lib.RIG_OK for r in res)
    for k, p in enumerate(ps):
        alone = _ctx().calibrate_rigs(*ru.pack([p], flags=flags[k], guess=[guess[k]]))
        R = packed[0][k]
        assert bytes(alone[0][0]) == bytes(res[k])
        assert all(bytes(alone[1][j]) == bytes(cres[R.first_camera + j]) for j in range(R.n_cameras))
        assert all(bytes(alone[2][j]) == bytes(frames[R.first_frame + j]) for j in range(R.n_frames))
        assert all(bytes(alone[3][j]) == bytes(ores[R.first_obs + j]) for j in range(R.n_obs))


def test_refusals_and_detection_unchanged():
    """C = 1 or 9, a duplicate (camera, frame) and the other input errors are refused, the context stays usable, and a detection batch
    gives the same bytes before and after rig calls"""
    from aruco3_amd import _lib as A, synth
    from aruco3_amd.dictionaries import ARDictionary

    torch = _torch()
    L = A.load()
    d = ARDictionary.new_from_named_dict("ARUCO_DEFAULT")
    ctx = A.Context(A.default_config(), d.code_list, d.num_bits, d._tau)
    frames_rgb, _ = synth.config_frames(1, 4)
    dev = torch.from_numpy(frames_rgb).cuda()
    torch.cuda.synchronize()
    n, h, w = frames_rgb.shape[:3]
    before = ctx.detect_batch(dev.data_ptr(), A.MEM_DEVICE, A.FMT_RGB8, w, h, w * 3, w * h * 3, n)
    p = ru.make_rig(2, 3, seed=1)
    f32p = C.POINTER(C.c_float)
    res, cres = (A.RigResult * 1)(), (A.RigCameraResult * 16)()
    frames, ores = (A.RigFrame * 8)(), (A.RigObservationResult * 16)()

    def call(mod=None, null=None, n_rigs=1, **kw):
        rigs, cams, obs, obj, img = ru.pack([p], **kw)
        if mod:
            mod(rigs, cams, obs, obj, img)
        args = dict(rigs=rigs, cams=cams, obs=obs, obj=obj.ctypes.data_as(f32p), img=img.ctypes.data_as(f32p), res=res, cres=cres)
        if null:
            args[null] = None
        return L.a3_calibrate_rigs(ctx.handle, args["rigs"], n_rigs, args["cams"], 2, args["obs"], len(p["obs"]), args["obj"], args["img"],
                                   args["res"], args["cres"], frames, ores)

    def setter(what, field, value, index=0):
        def mod(rigs, cams, obs, obj, img):
            setattr({"rig": rigs, "obs": obs}[what][index], field, value)
        return mod

    assert call() == A.OK and res[0].status == A.RIG_OK
    for null in ("rigs", "cams", "obs", "obj", "img", "res", "cres"):
        assert call(null=null) == A.ERR_INVALID, null
    assert call(n_rigs=0) == A.ERR_INVALID
    for what, field, value in (("rig", "n_cameras", 1), ("rig", "n_cameras", 9), ("rig", "flags", 4), ("rig", "max_iterations", 1001),
                               ("rig", "n_frames", 0), ("rig", "n_frames", 4097), ("rig", "n_obs", 0), ("rig", "n_obs", 7),
                               ("rig", "first_camera", 1), ("obs", "camera", 2), ("obs", "frame", 3), ("obs", "n_points", 4097)):
        assert call(setter(what, field, value)) == A.ERR_INVALID, (what, field, value)

    def duplicate(rigs, cams, obs, obj, img):
        obs[1].camera, obs[1].frame = obs[0].camera, obs[0].frame

    def bad_focal(rigs, cams, obs, obj, img):
        cams[1].a[0] = 0.0

    def nan_lens(rigs, cams, obs, obj, img):
        cams[0].a[5] = float("nan")

    def nan_point(rigs, cams, obs, obj, img):
        img[7, 1] = np.nan

    def inf_guess(rigs, cams, obs, obj, img):
        cams[1].guess_translation[2] = float("inf")

    for mod in (duplicate, bad_focal, nan_lens, nan_point):
        assert call(mod) == A.ERR_INVALID, mod.__name__
    assert call(inf_guess, flags=A.RIG_USE_EXTRINSIC_GUESS) == A.ERR_INVALID and call(inf_guess, flags=A.RIG_FIX_EXTRINSICS) == A.ERR_INVALID
    assert call(inf_guess) == A.OK                     # (not read without the flags)
    # a batch in flight
    ctx.submit(dev.data_ptr(), A.MEM_DEVICE, A.FMT_RGB8, w, h, w * 3, w * h * 3, n)
    assert call() == A.ERR_INVALID
    mid = ctx.collect()
    assert call() == A.OK
    want = ro.calibrate_rigs(*ru.pack([p]))
    assert bytes(res[0]) == bytes(want[0][0]) and bytes(cres[1]) == bytes(want[1][1]) and bytes(frames[2]) == bytes(want[2][2])
    after = ctx.detect_batch(dev.data_ptr(), A.MEM_DEVICE, A.FMT_RGB8, w, h, w * 3, w * h * 3, n)
    for a, b in ((before, mid), (before, after)):
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


def test_end_to_end_two_cameras_one_board():
    """Two simulated cameras (different K; camera 0 through the WEBCAM lens, camera 1 a pinhole, 120 board units to its right and turned
    towards the scene) look at one 5 x 7 GridBoard at 20 instants.  Frames are detected with refinement, each camera calibrated from
    its own 16 frames (calibrate_camera_board, outlier_passes=2), then the rig (calibrate_rig_board).  The yardstick is what the
    library offered before: per instant P_1f P_0f^-1 from the two cameras' board poses.  The joint solve must be no worse than the
    median single-instant estimate, in rotation and in translation.  Then rig_board_poses on the 4 held-out instants with the solved
    rig against the same call with the true extrinsics and cameras.

    First measured run (MI355X): 16 of 16 instants with both observations USED; joint 0.090 deg and 0.0017 of the baseline; single
    instants: median 0.228 deg / 0.0148, best 0.030 / 0.0031, worst 66.8 / 4.86 (a mirrored board pose); rig_board_poses median 0.186 deg
    with the solved rig, 0.219 deg with the true one."""
    from aruco3_amd import ARDictionary, CameraIntrinsics, Distortion
    from aruco3_amd import _lib as A
    from aruco3_amd import rig as rg
    from aruco3_amd.aruco import CornerRefinement, Detector, DetectorConfig
    from aruco3_amd.board import GridBoard
    from aruco3_amd.calibration import calibrate_camera_board
    from tests import board_util as bu
    from tests import calib_oracle as co
    from tests import lens_util as lu

    torch = _torch()
    d = ARDictionary.new_from_named_dict("ARUCO")
    board = GridBoard(5, 7, 30.0, 6.0)
    size = (lu.W720, lu.H720)
    Ks = [lu.K720, (850.0, 860.0, 630.0, 350.0)]
    lenses = [lu.WEBCAM, (0.0,) * 8]
    a_true = [np.array(list(K) + list(k), np.float64) for K, k in zip(Ks, lenses)]
    Rc = bu.rot_xyz(1.5, -12.0, 2.0).T
    E_true = (Rc, -Rc @ np.array([120.0, 8.0, -5.0]))
    baseline = float(np.linalg.norm(E_true[1]))
    pts = board.corners.reshape(-1, 2).astype(np.float64)
    rng = np.random.default_rng(5)
    T, frames = [], [[], []]
    while len(T) < 20:   # poses as test_end_to_end_through_a_lens draws them, kept when the whole board lies inside both fields of view
        off = (rng.uniform(-300, 300), rng.uniform(-120, 120))
        R, t = bu.board_pose_facing(board, rng.uniform(15, 40), rng.uniform(0, 360), rng.uniform(-20, 20), rng.uniform(470, 560), off, K=lu.K720)
        P = [(R, t), ru.mul(E_true, (R, t))]
        uv = [co.project(a_true[c], P[c][0], P[c][1], pts) for c in range(2)]
        if not all(np.all(np.isfinite(x)) and np.all(x >= 30) and np.all(x[:, 0] <= size[0] - 31) and np.all(x[:, 1] <= size[1] - 31) for x in uv):
            continue
        T.append((R, t))
        for c in range(2):
            frames[c].append(lu.render(board, d, P[c][0], P[c][1], k=lenses[c], K=Ks[c]))
    det = Detector(DetectorConfig(min_corner_separation_factor=bu.MIN_CORNER_SEPARATION_FACTOR), d, refinement=CornerRefinement(), board=board)
    dev = [torch.from_numpy(np.ascontiguousarray(np.stack(f)[..., None])).cuda() for f in frames]
    torch.cuda.synchronize()
    dets = [det.detect_batch(x) for x in dev]
    cals = [calibrate_camera_board(board, dets[c][:16], size, outlier_passes=2) for c in range(2)]
    assert all(c.ok for c in cals)
    rig = rg.calibrate_rig_board(board, [dets[0][:16], dets[1][:16]], cals, outlier_passes=2)
    assert rig.ok, rig.status
    both = sum(1 for f in rig.frames if f.obs_used == 2)
    print(f"{both} of 16 instants with both observations USED; rig rms {rig.rms_px:.4f} px, {rig.iterations} iterations, "
          f"{rig.points_used} points, deviations {np.round(rig.std_devs[1], 5)}")
    assert 4 * both >= 3 * 16       # the condition: the comparison below rests on at least three quarters of the instants
    # the yardstick: single-instant extrinsics from the two board poses the library returned before this feature
    bp = [det.detect_batch_with_board_pose(dev[c][:16], cals[c].intrinsics, 30.0) for c in range(2)]
    single_rot, single_tr = [], []
    for f in range(16):
        p0, p1 = bp[0][f][1], bp[1][f][1]
        if not (p0.ok and p1.ok):
            continue
        Ef = ru.mul((p1.rotation.astype(np.float64), p1.translation.astype(np.float64)), ru.inv((p0.rotation.astype(np.float64), p0.translation.astype(np.float64))))
        single_rot.append(ru.rotation_error_deg(Ef[0], E_true[0]))
        single_tr.append(float(np.linalg.norm(Ef[1] - E_true[1])) / baseline)
    assert 4 * len(single_rot) >= 3 * 16
    joint_rot = ru.rotation_error_deg(rig.rotations[1], E_true[0])
    joint_tr = float(np.linalg.norm(rig.translations[1] - E_true[1])) / baseline
    print(f"extrinsics: joint rotation error {joint_rot:.4f} deg, translation {joint_tr:.5f} of the baseline; single instants: median "
          f"{np.median(single_rot):.4f} deg / {np.median(single_tr):.5f}, best {np.min(single_rot):.4f} / {np.min(single_tr):.5f}, "
          f"worst {np.max(single_rot):.4f} / {np.max(single_tr):.5f}")
    assert joint_rot <= np.median(single_rot) and joint_tr <= np.median(single_tr)
    # fused board poses on the held-out instants
    held = [dets[0][16:], dets[1][16:]]
    true_rig = rg.RigCalibration(A.RIG_OK, np.stack(a_true), np.stack([np.eye(3), E_true[0]]), np.stack([np.zeros(3), E_true[1]]), np.zeros((2, 6)),
                                 np.zeros(2), 0.0, 0, True, 0, 0, 0)
    errs = {}
    for name, r in (("solved", rig), ("true", true_rig)):
        poses = rg.rig_board_poses(r, board, held)
        assert len(poses) == 4 and all(f.used and f.obs_used == 2 for f in poses)
        errs[name] = np.array([ru.rotation_error_deg(f.rotation, T[16 + k][0]) for k, f in enumerate(poses)])
        print(f"rig_board_poses, {name} rig: rotation error median {np.median(errs[name]):.4f} deg, max {np.max(errs[name]):.4f} deg; "
              f"rms_px {np.round([f.rms_px for f in poses], 3)}")
    assert np.median(errs["solved"]) <= 1.5 * np.median(errs["true"])
