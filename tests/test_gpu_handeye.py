"""Hand-eye calibration on the MI355X (k_handeye; a3_calibrate_hand_eyes): every output bit-equal to the CPU restatement
(tests/handeye_oracle.c) across frame and point counts, both set-ups, the mounts the four charts exist for, both flags, noise, an
iteration cap, bad frames and robots that do not move enough; several problems in one launch equal to each alone; the ABI's refusals;
detection unchanged around a call; and a camera on a simulated flange looking at a rendered board, detected and then calibrated."""
import ctypes as C

import numpy as np
import pytest

from tests import handeye_oracle as ho
from tests import handeye_util as hu

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
    """the device against the oracle, raw bits of every record -> the device's (results, frame results)"""
    dev = _ctx().calibrate_hand_eyes(*packed)
    ora = ho.calibrate_hand_eyes(*packed)
    for k in range(len(packed[0])):
        assert bytes(dev[0][k]) == bytes(ora[0][k]), (k, dev[0][k].status, ora[0][k].status, dev[0][k].iterations, ora[0][k].iterations,
                                                      dev[0][k].pairs_used, ora[0][k].pairs_used, dev[0][k].rms_px, ora[0][k].rms_px)
    for k in range(len(packed[1])):
        assert bytes(dev[1][k]) == bytes(ora[1][k]), ("frame", k, dev[1][k].status, ora[1][k].status)
    return dev


@pytest.mark.parametrize("setup", ["eye_in_hand", "eye_to_hand"])
@pytest.mark.parametrize("F", [3, 4, 25, 256])
def test_bit_equal_frames_and_setups(F, setup):
    from aruco3_amd import _lib

    p = hu.make_problem(F=F, seed=100 + F + (setup == "eye_to_hand"), setup=setup, mount="small" if setup == "eye_in_hand" else "y90")
    res = _check(hu.pack([p]))[0]
    assert res[0].status == _lib.HANDEYE_OK and res[0].frames_used == F and res[0].pairs_used > 0


@pytest.mark.parametrize("mount", list(hu.MOUNTS))
def test_bit_equal_mounts(mount):
    from aruco3_amd import _lib

    p = hu.make_problem(F=4, seed=200 + list(hu.MOUNTS).index(mount), mount=mount)
    res = _check(hu.pack([p]))[0]
    assert res[0].status == _lib.HANDEYE_OK and res[0].pairs_used == 6
    rot, tr = hu.errors(res, p)
    assert rot < 1e-3 and tr < 1e-2


def test_bit_equal_four_and_max_points():
    from aruco3_amd import _lib

    p = hu.make_problem(F=3, seed=31, kind="marker")
    assert all(len(o) == 4 for o, _ in p["obs"])
    res = _check(hu.pack([p]))[0]
    assert res[0].status == _lib.HANDEYE_OK and res[0].points_used == 12
    d = hu.make_problem(F=3, seed=32, kind="dense")
    assert len(d["obs"][0][0]) == _lib.CALIB_MAX_POINTS
    res = _check(hu.pack([d]))[0]
    assert res[0].status == _lib.HANDEYE_OK and res[0].points_used == 3 * _lib.CALIB_MAX_POINTS


def test_bit_equal_flags_noise_and_iteration_cap():
    from aruco3_amd import _lib

    p = hu.make_problem(F=25, seed=41, kind="grid", noise=0.2, mount="d120")
    near = ((hu.bu.rot_xyz(0.5, -0.4, 0.3) @ p["X"][0], p["X"][1] + [2.0, -1.0, 1.5]), (hu.bu.rot_xyz(-0.3, 0.6, 0.2) @ p["Y"][0], p["Y"][1] + [3.0, 1.0, -2.0]))
    far = ((hu.bu.rot_xyz(8.0, -6.0, 10.0) @ p["X"][0], p["X"][1] + [40.0, -30.0, 25.0]), (hu.bu.rot_xyz(-7.0, 9.0, 5.0) @ p["Y"][0], p["Y"][1] + [60.0, 40.0, -50.0]))
    free = _check(hu.pack([p]))[0]
    assert free[0].status == _lib.HANDEYE_OK and free[0].converged == 1
    _check(hu.pack([p], flags=_lib.HANDEYE_USE_GUESS, guess=[near]))
    res = _check(hu.pack([p], flags=_lib.HANDEYE_USE_GUESS, guess=[far]))[0]
    assert res[0].status == _lib.HANDEYE_OK and res[0].pairs_used == 0 and abs(res[0].rms_px - free[0].rms_px) < 1e-6
    res = _check(hu.pack([p], flags=_lib.HANDEYE_FIX_X, guess=[(p["X"], None)]))[0]
    assert list(res[0].std_dev[:6]) == [0.0] * 6 and list(res[0].x_translation) == list(p["X"][1])
    _check(hu.pack([p], flags=_lib.HANDEYE_FIX_X | _lib.HANDEYE_USE_GUESS, guess=[near], max_iterations=2))
    res = _check(hu.pack([p], flags=_lib.HANDEYE_USE_GUESS, guess=[far], max_iterations=2))[0]
    assert res[0].iterations == 2
    res = _check(hu.pack([p], max_iterations=1))[0]
    assert res[0].iterations == 1 and res[0].converged == 0


def test_bit_equal_bad_frames_and_robots_that_do_not_move_enough():
    from aruco3_amd import _lib

    ps = [hu.make_problem(F=6, seed=42, few=(1,), collinear=(4,)), hu.make_problem(F=4, seed=41, few=(1, 3)),
          hu.make_problem(F=8, seed=43, motion="translate"), hu.make_problem(F=8, seed=44, motion="one_axis"),
          hu.make_problem(F=6, seed=45, noise=0.1)]
    res, fres = _check(hu.pack(ps))
    assert [r.status for r in res] == [_lib.HANDEYE_OK, _lib.HANDEYE_TOO_FEW_FRAMES, _lib.HANDEYE_NO_MOTION, _lib.HANDEYE_NO_MOTION, _lib.HANDEYE_OK]
    assert fres[1].status == _lib.HANDEYE_FRAME_TOO_FEW_POINTS and fres[4].status == _lib.HANDEYE_FRAME_DEGENERATE and res[0].frames_used == 4
    assert res[2].pairs_used == 0 and res[3].pairs_used == 28 and res[1].rms_px == 0.0 and list(res[3].x_rotation) == [0.0] * 9


def test_sixteen_problems_in_one_launch_equal_each_alone():
    from aruco3_amd import _lib

    mounts = list(hu.MOUNTS)
    ps = [hu.make_problem(F=[3, 5, 12, 25][k % 4], seed=90 + k, kind=["charuco", "grid"][k % 2], noise=0.1 * (k % 3), mount=mounts[k % 5],
                          setup=["eye_in_hand", "eye_to_hand"][(k // 2) % 2]) for k in range(16)]
    flags = [0, 0, 2, 0, 1, 0, 2, 0, 0, 3, 0, 0, 1, 0, 2, 0]
    guess = [(p["X"], p["Y"]) for p in ps]
    packed = hu.pack(ps, flags=flags, guess=guess)
    res, fres = _check(packed)
    assert all(r.status == _lib.HANDEYE_OK for r in res)
    for k, p in enumerate(ps):
        alone = _ctx().calibrate_hand_eyes(*hu.pack([p], flags=flags[k], guess=[guess[k]]))
        R = packed[0][k]
        assert bytes(alone[0][0]) == bytes(res[k])
        assert all(bytes(alone[1][j]) == bytes(fres[R.first_frame + j]) for j in range(R.n_frames))


def test_refusals_and_detection_unchanged():
    """the input errors are refused with a message, the context stays usable, and a detection batch gives the same bytes before and
    after hand-eye calls"""
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
    p = hu.make_problem(F=3, seed=1)
    f32p = C.POINTER(C.c_float)
    res, fres = (A.HandEyeResult * 2)(), (A.HandEyeFrameResult * 8)()
    L.a3_last_error.restype = C.c_char_p

    def call(mod=None, null=None, n_problems=1, n_frames=3, **kw):
        probs, frames, obj, img = hu.pack([p], **kw)
        if mod:
            mod(probs, frames, obj, img)
        args = dict(probs=probs, frames=frames, obj=obj.ctypes.data_as(f32p), img=img.ctypes.data_as(f32p), res=res)
        if null:
            args[null] = None
        rc = L.a3_calibrate_hand_eyes(ctx.handle, args["probs"], n_problems, args["frames"], n_frames, args["obj"], args["img"], args["res"], fres)
        if rc != A.OK:
            assert b"a3_calibrate_hand_eyes" in L.a3_last_error(ctx.handle)
        return rc

    def setter(what, field, value, index=0):
        def mod(probs, frames, obj, img):
            setattr({"prob": probs, "frame": frames}[what][index], field, value)
        return mod

    assert call() == A.OK and res[0].status == A.HANDEYE_OK
    for null in ("probs", "frames", "obj", "img", "res"):
        assert call(null=null) == A.ERR_INVALID, null
    assert call(n_problems=0) == A.ERR_INVALID and call(n_problems=1025) == A.ERR_INVALID
    assert call(n_frames=0) == A.ERR_INVALID and call(n_frames=65537) == A.ERR_INVALID and call(n_frames=2) == A.ERR_INVALID
    for what, field, value in (("prob", "flags", 4), ("prob", "max_iterations", 1001), ("prob", "n_frames", 0), ("prob", "n_frames", 257),
                               ("prob", "first_frame", 1), ("frame", "n_points", 4097), ("frame", "first_point", 0xffffffff)):
        assert call(setter(what, field, value)) == A.ERR_INVALID, (what, field, value)

    def shared(probs, frames, obj, img):
        probs[0].n_frames = 2

    def bad_focal(probs, frames, obj, img):
        probs[0].a[1] = 0.0

    def nan_lens(probs, frames, obj, img):
        probs[0].a[5] = float("nan")

    def nan_point(probs, frames, obj, img):
        img[7, 1] = np.nan

    def nan_robot(probs, frames, obj, img):
        frames[1].rotation[4] = float("nan")

    def inf_robot(probs, frames, obj, img):
        frames[2].translation[0] = float("inf")

    def inf_guess_x(probs, frames, obj, img):
        probs[0].guess_x_translation[2] = float("inf")

    def inf_guess_y(probs, frames, obj, img):
        probs[0].guess_y_rotation[0] = float("inf")

    def skewed_robot(probs, frames, obj, img):   # not orthonormal: the caller's business, not refused
        frames[0].rotation[1] += 0.01

    for mod in (bad_focal, nan_lens, nan_point, nan_robot, inf_robot):
        assert call(mod) == A.ERR_INVALID, mod.__name__
    assert call(shared) == A.OK and res[0].status == A.HANDEYE_TOO_FEW_FRAMES        # (two frames of three: allowed, and too few)
    two = hu.pack([p, p])
    two[0][1].first_frame = 2                                                          # the second problem overlaps the first
    assert L.a3_calibrate_hand_eyes(ctx.handle, two[0], 2, two[1], 6, two[2].ctypes.data_as(f32p), two[3].ctypes.data_as(f32p), res, fres) == A.ERR_INVALID
    assert call(inf_guess_x, flags=A.HANDEYE_USE_GUESS) == A.ERR_INVALID and call(inf_guess_x, flags=A.HANDEYE_FIX_X) == A.ERR_INVALID
    assert call(inf_guess_y, flags=A.HANDEYE_USE_GUESS) == A.ERR_INVALID
    assert call(inf_guess_y, flags=A.HANDEYE_FIX_X, guess=[(p["X"], None)]) == A.OK     # (Y's guess is not read under FIX_X alone)
    assert call(inf_guess_x) == A.OK                                                   # (not read without the flags)
    assert call(skewed_robot) == A.OK
    # a batch in flight
    ctx.submit(dev.data_ptr(), A.MEM_DEVICE, A.FMT_RGB8, w, h, w * 3, w * h * 3, n)
    assert call() == A.ERR_INVALID
    mid = ctx.collect()
    assert call() == A.OK
    want = ho.calibrate_hand_eyes(*hu.pack([p]))
    assert bytes(res[0]) == bytes(want[0][0]) and bytes(fres[2]) == bytes(want[1][2])
    after = ctx.detect_batch(dev.data_ptr(), A.MEM_DEVICE, A.FMT_RGB8, w, h, w * 3, w * h * 3, n)
    for a, b in ((before, mid), (before, after)):
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


# The end-to-end scene on the CPU: its 12 frames through the detector's and the refinement's CPU restatements (hu.cpu_detections), then
# calibrate_hand_eye_board(outlier_passes=2) with the oracle in the device's place.  Measured (gcc 13, x86-64): 27 .. 35 markers per
# frame, rms 0.284 px, 4 iterations; camera -> gripper off the simulation's truth by 0.00444 degrees and 0.1033 board units, board ->
# base by 0.00834 degrees and 0.0414 units (without the outlier passes: rms 1.445 px, 0.0251 degrees, 0.420 units).  The bounds are
# ten times these.
E2E_MOUNT_DEG, E2E_MOUNT_T = 10 * 0.00444, 10 * 0.1033
E2E_BOARD_DEG, E2E_BOARD_T = 10 * 0.00834, 10 * 0.0414


def test_end_to_end_camera_on_a_flange():
    """A pinhole camera nearly upside down on a simulated flange looks at one 5 x 7 GridBoard from 12 robot poses.  The frames are
    detected with refinement on the device; calibrate_hand_eye_board(outlier_passes=2) then runs twice on those detections, on the
    device and with the oracle in its place: the two answers are the same bytes.  The mount and the board's place come back within
    ten times what the same pipeline achieves on the CPU (the figures above)."""
    from aruco3_amd import handeye as he
    from aruco3_amd.aruco import CornerRefinement, Detector, DetectorConfig

    torch = _torch()
    s = hu.scene()
    det = Detector(DetectorConfig(min_corner_separation_factor=hu.bu.MIN_CORNER_SEPARATION_FACTOR), s["dictionary"], refinement=CornerRefinement(),
                   board=s["board"])
    dev = torch.from_numpy(np.ascontiguousarray(np.stack(s["frames"])[..., None])).cuda()
    torch.cuda.synchronize()
    dets = det.detect_batch(dev)
    assert all(len(x.markers) >= 20 for x in dets)
    got = he.calibrate_hand_eye_board(s["board"], dets, s["robot"], s["a"], outlier_passes=2)
    old, he._solve = he._solve, lambda *a: ho.calibrate_hand_eyes(*a)
    try:
        want = he.calibrate_hand_eye_board(s["board"], dets, s["robot"], s["a"], outlier_passes=2)
    finally:
        he._solve = old
    assert got.ok and got.frames_used == hu.SCENE_FRAMES
    assert got.rms_px == want.rms_px and got.iterations == want.iterations
    for a, b in ((got.X, want.X), (got.Y, want.Y)):
        assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    assert np.array_equal(got.std_devs, want.std_devs) and all(np.array_equal(a, b) for a, b in zip(got.inliers, want.inliers))
    R, t = got.camera_to_gripper()
    Rt, tt = hu.inv(s["X"])
    mount = (hu.rotation_error_deg(R, Rt), float(np.linalg.norm(t - tt)))
    place = (hu.rotation_error_deg(got.board_to_base()[0], s["Y"][0]), float(np.linalg.norm(got.board_to_base()[1] - s["Y"][1])))
    print(f"rms {got.rms_px:.4f} px, {got.iterations} iterations, {got.points_used} points; camera -> gripper off by {mount[0]:.5f} deg, "
          f"{mount[1]:.4f} units; board -> base by {place[0]:.5f} deg, {place[1]:.4f} units")
    assert mount[0] <= E2E_MOUNT_DEG and mount[1] <= E2E_MOUNT_T and place[0] <= E2E_BOARD_DEG and place[1] <= E2E_BOARD_T
