"""Camera calibration on the MI355X (k_calibrate; a3_calibrate_cameras): every output bit-equal to the CPU restatement
(tests/calib_oracle.c) across view counts, point counts, flags, noise, bad views and an iteration cap; several cameras in one launch
equal to each alone; the ABI's refusals; detection unchanged around a call; and a camera calibrated from detected markers of frames
rendered through a real lens, then used for board poses."""
import ctypes as C

import numpy as np
import pytest

from tests import calib_oracle as co
from tests import calib_util as cu

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


def _check(cams, offsets, obj, img):
    """the device against the oracle, raw bits of every record -> the device's (results, views)"""
    res, views = _ctx().calibrate_cameras(cams, offsets, obj, img)
    ores, oviews = co.calibrate(cams, offsets, obj, img)
    n_views = len(offsets) - 1
    for k in range(len(cams)):
        assert bytes(res[k]) == bytes(ores[k]), (k, cu.params(res[k]) - cu.params(ores[k]), res[k].iterations, ores[k].iterations)
    for v in range(n_views):
        assert bytes(views[v]) == bytes(oviews[v]), v
    return res, views


def _one(p, **kw):
    return _check(cu.one_camera(p, **kw), p["offsets"], p["obj"], p["img"])


@pytest.mark.parametrize("kind,n_views", [("charuco", 1), ("charuco", 3), ("charuco", 25), ("grid", 25), ("charuco", 500), ("grid", 3)])
def test_bit_equal_views_and_points(kind, n_views):
    from aruco3_amd import _lib

    p = cu.problem(kind, n_views, seed=n_views, coeffs=cu.WEBCAM)
    res, _ = _one(p)
    assert n_views == 1 or res[0].status == _lib.CALIB_OK


def test_bit_equal_four_and_max_points():
    from aruco3_amd import _lib

    p = cu.problem("grid", 25, seed=31, coeffs=cu.WEBCAM)
    keep = np.concatenate([np.arange(p["offsets"][v], p["offsets"][v] + 4) for v in range(25)])   # one marker's 4 corners per view
    res, _ = _check(cu.one_camera(p), np.arange(26, dtype=np.uint32) * 4, p["obj"][keep], p["img"][keep])
    assert res[0].views_used == 25
    d = cu.problem("dense", 3, seed=32, coeffs=cu.WEBCAM)
    assert int(d["offsets"][1]) == _lib.CALIB_MAX_POINTS
    res, _ = _one(d)
    assert res[0].status == _lib.CALIB_OK


@pytest.mark.parametrize("flags", [0, 1, 2, 4, 8, 1 | 2 | 4, 8 | 2])
def test_bit_equal_flags_and_noise(flags):
    coeffs = cu.RATIONAL if flags & 8 else cu.WEBCAM5
    _one(cu.problem("grid", 25, seed=40 + flags, coeffs=coeffs, noise=0.2), flags=flags)
    _one(cu.problem("charuco", 25, seed=60 + flags, coeffs=coeffs), flags=flags)


def test_bit_equal_guess_and_iteration_cap():
    from aruco3_amd import _lib

    p = cu.problem("grid", 25, seed=70, coeffs=cu.WEBCAM, noise=0.1)
    guess = [v * 1.2 for v in p["truth"][:4]] + [-0.2, 0.05, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0]
    _one(p, flags=_lib.CALIB_USE_INTRINSIC_GUESS, guess=guess)
    _one(p, flags=_lib.CALIB_USE_INTRINSIC_GUESS | _lib.CALIB_FIX_PRINCIPAL_POINT | _lib.CALIB_FIX_K3, guess=guess)
    res, _ = _one(p, max_iterations=3)
    assert res[0].iterations == 3 and res[0].converged == 0


def test_bit_equal_bad_views_and_failed_cameras():
    from aruco3_amd import _lib

    p = cu.problem("grid", 6, seed=80, coeffs=cu.WEBCAM)
    obj, img = list(np.split(p["obj"], p["offsets"][1:-1])), list(np.split(p["img"], p["offsets"][1:-1]))
    obj[1], img[1] = obj[1][:3], img[1][:3]
    line = np.array([[x, 0.0] for x in range(8)], np.float32)
    obj[2], img[2] = line, np.stack([100.0 + 10 * line[:, 0], 200.0 + 3 * line[:, 0]], 1).astype(np.float32)
    offs = np.concatenate([[0], np.cumsum([len(o) for o in obj])]).astype(np.uint32)
    # camera 0: the six views; camera 1: one view of 4 points (TOO_FEW); camera 2: fronto-parallel views (NO_INIT)
    pts = cu.target_points("grid")
    a = list(cu.K720) + [0.0] * 8
    for k in range(4):
        obj.append(pts.astype(np.float32))
        img.append(co.project(a, np.diag([1.0, -1.0, -1.0]), np.array([-60.0 + 10 * k, 50.0 - 5 * k, 500.0 + 30 * k]), pts).astype(np.float32))
    obj.insert(6, obj[0][:4])
    img.insert(6, img[0][:4])
    offs = np.concatenate([[0], np.cumsum([len(o) for o in obj])]).astype(np.uint32)
    cams = cu.cameras([dict(size=p["size"], first_view=0, n_views=6), dict(size=p["size"], first_view=6, n_views=1),
                       dict(size=p["size"], first_view=7, n_views=4)])
    res, views = _check(cams, offs, np.concatenate(obj), np.concatenate(img))
    assert [r.status for r in res] == [_lib.CALIB_OK, _lib.CALIB_TOO_FEW, _lib.CALIB_NO_INIT]
    assert [views[i].status for i in range(3)] == [_lib.CALIB_VIEW_USED, _lib.CALIB_VIEW_TOO_FEW_POINTS, _lib.CALIB_VIEW_DEGENERATE]


def test_several_cameras_in_one_launch_equal_each_alone():
    ps = [cu.problem(["charuco", "grid"][k % 2], 25, seed=90 + k, coeffs=[cu.WEBCAM, cu.WEBCAM5][k % 2], noise=0.1 * (k % 3)) for k in range(16)]
    flags = [0, 1, 2, 4, 0, 3, 5, 6, 0, 1, 2, 4, 7, 0, 2, 0]
    obj = np.concatenate([p["obj"] for p in ps])
    img = np.concatenate([p["img"] for p in ps])
    offs = [0]
    for p in ps:
        offs += list(p["offsets"][1:] + offs[-1])
    specs = [dict(size=p["size"], first_view=25 * k, n_views=25, flags=flags[k]) for k, p in enumerate(ps)]
    res, views = _check(cu.cameras(specs), np.array(offs, np.uint32), obj, img)
    for k, p in enumerate(ps):
        alone, aviews = _ctx().calibrate_cameras(cu.one_camera(p, flags=flags[k]), p["offsets"], p["obj"], p["img"])
        assert bytes(alone[0]) == bytes(res[k])
        assert all(bytes(aviews[j]) == bytes(views[25 * k + j]) for j in range(25))


def test_refusals_and_detection_unchanged():
    from aruco3_amd import _lib, synth
    from aruco3_amd.dictionaries import ARDictionary

    torch = _torch()
    L = _lib.load()
    d = ARDictionary.new_from_named_dict("ARUCO_DEFAULT")
    ctx = _lib.Context(_lib.default_config(), d.code_list, d.num_bits, d._tau)
    frames, _ = synth.config_frames(1, 4)
    dev = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    n, h, w = frames.shape[:3]
    before = ctx.detect_batch(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, n)
    p = cu.problem("charuco", 5, seed=5, coeffs=cu.WEBCAM)
    off = np.ascontiguousarray(p["offsets"])
    obj, img = np.ascontiguousarray(p["obj"]), np.ascontiguousarray(p["img"])
    res = (_lib.CalibResult * 2)()
    views = (_lib.CalibView * 5)()
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)

    def call(cams, n_cams=None, offsets=off, o=obj, i=img, r=res):
        return L.a3_calibrate_cameras(ctx.handle, cams, len(cams) if n_cams is None else n_cams, offsets.ctypes.data_as(u32p) if offsets is not None else None,
                                      5, o.ctypes.data_as(f32p) if o is not None else None, i.ctypes.data_as(f32p), r, views)

    good = cu.one_camera(p)
    assert call(good) == _lib.OK
    assert call(good, offsets=None) == _lib.ERR_INVALID
    assert call(good, o=None) == _lib.ERR_INVALID
    assert call(good, r=None) == _lib.ERR_INVALID
    assert call(good, n_cams=0) == _lib.ERR_INVALID
    for field, value in (("flags", 32), ("image_width", 0), ("image_height", 70000), ("max_iterations", 1001), ("n_views", 0), ("n_views", 6)):
        bad = cu.one_camera(p)
        setattr(bad[0], field, value)
        assert call(bad) == _lib.ERR_INVALID, field
    bad = cu.one_camera(p, flags=_lib.CALIB_USE_INTRINSIC_GUESS, guess=[0.0] * 12)
    assert call(bad) == _lib.ERR_INVALID
    overlap = cu.cameras([dict(size=p["size"], first_view=0, n_views=3), dict(size=p["size"], first_view=2, n_views=3)])
    assert call(overlap) == _lib.ERR_INVALID
    nan = img.copy()
    nan[7, 1] = np.nan
    assert call(good, i=nan) == _lib.ERR_INVALID
    # a batch in flight
    ctx.submit(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, n)
    assert call(good) == _lib.ERR_INVALID
    mid = ctx.collect()
    assert call(good) == _lib.OK
    after = ctx.detect_batch(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, n)
    for a, b in ((before, mid), (before, after)):
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


def test_views_no_camera_owns_come_back_zero():
    """ranges need not cover every view: one left out is all zero, not what an earlier call left in the device buffer"""
    from aruco3_amd import _lib

    p = cu.problem("charuco", 6, seed=9, coeffs=cu.WEBCAM)
    _, views = _ctx().calibrate_cameras(cu.one_camera(p), p["offsets"], p["obj"], p["img"])
    assert views[5].status == _lib.CALIB_VIEW_USED
    cams = cu.cameras([dict(size=p["size"], first_view=0, n_views=5)])
    res, views = _check(cams, p["offsets"], p["obj"], p["img"])
    assert res[0].status == _lib.CALIB_OK and bytes(views[5]) == bytes(_lib.CalibView())


def _lens_displacement_px(params, pts):
    """how far the solved lens moves the pixels `pts` (n, 2): max over the points, in pixels"""
    from aruco3_amd import Distortion

    a = np.asarray(params, np.float64)
    x = (np.asarray(pts, np.float64) - a[[2, 3]]) / a[[0, 1]]
    xd = Distortion(*[float(v) for v in a[4:12]]).distort_normalized(x)
    return float(np.max(np.linalg.norm((xd - x) * a[[0, 1]], axis=1)))


def test_end_to_end_through_a_lens():
    """16 views of a 5 x 7 GridBoard rendered at 1280 x 720 through the WEBCAM lens, detected with refinement and calibrated by
    calibrate_camera_board; then board poses of 4 held-out frames with the calibrated camera against the same call with the true one.
    The detected corners carry outliers (a corner whose refinement fell back to the integer quad corner is 2-8 px off; now and then a
    marker is misread): the plain solve misses the principal point by about 10 px, the helper's outlier_passes=2 meets every target."""
    from aruco3_amd import ARDictionary, CameraIntrinsics, Distortion
    from aruco3_amd.aruco import CornerRefinement, Detector, DetectorConfig
    from aruco3_amd.board import GridBoard
    from aruco3_amd.calibration import calibrate_camera_board
    from tests import board_util as bu
    from tests import lens_util as lu

    torch = _torch()
    d = ARDictionary.new_from_named_dict("ARUCO")
    board = GridBoard(5, 7, 30.0, 6.0)
    rng = np.random.default_rng(5)
    scenes, frames = [], []
    while len(frames) < 20:
        off = (rng.uniform(-300, 300), rng.uniform(-120, 120))
        R, t = bu.board_pose_facing(board, rng.uniform(15, 40), rng.uniform(0, 360), rng.uniform(-20, 20), rng.uniform(470, 560), off, K=lu.K720)
        scenes.append((R, t))
        frames.append(lu.render(board, d, R, t))
    dev = torch.from_numpy(np.ascontiguousarray(np.stack(frames)[..., None])).cuda()
    torch.cuda.synchronize()
    det = Detector(DetectorConfig(min_corner_separation_factor=bu.MIN_CORNER_SEPARATION_FACTOR), d, refinement=CornerRefinement(), board=board)
    dets = det.detect_batch(dev[:16])
    size = (lu.W720, lu.H720)
    plain = calibrate_camera_board(board, dets, size)
    assert plain.ok
    print(f"plain solve: {np.round(plain.params[:5], 3)} rms {plain.rms_px:.3f} px")
    cal = calibrate_camera_board(board, dets, size, outlier_passes=2)
    assert cal.ok, cal.status
    assert len(cal.inliers) == 16 and sum(int(k.sum()) for k in cal.inliers) == cal.points_used
    fx, fy, cx, cy = cal.params[:4]
    print(f"calibrated: fx {fx:.3f} fy {fy:.3f} cx {cx:.3f} cy {cy:.3f} k {np.round(cal.params[4:9], 5)} rms {cal.rms_px:.4f} px, "
          f"{cal.views_used} views, {cal.points_used} of {plain.points_used} points, {cal.iterations} iterations")
    # first measured run: fx 899.26, fy 899.56, cx 639.07, cy 359.64, k1 -0.2786, rms 0.30 px (truth 900, 900, 640, 360, -0.28)
    K = lu.K720
    assert abs(fx - K[0]) < 0.005 * K[0] and abs(fy - K[1]) < 0.005 * K[1]
    assert abs(cx - K[2]) < 3.0 and abs(cy - K[3]) < 3.0
    assert abs(cal.params[4] - lu.WEBCAM[0]) < 0.02
    truth = CameraIntrinsics(lu.W720, lu.H720, *K, distortion=Distortion(*lu.WEBCAM))
    errs, rms = {}, {}
    for name, intr in (("calibrated", cal.intrinsics), ("true", truth)):
        out = det.detect_batch_with_board_pose(dev[16:], intr, 30.0)
        assert all(bp.ok for _, bp in out)
        errs[name] = np.array([bu.rotation_error_deg(bp.rotation, scenes[16 + f][0]) for f, (_, bp) in enumerate(out)])
        rms[name] = np.array([bp.rms_px for _, bp in out])
        print(f"{name}: board rotation error median {np.median(errs[name]):.3f} deg, max {np.max(errs[name]):.3f} deg; "
              f"board rms_px per frame {np.round(rms[name], 3)}")
    # The board pose keeps every detected corner, outliers included, so its rms_px on these frames is set by the detections: the
    # true camera and lens give 1.9 px at most.  What the calibration controls is how far its camera is from the true one's.
    assert np.all(rms["calibrated"] <= 1.05 * rms["true"] + 0.02)
    assert np.median(errs["calibrated"]) <= 1.5 * np.median(errs["true"])


def test_end_to_end_charuco():
    """30 ChArUco frames (5 x 7 board, 1080p, pinhole K1080, tilted 15 .. 50 degrees) rendered on the device, detection-only batches,
    calibrate_camera_charuco from Detection.charuco_ids / .charuco_corners: K1080 comes back and the lens stays near zero.  A view
    without corners passes through, so that view indices match the frames."""
    from aruco3_amd import ARDictionary, calibrate_camera_charuco
    from aruco3_amd import _lib
    from aruco3_amd.aruco import CornerRefinement, Detector, DetectorConfig
    from aruco3_amd.board import CharucoBoard
    from tests import board_util as bu
    from tests import charuco_util as chu

    torch = _torch()
    d = ARDictionary.new_from_named_dict("ARUCO_DEFAULT")
    board = CharucoBoard(5, 7, 40.0, 28.0, first_id=5)
    scenes = [chu.Scene(board, R, t) for R, t in chu.tilted_poses(board, 30, seed=21, tilt=(15.0, 50.0), distance=900.0)]
    dev = chu.render(scenes, d)
    torch.cuda.synchronize()
    det = Detector(DetectorConfig(min_corner_separation_factor=bu.MIN_CORNER_SEPARATION_FACTOR), d, refinement=CornerRefinement(), board=board)
    dets = det.detect_batch(dev)
    truth = np.concatenate([chu.true_corners(board, sc.R, sc.t)[x.charuco_ids] for x, sc in zip(dets, scenes)])
    seen = np.concatenate([x.charuco_corners for x in dets])
    print(f"{len(seen)} corners in {len(dets)} frames, median error {np.median(np.linalg.norm(seen - truth, axis=1)):.4f} px")
    views = list(dets) + [(None, None)]
    cal = calibrate_camera_charuco(board, views, (bu.W1080, bu.H1080))
    assert cal.ok, cal.status
    assert len(cal.views) == 31 and cal.views[30].status == _lib.CALIB_VIEW_TOO_FEW_POINTS
    # a frame whose corners all lie on one chessboard row is DEGENERATE (collinear points fix no homography) and left out
    assert cal.points_used == sum(v.points for v in cal.views if v.used)
    assert all(v.used or v.status == _lib.CALIB_VIEW_DEGENERATE for v in cal.views[:30] if v.points >= 4)
    fx, fy, cx, cy = cal.params[:4]
    lens_seen = _lens_displacement_px(cal.params, seen)
    lens_frame = _lens_displacement_px(cal.params, np.stack(np.meshgrid([0.0, bu.W1080 - 1.0], [0.0, bu.H1080 - 1.0]), -1).reshape(-1, 2))
    print(f"calibrated: fx {fx:.3f} fy {fy:.3f} cx {cx:.3f} cy {cy:.3f} k {np.round(cal.params[4:9], 5)} rms {cal.rms_px:.4f} px, "
          f"{cal.views_used} of 30 views, {cal.points_used} points; lens moves the seen corners by {lens_seen:.3f} px at most, "
          f"the frame corners by {lens_frame:.3f} px")
    K = bu.K1080
    assert abs(fx - K[0]) < 0.005 * K[0] and abs(fy - K[1]) < 0.005 * K[1]
    assert abs(cx - K[2]) < 3.0 and abs(cy - K[3]) < 3.0
    # The views cover the middle of the frame only, where k2 and k3 barely act: over the corners seen the solved lens is near zero,
    # and every coefficient lies within 4 of its deviations of the true 0; outside them the free k3 extrapolates to anything.
    assert lens_seen < 0.5 and cal.rms_px < 0.2
    for c in (cal, calibrate_camera_charuco(board, views, (bu.W1080, bu.H1080), fix_k3=True)):
        free = c.std_devs[4:] > 0
        print(f"k {np.round(c.params[4:9], 5)} +- {np.round(c.std_devs[4:9], 5)}")
        assert np.all(np.abs(c.params[4:][free]) <= 4.0 * c.std_devs[4:][free])
