"""Fisheye camera calibration on the MI355X (k_calibrate_fisheye; a3_calibrate_fisheye_cameras): every output bit-equal to the CPU
restatement (tests/fisheye_calib_oracle.c) across view counts, point counts, flags, noise, guesses, bad views and an iteration cap;
several cameras in one launch equal to each alone; the ABI's refusals; detection and the rational calibration unchanged around a call;
and a camera calibrated from detected markers of frames rendered through a fisheye lens, then used for rectification and board poses."""
import ctypes as C

import numpy as np
import pytest

from tests import calib_oracle as co
from tests import calib_util as cu
from tests import fisheye_calib_oracle as fco
from tests import fisheye_calib_util as fu

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
    res, views = _ctx().calibrate_fisheye_cameras(cams, offsets, obj, img)
    ores, oviews = fco.calibrate(cams, offsets, obj, img)
    n_views = len(offsets) - 1
    for k in range(len(cams)):
        assert bytes(res[k]) == bytes(ores[k]), (k, fu.params(res[k]) - fu.params(ores[k]), res[k].status, ores[k].status, res[k].iterations,
                                                 ores[k].iterations)
    for v in range(n_views):
        assert bytes(views[v]) == bytes(oviews[v]), v
    return res, views


def _one(p, **kw):
    return _check(fu.one_camera(p, **kw), p["offsets"], p["obj"], p["img"])


def _first_points(p, n):
    """the problem with the first n points of every view"""
    nv = len(p["offsets"]) - 1
    keep = np.concatenate([np.arange(p["offsets"][v], p["offsets"][v] + n) for v in range(nv)])
    return dict(p, obj=p["obj"][keep], img=p["img"][keep], offsets=(np.arange(nv + 1) * n).astype(np.uint32))


@pytest.mark.parametrize("n_views", [1, 3, 5, 25])
def test_bit_equal_views(n_views):
    from aruco3_amd import _lib

    res, views = _one(fu.problem("charuco", n_views, seed=n_views, coeffs=fu.MILD))
    assert all(views[v].status == _lib.CALIB_VIEW_USED for v in range(n_views))
    assert n_views == 1 or res[0].status == _lib.CALIB_OK


@pytest.mark.parametrize("n_points", [4, 24, 64, 65, 140])
def test_bit_equal_points_per_view(n_points):
    """(65 crosses the 64-row LDS chunk)"""
    p = fu.problem("grid", 25, seed=31, coeffs=fu.STRONG)
    res, _ = _one(_first_points(p, n_points))
    assert res[0].views_used == 25 and res[0].points_used == 25 * n_points


def test_bit_equal_max_points():
    from aruco3_amd import _lib

    d = fu.problem("dense", 3, seed=32, coeffs=fu.MILD)
    assert int(d["offsets"][1]) == _lib.CALIB_MAX_POINTS
    res, _ = _one(d)
    assert res[0].status == _lib.CALIB_OK


@pytest.mark.parametrize("flags", [0, 1, 2, 4, 8, 16, 1 | 8 | 16])
def test_bit_equal_flags_and_noise(flags):
    from aruco3_amd import _lib

    res, _ = _one(fu.problem("grid", 25, seed=40 + flags, coeffs=fu.STRONG, noise=0.2), flags=flags)
    assert res[0].status == _lib.CALIB_OK
    res, _ = _one(fu.problem("charuco", 25, seed=60 + flags, coeffs=fu.MILD), flags=flags)
    assert res[0].status == _lib.CALIB_OK


def test_bit_equal_guess_and_iteration_cap():
    from aruco3_amd import _lib

    p = fu.problem("grid", 25, seed=70, coeffs=fu.STRONG, noise=0.1)
    guess = [v * 1.2 for v in p["truth"][:4]] + [0.05, -0.01, 0.004, -0.001]
    G = _lib.FISHEYE_USE_INTRINSIC_GUESS
    res, _ = _one(p, flags=G, guess=guess)
    assert res[0].status == _lib.CALIB_OK
    res, _ = _one(p, flags=G | _lib.FISHEYE_FIX_PRINCIPAL_POINT | _lib.FISHEYE_FIX_K3 | _lib.FISHEYE_FIX_K4, guess=guess)
    assert res[0].cx == np.float32(guess[2]) and res[0].dist[4] == np.float32(guess[6]) and res[0].dist[5] == np.float32(guess[7])
    res, _ = _one(p, max_iterations=3)
    assert res[0].iterations == 3 and res[0].converged == 0


def test_bit_equal_bad_views_and_failed_cameras():
    from aruco3_amd import _lib
    from tests.test_oracle_fisheye_calib import bad_view_mix

    obj, img, want, size = bad_view_mix()
    # camera 0: the six views of the mix; camera 1: one view of 4 points (TOO_FEW)
    obj.append(obj[0][:4])
    img.append(img[0][:4])
    offs = np.concatenate([[0], np.cumsum([len(o) for o in obj])]).astype(np.uint32)
    cams = fu.cameras([dict(size=size, first_view=0, n_views=6), dict(size=size, first_view=6, n_views=1)])
    res, views = _check(cams, offs, np.concatenate(obj), np.concatenate(img))
    assert [r.status for r in res] == [_lib.CALIB_OK, _lib.CALIB_TOO_FEW]
    assert [views[i].status for i in range(7)] == want + [_lib.CALIB_VIEW_USED]
    assert res[0].views_used == 3 and res[0].points_used == 140 + 24 + 140


def test_several_cameras_in_one_launch_equal_each_alone():
    ps = [fu.problem(["charuco", "grid"][k % 2], 25, seed=90 + k, coeffs=[fu.MILD, fu.STRONG][k % 2], noise=0.1 * (k % 3)) for k in range(16)]
    flags = [0, 1, 2, 4, 8, 16, 3, 5, 24, 0, 1, 2, 25, 0, 16, 0]
    obj = np.concatenate([p["obj"] for p in ps])
    img = np.concatenate([p["img"] for p in ps])
    offs = [0]
    for p in ps:
        offs += list(p["offsets"][1:] + offs[-1])
    specs = [dict(size=p["size"], first_view=25 * k, n_views=25, flags=flags[k]) for k, p in enumerate(ps)]
    res, views = _check(fu.cameras(specs), np.array(offs, np.uint32), obj, img)
    for k, p in enumerate(ps):
        alone, aviews = _ctx().calibrate_fisheye_cameras(fu.one_camera(p, flags=flags[k]), p["offsets"], p["obj"], p["img"])
        assert bytes(alone[0]) == bytes(res[k])
        assert all(bytes(aviews[j]) == bytes(views[25 * k + j]) for j in range(25))


def test_refusals_and_the_rest_unchanged():
    """the ABI's refusals; detection batches byte-equal before and after a call; a3_calibrate_cameras byte-equal to its oracle after a
    fisheye call on the same context"""
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
    p = fu.problem("charuco", 5, seed=5, coeffs=fu.MILD)
    off = np.ascontiguousarray(p["offsets"])
    obj, img = np.ascontiguousarray(p["obj"]), np.ascontiguousarray(p["img"])
    res = (_lib.CalibResult * 2)()
    views = (_lib.CalibView * 5)()
    u32p, f32p = C.POINTER(C.c_uint32), C.POINTER(C.c_float)

    def call(cams, n_cams=None, offsets=off, o=obj, i=img, r=res, n_views=5):
        return L.a3_calibrate_fisheye_cameras(ctx.handle, cams, len(cams) if n_cams is None else n_cams,
                                              offsets.ctypes.data_as(u32p) if offsets is not None else None, n_views,
                                              o.ctypes.data_as(f32p) if o is not None else None, i.ctypes.data_as(f32p), r, views)

    good = fu.one_camera(p)
    assert call(good) == _lib.OK
    ores, oviews = fco.calibrate(good, off, obj, img)
    assert bytes(res[0]) == bytes(ores[0]) and all(bytes(views[v]) == bytes(oviews[v]) for v in range(5))
    assert call(good, offsets=None) == _lib.ERR_INVALID
    assert call(good, o=None) == _lib.ERR_INVALID
    assert call(good, r=None) == _lib.ERR_INVALID
    assert call(None, n_cams=1) == _lib.ERR_INVALID
    assert call(good, n_cams=0) == _lib.ERR_INVALID
    assert call(good, n_views=0) == _lib.ERR_INVALID
    for field, value in (("flags", 64), ("flags", 128 | 1), ("image_width", 0), ("image_height", 70000), ("max_iterations", 1001), ("n_views", 0),
                         ("n_views", 6)):
        bad = fu.one_camera(p)
        setattr(bad[0], field, value)
        assert call(bad) == _lib.ERR_INVALID, field
    G = _lib.FISHEYE_USE_INTRINSIC_GUESS
    assert call(fu.one_camera(p, flags=G, guess=[0.0] * 8)) == _lib.ERR_INVALID                 # focal lengths <= 0
    ok_guess = list(p["truth"])
    assert call(fu.one_camera(p, flags=G, guess=ok_guess)) == _lib.OK
    for field in ("p1", "p2", "k5", "k6"):
        bad = fu.one_camera(p, flags=G, guess=ok_guess)
        setattr(bad[0].guess_distortion, field, 1e-3)
        assert call(bad) == _lib.ERR_INVALID, field                                            # a rational coefficient in the guess
        bad[0].flags = 0
        assert call(bad) == _lib.OK                                                            # ... which is not read without the flag
    bad = fu.one_camera(p, flags=G, guess=ok_guess)
    bad[0].guess_distortion.k3 = float("nan")
    assert call(bad) == _lib.ERR_INVALID
    overlap = fu.cameras([dict(size=p["size"], first_view=0, n_views=3), dict(size=p["size"], first_view=2, n_views=3)])
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
    # the rational calibration on the same context, after the fisheye call used its buffers
    q = cu.problem("charuco", 9, seed=6, coeffs=cu.WEBCAM)
    qc = cu.one_camera(q)
    rres, rviews = ctx.calibrate_cameras(qc, q["offsets"], q["obj"], q["img"])
    wres, wviews = co.calibrate(qc, q["offsets"], q["obj"], q["img"])
    assert rres[0].status == _lib.CALIB_OK and bytes(rres[0]) == bytes(wres[0])
    assert all(bytes(rviews[v]) == bytes(wviews[v]) for v in range(9))


def test_views_no_camera_owns_come_back_zero():
    from aruco3_amd import _lib

    p = fu.problem("charuco", 6, seed=9, coeffs=fu.MILD)
    _, views = _ctx().calibrate_fisheye_cameras(fu.one_camera(p), p["offsets"], p["obj"], p["img"])
    assert views[5].status == _lib.CALIB_VIEW_USED
    cams = fu.cameras([dict(size=p["size"], first_view=0, n_views=5)])
    res, views = _check(cams, p["offsets"], p["obj"], p["img"])
    assert res[0].status == _lib.CALIB_OK and bytes(views[5]) == bytes(_lib.CalibView())


# the end-to-end frames: 960 x 540, lens_util's K720 scaled by 3 / 4 (tests/fisheye_util.py renders on the host, inverting the lens for
# nine subsamples of every pixel: a 1280 x 720 frame costs 1.8 times as much, and 12 + 3 frames of it can pass 20 s on a slow host)
E2E_SIZE = (960, 540)
E2E_K = (675.0, 675.0, 480.0, 270.0)


def test_end_to_end_through_a_fisheye_lens():
    """12 views of a 5 x 7 GridBoard rendered through the MILD fisheye lens, detected with refinement and calibrated by
    calibrate_camera_board(model="fisheye"); a held-out frame rectified with the result; board poses of 3 held-out frames with the
    calibrated camera against the same call with the true one."""
    from aruco3_amd import ARDictionary, CameraIntrinsics, Distortion, rectify_frames
    from aruco3_amd.aruco import CornerRefinement, Detector, DetectorConfig
    from aruco3_amd.board import GridBoard
    from aruco3_amd.calibration import calibrate_camera_board
    from tests import board_util as bu
    from tests import fisheye_util as fzu

    torch = _torch()
    d = ARDictionary.new_from_named_dict("ARUCO")
    board = GridBoard(5, 7, 30.0, 6.0)
    rng = np.random.default_rng(5)
    W, H = E2E_SIZE
    scenes, frames = [], []
    while len(frames) < 15:
        off = (rng.uniform(-225, 225), rng.uniform(-90, 90))
        R, t = bu.board_pose_facing(board, rng.uniform(15, 40), rng.uniform(0, 360), rng.uniform(-20, 20), rng.uniform(470, 560), off, K=E2E_K)
        scenes.append((R, t))
        frames.append(fzu.render(board, d, R, t, K=E2E_K, width=W, height=H))
    dev = torch.from_numpy(np.ascontiguousarray(np.stack(frames)[..., None])).cuda()
    torch.cuda.synchronize()
    det = Detector(DetectorConfig(min_corner_separation_factor=bu.MIN_CORNER_SEPARATION_FACTOR), d, refinement=CornerRefinement(), board=board)
    dets = det.detect_batch(dev[:12])
    cal = calibrate_camera_board(board, dets, (W, H), model="fisheye", fix_k3=True, fix_k4=True, outlier_passes=2)
    assert cal.ok and cal.model == "fisheye", cal.status
    assert len(cal.inliers) == 12 and sum(int(k.sum()) for k in cal.inliers) == cal.points_used
    fx, fy, cx, cy = cal.params[:4]
    print(f"calibrated: fx {fx:.3f} fy {fy:.3f} cx {cx:.3f} cy {cy:.3f} D {np.round(cal.distortion_coeffs, 5)} rms {cal.rms_px:.4f} px, "
          f"{cal.views_used} views, {cal.points_used} points, {cal.iterations} iterations")
    K = E2E_K
    assert abs(fx - K[0]) < 0.005 * K[0] and abs(fy - K[1]) < 0.005 * K[1]
    assert abs(cx - K[2]) < 3.0 and abs(cy - K[3]) < 3.0
    assert cal.params[8] == 0.0 and cal.params[9] == 0.0
    # a held-out frame rectified with the result: the board's markers are found in the rectified view
    flat = rectify_frames(frames[12], cal.intrinsics)
    assert flat.shape == (1, H, W, 1)
    fdev = torch.from_numpy(np.ascontiguousarray(flat)).cuda()
    assert len(det.detect_batch(fdev)[0].markers) >= 30
    truth = CameraIntrinsics(W, H, *K, distortion=Distortion.fisheye(*fzu.MILD))
    errs = {}
    for name, intr in (("calibrated", cal.intrinsics), ("true", truth)):
        out = det.detect_batch_with_board_pose(dev[12:], intr, 30.0)
        assert all(bp.ok for _, bp in out)
        errs[name] = np.array([bu.rotation_error_deg(bp.rotation, scenes[12 + f][0]) for f, (_, bp) in enumerate(out)])
        print(f"{name}: board rotation error per held-out frame {np.round(errs[name], 4)} deg")
    assert np.max(errs["calibrated"]) <= 1.5 * np.max(errs["true"])
