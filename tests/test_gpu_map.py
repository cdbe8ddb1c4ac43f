"""Marker maps on the MI355X (k_map; a3_build_marker_maps): every output bit-equal to the CPU restatement (tests/map_oracle.c) across
marker and frame counts, a map at A3_MAP_MAX_MARKERS, both flags, noise, an iteration cap, unseen and unreached markers and a
degenerate observation; several maps in one launch equal to each alone; a FIX_MAP frame equal to its one-frame call; the ABI's
refusals; detection unchanged around a call; and a rendered room corner detected, mapped and localised in."""
import ctypes as C

import numpy as np
import pytest

from tests import map_oracle as mo
from tests import map_util as mu

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
    """the device against the oracle, raw bits of every record -> the device's (results, marker results, frames, observation results)"""
    dev = _ctx().build_marker_maps(*packed)
    ora = mo.build_marker_maps(*packed)
    maps, markers, obs = packed[:3]
    n_frames = max(int(r.first_frame) + int(r.n_frames) for r in maps)
    for k in range(len(maps)):
        assert bytes(dev[0][k]) == bytes(ora[0][k]), (k, dev[0][k].status, ora[0][k].status, dev[0][k].iterations, ora[0][k].iterations,
                                                      dev[0][k].rms_px, ora[0][k].rms_px)
    for k in range(len(markers)):
        assert bytes(dev[1][k]) == bytes(ora[1][k]), ("marker", k, list(dev[1][k].translation), list(ora[1][k].translation),
                                                      list(dev[1][k].std_dev), list(ora[1][k].std_dev))
    for k in range(n_frames):
        assert bytes(dev[2][k]) == bytes(ora[2][k]), ("frame", k)
    for k in range(len(obs)):
        assert bytes(dev[3][k]) == bytes(ora[3][k]), ("observation", k)
    return dev


@pytest.mark.parametrize("M,F,pattern", [(2, 1, "full"), (2, 3, "full"), (3, 3, "chain"), (8, 25, "missing")])
def test_bit_equal_markers_and_frames(M, F, pattern):
    from aruco3_amd import _lib

    p = mu.make_map(M, F, seed=100 + M + F, pattern=pattern)
    res = _check(mu.pack([p]))[0]
    assert res[0].status == _lib.MAP_OK and res[0].frames_used == F and res[0].markers_used == M


def test_bit_equal_at_the_marker_limit():
    """128 markers, four per frame: the reduced system of order 762 in device scratch, its workgroup LDL^T and solve, the sparse block
    terms and the 762 unit-vector solves"""
    from aruco3_amd import _lib

    p = mu.make_map(_lib.MAP_MAX_MARKERS, 63, seed=7, pattern="window")
    res, mres = _check(mu.pack([p]))[:2]
    assert res[0].status == _lib.MAP_OK and res[0].markers_used == _lib.MAP_MAX_MARKERS and res[0].obs_used == 252
    assert all(np.isfinite(list(mres[m].std_dev)).all() for m in range(_lib.MAP_MAX_MARKERS))


@pytest.mark.parametrize("M", [2, 3, 8])
def test_bit_equal_flags_noise_and_iteration_cap(M):
    from aruco3_amd import _lib
    from tests import board_util as bu

    p = mu.make_map(M, 25, seed=40 + M, noise=0.2, pattern="missing", lens="webcam")
    near = [(bu.rot_xyz(0.5, -0.4, 0.3) @ R, t + np.array([0.01, -0.02, 0.015])) for R, t in p["Mw"]]
    _check(mu.pack([p]))
    _check(mu.pack([p], flags=_lib.MAP_USE_GUESS, guess=[near]))
    _check(mu.pack([p], flags=_lib.MAP_FIX_MAP, guess=[p["Mw"]]))
    _check(mu.pack([p], flags=_lib.MAP_FIX_MAP | _lib.MAP_USE_GUESS, guess=[near], max_iterations=2))
    res = _check(mu.pack([p], max_iterations=1))[0]
    assert res[0].iterations == 1 and res[0].converged == 0


def test_bit_equal_unseen_unreached_degenerate_and_a_map_that_is_not_connected():
    from aruco3_amd import _lib

    ps = mu.odd_maps()
    res, mres, frames, ores = _check(mu.pack(ps))
    assert [r.status for r in res] == [_lib.MAP_OK, _lib.MAP_NOT_CONNECTED, _lib.MAP_OK]
    assert mres[4].status == _lib.MAP_MARKER_UNSEEN and mres[3].status == _lib.MAP_MARKER_UNREACHED and res[0].markers_used == 3
    assert ores[1].status == _lib.MAP_OBS_DEGENERATE and any(o.status == _lib.MAP_OBS_UNREACHED for o in ores)
    assert frames[ps[0]["F"] - 1].status == _lib.MAP_FRAME_UNUSED and res[1].rms_px == 0.0


def test_sixteen_maps_in_one_launch_equal_each_alone():
    from aruco3_amd import _lib

    ps = [mu.make_map([2, 3, 5][k % 3], 12, seed=90 + k, noise=0.1 * (k % 3), lens=["none", "k1", "rational"][k % 3],
                      pattern=["full", "missing", "chain"][k % 3 if k % 3 != 2 else 1 + (k // 3) % 2]) for k in range(16)]
    flags = [0, 0, 2, 0, 1, 0, 2, 0, 0, 3, 0, 0, 1, 0, 2, 0]
    guess = [p["Mw"] for p in ps]
    packed = mu.pack(ps, flags=flags, guess=guess)
    res, mres, frames, ores = _check(packed)
    assert all(r.status == _lib.MAP_OK for r in res)
    for k, p in enumerate(ps):
        alone = _ctx().build_marker_maps(*mu.pack([p], flags=flags[k], guess=[guess[k]]))
        R = packed[0][k]
        assert bytes(alone[0][0]) == bytes(res[k])
        assert all(bytes(alone[1][j]) == bytes(mres[R.first_marker + j]) for j in range(R.n_markers))
        assert all(bytes(alone[2][j]) == bytes(frames[R.first_frame + j]) for j in range(R.n_frames))
        assert all(bytes(alone[3][j]) == bytes(ores[R.first_obs + j]) for j in range(R.n_obs))


def test_a_fix_map_frame_equals_its_one_frame_call():
    from aruco3_amd import _lib

    p = mu.make_map(6, 9, seed=17, noise=0.2, pattern="missing", lens="k1")
    whole = _check(mu.pack([p], flags=_lib.MAP_FIX_MAP, guess=[p["Mw"]]))
    for f in range(p["F"]):
        one = dict(p, F=1, T=[p["T"][f]], obs=[(m, 0, uv) for m, g, uv in p["obs"] if g == f])
        alone = _check(mu.pack([one], flags=_lib.MAP_FIX_MAP, guess=[p["Mw"]]))
        assert bytes(alone[2][0]) == bytes(whole[2][f]), f


def test_refusals_and_detection_unchanged():
    """the input errors are refused, the context stays usable, and a detection batch gives the same bytes before and after map calls"""
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
    p = mu.make_map(2, 3, seed=1)
    f32p = C.POINTER(C.c_float)
    res, mres = (A.MapResult * 1)(), (A.MapMarkerResult * 16)()
    frames, ores = (A.MapFrame * 8)(), (A.MapObservationResult * 16)()

    def call(mod=None, null=None, n_maps=1, **kw):
        maps, markers, obs, img = mu.pack([p], **kw)
        if mod:
            mod(maps, markers, obs, img)
        args = dict(maps=maps, markers=markers, obs=obs, img=img.ctypes.data_as(f32p), res=res, mres=mres)
        if null:
            args[null] = None
        return L.a3_build_marker_maps(ctx.handle, args["maps"], n_maps, args["markers"], 2, args["obs"], len(p["obs"]), args["img"], args["res"],
                                      args["mres"], frames, ores)

    def setter(what, field, value, index=0):
        def mod(maps, markers, obs, img):
            setattr({"map": maps, "obs": obs}[what][index], field, value)
        return mod

    assert call() == A.OK and res[0].status == A.MAP_OK
    for null in ("maps", "markers", "obs", "img", "res", "mres"):
        assert call(null=null) == A.ERR_INVALID, null
    assert call(n_maps=0) == A.ERR_INVALID
    for what, field, value in (("map", "n_markers", 0), ("map", "n_markers", 129), ("map", "flags", 4), ("map", "max_iterations", 1001),
                               ("map", "n_frames", 0), ("map", "n_frames", 4097), ("map", "n_obs", 0), ("map", "n_obs", 7),
                               ("map", "first_marker", 1), ("map", "marker_length", 0.0), ("map", "marker_length", float("nan")),
                               ("obs", "marker", 2), ("obs", "frame", 3)):
        assert call(setter(what, field, value)) == A.ERR_INVALID, (what, field, value)

    def duplicate(maps, markers, obs, img):
        obs[1].marker, obs[1].frame = obs[0].marker, obs[0].frame

    def out_of_order(maps, markers, obs, img):
        obs[0].frame, obs[2].frame = obs[2].frame, obs[0].frame

    def bad_focal(maps, markers, obs, img):
        maps[0].a[0] = 0.0

    def nan_lens(maps, markers, obs, img):
        maps[0].a[5] = float("nan")

    def nan_corner(maps, markers, obs, img):
        img[3, 1] = np.nan

    def inf_guess(maps, markers, obs, img):
        markers[1].guess_translation[2] = float("inf")

    for mod in (duplicate, out_of_order, bad_focal, nan_lens, nan_corner):
        assert call(mod) == A.ERR_INVALID, mod.__name__
    assert call(inf_guess, flags=A.MAP_USE_GUESS) == A.ERR_INVALID and call(inf_guess, flags=A.MAP_FIX_MAP) == A.ERR_INVALID
    assert call(inf_guess) == A.OK                     # (not read without the flags)
    # a batch in flight
    ctx.submit(dev.data_ptr(), A.MEM_DEVICE, A.FMT_RGB8, w, h, w * 3, w * h * 3, n)
    assert call() == A.ERR_INVALID
    mid = ctx.collect()
    assert call() == A.OK
    want = mo.build_marker_maps(*mu.pack([p]))
    assert bytes(res[0]) == bytes(want[0][0]) and bytes(mres[1]) == bytes(want[1][1]) and bytes(frames[2]) == bytes(want[2][2])
    after = ctx.detect_batch(dev.data_ptr(), A.MEM_DEVICE, A.FMT_RGB8, w, h, w * 3, w * h * 3, n)
    for a, b in ((before, mid), (before, after)):
        assert a[0].tobytes() == b[0].tobytes() and np.array_equal(a[1], b[1])


E2E_IDS = [3, 7, 11, 20, 25, 31]
# Tolerances of the end-to-end test: the oracle on this scene's true projections plus Gaussian noise of 0.3 px
# per coordinate (above the detector's refined-corner error, median 0.20 px radial, section 4.5), worst of ten noise seeds: markers
# 0.434 degrees / 0.0203 marker lengths, held-out camera poses 0.332 degrees / 0.0813 lengths.  The bounds are three times that: one
# homography per marker keeps a marker's edges straight where the k1 lens bends them (a quarter of a pixel at an edge's middle),
# and the refinement's error is not Gaussian.
E2E_MARKER_ROT_DEG, E2E_MARKER_T = 3 * 0.434, 3 * 0.0203
E2E_FRAME_ROT_DEG, E2E_FRAME_T = 3 * 0.332, 3 * 0.0813


def e2e_scene():
    """6 markers on three planes, 16 camera poses seeing all of them through the k1 lens: 12 to map with, 4 held out"""
    return mu.make_map(6, 16, seed=5, lens="k1", far=0.8)


def _render(p, d):
    """the scene's frames on the device (a3_synth_render): every marker a sticker painted through the homography of its four
    projected corners -> (N, H, W, 3) uint8 CUDA tensor"""
    import math

    from aruco3_amd import _lib, synth

    torch = _torch()
    w, h = mu.SIZE
    frames = np.zeros(p["F"], dtype=synth.SYNTH_FRAME_DTYPE)
    recs = []
    for f in range(p["F"]):
        mine = [(m, uv) for m, g, uv in p["obs"] if g == f]
        frames[f] = (200.0, 6.0, -4.0, 0.0, len(recs), len(mine), f + 1)
        for m, uv in mine:
            cells = synth.marker_cells(int(d.code_list[E2E_IDS[m]]), d.num_bits)
            n = cells.shape[0]
            H = synth._homography(np.array([[0, 0], [n, 0], [n, n], [0, n]], np.float64), uv.astype(np.float64))
            outer = (H @ np.array([[-1, -1, 1], [n + 1, -1, 1], [n + 1, n + 1, 1], [-1, n + 1, 1]], np.float64).T).T
            outer = outer[:, :2] / outer[:, 2:3]
            x0, x1 = max(int(math.floor(outer[:, 0].min())) - 1, 0), min(int(math.ceil(outer[:, 0].max())) + 2, w)
            y0, y1 = max(int(math.floor(outer[:, 1].min())) - 1, 0), min(int(math.ceil(outer[:, 1].max())) + 2, h)
            bits = 0
            for r in range(n):
                for c in range(n):
                    bits |= int(cells[r, c]) << (r * n + c)
            recs.append((np.linalg.inv(H).astype(np.float32).reshape(9), x0, y0, x1, y1, (bits & (2 ** 64 - 1), bits >> 64), n, 0))
    marr = np.zeros(len(recs), dtype=synth.SYNTH_MARKER_DTYPE)
    for i, r in enumerate(recs):
        marr[i] = r
    out = torch.empty((p["F"], h, w, 3), dtype=torch.uint8, device="cuda")
    _lib.synth_render(0, frames, marr, w, h, False, 25.0, 235.0, 3, out.data_ptr(), w * 3, w * h * 3)
    torch.cuda.synchronize()
    return out


def test_end_to_end_a_room_corner_mapped_and_localised_in():
    """16 frames of 1280 x 720 rendered on the device: 6 markers on three planes (one homography per marker, its corners where the k1
    lens puts them), detected with refinement.  build_marker_map(outlier_passes=2) on the first 12, locate_in_map on the other 4;
    marker poses and camera poses against the truth, within E2E_* (set from the oracle and the detector's corner error, not from this
    kernel: see above).  The device's map equals the oracle's on the same detections bit for bit."""
    from aruco3_amd import ARDictionary
    from aruco3_amd import _lib as A
    from aruco3_amd import markermap as mm
    from aruco3_amd.aruco import CornerRefinement, Detector, DetectorConfig
    from tests import board_util as bu

    p = e2e_scene()
    d = ARDictionary.new_from_named_dict("ARUCO")
    det = Detector(DetectorConfig(min_corner_separation_factor=bu.MIN_CORNER_SEPARATION_FACTOR), d, refinement=CornerRefinement())
    dets = det.detect_batch(_render(p, d))
    found = sum(1 for x in dets for m in x.markers if m.id in E2E_IDS)
    errs = [float(np.linalg.norm(np.asarray(k.corners_refined if k.corners_refined is not None else k.corners, np.float64)[j] - uv[j]))
            for m, f, uv in p["obs"] for k in dets[f].markers if k.id == E2E_IDS[m] for j in range(4)]
    print(f"{found} of {len(p['obs'])} markers found; corner error median {np.median(errs):.3f} px, 90th percentile {np.percentile(errs, 90):.3f} px, "
          f"max {np.max(errs):.3f} px")
    assert 10 * found >= 9 * len(p["obs"])       # the condition: the comparison rests on at least nine tenths of the markers
    cam = p["a"]
    got = mm.build_marker_map(dets[:12], cam, p["length"], reference_id=E2E_IDS[0], outlier_passes=2)
    assert got.ok, got.status
    old, mm._solve = mm._solve, lambda *a: mo.build_marker_maps(*a)
    try:
        want = mm.build_marker_map(dets[:12], cam, p["length"], reference_id=E2E_IDS[0], outlier_passes=2)
    finally:
        mm._solve = old
    assert np.array_equal(got.rotations, want.rotations) and np.array_equal(got.translations, want.translations)
    assert np.array_equal(got.std_devs, want.std_devs) and got.rms_px == want.rms_px and got.obs_used == want.obs_used
    rot = tr = 0.0
    for m in range(1, 6):
        assert got.marker_status[got.index(E2E_IDS[m])] == A.MAP_MARKER_USED
        R, t = got.pose(E2E_IDS[m])
        rot = max(rot, mu.rotation_error_deg(R, p["Mw"][m][0]))
        tr = max(tr, float(np.linalg.norm(t - p["Mw"][m][1]) / p["length"]))
    print(f"map: rms {got.rms_px:.3f} px over {got.obs_used} observations, {got.iterations} iterations; markers {rot:.3f} deg, {tr:.4f} lengths; "
          f"deviations of marker {E2E_IDS[1]}: {np.round(got.std_devs[got.index(E2E_IDS[1])], 5)}")
    assert rot <= E2E_MARKER_ROT_DEG and tr <= E2E_MARKER_T
    held = mm.locate_in_map(got, dets[12:], cam)
    assert len(held) == 4 and all(x.used for x in held)
    frot = max(mu.rotation_error_deg(x.rotation, p["T"][12 + k][0]) for k, x in enumerate(held))
    ftr = max(float(np.linalg.norm(x.position + p["T"][12 + k][0].T @ p["T"][12 + k][1]) / p["length"]) for k, x in enumerate(held))
    print(f"held-out frames: camera {frot:.3f} deg, {ftr:.4f} lengths; rms_px {np.round([x.rms_px for x in held], 3)}")
    assert frot <= E2E_FRAME_ROT_DEG and ftr <= E2E_FRAME_T
