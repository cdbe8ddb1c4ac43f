"""Marker maps on the CPU (tests/map_oracle.c, the restatement k_map is held to): recovery of known maps, an independent least-squares
cross-check, the deviations against noisy solves, a scene in which single observations pick the mirrored pose, a chain map, a fixed map
frame by frame, unseen / unreached / degenerate input, several maps in one call, the Python front end, and the struct layouts across
the C header, ctypes and the Rust mirror."""
import math
import re
from pathlib import Path

import numpy as np
import pytest

from aruco3_amd import _lib as A
from tests import calib_oracle as co
from tests import map_oracle as mo
from tests import map_util as mu

ROOT = Path(__file__).resolve().parent.parent

# Noise-free recovery, measured with this oracle on the problems below (gcc, x86-64).  The five room-corner maps: worst marker rotation
# error 1.25e-5 degrees and position error 4.07e-7 marker lengths, worst frame rotation error 2.82e-5 degrees and camera position
# error 6.43e-6 marker lengths; rms_px 1.5e-5 .. 1.8e-5, the rounding of the image corners to f32.  The map at the marker limit is a
# chain of 63 frames of four markers each, every link resting on two shared markers: 6.21e-4 degrees / 1.61e-4 lengths for the
# markers, 5.97e-4 degrees / 4.44e-4 lengths for the frames.  The bounds are ten times the worst value seen: the f32 corners set the
# floor, the factor covers other compilers.
RECOVERY = [(2, 12, "full", 11, "none"), (3, 15, "chain", 13, "webcam"), (8, 25, "missing", 15, "none"), (6, 16, "full", 16, "k1"),
            (5, 20, "missing", 14, "rational")]
MARKER_ROT_DEG, MARKER_T = 10 * 1.25e-5, 10 * 4.07e-7
FRAME_ROT_DEG, FRAME_T = 10 * 2.82e-5, 10 * 6.43e-6
LIMIT_MARKER_ROT_DEG, LIMIT_MARKER_T = 10 * 6.21e-4, 10 * 1.61e-4
LIMIT_FRAME_ROT_DEG, LIMIT_FRAME_T = 10 * 5.97e-4, 10 * 4.44e-4


def _solve(p, **kw):
    res, mres, frames, ores = mo.build_marker_maps(*mu.pack([p], **kw))
    return res[0], mres, frames, ores


@pytest.mark.parametrize("M,F,pattern,seed,lens", RECOVERY)
def test_noise_free_recovery(M, F, pattern, seed, lens):
    """markers on the three planes of a room corner, several lenses, observations missing, and a chain map in which marker 2 never
    shares a frame with marker 0"""
    p = mu.make_map(M, F, seed=seed, pattern=pattern, lens=lens)
    if pattern == "chain":
        seen = {(m, f) for m, f, _ in p["obs"]}
        assert not any((0, f) in seen and (2, f) in seen for f in range(F))
    if pattern == "missing":
        assert len(p["obs"]) < M * F
    if M >= 3:   # three planes that are not parallel
        assert abs(np.linalg.det(np.stack([p["Mw"][m][0][:, 2] for m in range(3)]))) > 0.5
    r, mres, frames, ores = _solve(p)
    assert r.status == A.MAP_OK and r.frames_used == F and r.obs_used == len(p["obs"]) and r.markers_used == M
    rot, tr = mu.marker_errors(mres, p["Mw"])
    frot, ftr = mu.frame_errors(frames, p["T"])
    print(f"M {M} F {F} {pattern}: markers {rot:.3e} deg {tr:.3e} lengths, frames {frot:.3e} deg {ftr:.3e} lengths, rms {r.rms_px:.3e} px, "
          f"{r.iterations} iterations")
    assert rot <= MARKER_ROT_DEG and tr <= MARKER_T and frot <= FRAME_ROT_DEG and ftr <= FRAME_T
    assert r.rms_px < 1e-3 and all(mres[m].rms_px < 1e-3 for m in range(M))
    assert list(mres[0].rotation) == [1, 0, 0, 0, 1, 0, 0, 0, 1] and list(mres[0].translation) == [0, 0, 0] and list(mres[0].std_dev) == [0] * 6
    h = float(np.float32(p["length"]) * np.float32(0.5))
    assert list(mres[0].corners) == [-h, h, 0, h, h, 0, h, -h, 0, -h, -h, 0]
    sq = np.concatenate([mu.square(p["length"]), np.zeros((4, 1))], 1)
    np.testing.assert_allclose(np.array(mres[1].corners).reshape(4, 3), sq @ p["Mw"][1][0].T + p["Mw"][1][1], atol=1e-5 * p["length"])
    # the float copies are the doubles rounded
    assert mres[1].translation_f[0] == np.float32(mres[1].translation[0]) and frames[0].rotation_f[4] == np.float32(frames[0].rotation[4])


def test_noise_free_recovery_at_the_marker_limit():
    p = mu.make_map(A.MAP_MAX_MARKERS, 63, seed=7, pattern="window")
    r, mres, frames, _ = _solve(p)
    assert r.status == A.MAP_OK and r.markers_used == A.MAP_MAX_MARKERS and r.frames_used == 63 and r.obs_used == 252 and r.converged
    rot, tr = mu.marker_errors(mres, p["Mw"])
    frot, ftr = mu.frame_errors(frames, p["T"])
    print(f"markers {rot:.3e} deg {tr:.3e} lengths, frames {frot:.3e} deg {ftr:.3e} lengths, rms {r.rms_px:.3e} px, {r.iterations} iterations")
    assert rot <= LIMIT_MARKER_ROT_DEG and tr <= LIMIT_MARKER_T and frot <= LIMIT_FRAME_ROT_DEG and ftr <= LIMIT_FRAME_T


def test_independent_least_squares_reaches_the_same_optimum():
    """scipy.optimize.least_squares on the same residuals, every pose a Rodrigues vector and a translation, started from the oracle's
    answer perturbed"""
    opt = pytest.importorskip("scipy.optimize")
    from scipy.spatial.transform import Rotation

    p = mu.make_map(4, 10, seed=7, noise=0.2, pattern="missing", lens="k1")
    r, mres, frames, _ = _solve(p)
    assert r.status == A.MAP_OK and r.converged
    M, F = p["M"], p["F"]
    sq = mu.square(p["length"])
    obs = [(m, f, uv.astype(np.float64)) for m, f, uv in p["obs"]]

    def poses(x, k0, n):
        return [(Rotation.from_rotvec(x[k0 + 6 * k: k0 + 6 * k + 3]).as_matrix(), x[k0 + 6 * k + 3: k0 + 6 * k + 6]) for k in range(n)]

    def residuals(x):
        Mw = [(np.eye(3), np.zeros(3))] + poses(x, 0, M - 1)
        T = poses(x, 6 * (M - 1), F)
        return np.concatenate([(co.project(p["a"], *mu.mul(T[f], Mw[m]), sq) - uv).ravel() for m, f, uv in obs])

    x0 = []
    for m in range(1, M):
        x0 += [Rotation.from_matrix(np.array(mres[m].rotation).reshape(3, 3)).as_rotvec() + 1e-3, np.array(mres[m].translation) * (1 + 1e-3)]
    for f in range(F):
        x0 += [Rotation.from_matrix(np.array(frames[f].rotation).reshape(3, 3)).as_rotvec() + 1e-3, np.array(frames[f].translation) * (1 + 1e-3)]
    sol = opt.least_squares(residuals, np.concatenate(x0), method="lm", xtol=1e-15, ftol=1e-15, gtol=1e-15, max_nfev=20000)
    rms = math.sqrt(float(np.sum(sol.fun ** 2)) / (4 * r.obs_used))
    assert abs(rms - r.rms_px) <= 1e-9 * r.rms_px
    for m in range(1, M):
        R, t = poses(sol.x, 0, M - 1)[m - 1]
        assert math.radians(mu.rotation_error_deg(R, np.array(mres[m].rotation).reshape(3, 3))) <= 1e-6
        np.testing.assert_allclose(np.array(mres[m].translation), t, rtol=0, atol=1e-6 * np.linalg.norm(t))


def test_std_dev_covers_the_truth_under_noise():
    """sigma = 0.2 px on every image coordinate, six seeds: every marker parameter within 4 of its deviations of the truth.  A
    rotation's deviations are those of the Cayley increment at the solution: compared is the w of R_true R_solved^T."""
    hits = total = 0
    for seed in range(6):
        p = mu.make_map(6, 30, seed=100 + seed, noise=0.2, pattern="missing")
        r, mres, _, _ = _solve(p)
        assert r.status == A.MAP_OK and 0.22 < r.rms_px < 0.29   # (sqrt(2) sigma less the degrees of freedom the poses absorb)
        for m in range(1, 6):
            sd = np.array(mres[m].std_dev)
            assert np.all(np.isfinite(sd)) and np.all(sd > 0)
            w = mu.cayley_w(p["Mw"][m][0] @ np.array(mres[m].rotation).reshape(3, 3).T)
            err = np.concatenate([w, p["Mw"][m][1] - np.array(mres[m].translation)])
            ok = np.abs(err) <= 4 * sd
            hits += int(ok.sum())
            total += 6
            assert ok.all(), (seed, m, err / sd)
    assert total == 6 * 30 and hits == total


@pytest.mark.parametrize("seed", [300, 301, 302, 303, 304, 305])
def test_mirrored_single_marker_poses_do_not_spoil_the_map(seed):
    """Small markers far from the camera, 0.3 px of noise: for some observations the lower-cost of step 1's two candidates is the
    mirrored pose (checked here against the true pose of that marker in that frame).  The start chooses by costs over all
    observations, so the map is the one the solve reaches when started from the true marker poses: the same optimum."""
    p = mu.make_map(5, 12, seed=seed, noise=0.3, far=2.0, frontal=0.3, length=0.08)
    flipped = 0
    for m, f, uv in p["obs"]:
        used, P, c = mo.candidates(p["a"], p["length"], uv)
        assert used
        G = mu.mul(p["T"][f], p["Mw"][m])
        lo = 0 if c[0] <= c[1] else 1
        flipped += mu.rotation_error_deg(P[lo][0], G[0]) > mu.rotation_error_deg(P[1 - lo][0], G[0])
    assert flipped >= 1, "the scene must contain a mirrored single-marker pose"
    r, mres, frames, _ = _solve(p)
    t, tm, _, _ = _solve(p, flags=A.MAP_USE_GUESS, guess=[p["Mw"]])
    print(f"seed {seed}: {flipped} of {len(p['obs'])} observations mirrored; rms {r.rms_px:.6f} px, from the truth {t.rms_px:.6f} px")
    assert r.status == A.MAP_OK and r.converged and t.converged and r.markers_used == 5
    assert abs(r.rms_px - t.rms_px) <= 1e-6 * t.rms_px
    for m in range(1, 5):
        assert mu.rotation_error_deg(np.array(mres[m].rotation).reshape(3, 3), np.array(tm[m].rotation).reshape(3, 3)) < 1e-3
        assert np.linalg.norm(np.array(mres[m].translation) - np.array(tm[m].translation)) < 1e-4 * p["length"]
    rot, tr = mu.marker_errors(mres, p["Mw"], length=p["length"])
    assert rot < 5.0 and tr < 0.2   # (a mirrored marker is tens of degrees off)


def test_fixed_map_solves_every_frame_alone_bit_for_bit():
    p = mu.make_map(6, 9, seed=17, noise=0.2, pattern="missing", lens="k1")
    r, mres, frames, ores = _solve(p, flags=A.MAP_FIX_MAP, guess=[p["Mw"]])
    assert r.status == A.MAP_OK and r.frames_used == 9
    assert list(mres[0].rotation) == [1, 0, 0, 0, 1, 0, 0, 0, 1]     # (the first marker's guess is not read)
    for m in range(1, 6):
        assert np.array_equal(np.array(mres[m].rotation).reshape(3, 3), p["Mw"][m][0]) and list(mres[m].std_dev) == [0] * 6
    its = []
    for f in range(9):
        one = dict(p, F=1, T=[p["T"][f]], obs=[(m, 0, uv) for m, g, uv in p["obs"] if g == f])
        r1, _, f1, _ = _solve(one, flags=A.MAP_FIX_MAP, guess=[p["Mw"]])
        assert bytes(f1[0]) == bytes(frames[f]), f
        its.append((r1.iterations, r1.converged))
        assert mu.rotation_error_deg(np.array(frames[f].rotation).reshape(3, 3), p["T"][f][0]) < 0.5
    assert r.iterations == max(i for i, _ in its) and r.converged == min(c for _, c in its)


def test_unseen_unreached_degenerate_and_not_connected():
    ps = mu.odd_maps()
    res, mres, frames, ores = mo.build_marker_maps(*mu.pack(ps))
    a = ps[0]
    assert [r.status for r in res] == [A.MAP_OK, A.MAP_NOT_CONNECTED, A.MAP_OK]
    assert [mres[m].status for m in range(5)] == [A.MAP_MARKER_USED] * 3 + [A.MAP_MARKER_UNREACHED, A.MAP_MARKER_UNSEEN]
    assert res[0].markers_used == 3 and res[0].frames_used == 6 and res[0].obs_used == len(a["obs"]) - 2
    assert ores[1].status == A.MAP_OBS_DEGENERATE and ores[1].rms_px == 0.0 and ores[len(a["obs"]) - 1].status == A.MAP_OBS_UNREACHED
    assert frames[6].status == A.MAP_FRAME_UNUSED and frames[6].obs_used == 0 and list(frames[6].rotation) == [0.0] * 9
    assert list(mres[3].rotation) == [0.0] * 9 and list(mres[4].corners) == [0.0] * 12 and mres[3].obs_used == 0
    rot, tr = mu.marker_errors(mres, a["Mw"], only=[1, 2])
    assert rot <= MARKER_ROT_DEG and tr <= MARKER_T
    # markers 0 and 1 never share a frame: counts and statuses, zeros elsewhere
    assert res[1].rms_px == 0.0 and res[1].iterations == 0 and res[1].markers_used == 1 and mres[6].status == A.MAP_MARKER_UNREACHED
    assert list(mres[5].rotation) == [0.0] * 9
    vals = [v for m in mres for v in list(m.rotation) + list(m.translation) + list(m.std_dev) + list(m.corners) + [m.rms_px]]
    vals += [v for f in frames for v in list(f.rotation) + list(f.translation) + [f.rms_px]] + [o.rms_px for o in ores]
    assert not any(math.isnan(v) for v in vals)
    # with the map given and fixed, the same observations are one camera pose per frame
    r, _, fr, _ = _solve(ps[1], flags=A.MAP_FIX_MAP, guess=[ps[1]["Mw"]])
    assert r.status == A.MAP_OK and r.frames_used == 6 and r.rms_px < 1e-3


def test_several_maps_equal_each_alone():
    ps = [mu.make_map([2, 3, 5][k], 9, seed=20 + k, noise=0.1 * k, pattern=["full", "chain", "missing"][k]) for k in range(3)]
    flags = [0, A.MAP_USE_GUESS, A.MAP_FIX_MAP]
    guess = [p["Mw"] for p in ps]
    packed = mu.pack(ps, flags=flags, guess=guess)
    res, mres, frames, ores = mo.build_marker_maps(*packed)
    for k, p in enumerate(ps):
        alone = mo.build_marker_maps(*mu.pack([p], flags=flags[k], guess=[guess[k]]))
        R = packed[0][k]
        assert bytes(alone[0][0]) == bytes(res[k])
        assert all(bytes(alone[1][j]) == bytes(mres[R.first_marker + j]) for j in range(R.n_markers))
        assert all(bytes(alone[2][j]) == bytes(frames[R.first_frame + j]) for j in range(R.n_frames))
        assert all(bytes(alone[3][j]) == bytes(ores[R.first_obs + j]) for j in range(R.n_obs))


def test_python_front_end_builds_the_call(tmp_path):
    """markermap's arrays through the oracle instead of the device: the same answer as the packed problem; ids map to slots, an id seen
    twice in a frame is dropped, save / load round-trip, and locate_in_map is the fixed-map call"""
    import aruco3_amd
    from aruco3_amd import markermap as mm
    from aruco3_amd.aruco import Detection, Marker

    p = mu.make_map(4, 8, seed=9, noise=0.1, pattern="missing")
    ids = [7, 3, 5, 12]     # marker k of the problem carries id ids[k]: the reference first, the others ascending
    dets = []
    for f in range(p["F"]):
        ms = [Marker(ids[m], 0, [(int(x), int(y)) for x, y in uv], 0, corners_refined=[(float(x), float(y)) for x, y in uv])
              for m, g, uv in p["obs"] if g == f]
        dets.append(Detection(markers=ms))
    dets[2].markers += [Marker(99, 0, [(1, 1), (9, 1), (9, 9), (1, 9)], 0)] * 2          # an id seen twice: dropped
    want = mo.build_marker_maps(*mu.pack([p]))
    old, mm._solve = mm._solve, lambda *a: mo.build_marker_maps(*a)
    try:
        out = aruco3_amd.build_marker_map(dets, p["a"], p["length"], reference_id=7)
        again = mm.build_marker_map(dets, p["a"], p["length"], reference_id=7, outlier_passes=1)
        held = mm.locate_in_map(out, dets[:3] + [Detection()], p["a"])
        direct = mo.build_marker_maps(*mu.pack([dict(p, F=3, T=p["T"][:3], obs=[o for o in p["obs"] if o[1] < 3])], flags=A.MAP_FIX_MAP,
                                               guess=[[out.pose(i) for i in ids]]))
    finally:
        mm._solve = old
    assert out.ok and list(out.ids) == ids and out.rms_px == want[0][0].rms_px and out.iterations == want[0][0].iterations
    for k in range(4):
        assert np.array_equal(out.rotations[k].ravel(), np.array(want[1][k].rotation)) and np.array_equal(out.std_devs[k], np.array(want[1][k].std_dev))
        assert np.array_equal(out.corners_3d(ids[k]).ravel(), np.array(want[1][k].corners))
    assert len(out.frames) == 8 and np.array_equal(out.frames[3].translation, np.array(want[2][3].translation))
    assert [(o.marker_id, o.frame) for o in out.observations] == [(ids[m], f) for m, f, _ in p["obs"]]
    assert again.ok and again.obs_used <= out.obs_used
    assert len(held) == 4 and not held[3].used and all(h.used for h in held[:3])
    assert all(np.array_equal(held[f].rotation.ravel(), np.array(direct[2][f].rotation)) for f in range(3))
    for name in ("m.json", "m.npz"):
        out.save(tmp_path / name)
        back = mm.MarkerMap.load(tmp_path / name)
        assert back.ok and np.array_equal(back.ids, out.ids) and np.array_equal(back.rotations, out.rotations)
        assert np.array_equal(back.corners, out.corners) and back.marker_length == out.marker_length and np.array_equal(back.std_devs, out.std_devs)
    with pytest.raises(ValueError):
        mm.build_marker_map(dets, p["a"], p["length"], reference_id=1000)


def test_layouts_match_across_c_ctypes_and_rust():
    import ctypes as C

    lay = mo.layout()
    py = [C.sizeof(A.Map), A.Map.a.offset, A.Map.marker_length.offset, C.sizeof(A.MapMarker), A.MapMarker.guess_translation.offset,
          C.sizeof(A.MapObservation), C.sizeof(A.MapResult), A.MapResult.rms_px.offset, C.sizeof(A.MapMarkerResult),
          A.MapMarkerResult.std_dev.offset, A.MapMarkerResult.corners.offset, A.MapMarkerResult.rotation_f.offset, A.MapMarkerResult.status.offset,
          C.sizeof(A.MapFrame), A.MapFrame.rotation.offset, A.MapFrame.rotation_f.offset, C.sizeof(A.MapObservationResult),
          A.MapObservationResult.start_rms_px.offset]
    assert lay == py == [136, 32, 128, 96, 72, 8, 32, 24, 304, 96, 152, 248, 296, 160, 16, 112, 16, 8]
    text = re.sub(r"//[^\n]*", "", (ROOT / "integration" / "aruco3_hip.rs").read_text())
    header = re.sub(r"/\*.*?\*/", "", (ROOT / "include" / "aruco3_hip.h").read_text(), flags=re.S)
    for c_name, r_name in (("a3_map", "A3Map"), ("a3_map_marker", "A3MapMarker"), ("a3_map_observation", "A3MapObservation"),
                           ("a3_map_result", "A3MapResult"), ("a3_map_marker_result", "A3MapMarkerResult"), ("a3_map_frame", "A3MapFrame"),
                           ("a3_map_observation_result", "A3MapObservationResult")):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (c_name, c_name), header, flags=re.S).group(1)
        c_fields = []
        for decl in body.split(";"):
            decl = decl.strip()
            if decl:
                for n in decl.split(None, 1)[1].split(","):
                    c_fields.append(re.sub(r"\[.*?\]", "", n).split()[-1])
        m = re.search(r"#\[repr\(C\)\]\s*(?:#\[derive\([^\]]*\)\]\s*)?pub struct %s \{(.*?)\}" % r_name, text, flags=re.S)
        assert m and re.findall(r"pub\s+([a-z0-9_]+)\s*:", m.group(1)) == c_fields, c_name
