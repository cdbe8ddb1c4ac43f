"""Marker map problems with a known answer: square markers on the three planes of a room corner, camera poses drawn so that every
marker a frame is meant to see lies inside the image and faces the camera, projected in f64 through the contract's forward model
(tests/calib_oracle.c) and rounded to f32 image corners.  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

from aruco3_amd import _lib as A
from tests import calib_oracle as co
from tests import calib_util as cu
from tests.rig_util import cayley_w, inv, mul, records_equal, rotation_error_deg  # noqa: F401  (shared helpers)

SIZE = (1280, 720)
LENGTH = 0.15   # metres
K = (900.0, 905.0, 641.5, 357.25)
LENSES = {"none": (0.0,) * 8, "k1": (-0.1, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0), "webcam": cu.WEBCAM, "rational": cu.RATIONAL}
# marker axes (x, y, normal) in room coordinates on the floor z = 0 and the walls x = 0 and y = 0
PLANES = [np.array([[1.0, 0, 0], [0, 1.0, 0], [0, 0, 1.0]]).T, np.array([[0, 1.0, 0], [0, 0, 1.0], [1.0, 0, 0]]).T,
          np.array([[0, 0, 1.0], [1.0, 0, 0], [0, 1.0, 0]]).T]


def square(length=LENGTH) -> np.ndarray:
    """the four object points of a marker, a3_marker order, exactly as the contract forms them (h in float)"""
    h = float(np.float32(length) * np.float32(0.5))
    return np.array([[-h, h], [h, h], [h, -h], [-h, -h]], np.float64)


def camera_params(lens="none") -> np.ndarray:
    return np.array(list(K) + list(LENSES[lens]), np.float64)


def room_markers(M: int, rng, length=LENGTH):
    """marker -> room (R, t): marker k on plane k % 3, grid slot k // 3 (a snake over the grid), turned in its plane"""
    per = (M + 2) // 3
    g = max(1, math.ceil(math.sqrt(per)))
    out = []
    for k in range(M):
        s = k // 3
        i, j = s // g, s % g
        if i % 2:
            j = g - 1 - j
        u, v = (1.5 + 2.2 * i) * length + rng.uniform(-0.2, 0.2) * length, (1.5 + 2.2 * j) * length + rng.uniform(-0.2, 0.2) * length
        B = PLANES[k % 3]
        th = rng.uniform(0, 2 * math.pi)
        Rz = np.array([[math.cos(th), -math.sin(th), 0], [math.sin(th), math.cos(th), 0], [0, 0, 1.0]])
        out.append((B @ Rz, B[:, 0] * u + B[:, 1] * v))
    return out


def visibility(M: int, F: int, pattern: str, rng) -> np.ndarray:
    """sees[f, m].  'full'; 'missing': about a third of the observations dropped, every third frame tying a marker to its successor;
    'chain': frame f sees markers f % (M - 1) and the next, so that marker 2 never shares a frame with marker 0; 'window': frame f
    sees the four markers from 2 f on (wrapping back so that the last window ends at the last marker)"""
    sees = np.ones((F, M), bool)
    if pattern == "missing":
        sees = rng.uniform(size=(F, M)) > 0.33
        for f in range(F):
            if f % 3 == 0:
                m = (f // 3) % M
                sees[f, m] = sees[f, (m + 1) % M] = True
            elif not sees[f].any():
                sees[f, f % M] = True
    elif pattern == "chain":
        sees[:] = False
        for f in range(F):
            m = f % (M - 1)
            sees[f, m] = sees[f, m + 1] = True
    elif pattern == "window":
        sees[:] = False
        for f in range(F):
            s = min((2 * f) % max(M - 2, 1), max(M - 4, 0))
            sees[f, s:s + 4] = True
    return sees


def look_at(pos, target, roll_deg):
    """room -> camera (R, t) of a camera at pos looking at target, z up, rolled about its axis"""
    fw = (target - pos) / np.linalg.norm(target - pos)
    right = np.cross(fw, np.array([0, 0, 1.0]))
    right /= np.linalg.norm(right)
    down = np.cross(fw, right)
    c, s = math.cos(math.radians(roll_deg)), math.sin(math.radians(roll_deg))
    R = np.array([[c, -s, 0], [s, c, 0], [0, 0, 1.0]]) @ np.stack([right, down, fw])
    return R, -R @ pos


def make_map(M=3, F=6, seed=0, noise=0.0, pattern="full", lens="none", length=LENGTH, far=1.0, frontal=0.6):
    """-> dict(a (12,), length, Mw [M] (R, t) marker -> world (marker 0's frame), T [F] (R, t) world -> camera, obs: list of (marker,
    frame, img (4, 2) f32) in (frame, marker) order, M, F).  far scales the camera distance, frontal the spread of its direction
    about the room's diagonal"""
    rng = np.random.default_rng(seed)
    a = camera_params(lens)
    room = room_markers(M, rng, length)
    sq = square(length)
    sees = visibility(M, F, pattern, rng)
    T, obs = [], []
    for f in range(F):
        want = [m for m in range(M) if sees[f, m]]
        cen = np.mean([room[m][1] for m in want], axis=0)
        rad = max(np.linalg.norm(room[m][1] - cen) for m in want) + length
        for _ in range(4000):
            d = np.array([1.0, 1.0, 1.0]) + rng.uniform(-frontal, frontal, 3)
            d /= np.linalg.norm(d)
            P = look_at(cen + d * rad * far * rng.uniform(2.5, 5.0), cen + rng.uniform(-0.3, 0.3, 3) * rad, rng.uniform(-25, 25))
            uvs, ok = [], True
            for m in want:
                G = mul(P, room[m])
                uv = co.project(a, G[0], G[1], sq)
                facing = -(G[0][:, 2] @ G[1]) / np.linalg.norm(G[1])     # cosine between the marker's normal and the ray to the camera
                ok = ok and facing > 0.25 and bool(np.all(np.isfinite(uv)) and np.all(uv >= 10.0) and np.all(uv[:, 0] <= SIZE[0] - 11.0)
                                                   and np.all(uv[:, 1] <= SIZE[1] - 11.0))
                uvs.append(uv)
            if ok:
                break
        else:
            raise RuntimeError(f"no camera pose sees markers {want}")
        T.append(mul(P, room[0]))   # world = marker 0's frame
        for m, uv in zip(want, uvs):
            if noise:
                uv = uv + rng.normal(0.0, noise, uv.shape)
            obs.append((m, f, uv.astype(np.float32)))
    Mw = [mul(inv(room[0]), room[m]) for m in range(M)]
    return dict(a=a, length=length, Mw=Mw, T=T, obs=obs, M=M, F=F)


def pack(problems, flags=0, max_iterations=0, guess=None):
    """several maps into one call's arrays -> (Map array, MapMarker array, MapObservation array, img (n_obs, 8) f32).  flags /
    max_iterations: one value or one per map; guess: per map None or a list of (R, t) per marker"""
    n = len(problems)
    flags = flags if isinstance(flags, (list, tuple)) else [flags] * n
    max_iterations = max_iterations if isinstance(max_iterations, (list, tuple)) else [max_iterations] * n
    guess = guess if guess is not None else [None] * n
    maps = (A.Map * n)()
    markers = (A.MapMarker * sum(p["M"] for p in problems))()
    obs = (A.MapObservation * max(sum(len(p["obs"]) for p in problems), 1))()
    img = []
    m0 = f0 = o0 = 0
    for r, p in enumerate(problems):
        maps[r] = A.Map(m0, p["M"], f0, p["F"], o0, len(p["obs"]), flags[r], max_iterations[r])
        maps[r].a[:] = [float(v) for v in p["a"]]
        maps[r].marker_length = float(p["length"])
        for m in range(p["M"]):
            R, t = guess[r][m] if guess[r] is not None else (np.eye(3), np.zeros(3))
            markers[m0 + m].guess_rotation[:] = [float(v) for v in np.asarray(R, np.float64).reshape(9)]
            markers[m0 + m].guess_translation[:] = [float(v) for v in np.asarray(t, np.float64).reshape(3)]
        for j, (m, f, uv) in enumerate(p["obs"]):
            obs[o0 + j] = A.MapObservation(m0 + m, f0 + f)
            img.append(np.asarray(uv, np.float32).reshape(8))
        m0 += p["M"]
        f0 += p["F"]
        o0 += len(p["obs"])
    return maps, markers, obs, (np.stack(img) if img else np.zeros((0, 8), np.float32))


def marker_errors(mres, Mw, m0=0, length=LENGTH, only=None):
    """-> (worst rotation error in degrees, worst translation error in marker lengths) over the markers 1 .. (or `only`)"""
    rot = tr = 0.0
    for m in (only if only is not None else range(1, len(Mw))):
        R = np.array(mres[m0 + m].rotation).reshape(3, 3)
        t = np.array(mres[m0 + m].translation)
        rot = max(rot, rotation_error_deg(R, Mw[m][0]))
        tr = max(tr, float(np.linalg.norm(t - Mw[m][1]) / length))
    return rot, tr


def frame_errors(frames, T, f0=0, length=LENGTH, only=None):
    """-> (worst rotation error in degrees, worst camera position error in marker lengths) over the frames"""
    rot = tr = 0.0
    for f in (only if only is not None else range(len(T))):
        R = np.array(frames[f0 + f].rotation).reshape(3, 3)
        t = np.array(frames[f0 + f].translation)
        rot = max(rot, rotation_error_deg(R, T[f][0]))
        tr = max(tr, float(np.linalg.norm(R.T @ t - T[f][0].T @ T[f][1]) / length))
    return rot, tr


def odd_maps():
    """map 0: markers 0-2 good but for one observation of four collinear points, marker 3 seen only in a frame that sees nothing else
    (UNREACHED, the frame UNUSED), marker 4 never seen (UNSEEN); map 1: markers 0 and 1 never share a frame; map 2: good"""
    a = make_map(3, 6, seed=80)
    obs = list(a["obs"])
    m, f, _ = obs[1]
    x = np.arange(4, dtype=np.float32)
    obs[1] = (m, f, np.stack([100.0 + 10 * x, 200.0 + 3 * x], 1).astype(np.float32))
    obs.append((3, 6, obs[0][2] + np.float32(5.0)))
    eye = (np.eye(3), np.zeros(3))
    a.update(obs=obs, M=5, F=7, Mw=a["Mw"] + [eye, eye], T=a["T"] + [eye])
    b = make_map(2, 6, seed=81)
    b["obs"] = [o for o in b["obs"] if o[1] % 2 == o[0]]
    return [a, b, make_map(2, 6, seed=82, noise=0.1)]
