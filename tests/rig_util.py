"""Rig calibration problems with a known answer: cameras with known intrinsics at known extrinsics, board poses in the rig frame drawn
so that every point stays inside every image that is meant to see it, projected in f64 through the contract's forward model
(tests/calib_oracle.c) and rounded to f32 image points.  TEST INFRASTRUCTURE ONLY."""
import math

import numpy as np

from aruco3_amd import _lib as A
from tests import board_util as bu
from tests import calib_oracle as co
from tests import calib_util as cu

SIZE = (1280, 720)
LENSES = [cu.WEBCAM, cu.WEBCAM5, (0.0,) * 8, (-0.1, 0.02, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0), cu.RATIONAL]


def mul(A_, B_):
    """(R, t) . (R, t)"""
    return A_[0] @ B_[0], A_[0] @ B_[1] + A_[1]


def inv(A_):
    return A_[0].T, -A_[0].T @ A_[1]


def camera_params(c: int) -> np.ndarray:
    """the 12 intrinsics of the rig's camera c: every camera its own focal lengths, principal point and lens"""
    K = (900.0 + 35.0 * c, 905.0 + 31.0 * c, 641.5 - 7.0 * c, 357.25 + 5.0 * c)
    return np.array(list(K) + list(LENSES[c % len(LENSES)]), np.float64)


def true_extrinsics(C: int, rng, baseline=45.0):
    """rig -> camera (R, t): camera c sits c baselines along x (with some jitter), turned towards a point 600 in front of the rig"""
    out = [(np.eye(3), np.zeros(3))]
    for c in range(1, C):
        pos = np.array([baseline * c + rng.uniform(-5, 5), rng.uniform(-15, 15), rng.uniform(-15, 15)])
        yaw = -math.degrees(math.atan2(pos[0], 600.0)) + rng.uniform(-2, 2)
        R = bu.rot_xyz(rng.uniform(-3, 3), yaw, rng.uniform(-4, 4)).T      # camera axes in the rig frame, transposed: rig -> camera
        out.append((R, -R @ pos))
    return out


def visibility(C: int, F: int, pattern: str, rng) -> np.ndarray:
    """sees[f, c].  'full'; 'missing': about a third of the observations dropped, every third frame tying a camera to its
    successor; 'chain': camera c sees frame f when f % (C - 1) is c - 1 or c, so that camera 2 never shares a frame with camera 0"""
    sees = np.ones((F, C), bool)
    if pattern == "missing":
        sees = rng.uniform(size=(F, C)) > 0.33
        for f in range(F):
            if f % 3 == 0:     # every third frame ties a camera to its successor ...
                c = (f // 3) % C
                sees[f, c] = sees[f, (c + 1) % C] = True
            elif not sees[f].any():   # ... and no frame goes unseen
                sees[f, f % C] = True
    elif pattern == "chain":
        for f in range(F):
            for c in range(C):
                sees[f, c] = f % (C - 1) in (c - 1, c)
    return sees


def inside(a, P, pts, margin=10.0):
    uv = co.project(a, P[0], P[1], pts)
    ok = np.all(np.isfinite(uv)) and np.all(uv >= margin) and np.all(uv[:, 0] <= SIZE[0] - 1 - margin) and np.all(uv[:, 1] <= SIZE[1] - 1 - margin)
    return ok, uv


def make_rig(C=2, F=12, seed=0, kind="charuco", noise=0.0, pattern="full", subsets=True, min_points=8):
    """-> dict(a [C] (12,), E [C] (R, t) rig -> camera, T [F] (R, t) board -> rig, obs: list of (camera, frame, obj (n, 2) f32, img (n, 2)
    f32) in (frame, camera) order, C, F)"""
    rng = np.random.default_rng(seed)
    pts = cu.target_points(kind)
    a = [camera_params(c) for c in range(C)]
    E = true_extrinsics(C, rng)
    sees = visibility(C, F, pattern, rng)
    centre = pts.mean(axis=0)
    ext = float(np.max(np.linalg.norm(pts - centre, axis=1)))
    holder = type("B", (), {"corners": pts.reshape(-1, 1, 2)})()
    T, obs = [], []
    for f in range(F):
        cams = [c for c in range(C) if sees[f, c]]
        while True:   # the acceptance loop of calib_util.random_poses, for every camera that is meant to see the frame
            anchor = cams[int(rng.integers(len(cams)))]
            K = tuple(a[anchor][:4])
            dist = ext * K[0] / rng.uniform(120.0, 260.0)
            off = (rng.uniform(-0.2, 0.2) * SIZE[0], rng.uniform(-0.2, 0.2) * SIZE[1])
            P = bu.board_pose_facing(holder, rng.uniform(10.0, 40.0), rng.uniform(0, 360), rng.uniform(-30, 30), dist, off, K=K)
            Tf = mul(inv(E[anchor]), P)
            if all(inside(a[c], mul(E[c], Tf), pts)[0] for c in cams):
                break
        T.append(Tf)
        for c in cams:
            uv = inside(a[c], mul(E[c], Tf), pts)[1]
            sel = np.arange(len(pts))
            if subsets and len(pts) > min_points:
                n = int(rng.integers(max(min_points, (len(pts) * 3) // 5), len(pts) + 1))
                sel = np.sort(rng.choice(len(pts), n, replace=False))
            if noise:
                uv = uv + rng.normal(0.0, noise, uv.shape)
            obs.append((c, f, pts[sel].astype(np.float32), uv[sel].astype(np.float32)))
    return dict(a=a, E=E, T=T, obs=obs, C=C, F=F)


def pack(problems, flags=0, max_iterations=0, guess=None):
    """several rigs into one call's arrays -> (Rig array, RigCamera array, RigObservation array, obj (N, 2) f32, img (N, 2) f32).
    flags / max_iterations: one value or one per rig; guess: per rig None or a list of (R, t) per camera"""
    n = len(problems)
    flags = flags if isinstance(flags, (list, tuple)) else [flags] * n
    max_iterations = max_iterations if isinstance(max_iterations, (list, tuple)) else [max_iterations] * n
    guess = guess if guess is not None else [None] * n
    rigs = (A.Rig * n)()
    cams = (A.RigCamera * sum(p["C"] for p in problems))()
    obs = (A.RigObservation * max(sum(len(p["obs"]) for p in problems), 1))()
    obj, img = [], []
    c0 = f0 = o0 = p0 = 0
    for r, p in enumerate(problems):
        rigs[r] = A.Rig(c0, p["C"], f0, p["F"], o0, len(p["obs"]), flags[r], max_iterations[r])
        for c in range(p["C"]):
            cams[c0 + c].a[:] = [float(v) for v in p["a"][c]]
            R, t = guess[r][c] if guess[r] is not None else (np.eye(3), np.zeros(3))
            cams[c0 + c].guess_rotation[:] = [float(v) for v in np.asarray(R, np.float64).reshape(9)]
            cams[c0 + c].guess_translation[:] = [float(v) for v in np.asarray(t, np.float64).reshape(3)]
        for j, (c, f, o, i) in enumerate(p["obs"]):
            obs[o0 + j] = A.RigObservation(c0 + c, f0 + f, p0, len(o))
            obj.append(np.asarray(o, np.float32).reshape(-1, 2))
            img.append(np.asarray(i, np.float32).reshape(-1, 2))
            p0 += len(o)
        c0 += p["C"]
        f0 += p["F"]
        o0 += len(p["obs"])
    cat = lambda v: np.concatenate(v) if v else np.zeros((0, 2), np.float32)   # noqa: E731
    return rigs, cams, obs, cat(obj), cat(img)


def cayley_w(R) -> np.ndarray:
    """w with cay(w) = R: the Cayley increment a rotation's std_dev is stated in"""
    R = np.asarray(R, np.float64)
    S = (R - np.eye(3)) @ np.linalg.inv(R + np.eye(3))
    return np.array([S[2, 1], S[0, 2], S[1, 0]])


def rotation_error_deg(Ra, Rb) -> float:
    """the angle of Ra Rb^T from its skew part (resolves 1e-10 degrees, where acos of the trace stops near 1e-6)"""
    D = np.asarray(Ra, np.float64) @ np.asarray(Rb, np.float64).T
    s = 0.5 * math.sqrt((D[2, 1] - D[1, 2]) ** 2 + (D[0, 2] - D[2, 0]) ** 2 + (D[1, 0] - D[0, 1]) ** 2)
    return math.degrees(math.atan2(s, (np.trace(D) - 1.0) / 2.0))


def extrinsic_errors(cres, E, c0=0):
    """-> (worst rotation error in degrees, worst translation error relative to that camera's baseline length) over cameras 1 .."""
    rot = tr = 0.0
    for c in range(1, len(E)):
        R = np.array(cres[c0 + c].rotation).reshape(3, 3)
        t = np.array(cres[c0 + c].translation)
        rot = max(rot, rotation_error_deg(R, E[c][0]))
        tr = max(tr, float(np.linalg.norm(t - E[c][1]) / np.linalg.norm(E[c][1])))
    return rot, tr


def records_equal(a, b) -> bool:
    """two ctypes record arrays (or records), byte for byte"""
    return bytes(a) == bytes(b)
