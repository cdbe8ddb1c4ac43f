"""Hand-eye calibration problems with a known answer: a camera with known intrinsics, a mount X and a board placement Y, board ->
camera poses drawn so that every point stays inside the image, the robot poses that produce them (M_f = X^-1 . P_f . Y^-1), and the
points projected in f64 through the contract's forward model (tests/calib_oracle.c) and rounded to f32.  TEST INFRASTRUCTURE ONLY."""
import numpy as np

from aruco3_amd import _lib as A
from tests import board_util as bu
from tests import calib_oracle as co
from tests import calib_util as cu
from tests.rig_util import inv, mul, rotation_error_deg, records_equal, cayley_w  # noqa: F401  (re-exported)

SIZE = (1280, 720)
INTRINSICS = np.array(list(cu.K720) + list(cu.WEBCAM5), np.float64)
MOUNTS = {
    "small": bu.rot_xyz(3.0, -4.0, 5.0),
    "y90": np.array([[0.0, 0.0, 1.0], [0.0, 1.0, 0.0], [-1.0, 0.0, 0.0]]),
    "d120": np.array([[0.0, 0.0, 1.0], [1.0, 0.0, 0.0], [0.0, 1.0, 0.0]]),     # 120 degrees about (1, 1, 1)
    "z180": np.diag([-1.0, -1.0, 1.0]),
    "x180": np.diag([1.0, -1.0, -1.0]),
}
MOUNT_T = np.array([35.0, -20.0, 60.0])
BOARD_Y = (bu.rot_xyz(170.0, 12.0, -25.0), np.array([520.0, 140.0, -80.0]))


def points(kind):
    """'marker': the 4 corners of one marker; else calib_util.target_points"""
    return cu.target_points("grid")[:4] if kind == "marker" else cu.target_points(kind)


def camera_poses(pts, F, rng, motion="general"):
    """F board -> camera poses.  'general': tilted every way; 'translate': one rotation, the board shifted about; 'one_axis': one
    tilt, the board rolled about its own normal, so that every relative rotation shares an axis"""
    holder = type("B", (), {"corners": pts.reshape(-1, 1, 2)})()
    ext = float(np.max(np.linalg.norm(pts - pts.mean(axis=0), axis=1)))
    if motion == "general":   # the acceptance loop of calib_util.random_poses, the tilt directions spread round the circle
        out = []
        while len(out) < F:
            dist = ext * cu.K720[0] / rng.uniform(180.0, 330.0)
            off = (rng.uniform(-0.25, 0.25) * SIZE[0], rng.uniform(-0.25, 0.25) * SIZE[1])
            R, t = bu.board_pose_facing(holder, rng.uniform(20.0, 40.0), 360.0 * len(out) / F + rng.uniform(-25.0, 25.0), rng.uniform(-30, 30),
                                        dist, off, K=cu.K720)
            uv = co.project(INTRINSICS, R, t, pts)
            if np.all(np.isfinite(uv)) and np.all(uv >= 10.0) and np.all(uv[:, 0] <= SIZE[0] - 11.0) and np.all(uv[:, 1] <= SIZE[1] - 11.0):
                out.append((R, t))
        return out
    out = []
    for f in range(F):
        dist = ext * cu.K720[0] / (200.0 + 12.0 * (f % 7))
        if motion == "translate":
            off = (0.12 * SIZE[0] * np.cos(2.4 * f), 0.12 * SIZE[1] * np.sin(1.7 * f))
            out.append(bu.board_pose_facing(holder, 25.0, 40.0, 10.0, dist, off, K=cu.K720))
        else:
            out.append(bu.board_pose_facing(holder, 25.0, 40.0, -60.0 + 120.0 * f / max(F - 1, 1), dist, (20.0 * (f % 3), -15.0 * (f % 2)), K=cu.K720))
    return out


def make_problem(F=12, seed=0, setup="eye_in_hand", mount="small", noise=0.0, kind="charuco", motion="general", few=(), collinear=(),
                 board_y=BOARD_Y):
    """-> dict(a (12,), X, Y (R, t): the truth, M [F] (R, t), robot [F] (R, t) gripper -> base, P [F] board -> camera, obs [F] (obj
    (n, 2) f32, img (n, 2) f32), setup).  few / collinear: frames cut down to 3 points / to points on one line"""
    rng = np.random.default_rng(seed)
    pts = points(kind)
    X = (MOUNTS[mount], MOUNT_T.copy())
    Y = (np.asarray(board_y[0], np.float64), np.asarray(board_y[1], np.float64))
    P = camera_poses(pts, F, rng, motion)
    M = [mul(inv(X), mul(Pf, inv(Y))) for Pf in P]
    robot = [inv(Mf) for Mf in M] if setup == "eye_in_hand" else list(M)
    obs = []
    for f, Pf in enumerate(P):
        G = mul(X, mul(M[f], Y))
        o = pts
        if f in few:
            o = pts[:3]
        elif f in collinear:
            o = np.stack([np.linspace(0.0, 100.0, 6), np.linspace(0.0, 50.0, 6)], axis=1)
        uv = co.project(INTRINSICS, G[0], G[1], o)
        if noise:
            uv = uv + rng.normal(0.0, noise, uv.shape)
        obs.append((o.astype(np.float32), uv.astype(np.float32)))
    return dict(a=INTRINSICS, X=X, Y=Y, M=M, robot=robot, P=P, obs=obs, setup=setup, F=F)


def pack(problems, flags=0, max_iterations=0, guess=None):
    """several problems into one call's arrays -> (HandEyeProblem array, HandEyeFrame array, obj (N, 2) f32, img (N, 2) f32).
    flags / max_iterations: one value or one per problem; guess: per problem None or (X, Y) as (R, t) pairs (Y may be None)"""
    n = len(problems)
    flags = flags if isinstance(flags, (list, tuple)) else [flags] * n
    max_iterations = max_iterations if isinstance(max_iterations, (list, tuple)) else [max_iterations] * n
    guess = guess if guess is not None else [None] * n
    probs = (A.HandEyeProblem * n)()
    frames = (A.HandEyeFrame * sum(p["F"] for p in problems))()
    obj, img = [], []
    f0 = p0 = 0
    for r, p in enumerate(problems):
        pr = probs[r]
        pr.first_frame, pr.n_frames, pr.flags, pr.max_iterations = f0, p["F"], flags[r], max_iterations[r]
        pr.a[:] = [float(v) for v in p["a"]]
        gx, gy = guess[r] if guess[r] is not None else (None, None)
        gx = gx if gx is not None else (np.eye(3), np.zeros(3))
        gy = gy if gy is not None else (np.eye(3), np.zeros(3))
        pr.guess_x_rotation[:] = [float(v) for v in np.asarray(gx[0], np.float64).reshape(9)]
        pr.guess_x_translation[:] = [float(v) for v in np.asarray(gx[1], np.float64).reshape(3)]
        pr.guess_y_rotation[:] = [float(v) for v in np.asarray(gy[0], np.float64).reshape(9)]
        pr.guess_y_translation[:] = [float(v) for v in np.asarray(gy[1], np.float64).reshape(3)]
        for f in range(p["F"]):
            fr = frames[f0 + f]
            fr.rotation[:] = [float(v) for v in np.asarray(p["M"][f][0], np.float64).reshape(9)]
            fr.translation[:] = [float(v) for v in np.asarray(p["M"][f][1], np.float64).reshape(3)]
            o, i = p["obs"][f]
            fr.first_point, fr.n_points = p0, len(o)
            obj.append(np.asarray(o, np.float32).reshape(-1, 2))
            img.append(np.asarray(i, np.float32).reshape(-1, 2))
            p0 += len(o)
        f0 += p["F"]
    return probs, frames, np.concatenate(obj), np.concatenate(img)


def solved(res, k=0):
    """X, Y of result k as (R, t) pairs"""
    r = res[k]
    return ((np.array(r.x_rotation).reshape(3, 3), np.array(r.x_translation)), (np.array(r.y_rotation).reshape(3, 3), np.array(r.y_translation)))


def errors(res, p, k=0):
    """-> (worst rotation error in degrees, worst translation error in board units) of X and Y against the truth"""
    X, Y = solved(res, k)
    rot = max(rotation_error_deg(X[0], p["X"][0]), rotation_error_deg(Y[0], p["Y"][0]))
    tr = max(float(np.linalg.norm(X[1] - p["X"][1])), float(np.linalg.norm(Y[1] - p["Y"][1])))
    return rot, tr


def axis_spread_deg(p) -> float:
    """the largest angle between the rotation axes (as lines) of two frame pairs' relative robot rotations M_i M_j^-1"""
    axes = []
    for i in range(p["F"]):
        for j in range(i + 1, p["F"]):
            D = p["M"][i][0] @ p["M"][j][0].T
            v = np.array([D[2, 1] - D[1, 2], D[0, 2] - D[2, 0], D[1, 0] - D[0, 1]])
            if np.linalg.norm(v) > 1e-6:
                axes.append(v / np.linalg.norm(v))
    A_ = np.array(axes)
    c = np.clip(np.abs(A_ @ A_.T), 0.0, 1.0)
    return float(np.degrees(np.arccos(c.min())))


# ---- the end-to-end scene: a GridBoard fixed in the cell, seen by a camera on the flange at SCENE_FRAMES robot poses ----
SCENE_FRAMES = 12
SCENE_MOUNT = (bu.rot_xyz(4.0, -3.0, 178.0), np.array([40.0, -25.0, 70.0]))        # gripper -> camera: nearly upside down on the flange
SCENE_BOARD = (bu.rot_xyz(178.0, 5.0, -30.0), np.array([600.0, 150.0, -40.0]))     # board -> base


def scene():
    """-> dict(board, dictionary, a (12,), X, Y, robot [n] gripper -> base, P [n] board -> camera, frames [n] (720, 1280) uint8): a pinhole
    camera, every marker painted on the host through its quad's homography (aruco3_amd.synth, the host form of a3_synth_render), poses
    drawn as tests/test_gpu_rig.py's end-to-end scene draws them"""
    from aruco3_amd import ARDictionary, synth
    from aruco3_amd.board import GridBoard

    d = ARDictionary.new_from_named_dict("ARUCO")
    board = GridBoard(5, 7, 30.0, 6.0)
    a = np.array(list(cu.K720) + [0.0] * 8, np.float64)
    rng = np.random.default_rng(11)
    spec = synth.SynthSpec(SIZE[0], SIZE[1])
    P, frames = [], []
    while len(P) < SCENE_FRAMES:
        off = (rng.uniform(-300, 300), rng.uniform(-120, 120))
        R, t = bu.board_pose_facing(board, rng.uniform(15, 40), 360.0 * len(P) / SCENE_FRAMES + rng.uniform(-20, 20), rng.uniform(-20, 20),
                                    rng.uniform(470, 560), off, K=cu.K720)
        quads = bu.project(board, R, t, cu.K720)
        if not (np.all(quads >= 30) and np.all(quads[..., 0] <= SIZE[0] - 31) and np.all(quads[..., 1] <= SIZE[1] - 31)):
            continue
        grey = np.full((SIZE[1], SIZE[0]), 200.0, np.float32)
        for k, quad in enumerate(quads):
            synth._draw_marker(grey, synth.marker_cells(int(d.code_list[int(board.ids[k])]), d.num_bits), quad, spec)
        P.append((R, t))
        frames.append(np.rint(np.clip(grey, 0.0, 255.0)).astype(np.uint8))
    robot = [inv(mul(inv(SCENE_MOUNT), mul(Pf, inv(SCENE_BOARD)))) for Pf in P]
    return dict(board=board, dictionary=d, a=a, X=SCENE_MOUNT, Y=SCENE_BOARD, robot=robot, P=P, frames=frames)


def cpu_detections(s):
    """the scene's frames through the detector's CPU restatement (oracle/a3oracle.py) and the refinement's (tests/refine_oracle.py):
    per frame an object with .markers (id, corners, corners_refined), what calibrate_hand_eye_board reads"""
    from types import SimpleNamespace

    from oracle import a3oracle
    from tests import refine_oracle as refo

    d = s["dictionary"]
    cfg = a3oracle.Config.default()
    cfg.min_corner_separation_factor = bu.MIN_CORNER_SEPARATION_FACTOR
    cells = int(np.ceil(np.sqrt(d.num_bits))) + 2
    out = []
    for grey in s["frames"]:
        res = a3oracle.detect(grey, d.code_list, d.num_bits, d._tau, cfg, keep_debug=False)
        quads = [m["corners"] for m in res["markers"]]
        ref = refo.refine_markers(np.ascontiguousarray(grey), quads, cells)
        out.append(SimpleNamespace(markers=[SimpleNamespace(id=m["id"], corners=np.asarray(q, np.float32).reshape(4, 2), corners_refined=r)
                                            for m, q, r in zip(res["markers"], quads, ref)]))
    return out
