"""Marker maps on the device (a3_build_marker_maps): where markers taped around a room sit relative to one reference marker, from the
frames of a walk-through -- and, with a map, the camera pose of any frame from whichever map markers it sees.

Not part of the reference: an extension whose algorithm include/aruco3_hip.h fixes to the bit (the ArUco library's MarkerMap / marker
mapper: both planar pose candidates per observation, a start in rounds over the co-visibility graph that chooses every pose by its
cost over all observations bearing on it, then a Levenberg-Marquardt bundle over the markers with the frames eliminated, in f64, one
workgroup per map).  The camera is known: calibrate it first (aruco3_amd.calibration).  The world frame is the reference marker's;
marker poses are marker -> world, frame poses world -> camera."""
import json
from dataclasses import dataclass, field
from typing import Dict, List, Optional, Sequence

import numpy as np

from . import _lib, _solver
from .rig import camera_params


@dataclass
class MapFramePose:
    """one frame (a3_map_frame): status MAP_FRAME_USED / _UNUSED (no usable observation of a reached marker); the pose world -> camera"""
    status: int
    obs_used: int
    rms_px: float
    rotation: np.ndarray      # 3x3 float64
    translation: np.ndarray   # 3 float64, world units

    @property
    def used(self) -> bool:
        return self.status == _lib.MAP_FRAME_USED

    @property
    def position(self) -> np.ndarray:
        """the camera centre in world units"""
        return -self.rotation.T @ self.translation


@dataclass
class MapObservationResult:
    """one marker in one frame: status MAP_OBS_USED / _DEGENERATE / _UNREACHED; start_rms_px: the two planar candidates of step 1"""
    marker_id: int
    frame: int
    status: int
    rms_px: float
    start_rms_px: tuple

    @property
    def used(self) -> bool:
        return self.status == _lib.MAP_OBS_USED


@dataclass
class MarkerMap:
    """one map (a3_map_result and its marker records).  status MAP_OK, or MAP_NOT_CONNECTED (no marker shares a frame with the
    reference) / MAP_NOT_FINITE with zeros elsewhere.  ids[0] is the reference marker; marker_status per marker MAP_MARKER_USED /
    _UNSEEN / _UNREACHED (poses of the latter two are zero)."""
    status: int
    ids: np.ndarray            # int64 (M,)
    marker_length: float
    rotations: np.ndarray      # float64 (M, 3, 3), marker -> world; the first is the identity
    translations: np.ndarray   # float64 (M, 3), world units (those of marker_length)
    corners: np.ndarray        # float64 (M, 4, 3): the corners in world units, a3_marker order
    std_devs: np.ndarray       # float64 (M, 6): of (w, t), w the Cayley increment at the solution; 0 for the reference
    marker_status: np.ndarray  # int64 (M,)
    marker_rms_px: np.ndarray
    rms_px: float = 0.0
    iterations: int = 0
    converged: bool = False
    frames_used: int = 0
    obs_used: int = 0
    frames: List[MapFramePose] = field(default_factory=list)
    observations: List[MapObservationResult] = field(default_factory=list)

    @property
    def ok(self) -> bool:
        return self.status == _lib.MAP_OK

    def index(self, marker_id: int) -> int:
        return int(np.nonzero(self.ids == int(marker_id))[0][0])

    def pose(self, marker_id: int):
        """(R, t) marker -> world"""
        k = self.index(marker_id)
        return self.rotations[k], self.translations[k]

    def corners_3d(self, marker_id: int) -> np.ndarray:
        """the marker's four corners in world units, (4, 3)"""
        return self.corners[self.index(marker_id)]

    def save(self, path) -> None:
        """a JSON file of numbers (path ending in .json) or a plain .npz"""
        d = dict(status=int(self.status), ids=self.ids, marker_length=float(self.marker_length), rotations=self.rotations,
                 translations=self.translations, corners=self.corners, std_devs=self.std_devs, marker_status=self.marker_status,
                 marker_rms_px=self.marker_rms_px, rms_px=float(self.rms_px))
        if str(path).endswith(".json"):
            with open(path, "w") as fh:
                json.dump({k: (v.tolist() if isinstance(v, np.ndarray) else v) for k, v in d.items()}, fh)
        else:
            with open(path, "wb") as fh:
                np.savez(fh, **d)

    @classmethod
    def load(cls, path) -> "MarkerMap":
        if str(path).endswith(".json"):
            with open(path) as fh:
                d = json.load(fh)
        else:
            with np.load(path, allow_pickle=False) as z:
                d = {k: z[k] for k in z.files}
        f64 = lambda k: np.asarray(d[k], np.float64)   # noqa: E731
        return cls(int(d["status"]), np.asarray(d["ids"], np.int64), float(d["marker_length"]), f64("rotations"), f64("translations"),
                   f64("corners"), f64("std_devs"), np.asarray(d["marker_status"], np.int64), f64("marker_rms_px"), float(d["rms_px"]))


def _solve(*args):
    return _solver.call("build_marker_maps", *args)


def frame_observations(detection) -> Dict[int, np.ndarray]:
    """a Detection's markers as id -> corners (4, 2) float32: refined corners when present, else the integer corners; an id seen more
    than once in the frame is left out in all its instances (the board pose's rule)"""
    ids = [int(m.id) for m in detection.markers]
    return {int(m.id): np.asarray(m.corners_refined if m.corners_refined is not None else m.corners, np.float32).reshape(4, 2)
            for m in detection.markers if ids.count(int(m.id)) == 1}


def _as_frames(detections) -> List[Dict[int, np.ndarray]]:
    return [d if isinstance(d, dict) else frame_observations(d) for d in detections]


def build_marker_maps(problems: Sequence[dict]) -> List[MarkerMap]:
    """Several maps in one launch.  Each problem is a dict of build_marker_map's arguments: detections, camera, marker_length and
    optionally ids, reference_id, guess, fix_map, max_iterations."""
    n = len(problems)
    maps = (_lib.Map * max(n, 1))()
    plans = []
    for pr in problems:
        frames = _as_frames(pr["detections"])
        ids = pr.get("ids")
        if ids is None:
            ids = sorted({i for f in frames for i in f})
        ids = [int(i) for i in ids]
        ref = pr.get("reference_id")
        if ref is not None:
            if int(ref) not in ids:
                raise ValueError(f"reference marker {ref} is not among the map's markers")
            ids = [int(ref)] + [i for i in ids if i != int(ref)]
        if not ids:
            raise ValueError("no marker in any frame")
        if not frames:
            raise ValueError("no frame")
        slot = {i: k for k, i in enumerate(ids)}
        obs = [(slot[i], f, fr[i]) for f, fr in enumerate(frames) for i in sorted(fr, key=lambda i: slot.get(i, -1)) if i in slot]
        if not obs:
            raise ValueError("no frame shows a marker of the map")
        plans.append((ids, frames, obs))
    markers = (_lib.MapMarker * sum(len(p[0]) for p in plans))()
    obs_arr = (_lib.MapObservation * sum(len(p[2]) for p in plans))()
    img = []
    m0 = f0 = o0 = 0
    for r, (pr, (ids, frames, obs)) in enumerate(zip(problems, plans)):
        guess = pr.get("guess")
        fix = bool(pr.get("fix_map"))
        if fix and guess is None:
            raise ValueError("fix_map needs the marker poses (guess)")
        flags = (_lib.MAP_FIX_MAP if fix else 0) | (_lib.MAP_USE_GUESS if guess is not None else 0)
        maps[r] = _lib.Map(m0, len(ids), f0, len(frames), o0, len(obs), flags, int(pr.get("max_iterations") or 0))
        maps[r].a[:] = [float(v) for v in camera_params(pr["camera"])]
        maps[r].marker_length = float(pr["marker_length"])
        for k, i in enumerate(ids):
            pose = (np.eye(3), np.zeros(3))
            if guess is not None and k >= 1:
                pose = guess.pose(i) if isinstance(guess, MarkerMap) else guess[i]
            _solver.set_pose(markers[m0 + k], pose, "guess_")
        for j, (m, f, uv) in enumerate(obs):
            obs_arr[o0 + j] = _lib.MapObservation(m0 + m, f0 + f)
            img.append(np.asarray(uv, np.float32).reshape(8))
        m0 += len(ids)
        f0 += len(frames)
        o0 += len(obs)
    res, mres, fres, ores = _solve(maps, markers, obs_arr, np.stack(img))
    out = []
    for r, (pr, (ids, frames, obs)) in enumerate(zip(problems, plans)):
        R = maps[r]
        mr = [mres[R.first_marker + k] for k in range(len(ids))]
        mm = MarkerMap(int(res[r].status), np.asarray(ids, np.int64), float(maps[r].marker_length),
                       np.array([np.array(x.rotation).reshape(3, 3) for x in mr]), np.array([list(x.translation) for x in mr]),
                       np.array([np.array(x.corners).reshape(4, 3) for x in mr]), np.array([list(x.std_dev) for x in mr]),
                       np.array([x.status for x in mr], np.int64), np.array([x.rms_px for x in mr]), float(res[r].rms_px),
                       int(res[r].iterations), bool(res[r].converged), int(res[r].frames_used), int(res[r].obs_used))
        for f in range(len(frames)):
            x = fres[R.first_frame + f]
            mm.frames.append(MapFramePose(int(x.status), int(x.obs_used), float(x.rms_px), *_solver.get_pose(x)))
        for j, (m, f, _) in enumerate(obs):
            x = ores[R.first_obs + j]
            mm.observations.append(MapObservationResult(ids[m], f, int(x.status), float(x.rms_px), tuple(x.start_rms_px)))
        out.append(mm)
    return out


def build_marker_map(detections, camera, marker_length: float, *, reference_id: Optional[int] = None, guess=None,
                     max_iterations: Optional[int] = None, outlier_passes: int = 0, ids=None) -> MarkerMap:
    """The map of the markers seen in `detections`: one Detection per frame (or a dict id -> corners (4, 2)).  camera: a Calibration, a
    CameraIntrinsics or the 12 values fx .. k6; marker_length: the side of every marker, which sets the world's unit; reference_id:
    the marker whose frame is the world's (default: the lowest id seen); guess: a MarkerMap or a dict id -> (R, t) to start from; ids:
    the map's markers when they are known beforehand (ids never seen come back MAP_MARKER_UNSEEN).

    outlier_passes = k solves k more times, each time without the used observations whose rms_px exceeds max(1 px, 3 x the median
    over the used observations) of the previous solution (a misread marker, or a corner whose refinement fell back)."""
    frames = _as_frames(detections)
    kw = dict(camera=camera, marker_length=marker_length, reference_id=reference_id, guess=guess, max_iterations=max_iterations)
    if ids is None:
        ids = sorted({i for f in frames for i in f})
    kw["ids"] = ids
    mm = build_marker_maps([dict(detections=frames, **kw)])[0]
    for _ in range(int(outlier_passes)):
        if not mm.ok:
            break
        used = [o for o in mm.observations if o.used]
        limit = _solver.outlier_limit([o.rms_px for o in used])
        bad = [(o.frame, o.marker_id) for o in used if not o.rms_px < limit]
        if not bad:
            break
        frames = [dict(f) for f in frames]
        for f, i in bad:
            frames[f].pop(i, None)
        mm = build_marker_maps([dict(detections=frames, **kw)])[0]
    return mm


def locate_in_map(marker_map: MarkerMap, detections, camera) -> List[MapFramePose]:
    """One camera pose (world -> camera) per frame from whichever markers of `marker_map` it shows, the map held fixed (A3_MAP_FIX_MAP):
    every frame is solved on its own, so a frame's pose does not depend on the frames it is passed with.  A frame that shows no marker
    of the map comes back MAP_FRAME_UNUSED."""
    good = [int(i) for i, s in zip(marker_map.ids, marker_map.marker_status) if s == _lib.MAP_MARKER_USED]
    frames = [{i: c for i, c in f.items() if i in good} for f in _as_frames(detections)]
    unused = MapFramePose(_lib.MAP_FRAME_UNUSED, 0, 0.0, np.zeros((3, 3)), np.zeros(3))
    if not frames or not any(frames):
        return [unused for _ in frames]
    mm = build_marker_maps([dict(detections=frames, camera=camera, marker_length=marker_map.marker_length, ids=good,
                                 guess={i: marker_map.pose(i) for i in good}, fix_map=True)])[0]
    return mm.frames
