"""aruco3_amd -- MI355X-native ArUco/AprilTag detection behind the aruco3 crate's API.

Host-side mirror of the reference's public surface (src/lib.rs:6-9):
`Detector`, `DetectorConfig`, `Detection`, `Marker`, `ARDictionary`, `CameraIntrinsics`,
`MarkerPose` and the `pose` module.  All computation happens in hand-written HIP kernels
behind the C ABI declared in include/aruco3_hip.h (csrc/ -> libaruco3_hip.so).
"""
from .dictionaries import ARDictionary  # noqa: F401


def __getattr__(name):
    # GPU-backed names are imported lazily so that table handling works without the .so
    if name in ("Detector", "DetectorConfig", "Detection", "Marker", "Rectification", "Reduction"):
        from . import aruco

        return getattr(aruco, name)
    if name in ("CameraIntrinsics", "Distortion", "undistort_points"):
        from . import pinhole

        return getattr(pinhole, name)
    if name in ("MarkerPose",):
        from . import pose

        return getattr(pose, name)
    if name in ("Board", "GridBoard", "Board3D", "BoardPose", "CharucoBoard", "CharucoPose", "BoardRecovery", "recover_markers"):
        from . import board

        return getattr(board, name)
    if name in ("Calibration", "calibrate_camera", "calibrate_cameras", "calibrate_camera_board", "calibrate_camera_charuco",
                "calibrate_camera_fisheye", "calibrate_cameras_fisheye"):
        from . import calibration

        return getattr(calibration, name)
    if name in ("RigCalibration", "calibrate_rig", "calibrate_rigs", "calibrate_rig_board", "calibrate_rig_charuco", "stereo_calibrate",
                "rig_board_poses"):
        from . import rig

        return getattr(rig, name)
    if name in ("HandEyeCalibration", "calibrate_hand_eye", "calibrate_hand_eyes", "calibrate_hand_eye_board", "calibrate_hand_eye_charuco"):
        from . import handeye

        return getattr(handeye, name)
    if name in ("MarkerMap", "build_marker_map", "build_marker_maps", "locate_in_map"):
        from . import markermap

        return getattr(markermap, name)
    if name == "rectify_frames":
        from . import rectify

        return rectify.rectify_frames
    if name == "reduce_frames":
        from . import reduce

        return reduce.reduce_frames
    if name == "pose":
        import importlib

        return importlib.import_module(".pose", __name__)
    raise AttributeError(name)
