"""The argument checks of the solver entry points (aruco3_amd/csrc/a3_solve_check.h) without a GPU: tests/solver_checks.cpp runs them
on the smallest valid problem of each entry point and on one mutation at a time, compiled with the address and undefined-behaviour
sanitizers and run as an ordinary child process.  Every line it prints must be the message below: the literals of a3_api.hip as it was
before the checks moved into the header, the first failing check deciding.  A check that fires for another reason, or one that indexes a
map before it has bounded the index (the sanitizers stop the program), fails here."""
import os
import shutil
import subprocess
from pathlib import Path

HERE = Path(__file__).resolve().parent

NULL = ": null argument"
BUSY = ": a submitted batch has not been collected"
FLAGS = ": unknown flags"
ITERATIONS = ": max_iterations above A3_CALIB_MAX_ITERATIONS"
FOCAL = ": focal lengths must be > 0"
POINT = ": a point is not finite"
OK = None

CAMERAS = {
    "valid": OK,
    "null_cams": NULL,
    "null_offsets": NULL,
    "null_results": NULL,
    "null_object": ": null point array",
    "null_image": ": null point array",
    "busy": BUSY,
    "busy_null_results": NULL,
    "busy_n_cams_0": BUSY,
    "n_cams_0": ": n_cams must be in 1..A3_CALIB_MAX_CAMERAS",
    "n_cams_1025": ": n_cams must be in 1..A3_CALIB_MAX_CAMERAS",
    "n_views_0": ": n_views must be in 1..A3_CALIB_MAX_CALL_VIEWS",
    "n_views_65537": ": n_views must be in 1..A3_CALIB_MAX_CALL_VIEWS",
    "offsets_0_not_0": ": view_offsets[0] must be 0",
    "offsets_decrease": ": view_offsets must not decrease",
    "view_4097_points": ": a view has more than A3_CALIB_MAX_POINTS points",
    "no_points_null_arrays": OK,
    "nan_image_point": POINT,
    "inf_object_point": POINT,
    "unknown_flag": FLAGS,
    "unknown_flag_high": FLAGS,
    "image_width_0": ": image size must be in 1..65535",
    "image_height_70000": ": image size must be in 1..65535",
    "max_iterations_1000": OK,
    "max_iterations_1001": ITERATIONS,
    "camera_n_views_0": ": a camera's n_views must be in 1..A3_CALIB_MAX_VIEWS",
    "camera_n_views_4097": ": a camera's n_views must be in 1..A3_CALIB_MAX_VIEWS",
    "camera_n_views_6": ": a camera's views lie past n_views",
    "first_view_1": ": a camera's views lie past n_views",
    "first_view_max_n_1": ": a camera's views lie past n_views",
    "first_view_max_n_max": ": a camera's n_views must be in 1..A3_CALIB_MAX_VIEWS",
    "two_cameras": OK,
    "overlap": ": two cameras share a view",
    "view_not_owned": OK,
    "guess": OK,
    "guess_focal_0": ": the guess's focal lengths must be > 0",
    "guess_nan_k3": ": the guess is not finite",
    "guess_nan_k3_not_read": OK,
    "guess_p1": OK,
    "guess_p2": OK,
    "guess_k5": OK,
    "guess_k6": OK,
    "guess_p1_not_read": OK,
}
FISHEYE_LENS = ": the guess's lens reads k1 k2 k3 k4; p1, p2, k5 and k6 must be 0"
FISHEYE = dict(CAMERAS, guess_p1=FISHEYE_LENS, guess_p2=FISHEYE_LENS, guess_k5=FISHEYE_LENS, guess_k6=FISHEYE_LENS)

RIGS = {
    "valid": OK,
    "two_rigs": OK,
    "null_rigs": NULL,
    "null_cams": NULL,
    "null_obs": NULL,
    "null_obj": NULL,
    "null_img": NULL,
    "null_res": NULL,
    "null_cres": NULL,
    "busy": BUSY,
    "busy_null_res": NULL,
    "busy_n_rigs_0": BUSY,
    "n_rigs_0": ": n_rigs must be in 1..A3_RIG_MAX_RIGS",
    "n_rigs_1025": ": n_rigs must be in 1..A3_RIG_MAX_RIGS",
    "n_cameras_0": ": n_cameras out of range",
    "n_cameras_8193": ": n_cameras out of range",
    "n_obs_0": ": n_obs must be in 1..A3_RIG_MAX_CALL_OBSERVATIONS",
    "n_obs_262145": ": n_obs must be in 1..A3_RIG_MAX_CALL_OBSERVATIONS",
    "flags_4": FLAGS,
    "rig_n_cameras_1": ": a rig's n_cameras must be in 2..A3_RIG_MAX_CAMERAS",
    "rig_n_cameras_9": ": a rig's n_cameras must be in 2..A3_RIG_MAX_CAMERAS",
    "max_iterations_1001": ITERATIONS,
    "rig_n_frames_0": ": a rig's n_frames must be in 1..A3_RIG_MAX_FRAMES",
    "rig_n_frames_4097": ": a rig's n_frames must be in 1..A3_RIG_MAX_FRAMES",
    "rig_n_obs_0": ": a rig has no observations",
    "rig_n_obs_7": ": a rig's observations lie past n_obs",
    "first_camera_1": ": a rig's cameras lie past n_cameras",
    "first_camera_max_n_2": ": a rig's cameras lie past n_cameras",
    "first_camera_max_n_max": ": a rig's n_cameras must be in 2..A3_RIG_MAX_CAMERAS",
    "first_frame_65535": ": a rig's frames lie past A3_RIG_MAX_CALL_FRAMES",
    "first_frame_max_n_1": ": a rig's frames lie past A3_RIG_MAX_CALL_FRAMES",
    "first_frame_max_n_max": ": a rig's n_frames must be in 1..A3_RIG_MAX_FRAMES",
    "first_obs_max_n_1": ": a rig's observations lie past n_obs",
    "first_obs_max_n_max": ": a rig's observations lie past n_obs",
    "share_camera": ": two rigs share a camera",
    "share_frame": ": two rigs share a frame",
    "share_obs": ": two rigs share an observation",
    "obs_camera_2": ": an observation's camera lies outside its rig",
    "obs_camera_max": ": an observation's camera lies outside its rig",
    "obs_frame_3": ": an observation's frame lies outside its rig",
    "obs_frame_max": ": an observation's frame lies outside its rig",
    "obs_camera_below_rig": ": an observation's camera lies outside its rig",
    "obs_n_points_4097": ": an observation has more than A3_CALIB_MAX_POINTS points",
    "obs_first_point_max": ": an observation's points lie past 2^32",
    "duplicate": ": two observations of one (camera, frame)",
    "focal_0": FOCAL,
    "nan_lens": ": a camera's intrinsics are not finite",
    "nan_point": POINT,
    "inf_guess_use": ": the extrinsic guess is not finite",
    "inf_guess_fix": ": the extrinsic guess is not finite",
    "inf_guess_not_read": OK,
    "inf_guess_first_camera": OK,
}

HAND_EYES = {
    "valid": OK,
    "two_problems": OK,
    "null_probs": NULL,
    "null_frames": NULL,
    "null_obj": NULL,
    "null_img": NULL,
    "null_res": NULL,
    "busy": BUSY,
    "busy_null_res": NULL,
    "busy_n_problems_0": BUSY,
    "n_problems_0": ": n_problems must be in 1..A3_HANDEYE_MAX_PROBLEMS",
    "n_problems_1025": ": n_problems must be in 1..A3_HANDEYE_MAX_PROBLEMS",
    "n_frames_0": ": n_frames must be in 1..A3_HANDEYE_MAX_CALL_FRAMES",
    "n_frames_65537": ": n_frames must be in 1..A3_HANDEYE_MAX_CALL_FRAMES",
    "n_frames_2": ": a problem's frames lie past n_frames",
    "flags_4": FLAGS,
    "max_iterations_1001": ITERATIONS,
    "problem_n_frames_0": ": a problem's n_frames must be in 1..A3_HANDEYE_MAX_FRAMES",
    "problem_n_frames_257": ": a problem's n_frames must be in 1..A3_HANDEYE_MAX_FRAMES",
    "problem_n_frames_2": OK,
    "first_frame_1": ": a problem's frames lie past n_frames",
    "first_frame_max_n_1": ": a problem's frames lie past n_frames",
    "first_frame_max_n_max": ": a problem's n_frames must be in 1..A3_HANDEYE_MAX_FRAMES",
    "share_frame": ": two problems share a frame",
    "frame_n_points_4097": ": a frame has more than A3_CALIB_MAX_POINTS points",
    "frame_first_point_max": ": a frame's points lie past 2^32",
    "focal_0": FOCAL,
    "nan_lens": ": the camera's intrinsics are not finite",
    "nan_point": POINT,
    "nan_robot": ": a frame's robot pose is not finite",
    "inf_robot": ": a frame's robot pose is not finite",
    "skewed_robot": OK,
    "inf_guess_x_use": ": the guess is not finite",
    "inf_guess_x_fix": ": the guess is not finite",
    "inf_guess_x_not_read": OK,
    "inf_guess_y_use": ": the guess is not finite",
    "inf_guess_y_fix_x_alone": OK,
}

MAPS = {
    "valid": OK,
    "two_maps": OK,
    "null_maps": NULL,
    "null_markers": NULL,
    "null_obs": NULL,
    "null_img": NULL,
    "null_res": NULL,
    "null_mres": NULL,
    "busy": BUSY,
    "busy_null_res": NULL,
    "busy_n_maps_0": BUSY,
    "n_maps_0": ": n_maps must be in 1..A3_MAP_MAX_MAPS",
    "n_maps_1025": ": n_maps must be in 1..A3_MAP_MAX_MAPS",
    "n_markers_0": ": n_markers out of range",
    "n_markers_131073": ": n_markers out of range",
    "n_obs_0": ": n_obs must be in 1..A3_MAP_MAX_CALL_OBSERVATIONS",
    "n_obs_262145": ": n_obs must be in 1..A3_MAP_MAX_CALL_OBSERVATIONS",
    "flags_4": FLAGS,
    "map_n_markers_0": ": a map's n_markers must be in 1..A3_MAP_MAX_MARKERS",
    "map_n_markers_129": ": a map's n_markers must be in 1..A3_MAP_MAX_MARKERS",
    "max_iterations_1001": ITERATIONS,
    "map_n_frames_0": ": a map's n_frames must be in 1..A3_MAP_MAX_FRAMES",
    "map_n_frames_4097": ": a map's n_frames must be in 1..A3_MAP_MAX_FRAMES",
    "map_n_obs_0": ": a map has no observations",
    "map_n_obs_7": ": a map's observations lie past n_obs",
    "first_marker_1": ": a map's markers lie past n_markers",
    "first_marker_max_n_1": ": a map's markers lie past n_markers",
    "first_marker_max_n_max": ": a map's n_markers must be in 1..A3_MAP_MAX_MARKERS",
    "first_frame_65535": ": a map's frames lie past A3_MAP_MAX_CALL_FRAMES",
    "first_frame_max_n_1": ": a map's frames lie past A3_MAP_MAX_CALL_FRAMES",
    "first_frame_max_n_max": ": a map's n_frames must be in 1..A3_MAP_MAX_FRAMES",
    "first_obs_max_n_1": ": a map's observations lie past n_obs",
    "first_obs_max_n_max": ": a map's observations lie past n_obs",
    "marker_length_0": ": marker_length must be finite and > 0",
    "marker_length_nan": ": marker_length must be finite and > 0",
    "focal_0": FOCAL,
    "nan_lens": ": the camera's intrinsics are not finite",
    "share_marker": ": two maps share a marker",
    "share_frame": ": two maps share a frame",
    "share_obs": ": two maps share an observation",
    "obs_marker_2": ": an observation's marker lies outside its map",
    "obs_marker_max": ": an observation's marker lies outside its map",
    "obs_frame_3": ": an observation's frame lies outside its map",
    "obs_frame_max": ": an observation's frame lies outside its map",
    "duplicate": ": two observations of one (marker, frame)",
    "out_of_order": ": a map's observations must be listed by frame, then by marker",
    "markers_out_of_order": ": a map's observations must be listed by frame, then by marker",
    "nan_corner": ": a corner is not finite",
    "inf_guess_use": ": the marker guess is not finite",
    "inf_guess_fix": ": the marker guess is not finite",
    "inf_guess_not_read": OK,
    "inf_guess_first_marker": OK,
}

ENTRY_POINTS = (("a3_calibrate_cameras", CAMERAS), ("a3_calibrate_fisheye_cameras", FISHEYE), ("a3_calibrate_rigs", RIGS),
                ("a3_calibrate_hand_eyes", HAND_EYES), ("a3_build_marker_maps", MAPS))
# what a valid call hands to the staging: two rigs of 2 frames sharing 16 points; 3 frames of 4 points; two maps of 2 frames, the first
# free (two 6 x 6 reduced systems: 72 doubles), the second fixed (none)
OUTPUTS = ["outputs rigs: n_frames 4 n_pts 16", "outputs hand_eyes: n_pts 12", "outputs maps: n_frames 4 big_off 0 72 big_doubles 72"]


def test_every_check_gives_its_message(tmp_path):
    cxx = os.environ.get("CXX") or shutil.which("g++") or shutil.which("c++")
    assert cxx, "tests/solver_checks.cpp needs a C++ compiler (g++ or c++)"
    exe = tmp_path / "solver_checks"
    # the sanitizers' runtimes are linked into the program, so it does not depend on the order in which the loader brings libraries in
    clang = "clang" in subprocess.run([cxx, "--version"], stdout=subprocess.PIPE, text=True).stdout
    subprocess.check_call([cxx, "-std=c++20", "-O1", "-g", "-Wall", "-Wextra", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           *(["-static-libsan"] if clang else ["-static-libasan", "-static-libubsan"]), "-o", str(exe),
                           str(HERE / "solver_checks.cpp")])
    run = subprocess.run([str(exe)], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, stdin=subprocess.DEVNULL)
    assert run.returncode == 0, run.stderr[-4000:]
    want = [f"{entry} {name}: {'OK' if tail is OK else entry + tail}" for entry, cases in ENTRY_POINTS for name, tail in cases.items()] + OUTPUTS
    got = run.stdout.splitlines()
    for g, w in zip(got, want):
        assert g == w
    assert len(got) == len(want)
