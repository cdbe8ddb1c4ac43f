//! aruco3_hip.rs -- the Rust side of the drop-in boundary: binds the aruco3 crate to libaruco3_hip.so
//! (include/aruco3_hip.h), the MI355X implementation of `Detector::detect` and the pose solvers.
//!
//! How a maintainer adds it (INTEGRATION.md has the step-by-step):
//!   * copy this file to `src/hip.rs`, add `mod hip;` to `src/lib.rs` (next to `mod aruco;`, src/lib.rs:1-4);
//!   * delete the body of `impl Detector` in src/aruco.rs:51-122 and of the three public solvers in
//!     src/pose.rs:52-81 -- their replacements are the `impl Detector` block and `pub mod pose_hip` below;
//!   * `build.rs` links `aruco3_hip`.
//!
//! What does NOT change: `Detector { config, dictionary }` keeps exactly its two public fields
//! (src/aruco.rs:46-49), so every struct literal in the wild -- benches/detect_markers.rs:17,33,
//! examples/webcam_kamera.rs:14, examples/macroquad_detect.rs:18, README.md:14 -- compiles unchanged;
//! `detect(&self, image: DynamicImage) -> Detection` keeps its signature (src/aruco.rs:52) and its
//! error style (panic).  The device context (`a3_ctx`) therefore cannot live inside the struct: it
//! lives in a process-wide registry keyed by the detector's VALUE (config bits + dictionary identity),
//! see `registry()`.
//!
//! Status: written against include/aruco3_hip.h ABI version 3; NOT compiled in the build image (no
//! Rust toolchain there).  tests/test_rust_shim.py checks that every entry point of the header is
//! declared here with the same number of parameters and that the `#[repr(C)]` structs list the
//! header's fields in order.

#![allow(dead_code)]
#![allow(clippy::too_many_arguments)]

use std::collections::HashMap;
use std::ffi::CStr;
use std::os::raw::{c_char, c_int, c_void};
use std::sync::atomic::{AtomicBool, AtomicI32, Ordering};
use std::sync::{Arc, Mutex, OnceLock};

use image::{DynamicImage, GrayImage};
use imageproc::point::Point;
use nalgebra as na;

use crate::aruco::{Detection, Detector, DetectorConfig, Marker};
use crate::dictionaries::ARDictionary;
use crate::pinhole::CameraIntrinsics;
use crate::pose::MarkerPose;

// =====================================================================================================
// 1. The C ABI, one declaration per entry point of include/aruco3_hip.h
// =====================================================================================================

pub const A3_ABI_VERSION: c_int = 5;

pub const A3_OK: c_int = 0;
pub const A3_ERR_INVALID: c_int = -1;
pub const A3_ERR_HIP: c_int = -2;
pub const A3_ERR_CAPACITY: c_int = -3;
pub const A3_ERR_LIMIT: c_int = -6; // a fixed limit of the library (65536 candidates per frame): growing the output does not help
pub const A3_ERR_INTERNAL: c_int = -4;
pub const A3_ERR_NO_DEVICE: c_int = -5;

pub const A3_FMT_RGB8: c_int = 0;
pub const A3_FMT_RGBA8: c_int = 1;
pub const A3_FMT_L8: c_int = 2;
/// webcam byte order: examples/webcam_kamera.rs:38-52 re-orders it on the CPU today; the kernel reads it as it is
pub const A3_FMT_BGRA8: c_int = 3;
/// packed 4:2:2 as UVC webcams and capture cards deliver it, 2 bytes per pixel, read in place: the luma byte is the grey level as it
/// stands (Y0 U Y1 V: byte 2x of the row; U Y0 V Y1: byte 2x+1) and the result is, to the bit, that of the luma plane as A3_FMT_L8.
/// (4 is unassigned and refused.)  `DynamicImage` has no such variant: `Detector::detect_raw` takes the bytes.
pub const A3_FMT_YUYV8: c_int = 5;
pub const A3_FMT_UYVY8: c_int = 6;
pub const A3_MEM_HOST: c_int = 0;
pub const A3_MEM_DEVICE: c_int = 1;

pub const A3_STAGE_THRESHOLD: c_int = 0;
pub const A3_STAGE_CONTOUR: c_int = 1;
pub const A3_STAGE_DECODE: c_int = 2;
pub const A3_PROFILE_OFF: c_int = 0;
pub const A3_PROFILE_STAGES: c_int = 1;
pub const A3_PROFILE_THRESHOLD_ONLY: c_int = 2;
pub const A3_PROFILE_THRESHOLD_SAMPLED: c_int = 3;
pub const A3_REFINE_NONE: u32 = 0;
pub const A3_REFINE_SUBPIX: u32 = 1;
pub const A3_REFINE_EDGES: u32 = 2;
pub const A3_POLARITY_DARK: c_int = 0; // a3_set_marker_polarity: the reference (default)
pub const A3_POLARITY_BOTH: c_int = 1; // ... bright-on-dark markers are read too (OpenCV's detectInvertedMarker)
pub const A3_MARKER_INVERTED: u32 = 1; // a3_get_marker_flags: the marker was read complemented
pub const A3_BOARD_NONE: u32 = 0;
pub const A3_BOARD_OK: u32 = 1;
pub const A3_DIST_NONE: u32 = 0;
pub const A3_DIST_RATIONAL: u32 = 1;
pub const A3_DIST_FISHEYE: u32 = 3; // (2 is unassigned and refused)
pub const A3_BOARD_MAX_MARKERS: usize = 1024;
pub const A3_CALIB_FIX_PRINCIPAL_POINT: u32 = 1;
pub const A3_CALIB_ZERO_TANGENT_DIST: u32 = 2;
pub const A3_CALIB_FIX_K3: u32 = 4;
pub const A3_CALIB_RATIONAL_MODEL: u32 = 8;
pub const A3_CALIB_USE_INTRINSIC_GUESS: u32 = 16;
pub const A3_CALIB_OK: u32 = 1;
pub const A3_CALIB_VIEW_USED: u32 = 1;
// a3_calibrate_fisheye_cameras reads a3_calib_camera.flags as these
pub const A3_FISHEYE_FIX_PRINCIPAL_POINT: u32 = 1;
pub const A3_FISHEYE_FIX_K1: u32 = 2;
pub const A3_FISHEYE_FIX_K2: u32 = 4;
pub const A3_FISHEYE_FIX_K3: u32 = 8;
pub const A3_FISHEYE_FIX_K4: u32 = 16;
pub const A3_FISHEYE_USE_INTRINSIC_GUESS: u32 = 32;
pub const A3_FISHEYE_START_MAX_R: f64 = 4.0;

/// a3_config <-> DetectorConfig, src/aruco.rs:23-30
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct A3Config {
    pub threshold_window: u32,
    pub contour_simplification_epsilon: f64,
    pub min_side_length_factor: f32,
    pub min_corner_separation_factor: f32,
    pub homography_sample_size: u32, // usize in the reference (src/aruco.rs:28): narrowed with a check in `to_a3_config`
    pub filter_high_bit_errors: u8,
}

/// a3_marker <-> Marker, src/aruco.rs:8-13 (+ the frame it belongs to in a batch)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3Marker {
    pub frame: u32,
    pub id: u32,
    pub code: u64,
    pub corners: [u32; 8],
    pub hamming_distance: u8,
    pub rotation: u8,
    pub candidate_index: u16,
}

/// a3_pose <-> MarkerPose, src/pose.rs:8-12; rotation row-major, as `Matrix3::new(..)` is written
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3Pose {
    pub error: f32,
    pub rotation: [f32; 9],
    pub translation: [f32; 3],
}

/// a3_intrinsics <-> CameraIntrinsics, src/pinhole.rs:11-18
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct A3Intrinsics {
    pub image_width: u32,
    pub image_height: u32,
    pub focal_x: f32,
    pub focal_y: f32,
    pub principal_x: f32,
    pub principal_y: f32,
}

/// a3_refine_config: sub-pixel corner refinement (not in the reference; include/aruco3_hip.h states the algorithm)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3RefineConfig {
    pub method: u32,
    pub win_half: u32,
    pub relative_win: f32,
    pub max_iterations: u32,
    pub min_shift: f32,
}

/// a3_board_pose: one board pose per frame (not in the reference; include/aruco3_hip.h states the solve)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3BoardPose {
    pub status: u32,
    pub markers_used: u32,
    pub markers_rejected: u32,
    pub iterations: u32,
    pub rms_px: f32,
    pub alt_rms_px: f32,
    pub rotation: [f32; 9],
    pub translation: [f32; 3],
}

/// a3_charuco_config: ChArUco chessboard corners (not in the reference; include/aruco3_hip.h states the interpolation and refinement)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3CharucoConfig {
    pub min_markers: u32,
    pub refine: u32,
    pub win_half: u32,
    pub relative_win: f32,
    pub max_iterations: u32,
    pub min_shift: f32,
}

/// a3_charuco_corner: one chessboard corner found in a frame, raw image pixels
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3CharucoCorner {
    pub frame: u32,
    pub id: u32,
    pub x: f32,
    pub y: f32,
    pub interp_x: f32,
    pub interp_y: f32,
    pub markers_used: u32,
    pub window: u32,
}

/// a3_charuco_pose: one pose per frame from its chessboard corners, board -> camera
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3CharucoPose {
    pub status: u32,
    pub corners_used: u32,
    pub iterations: u32,
    pub reserved: u32,
    pub rms_px: f32,
    pub alt_rms_px: f32,
    pub rotation: [f32; 9],
    pub translation: [f32; 3],
}

/// a3_distortion: OpenCV's rational lens model or, with model A3_DIST_FISHEYE, its cv::fisheye one (not in the reference;
/// include/aruco3_hip.h states the undistortion)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3Distortion {
    pub model: u32,
    pub iterations: u32,
    pub k1: f32,
    pub k2: f32,
    pub p1: f32,
    pub p2: f32,
    pub k3: f32,
    pub k4: f32,
    pub k5: f32,
    pub k6: f32,
    pub max_residual_px: f32,
}

/// a3_calib_camera: one calibration problem (not in the reference; include/aruco3_hip.h states the algorithm)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct A3CalibCamera {
    pub image_width: u32,
    pub image_height: u32,
    pub first_view: u32,
    pub n_views: u32,
    pub flags: u32,
    pub max_iterations: u32,
    pub guess: A3Intrinsics,
    pub guess_distortion: A3Distortion,
}

/// a3_calib_result: one camera's intrinsics, lens model, deviations and fit
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct A3CalibResult {
    pub status: u32,
    pub views_used: u32,
    pub points_used: u32,
    pub iterations: u32,
    pub converged: u32,
    pub reserved: u32,
    pub fx: f64,
    pub fy: f64,
    pub cx: f64,
    pub cy: f64,
    pub dist: [f64; 8],
    pub std_dev: [f64; 12],
    pub rms_px: f64,
    pub intrinsics: A3Intrinsics,
    pub distortion: A3Distortion,
    pub reserved2: u32,
}

/// a3_calib_view: one view's status and pose, board -> camera
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3CalibView {
    pub status: u32,
    pub points: u32,
    pub rms_px: f32,
    pub rotation: [f32; 9],
    pub translation: [f32; 3],
}

/// a3_rig: one rig calibration problem (not in the reference; include/aruco3_hip.h states the algorithm)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3Rig {
    pub first_camera: u32,
    pub n_cameras: u32,
    pub first_frame: u32,
    pub n_frames: u32,
    pub first_obs: u32,
    pub n_obs: u32,
    pub flags: u32,
    pub max_iterations: u32,
}

/// a3_rig_camera: a rig camera's known intrinsics and lens (fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6) and its extrinsic guess
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct A3RigCamera {
    pub a: [f64; 12],
    pub guess_rotation: [f64; 9],
    pub guess_translation: [f64; 3],
}

/// a3_rig_observation: what one camera saw of the board at one instant
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3RigObservation {
    pub camera: u32,
    pub frame: u32,
    pub first_point: u32,
    pub n_points: u32,
}

/// a3_rig_result: one rig's status and fit
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3RigResult {
    pub status: u32,
    pub frames_used: u32,
    pub obs_used: u32,
    pub points_used: u32,
    pub iterations: u32,
    pub converged: u32,
    pub rms_px: f64,
}

/// a3_rig_camera_result: rig -> camera, its deviations and fit
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3RigCameraResult {
    pub rotation: [f64; 9],
    pub translation: [f64; 3],
    pub std_dev: [f64; 6],
    pub rms_px: f64,
    pub rotation_f: [f32; 9],
    pub translation_f: [f32; 3],
    pub obs_used: u32,
    pub points_used: u32,
}

/// a3_rig_frame: one instant's status and pose, board -> rig
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3RigFrame {
    pub status: u32,
    pub obs_used: u32,
    pub points_used: u32,
    pub rms_px: f32,
    pub rotation: [f64; 9],
    pub translation: [f64; 3],
    pub rotation_f: [f32; 9],
    pub translation_f: [f32; 3],
}

/// a3_rig_observation_result: one observation's status and fit
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3RigObservationResult {
    pub status: u32,
    pub points: u32,
    pub rms_px: f32,
    pub reserved: u32,
}

/// a3_handeye_problem: one hand-eye calibration problem, board -> camera G_f = X . M_f . Y (not in the reference; include/aruco3_hip.h
/// states the algorithm)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3HandEyeProblem {
    pub first_frame: u32,
    pub n_frames: u32,
    pub flags: u32,
    pub max_iterations: u32,
    pub a: [f64; 12],
    pub guess_x_rotation: [f64; 9],
    pub guess_x_translation: [f64; 3],
    pub guess_y_rotation: [f64; 9],
    pub guess_y_translation: [f64; 3],
}

/// a3_handeye_frame: the known transform M_f of one frame and its points
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3HandEyeFrame {
    pub rotation: [f64; 9],
    pub translation: [f64; 3],
    pub first_point: u32,
    pub n_points: u32,
}

/// a3_handeye_result: one problem's status, X, Y, their deviations and the fit
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3HandEyeResult {
    pub status: u32,
    pub frames_used: u32,
    pub points_used: u32,
    pub pairs_used: u32,
    pub iterations: u32,
    pub converged: u32,
    pub rms_px: f64,
    pub x_rotation: [f64; 9],
    pub x_translation: [f64; 3],
    pub y_rotation: [f64; 9],
    pub y_translation: [f64; 3],
    pub std_dev: [f64; 12],
    pub x_rotation_f: [f32; 9],
    pub x_translation_f: [f32; 3],
    pub y_rotation_f: [f32; 9],
    pub y_translation_f: [f32; 3],
}

/// a3_handeye_frame_result: one frame's status, fit and own pose board -> camera
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3HandEyeFrameResult {
    pub status: u32,
    pub points: u32,
    pub rms_px: f32,
    pub reserved: u32,
    pub rotation: [f64; 9],
    pub translation: [f64; 3],
    pub rotation_f: [f32; 9],
    pub translation_f: [f32; 3],
}

pub const A3_HANDEYE_USE_GUESS: u32 = 1;
pub const A3_HANDEYE_FIX_X: u32 = 2;
pub const A3_HANDEYE_OK: u32 = 1;
pub const A3_HANDEYE_TOO_FEW_FRAMES: u32 = 2;
pub const A3_HANDEYE_NO_MOTION: u32 = 3;
pub const A3_HANDEYE_NOT_FINITE: u32 = 4;
pub const A3_HANDEYE_FRAME_USED: u32 = 1;
pub const A3_HANDEYE_FRAME_TOO_FEW_POINTS: u32 = 2;
pub const A3_HANDEYE_FRAME_DEGENERATE: u32 = 3;
pub const A3_HANDEYE_MAX_FRAMES: usize = 256;
pub const A3_HANDEYE_MAX_PROBLEMS: usize = 1024;
pub const A3_HANDEYE_MAX_CALL_FRAMES: usize = 65536;

/// a3_map: one marker map problem (not in the reference; include/aruco3_hip.h states the algorithm)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3Map {
    pub first_marker: u32,
    pub n_markers: u32,
    pub first_frame: u32,
    pub n_frames: u32,
    pub first_obs: u32,
    pub n_obs: u32,
    pub flags: u32,
    pub max_iterations: u32,
    pub a: [f64; 12],
    pub marker_length: f32,
    pub reserved: u32,
}

/// a3_map_marker: a marker's guess, marker -> world
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct A3MapMarker {
    pub guess_rotation: [f64; 9],
    pub guess_translation: [f64; 3],
}

/// a3_map_observation: one marker seen in one frame (its four corners are 8 floats of image_xy)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3MapObservation {
    pub marker: u32,
    pub frame: u32,
}

/// a3_map_result: one map's status and fit
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3MapResult {
    pub status: u32,
    pub markers_used: u32,
    pub frames_used: u32,
    pub obs_used: u32,
    pub iterations: u32,
    pub converged: u32,
    pub rms_px: f64,
}

/// a3_map_marker_result: marker -> world, its deviations, fit and corners in world units
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3MapMarkerResult {
    pub rotation: [f64; 9],
    pub translation: [f64; 3],
    pub std_dev: [f64; 6],
    pub rms_px: f64,
    pub corners: [f64; 12],
    pub rotation_f: [f32; 9],
    pub translation_f: [f32; 3],
    pub status: u32,
    pub obs_used: u32,
}

/// a3_map_frame: one frame's status and pose, world -> camera
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3MapFrame {
    pub status: u32,
    pub obs_used: u32,
    pub rms_px: f32,
    pub reserved: u32,
    pub rotation: [f64; 9],
    pub translation: [f64; 3],
    pub rotation_f: [f32; 9],
    pub translation_f: [f32; 3],
}

/// a3_map_observation_result: one observation's status, fit and the fit of step 1's two planar candidates
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3MapObservationResult {
    pub status: u32,
    pub rms_px: f32,
    pub start_rms_px: [f32; 2],
}

/// a3_recover_config: board-aided recovery of markers the decoder rejected (not in the reference; include/aruco3_hip.h states the
/// algorithm; OpenCV's refineDetectedMarkers).  Fill it with a3_default_recover_config: max_hamming is derived from the dictionary.
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3RecoverConfig {
    pub mode: u32,
    pub min_markers: u32,
    pub max_distance_px: f32,
    pub max_hamming: u8,
    pub reserved: [u8; 3],
}

/// a3_rectify: one frame rectification (not in the reference; include/aruco3_hip.h states the map and the blend)
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct A3Rectify {
    pub src: A3Intrinsics,
    pub distortion: A3Distortion,
    pub dst: A3Intrinsics,
    pub rotation: [f32; 9],
    pub fill: u8,
    pub reserved: [u8; 3],
}

/// a3_rectify_info: output tiles per frame and how many of them each launch path of the kernel took
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3RectifyInfo {
    pub tiles: u32,
    pub path_tiles: [u32; 4],
    pub reserved: [u32; 3],
}

/// a3_reduction: detection on frames reduced by `factor` (2, 3 or 4); reserved 0
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3Reduction {
    pub factor: u32,
    pub reserved: [u32; 3],
}

/// a3_stats: per-batch stage counters (the reference prints its rejects in debug builds, src/aruco.rs:163-164)
#[repr(C)]
#[derive(Clone, Copy, Debug, Default)]
pub struct A3Stats {
    pub darts: u64,
    pub contours_traced: u64,
    pub contours_materialised: u64,
    pub candidates_pre: u64,
    pub candidates: u64,
    pub markers: u64,
    pub resolve_iterations: u32,
    pub jump_rounds: u32,
    pub chunks: u32,
    /// bits 0-7: A3_STEP_* (how the library scheduled the batch: 0 whole, 1 decode deferred, 2 chain held and released by the burst's
    /// last member, 3 chain held and released early, 4 the burst's last member, 5 chain still held: between submit and collect only); bits 8-15: other contexts' chains this submit released;
    /// bits 16-23: synchronous re-runs of the batch the device asked for
    pub stepping: u32,
}

/// a3_synth_marker / a3_synth_frame: layouts for the device-side synthetic frame generator
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct A3SynthMarker {
    pub hinv: [f32; 9],
    pub x0: i32,
    pub y0: i32,
    pub x1: i32,
    pub y1: i32,
    pub cells: [u64; 2],
    pub n: u32,
    pub reserved: u32,
}
#[repr(C)]
#[derive(Clone, Copy, Debug)]
pub struct A3SynthFrame {
    pub base: f32,
    pub gx: f32,
    pub gy: f32,
    pub noise_sigma: f32,
    pub first_marker: u32,
    pub n_markers: u32,
    pub seed: u64,
}

/// opaque a3_ctx
#[repr(C)]
pub struct A3Ctx {
    _private: [u8; 0],
}

extern "C" {
    pub fn a3_abi_version() -> c_int;
    pub fn a3_default_config(cfg: *mut A3Config);
    pub fn a3_create(device: c_int, cfg: *const A3Config, codes: *const u64, n_codes: usize, num_bits: u8, tau: u8,
                     out: *mut *mut A3Ctx) -> c_int;
    pub fn a3_destroy(ctx: *mut A3Ctx);
    pub fn a3_last_error(ctx: *const A3Ctx) -> *const c_char;
    pub fn a3_set_stream(ctx: *mut A3Ctx, hip_stream: *mut c_void) -> c_int;
    pub fn a3_get_stream(ctx: *const A3Ctx, hip_stream: *mut *mut c_void) -> c_int;
    pub fn a3_set_pool_limits(ctx: *mut A3Ctx, max_darts: u64, max_points: u64) -> c_int;
    pub fn a3_get_tau(ctx: *const A3Ctx, tau: *mut u8) -> c_int;
    pub fn a3_set_debug_taps(ctx: *mut A3Ctx, enabled: c_int) -> c_int;
    pub fn a3_order_after(ctx: *mut A3Ctx, other: *mut A3Ctx) -> c_int;
    pub fn a3_detect_batch(ctx: *mut A3Ctx, pixels: *const c_void, memory: c_int, fmt: c_int, width: u32, height: u32,
                           row_stride: usize, frame_stride: usize, n_frames: u32, out: *mut A3Marker, out_cap: usize,
                           per_frame_count: *mut u32, out_n: *mut usize) -> c_int;
    pub fn a3_detect_batch_pose(ctx: *mut A3Ctx, pixels: *const c_void, memory: c_int, fmt: c_int, width: u32, height: u32,
                                row_stride: usize, frame_stride: usize, n_frames: u32, marker_size_mm: f32,
                                intr: *const A3Intrinsics, out: *mut A3Marker, poses: *mut A3Pose, out_cap: usize,
                                per_frame_count: *mut u32, out_n: *mut usize) -> c_int;
    pub fn a3_detect_batch_submit(ctx: *mut A3Ctx, pixels: *const c_void, memory: c_int, fmt: c_int, width: u32, height: u32,
                                  row_stride: usize, frame_stride: usize, n_frames: u32, out_cap: usize) -> c_int;
    pub fn a3_detect_batch_collect(ctx: *mut A3Ctx, out: *mut A3Marker, out_cap: usize, per_frame_count: *mut u32,
                                   out_n: *mut usize) -> c_int;
    pub fn a3_detect_batch_pose_submit(ctx: *mut A3Ctx, pixels: *const c_void, memory: c_int, fmt: c_int, width: u32, height: u32,
                                       row_stride: usize, frame_stride: usize, n_frames: u32, marker_size_mm: f32,
                                       intr: *const A3Intrinsics, out_cap: usize) -> c_int;
    pub fn a3_detect_batch_pose_collect(ctx: *mut A3Ctx, out: *mut A3Marker, poses: *mut A3Pose, out_cap: usize,
                                        per_frame_count: *mut u32, out_n: *mut usize) -> c_int;
    pub fn a3_host_alloc(bytes: usize, out: *mut *mut c_void) -> c_int;
    pub fn a3_host_free(p: *mut c_void) -> c_int;
    pub fn a3_host_register(p: *mut c_void, bytes: usize) -> c_int;
    pub fn a3_host_unregister(p: *mut c_void) -> c_int;
    pub fn a3_get_stats(ctx: *const A3Ctx, stats: *mut A3Stats) -> c_int;
    pub fn a3_download_grey(ctx: *mut A3Ctx, frame: u32, dst: *mut u8) -> c_int;
    pub fn a3_download_thresholded(ctx: *mut A3Ctx, frame: u32, dst: *mut u8) -> c_int;
    pub fn a3_candidate_count(ctx: *mut A3Ctx, frame: u32, n_pre: *mut u32, n_final: *mut u32) -> c_int;
    pub fn a3_download_candidates(ctx: *mut A3Ctx, frame: u32, before_discard: c_int, dst_xy: *mut u32, cap_quads: usize) -> c_int;
    pub fn a3_download_homographies(ctx: *mut A3Ctx, frame: u32, dst: *mut u8, ok: *mut u8, codes4: *mut u64,
                                    decode_ok: *mut i32, cap: usize) -> c_int;
    pub fn a3_contour_count(ctx: *mut A3Ctx, frame: u32, n_contours: *mut u32, n_points: *mut u64) -> c_int;
    pub fn a3_download_contours(ctx: *mut A3Ctx, frame: u32, start_keys: *mut u32, lengths: *mut u32, points_xy: *mut u32,
                                cap_contours: usize, cap_points: usize) -> c_int;
    pub fn a3_detection_record_bytes(max_markers_per_frame: u32, with_poses: c_int) -> usize;
    pub fn a3_pack_detections(ctx: *mut A3Ctx, first_frame_global: u32, max_markers_per_frame: u32, with_poses: c_int,
                              dst_device: *mut c_void, dst_bytes: usize) -> c_int;
    pub fn a3_estimate_pose(ctx: *mut A3Ctx, corners_xy: *const u32, n: usize, marker_size_mm: f32, intr: *const A3Intrinsics,
                            image_width: u32, image_height: u32, out: *mut A3Pose) -> c_int;
    pub fn a3_estimate_pose_normalized(ctx: *mut A3Ctx, points_xy: *const f32, n: usize, marker_size_mm: f32,
                                       out: *mut A3Pose) -> c_int;
    pub fn a3_find_nearest(ctx: *mut A3Ctx, bits: *const u64, n: usize, idx: *mut u32, dist: *mut u8) -> c_int;
    pub fn a3_default_refine_config(cfg: *mut A3RefineConfig);
    pub fn a3_set_corner_refinement(ctx: *mut A3Ctx, cfg: *const A3RefineConfig) -> c_int;
    pub fn a3_get_refined_corners(ctx: *mut A3Ctx, dst_xy: *mut f32, cap_markers: usize, n: *mut usize) -> c_int;
    pub fn a3_refine_corners(ctx: *mut A3Ctx, pixels: *const c_void, memory: c_int, fmt: c_int, width: u32, height: u32,
                             row_stride: usize, corners_xy: *mut f32, cell_px: *const f32, n: usize) -> c_int;
    pub fn a3_set_board(ctx: *mut A3Ctx, ids: *const u32, corners_xy: *const f32, n: usize) -> c_int;
    pub fn a3_get_board_poses(ctx: *mut A3Ctx, dst: *mut A3BoardPose, cap_frames: usize, n: *mut usize) -> c_int;
    pub fn a3_estimate_board_pose(ctx: *mut A3Ctx, ids: *const u32, corners_xy: *const f32, n_markers: usize, intr: *const A3Intrinsics,
                                  image_width: u32, image_height: u32, out: *mut A3BoardPose) -> c_int;
    pub fn a3_set_board3d(ctx: *mut A3Ctx, ids: *const u32, corners_xyz: *const f32, n: usize) -> c_int;
    pub fn a3_default_recover_config(ctx: *const A3Ctx, cfg: *mut A3RecoverConfig) -> c_int;
    pub fn a3_set_board_recovery(ctx: *mut A3Ctx, cfg: *const A3RecoverConfig) -> c_int;
    pub fn a3_get_board_recovery(ctx: *const A3Ctx, cfg: *mut A3RecoverConfig) -> c_int;
    pub fn a3_get_recovered_counts(ctx: *mut A3Ctx, per_frame_recovered: *mut u32, n_frames: usize) -> c_int;
    pub fn a3_recover_markers(ctx: *mut A3Ctx, detected_ids: *const u32, detected_corners_xy: *const u32, n_detected: usize,
                              candidate_corners_xy: *const u32, codes4: *const u64, has_codes: *const u8, n_candidates: usize,
                              cfg: *const A3RecoverConfig, out: *mut A3Marker, out_cap: usize, out_n: *mut usize) -> c_int;
    pub fn a3_default_distortion(d: *mut A3Distortion);
    pub fn a3_set_distortion(ctx: *mut A3Ctx, d: *const A3Distortion) -> c_int;
    pub fn a3_get_undistorted_corners(ctx: *mut A3Ctx, dst_xy: *mut f32, residual_px: *mut f32, cap_markers: usize, n: *mut usize) -> c_int;
    pub fn a3_undistort_points(ctx: *mut A3Ctx, xy: *const f32, n: usize, intr: *const A3Intrinsics, d: *const A3Distortion, out_xy: *mut f32,
                               residual_px: *mut f32) -> c_int;
    pub fn a3_default_charuco_config(cfg: *mut A3CharucoConfig);
    pub fn a3_set_charuco(ctx: *mut A3Ctx, corners_xy: *const f32, adjacent_ids: *const u32, n_corners: usize, cfg: *const A3CharucoConfig) -> c_int;
    pub fn a3_get_charuco_corners(ctx: *mut A3Ctx, dst: *mut A3CharucoCorner, cap: usize, n: *mut usize) -> c_int;
    pub fn a3_get_charuco_poses(ctx: *mut A3Ctx, dst: *mut A3CharucoPose, cap_frames: usize, n: *mut usize) -> c_int;
    pub fn a3_interpolate_charuco(ctx: *mut A3Ctx, pixels: *const c_void, memory: c_int, fmt: c_int, width: u32, height: u32, row_stride: usize,
                                  ids: *const u32, corners_xy: *const f32, n_markers: usize, dst: *mut A3CharucoCorner, cap: usize,
                                  n: *mut usize) -> c_int;
    pub fn a3_calibrate_cameras(ctx: *mut A3Ctx, cams: *const A3CalibCamera, n_cams: usize, view_offsets: *const u32, n_views: usize,
                                object_xy: *const f32, image_xy: *const f32, results: *mut A3CalibResult, views: *mut A3CalibView) -> c_int;
    pub fn a3_calibrate_fisheye_cameras(ctx: *mut A3Ctx, cams: *const A3CalibCamera, n_cams: usize, view_offsets: *const u32, n_views: usize,
                                        object_xy: *const f32, image_xy: *const f32, results: *mut A3CalibResult, views: *mut A3CalibView) -> c_int;
    pub fn a3_calibrate_rigs(ctx: *mut A3Ctx, rigs: *const A3Rig, n_rigs: usize, cameras: *const A3RigCamera, n_cameras: usize,
                             obs: *const A3RigObservation, n_obs: usize, object_xy: *const f32, image_xy: *const f32,
                             results: *mut A3RigResult, camera_results: *mut A3RigCameraResult, frames: *mut A3RigFrame,
                             obs_results: *mut A3RigObservationResult) -> c_int;
    pub fn a3_calibrate_hand_eyes(ctx: *mut A3Ctx, problems: *const A3HandEyeProblem, n_problems: usize, frames: *const A3HandEyeFrame,
                                  n_frames: usize, object_xy: *const f32, image_xy: *const f32, results: *mut A3HandEyeResult,
                                  frame_results: *mut A3HandEyeFrameResult) -> c_int;
    pub fn a3_build_marker_maps(ctx: *mut A3Ctx, maps: *const A3Map, n_maps: usize, markers: *const A3MapMarker, n_markers: usize,
                                obs: *const A3MapObservation, n_obs: usize, image_xy: *const f32, results: *mut A3MapResult,
                                marker_results: *mut A3MapMarkerResult, frames: *mut A3MapFrame,
                                obs_results: *mut A3MapObservationResult) -> c_int;
    pub fn a3_default_rectify(r: *mut A3Rectify, src: *const A3Intrinsics, d: *const A3Distortion);
    pub fn a3_rectify_frames(ctx: *mut A3Ctx, src: *const c_void, src_memory: c_int, fmt: c_int, src_row_stride: usize, src_frame_stride: usize,
                             n_frames: u32, r: *const A3Rectify, dst: *mut c_void, dst_memory: c_int, dst_row_stride: usize,
                             dst_frame_stride: usize, info: *mut A3RectifyInfo) -> c_int;
    pub fn a3_set_rectification(ctx: *mut A3Ctx, r: *const A3Rectify) -> c_int;
    pub fn a3_get_rectification(ctx: *const A3Ctx, r: *mut A3Rectify, enabled: *mut c_int) -> c_int;
    pub fn a3_reduce_frames(ctx: *mut A3Ctx, src: *const c_void, src_memory: c_int, fmt: c_int, width: u32, height: u32,
                            src_row_stride: usize, src_frame_stride: usize, n_frames: u32, factor: u32, dst: *mut c_void,
                            dst_memory: c_int, dst_row_stride: usize, dst_frame_stride: usize) -> c_int;
    pub fn a3_set_reduction(ctx: *mut A3Ctx, r: *const A3Reduction) -> c_int;
    pub fn a3_get_reduction(ctx: *const A3Ctx, r: *mut A3Reduction, enabled: *mut c_int) -> c_int;
    pub fn a3_set_threshold_windows(ctx: *mut A3Ctx, radii: *const u32, n: usize) -> c_int;
    pub fn a3_get_threshold_windows(ctx: *const A3Ctx, radii: *mut u32, cap: usize, n: *mut usize) -> c_int;
    pub fn a3_set_marker_polarity(ctx: *mut A3Ctx, mode: c_int) -> c_int;
    pub fn a3_get_marker_polarity(ctx: *const A3Ctx, mode: *mut c_int) -> c_int;
    pub fn a3_get_marker_flags(ctx: *mut A3Ctx, dst: *mut u32, cap_markers: usize, n: *mut usize) -> c_int;
    pub fn a3_calculate_tau(device: c_int, codes: *const u64, n_codes: usize, tau: *mut u8) -> c_int;
    pub fn a3_set_profiling(ctx: *mut A3Ctx, mode: c_int) -> c_int;
    pub fn a3_get_profile(ctx: *mut A3Ctx, stage: c_int, total_ms: *mut f64, launches: *mut u64, reset: c_int) -> c_int;
    pub fn a3_synth_render(device: c_int, hip_stream: *mut c_void, frames: *const A3SynthFrame, n_frames: u32,
                           markers: *const A3SynthMarker, n_markers: u32, width: u32, height: u32, paper: c_int, black: f32,
                           white: f32, supersample: c_int, out_rgb_device: *mut c_void, row_stride: usize,
                           frame_stride: usize) -> c_int;
}

// =====================================================================================================
// 2. Contexts: owned by a process-wide registry, never by `Detector`
// =====================================================================================================

/// One `a3_ctx`.  A context is not re-entrant (header: "one a3_ctx per (device, stream)"), so it is only ever touched
/// through the `Mutex` of its registry slot; that keeps `&Detector` `Sync`, as the reference's plain struct is.
pub struct HipCtx {
    raw: *mut A3Ctx,
    /// pinned staging for the frames of a call, grow-only and re-used from call to call (page-locking memory costs far more
    /// than a frame's copy: it is not done per `detect()`)
    staging: PinnedBytes,
}
// the raw pointer is only dereferenced by the library, under the slot's Mutex
unsafe impl Send for HipCtx {}

impl HipCtx {
    fn create(device: c_int, cfg: &A3Config, dict: &ARDictionary) -> HipCtx {
        let mut raw: *mut A3Ctx = std::ptr::null_mut();
        // tau == 0 would ask the library to compute it (src/dictionaries.rs:124); ARDictionary::new_from_ar_dictionary has
        // already done so, the value is simply passed on
        let rc = unsafe { a3_create(device, cfg, dict.code_list.as_ptr(), dict.code_list.len(), dict.num_bits, dict.tau, &mut raw) };
        if rc != A3_OK {
            // the reference's error style: threshold_window == 0 trips an assert inside imageproc, a bad dictionary panics
            // (src/dictionaries.rs:144); a missing GPU has no precedent and panics with the library's message
            panic!("aruco3_hip: a3_create failed ({}): {}", rc, last_error(std::ptr::null()));
        }
        HipCtx { raw, staging: PinnedBytes::empty() }
    }
    fn check(&self, rc: c_int, what: &str) {
        if rc != A3_OK {
            panic!("aruco3_hip: {} failed ({}): {}", what, rc, last_error(self.raw));
        }
    }
}

impl Drop for HipCtx {
    fn drop(&mut self) {
        if !self.raw.is_null() {
            unsafe { a3_destroy(self.raw) };
            self.raw = std::ptr::null_mut();
        }
    }
}

fn last_error(ctx: *const A3Ctx) -> String {
    // ctx may be NULL: the message of the last failed a3_create
    let p = unsafe { a3_last_error(ctx) };
    if p.is_null() {
        return String::new();
    }
    unsafe { CStr::from_ptr(p) }.to_string_lossy().into_owned()
}

/// What makes two `Detector` values the same detector: every config field bit for bit, the dictionary's table
/// (`&'static [u64]`: address + length identify it for the life of the process), num_bits, tau, and the device.
#[derive(Clone, Copy, PartialEq, Eq, Hash, Debug)]
struct Key {
    threshold_window: u32,
    eps_bits: u64,
    min_side_bits: u32,
    min_sep_bits: u32,
    sample: usize,
    filter: bool,
    codes_ptr: usize,
    codes_len: usize,
    num_bits: u8,
    tau: u8,
    device: c_int,
}

fn key_of(d: &Detector, device: c_int) -> Key {
    Key {
        threshold_window: d.config.threshold_window,
        eps_bits: d.config.contour_simplification_epsilon.to_bits(),
        min_side_bits: d.config.min_side_length_factor.to_bits(),
        min_sep_bits: d.config.min_corner_separation_factor.to_bits(),
        sample: d.config.homography_sample_size,
        filter: d.config.filter_high_bit_errors,
        codes_ptr: d.dictionary.code_list.as_ptr() as usize,
        codes_len: d.dictionary.code_list.len(),
        num_bits: d.dictionary.num_bits,
        tau: d.dictionary.tau,
        device,
    }
}

fn to_a3_config(c: &DetectorConfig) -> A3Config {
    // usize -> u32 (src/aruco.rs:28 vs a3_config): the library accepts 1..=200, which covers every marker family
    // (the patch only has to hold the mark_size x mark_size grid); anything else is a caller error
    if c.homography_sample_size == 0 || c.homography_sample_size > 200 {
        panic!("aruco3_hip: homography_sample_size must be in 1..=200, got {}", c.homography_sample_size);
    }
    A3Config {
        threshold_window: c.threshold_window,
        contour_simplification_epsilon: c.contour_simplification_epsilon,
        min_side_length_factor: c.min_side_length_factor,
        min_corner_separation_factor: c.min_corner_separation_factor,
        homography_sample_size: c.homography_sample_size as u32,
        filter_high_bit_errors: c.filter_high_bit_errors as u8,
    }
}

type Slot = Arc<Mutex<HipCtx>>;
struct Registry {
    slots: HashMap<Key, (Slot, u64)>, // context + last-use tick
    tick: u64,
}
/// more distinct detectors than this alive at once evicts the least recently used context (each owns device buffers)
const MAX_CONTEXTS: usize = 8;

fn registry() -> &'static Mutex<Registry> {
    static REG: OnceLock<Mutex<Registry>> = OnceLock::new();
    REG.get_or_init(|| Mutex::new(Registry { slots: HashMap::new(), tick: 0 }))
}

static DEVICE: AtomicI32 = AtomicI32::new(0);
static POPULATE: AtomicBool = AtomicBool::new(true);

/// HIP device the contexts are created on (default 0).  One process per GPU is the intended deployment.
pub fn set_device(device: i32) {
    DEVICE.store(device, Ordering::Relaxed);
}

/// `Detection.grey`, `.candidates` and `.homographies` (src/aruco.rs:115-120) are filled by default, exactly as the
/// reference returns them.  They cost a 2 MB read-back per 1080p frame and a grey plane K1 otherwise never writes;
/// callers that only read `.markers` (both webcam examples) switch them off here and get `grey: None`, empty vectors.
pub fn set_populate_debug_outputs(on: bool) {
    POPULATE.store(on, Ordering::Relaxed);
}

/// Destroys every context (device buffers, stream).  Optional: contexts otherwise live until the process exits.
pub fn shutdown() {
    registry().lock().unwrap().slots.clear();
}

fn slot_for(d: &Detector) -> Slot {
    let device = DEVICE.load(Ordering::Relaxed);
    let key = key_of(d, device);
    let mut reg = registry().lock().unwrap();
    reg.tick += 1;
    let tick = reg.tick;
    if let Some((slot, used)) = reg.slots.get_mut(&key) {
        *used = tick;
        return slot.clone();
    }
    if reg.slots.len() >= MAX_CONTEXTS {
        if let Some(oldest) = reg.slots.iter().min_by_key(|(_, (_, used))| *used).map(|(k, _)| *k) {
            reg.slots.remove(&oldest); // dropped (a3_destroy) once no call holds its Arc any more
        }
    }
    let slot: Slot = Arc::new(Mutex::new(HipCtx::create(device, &to_a3_config(&d.config), &d.dictionary)));
    reg.slots.insert(key, (slot.clone(), tick));
    slot
}

// =====================================================================================================
// 3. Detector::detect (replaces src/aruco.rs:52-121) + the batch form the GPU wants
// =====================================================================================================

/// Page-locked host memory from `a3_host_alloc`: frames packed here cross the link asynchronously and at its full rate
/// (include/aruco3_hip.h, "Host frames").  Falls back to nothing: an allocation failure panics like every other error.
struct PinnedBytes {
    ptr: *mut u8,
    len: usize,
    cap: usize,
}
// only ever touched under the Mutex of the context that owns it
unsafe impl Send for PinnedBytes {}
impl PinnedBytes {
    fn empty() -> PinnedBytes {
        PinnedBytes { ptr: std::ptr::null_mut(), len: 0, cap: 0 }
    }
    /// empty the buffer and make room for `cap` bytes (re-allocating only when it has to grow)
    fn reset(&mut self, cap: usize) {
        self.len = 0;
        if cap <= self.cap {
            return;
        }
        if !self.ptr.is_null() {
            unsafe { a3_host_free(self.ptr as *mut c_void) };
            self.ptr = std::ptr::null_mut();
            self.cap = 0;
        }
        let mut p: *mut c_void = std::ptr::null_mut();
        let rc = unsafe { a3_host_alloc(cap, &mut p) };
        if rc != A3_OK || p.is_null() {
            panic!("aruco3_hip: a3_host_alloc({}) failed ({}): {}", cap, rc, last_error(std::ptr::null()));
        }
        self.ptr = p as *mut u8;
        self.cap = cap;
    }
    fn extend_from_slice(&mut self, src: &[u8]) {
        assert!(self.len + src.len() <= self.cap, "aruco3_hip: packed batch larger than computed");
        unsafe { std::ptr::copy_nonoverlapping(src.as_ptr(), self.ptr.add(self.len), src.len()) };
        self.len += src.len();
    }
    fn as_ptr(&self) -> *const u8 {
        self.ptr
    }
}
impl Drop for PinnedBytes {
    fn drop(&mut self) {
        if !self.ptr.is_null() {
            unsafe { a3_host_free(self.ptr as *mut c_void) };
            self.ptr = std::ptr::null_mut();
        }
    }
}

/// One batch as the library wants it: frames of one size and one layout, back to back, in the context's pinned staging buffer.
struct Packed {
    fmt: c_int,
    bpp: usize,
    width: u32,
    height: u32,
    bytes: *const u8,
}

/// `DynamicImage` -> raw bytes without touching pixel values.  Rgb8 / Rgba8 / Luma8 buffers are handed over as they are
/// (the kernel applies `into_luma8`'s integer formula itself, src/aruco.rs:60); every other variant (16-bit, float,
/// LumaA) goes through the crate's own `into_luma8()` on the CPU first, so its result is the reference's by construction.
fn pack(images: &[DynamicImage], staging: &mut PinnedBytes) -> Packed {
    assert!(!images.is_empty(), "aruco3_hip: empty batch");
    let (width, height) = (images[0].width(), images[0].height());
    let kind = |im: &DynamicImage| -> (c_int, usize) {
        match im {
            DynamicImage::ImageRgb8(_) => (A3_FMT_RGB8, 3),
            DynamicImage::ImageRgba8(_) => (A3_FMT_RGBA8, 4),
            _ => (A3_FMT_L8, 1),
        }
    };
    let (fmt, bpp) = kind(&images[0]);
    let uniform = images.iter().all(|im| kind(im).0 == fmt);
    let (fmt, bpp) = if uniform { (fmt, bpp) } else { (A3_FMT_L8, 1) }; // mixed layouts: everything to Luma8
    staging.reset(images.len() * width as usize * height as usize * bpp);
    let bytes = staging;
    for im in images {
        assert!(im.width() == width && im.height() == height, "aruco3_hip: all frames of a batch must have one size");
        match (fmt, im) {
            (A3_FMT_RGB8, DynamicImage::ImageRgb8(b)) => bytes.extend_from_slice(b.as_raw()),
            (A3_FMT_RGBA8, DynamicImage::ImageRgba8(b)) => bytes.extend_from_slice(b.as_raw()),
            (_, DynamicImage::ImageLuma8(b)) => bytes.extend_from_slice(b.as_raw()),
            (_, other) => bytes.extend_from_slice(other.clone().into_luma8().as_raw()),
        }
    }
    Packed { fmt, bpp, width, height, bytes: bytes.as_ptr() }
}

fn marker_of(m: &A3Marker) -> Marker {
    Marker {
        id: m.id as usize,
        code: m.code,
        corners: (0..4).map(|i| (m.corners[2 * i], m.corners[2 * i + 1])).collect(),
        hamming_distance: m.hamming_distance,
    }
}

/// Detection.grey / .candidates / .homographies of frame `f` of the batch that just ran with debug taps on
fn fill_debug_outputs(ctx: &HipCtx, f: u32, width: u32, height: u32, sample: u32, det: &mut Detection) {
    let mut grey = vec![0u8; width as usize * height as usize];
    ctx.check(unsafe { a3_download_grey(ctx.raw, f, grey.as_mut_ptr()) }, "a3_download_grey");
    det.grey = GrayImage::from_raw(width, height, grey);
    let (mut n_pre, mut n_final) = (0u32, 0u32);
    ctx.check(unsafe { a3_candidate_count(ctx.raw, f, &mut n_pre, &mut n_final) }, "a3_candidate_count");
    let n = n_final as usize;
    let mut xy = vec![0u32; 8 * n.max(1)];
    ctx.check(unsafe { a3_download_candidates(ctx.raw, f, 0, xy.as_mut_ptr(), n.max(1)) }, "a3_download_candidates");
    det.candidates = (0..n).map(|k| (0..4).map(|i| Point::new(xy[8 * k + 2 * i], xy[8 * k + 2 * i + 1])).collect()).collect();
    let s2 = (sample * sample) as usize;
    let mut patches = vec![0u8; s2 * n.max(1)];
    let mut ok = vec![0u8; n.max(1)];
    ctx.check(unsafe { a3_download_homographies(ctx.raw, f, patches.as_mut_ptr(), ok.as_mut_ptr(), std::ptr::null_mut(),
                                                std::ptr::null_mut(), n.max(1)) }, "a3_download_homographies");
    det.homographies = (0..n).map(|k| {
        if ok[k] != 0 {
            GrayImage::from_raw(sample, sample, patches[k * s2..(k + 1) * s2].to_vec()).unwrap()
        } else {
            GrayImage::new(1, 1) // src/aruco.rs:256: a failed projection leaves a 1x1 black image
        }
    }).collect();
}

/// With `Detection.homographies` populated the library keeps one patch per candidate of the batch, up to 2^20 patches per call;
/// a populated call therefore never carries more frames than this (larger batches are split).
const MAX_TAPPED_FRAMES: usize = 1024;
/// The library's candidate tables grow to 65536 quads per frame (beyond that a3_detect_batch reports A3_ERR_LIMIT, which no retry
/// cures and which `check` turns into a panic at once): marker lists are grown and the batch re-run only on A3_ERR_CAPACITY, and at
/// most up to that many markers per frame.
const MAX_MARKERS_PER_FRAME: usize = 65536;

/// Sub-pixel corner refinement settings for `Detector::detect_refined` (an extension: the reference has no refinement).
/// `Default` gives a3_default_refine_config's values.
#[derive(Clone, Copy, Debug)]
pub struct RefineConfig {
    pub win_half: u32,       // 1..10
    pub relative_win: f32,   // 0 = always win_half
    pub max_iterations: u32, // at most 100
    pub min_shift: f32,      // px
    pub method: u32,         // A3_REFINE_SUBPIX (default) or A3_REFINE_EDGES
}
impl Default for RefineConfig {
    fn default() -> Self {
        RefineConfig { win_half: 5, relative_win: 0.4, max_iterations: 30, min_shift: 0.01, method: A3_REFINE_SUBPIX }
    }
}
impl RefineConfig {
    /// Edge-fit refinement (A3_REFINE_EDGES): corners from lines fitted to the sides.  `win_half` 10 is the search range that corners
    /// mapped up from a reduced plane want; the fit assumes straight sides (no uncorrected lens).
    pub fn edges() -> Self {
        RefineConfig { win_half: 10, method: A3_REFINE_EDGES, ..Default::default() }
    }
    /// the same settings with another method (A3_REFINE_SUBPIX or A3_REFINE_EDGES)
    pub fn method(mut self, method: u32) -> Self {
        self.method = method;
        self
    }
    fn to_a3(&self) -> A3RefineConfig {
        A3RefineConfig { method: self.method, win_half: self.win_half, relative_win: self.relative_win,
                         max_iterations: self.max_iterations, min_shift: self.min_shift }
    }
}

/// A calibrated lens for `Detector::detect_pose_distorted` (an extension: the reference assumes an ideal pinhole camera):
/// OpenCV's distCoeffs k1 k2 p1 p2 k3 [k4 k5 k6] (a 5-coefficient calibration leaves k4..k6 at 0).  `Default` gives
/// a3_default_distortion's values: no distortion, 20 iterations, 0.1 px accepted residual.  `model` A3_DIST_FISHEYE
/// (`Distortion::fisheye`) reads k1 k2 k3 k4 as cv::fisheye's D; p1 p2 k5 k6 must then be 0.
#[derive(Clone, Copy, Debug)]
pub struct Distortion {
    pub model: u32,           // A3_DIST_RATIONAL or A3_DIST_FISHEYE
    pub k1: f32,
    pub k2: f32,
    pub p1: f32,
    pub p2: f32,
    pub k3: f32,
    pub k4: f32,
    pub k5: f32,
    pub k6: f32,
    pub iterations: u32,      // 1..100
    pub max_residual_px: f32, // a corner whose undistortion reprojects farther than this is kept as detected (residual +inf)
}
impl Default for Distortion {
    fn default() -> Self {
        Distortion { model: A3_DIST_RATIONAL, k1: 0.0, k2: 0.0, p1: 0.0, p2: 0.0, k3: 0.0, k4: 0.0, k5: 0.0, k6: 0.0, iterations: 20, max_residual_px: 0.1 }
    }
}
impl Distortion {
    /// cv::fisheye's four coefficients (Kannala-Brandt: theta_d = theta (1 + k1 theta^2 + k2 theta^4 + k3 theta^6 + k4 theta^8))
    pub fn fisheye(k1: f32, k2: f32, k3: f32, k4: f32) -> Self {
        Distortion { model: A3_DIST_FISHEYE, k1, k2, k3, k4, ..Default::default() }
    }
    fn to_a3(&self) -> A3Distortion {
        A3Distortion { model: self.model, iterations: self.iterations, k1: self.k1, k2: self.k2, p1: self.p1, p2: self.p2, k3: self.k3,
                       k4: self.k4, k5: self.k5, k6: self.k6, max_residual_px: self.max_residual_px }
    }
}

/// What `Detector::detect_pose_distorted` returns per marker, in the order of `Detection.markers`.
#[derive(Clone, Debug)]
pub struct UndistortedMarker {
    pub poses: (MarkerPose, MarkerPose),       // lower error first, solved from the undistorted corners
    pub corners: [(f32, f32); 4],              // undistorted pixel corners, `Marker.corners` order
    pub residual_px: [f32; 4],                 // +inf: that corner could not be undistorted and kept its detected position
}

impl Detector {
    /// New (additive): `detect` of one image plus the pose of every marker, solved from its corners undistorted on the device
    /// through `dist` (the poses `estimate_pose` gives assume an ideal pinhole camera).  `Detector` itself gains no field: the
    /// distortion is handed to the shared context for this call only, under its lock.
    pub fn detect_pose_distorted(&self, image: DynamicImage, marker_size_mm: f32, intrinsics: &CameraIntrinsics, dist: &Distortion)
                                 -> (Detection, Vec<UndistortedMarker>) {
        let slot = slot_for(self);
        let mut ctx = slot.lock().unwrap();
        let images = std::slice::from_ref(&image);
        let p = pack(images, &mut ctx.staging);
        ctx.check(unsafe { a3_set_debug_taps(ctx.raw, 0) }, "a3_set_debug_taps");
        let d = dist.to_a3();
        ctx.check(unsafe { a3_set_distortion(ctx.raw, &d) }, "a3_set_distortion");
        let intr = to_a3_intrinsics(intrinsics);
        let mut cap = 64usize;
        let mut markers = vec![A3Marker::default(); cap];
        let mut poses = vec![A3Pose::default(); 2 * cap];
        let mut per = vec![0u32; 1];
        let mut found = 0usize;
        let rc = loop {
            let rc = unsafe {
                a3_detect_batch_pose(ctx.raw, p.bytes as *const c_void, A3_MEM_HOST, p.fmt, p.width, p.height, p.width as usize * p.bpp,
                                     p.width as usize * p.height as usize * p.bpp, 1, marker_size_mm, &intr, markers.as_mut_ptr(),
                                     poses.as_mut_ptr(), cap, per.as_mut_ptr(), &mut found)
            };
            if rc == A3_ERR_CAPACITY && cap < MAX_MARKERS_PER_FRAME {
                cap *= 4;
                markers.resize(cap, A3Marker::default());
                poses.resize(2 * cap, A3Pose::default());
                continue;
            }
            break rc;
        };
        let mut xy = vec![0f32; 8 * found.max(1)];
        let mut res = vec![0f32; 4 * found.max(1)];
        let mut n = 0usize;
        let rc2 = if rc == A3_OK {
            unsafe { a3_get_undistorted_corners(ctx.raw, xy.as_mut_ptr(), res.as_mut_ptr(), found.max(1), &mut n) }
        } else {
            rc
        };
        unsafe { a3_set_distortion(ctx.raw, std::ptr::null()) }; // the shared context goes back to the ideal pinhole
        ctx.check(rc, "a3_detect_batch_pose");
        ctx.check(rc2, "a3_get_undistorted_corners");
        let det = Detection { grey: None, candidates: vec![], homographies: vec![], markers: markers[..found].iter().map(marker_of).collect() };
        let out = (0..n).map(|i| {
            let q = &xy[8 * i..8 * i + 8];
            UndistortedMarker {
                poses: (to_marker_pose(&poses[2 * i]), to_marker_pose(&poses[2 * i + 1])),
                corners: [(q[0], q[1]), (q[2], q[3]), (q[4], q[5]), (q[6], q[7])],
                residual_px: [res[4 * i], res[4 * i + 1], res[4 * i + 2], res[4 * i + 3]],
            }
        }).collect();
        (det, out)
    }

    /// New (additive): `detect` plus the sub-pixel corners of every marker, in the order of `Detection.markers`, each
    /// in `Marker.corners` order.  The Detection is the one `detect` returns; `Detector` itself gains no field (the setting
    /// is handed to the shared context for this call only, under its lock).
    pub fn detect_refined(&self, image: DynamicImage, refine: &RefineConfig) -> (Detection, Vec<[(f32, f32); 4]>) {
        let populate = POPULATE.load(Ordering::Relaxed);
        let slot = slot_for(self);
        let mut ctx = slot.lock().unwrap();
        let images = std::slice::from_ref(&image);
        let p = pack(images, &mut ctx.staging);
        ctx.check(unsafe { a3_set_debug_taps(ctx.raw, populate as c_int) }, "a3_set_debug_taps");
        let cfg = refine.to_a3();
        ctx.check(unsafe { a3_set_corner_refinement(ctx.raw, &cfg) }, "a3_set_corner_refinement");
        let mut markers = vec![A3Marker::default(); 64];
        let mut per = vec![0u32; 1];
        let mut found = 0usize;
        let rc = loop {
            let rc = unsafe {
                a3_detect_batch(ctx.raw, p.bytes as *const c_void, A3_MEM_HOST, p.fmt, p.width, p.height, p.width as usize * p.bpp,
                                p.width as usize * p.height as usize * p.bpp, 1, markers.as_mut_ptr(), markers.len(), per.as_mut_ptr(),
                                &mut found)
            };
            if rc == A3_ERR_CAPACITY && markers.len() < MAX_MARKERS_PER_FRAME {
                markers.resize(markers.len() * 4, A3Marker::default());
                continue;
            }
            break rc;
        };
        let mut xy = vec![0f32; 8 * found.max(1)];
        let mut n = 0usize;
        let rc2 = if rc == A3_OK { unsafe { a3_get_refined_corners(ctx.raw, xy.as_mut_ptr(), found.max(1), &mut n) } } else { rc };
        unsafe { a3_set_corner_refinement(ctx.raw, std::ptr::null()) }; // the shared context goes back to the plain detect
        ctx.check(rc, "a3_detect_batch");
        ctx.check(rc2, "a3_get_refined_corners");
        let mut det = Detection { grey: None, candidates: vec![], homographies: vec![], markers: markers[..found].iter().map(marker_of).collect() };
        if populate {
            fill_debug_outputs(&ctx, 0, p.width, p.height, self.config.homography_sample_size as u32, &mut det);
        }
        let refined = (0..n).map(|i| {
            let q = &xy[8 * i..8 * i + 8];
            [(q[0], q[1]), (q[2], q[3]), (q[4], q[5]), (q[6], q[7])]
        }).collect();
        (det, refined)
    }

    /// New (additive): `detect` of an image seen through a lens, rectified inside the call (a3_set_rectification): `image` has the
    /// size of `rect.src`, the Detection is the one `detect` returns for the image a3_rectify_frames makes of it -- corners are pixels
    /// of `rect.dst`'s view, and the pose solvers take that view's plain intrinsics.  The Python twin is
    /// `Detector(rectification=...)`; here `Detector` itself gains no field (the setting is handed to the shared context for this call
    /// only, under its lock, as `detect_refined` hands over its refinement).
    pub fn detect_rectified(&self, image: DynamicImage, rect: &A3Rectify) -> Detection {
        let populate = POPULATE.load(Ordering::Relaxed);
        let slot = slot_for(self);
        let mut ctx = slot.lock().unwrap();
        let images = std::slice::from_ref(&image);
        let p = pack(images, &mut ctx.staging);
        ctx.check(unsafe { a3_set_debug_taps(ctx.raw, populate as c_int) }, "a3_set_debug_taps");
        ctx.check(unsafe { a3_set_rectification(ctx.raw, rect) }, "a3_set_rectification");
        let mut markers = vec![A3Marker::default(); 64];
        let mut per = vec![0u32; 1];
        let mut found = 0usize;
        let rc = loop {
            let rc = unsafe {
                a3_detect_batch(ctx.raw, p.bytes as *const c_void, A3_MEM_HOST, p.fmt, p.width, p.height, p.width as usize * p.bpp,
                                p.width as usize * p.height as usize * p.bpp, 1, markers.as_mut_ptr(), markers.len(), per.as_mut_ptr(),
                                &mut found)
            };
            if rc == A3_ERR_CAPACITY && markers.len() < MAX_MARKERS_PER_FRAME {
                markers.resize(markers.len() * 4, A3Marker::default());
                continue;
            }
            break rc;
        };
        unsafe { a3_set_rectification(ctx.raw, std::ptr::null()) }; // the shared context goes back to the plain detect
        ctx.check(rc, "a3_detect_batch");
        let mut det = Detection { grey: None, candidates: vec![], homographies: vec![], markers: markers[..found].iter().map(marker_of).collect() };
        if populate {   // (the taps report the rectified view)
            fill_debug_outputs(&ctx, 0, rect.dst.image_width, rect.dst.image_height, self.config.homography_sample_size as u32, &mut det);
        }
        det
    }

    /// New (additive): `detect` on the image reduced by `factor` (2, 3 or 4; a3_set_reduction): threshold, contours and decode run on
    /// the box-filtered grey plane a3_reduce_frames makes of it, and `Marker.corners` are full-size pixels (f x + f / 2).  For markers
    /// that are large in the image.  The Python twin is `Detector(reduction=Reduction(factor))`; here `Detector` itself gains no field
    /// (the setting is handed to the shared context for this call only, under its lock, as `detect_rectified` hands over its own).
    pub fn detect_reduced(&self, image: DynamicImage, factor: u32) -> Detection {
        let populate = POPULATE.load(Ordering::Relaxed);
        let slot = slot_for(self);
        let mut ctx = slot.lock().unwrap();
        let images = std::slice::from_ref(&image);
        let p = pack(images, &mut ctx.staging);
        ctx.check(unsafe { a3_set_debug_taps(ctx.raw, populate as c_int) }, "a3_set_debug_taps");
        let red = A3Reduction { factor, reserved: [0; 3] };
        ctx.check(unsafe { a3_set_reduction(ctx.raw, &red) }, "a3_set_reduction");
        let mut markers = vec![A3Marker::default(); 64];
        let mut per = vec![0u32; 1];
        let mut found = 0usize;
        let rc = loop {
            let rc = unsafe {
                a3_detect_batch(ctx.raw, p.bytes as *const c_void, A3_MEM_HOST, p.fmt, p.width, p.height, p.width as usize * p.bpp,
                                p.width as usize * p.height as usize * p.bpp, 1, markers.as_mut_ptr(), markers.len(), per.as_mut_ptr(),
                                &mut found)
            };
            if rc == A3_ERR_CAPACITY && markers.len() < MAX_MARKERS_PER_FRAME {
                markers.resize(markers.len() * 4, A3Marker::default());
                continue;
            }
            break rc;
        };
        unsafe { a3_set_reduction(ctx.raw, std::ptr::null()) }; // the shared context goes back to the plain detect
        ctx.check(rc, "a3_detect_batch");
        let mut det = Detection { grey: None, candidates: vec![], homographies: vec![], markers: markers[..found].iter().map(marker_of).collect() };
        if populate {   // (the taps report the reduced view)
            fill_debug_outputs(&ctx, 0, p.width / factor, p.height / factor, self.config.homography_sample_size as u32, &mut det);
        }
        det
    }

    /// New (additive): `detect` with several adaptive-threshold windows (a3_set_threshold_windows; OpenCV's adaptiveThreshWinSizeMin /
    /// Max / Step): the image is binarised once per radius of `windows` (2 to 4 radii, strictly ascending, each in 1..31; one radius:
    /// that radius in `config.threshold_window`'s place), quads are found in every binary image and merged into one candidate list on
    /// the device, ahead of the decoder.  The Python twin is `Detector(threshold_windows=(3, 7, 15))`; here `Detector` itself gains no
    /// field (the setting is handed to the shared context for this call only, under its lock, as `detect_reduced` hands over its own).
    pub fn detect_windows(&self, image: DynamicImage, windows: &[u32]) -> Detection {
        let populate = POPULATE.load(Ordering::Relaxed);
        let slot = slot_for(self);
        let mut ctx = slot.lock().unwrap();
        let images = std::slice::from_ref(&image);
        let p = pack(images, &mut ctx.staging);
        ctx.check(unsafe { a3_set_debug_taps(ctx.raw, populate as c_int) }, "a3_set_debug_taps");
        ctx.check(unsafe { a3_set_threshold_windows(ctx.raw, windows.as_ptr(), windows.len()) }, "a3_set_threshold_windows");
        let mut markers = vec![A3Marker::default(); 64];
        let mut per = vec![0u32; 1];
        let mut found = 0usize;
        let rc = loop {
            let rc = unsafe {
                a3_detect_batch(ctx.raw, p.bytes as *const c_void, A3_MEM_HOST, p.fmt, p.width, p.height, p.width as usize * p.bpp,
                                p.width as usize * p.height as usize * p.bpp, 1, markers.as_mut_ptr(), markers.len(), per.as_mut_ptr(),
                                &mut found)
            };
            if rc == A3_ERR_CAPACITY && markers.len() < MAX_MARKERS_PER_FRAME {
                markers.resize(markers.len() * 4, A3Marker::default());
                continue;
            }
            break rc;
        };
        unsafe { a3_set_threshold_windows(ctx.raw, std::ptr::null(), 0) }; // the shared context goes back to the plain detect
        ctx.check(rc, "a3_detect_batch");
        let mut det = Detection { grey: None, candidates: vec![], homographies: vec![], markers: markers[..found].iter().map(marker_of).collect() };
        if populate {   // (the taps serve the merged lists)
            fill_debug_outputs(&ctx, 0, p.width, p.height, self.config.homography_sample_size as u32, &mut det);
        }
        det
    }

    /// New (additive): `detect` of one image plus the pose of a planar board (OpenCV's estimatePoseBoard), solved on the device
    /// from every board marker of the image.  `board_ids[k]` is a dictionary index and `board_corners[k]` its four corners in board
    /// units (z = 0, x right, y up, `Marker.corners` order: a square).  `marker_size_mm` sizes the per-marker poses the same call
    /// solves (not returned here).  Panics, like the other calls, on an invalid board.  `Detector` itself gains no field: the board is
    /// handed to the shared context for this call only, under its lock.
    pub fn detect_board_pose(&self, image: DynamicImage, board_ids: &[u32], board_corners: &[[(f32, f32); 4]], marker_size_mm: f32,
                             intrinsics: Option<&CameraIntrinsics>) -> (Detection, A3BoardPose) {
        assert_eq!(board_ids.len(), board_corners.len(), "one corner quad per board id");
        let slot = slot_for(self);
        let mut ctx = slot.lock().unwrap();
        let images = std::slice::from_ref(&image);
        let p = pack(images, &mut ctx.staging);
        ctx.check(unsafe { a3_set_debug_taps(ctx.raw, 0) }, "a3_set_debug_taps");
        let xy: Vec<f32> = board_corners.iter().flat_map(|q| q.iter().flat_map(|&(x, y)| [x, y])).collect();
        ctx.check(unsafe { a3_set_board(ctx.raw, board_ids.as_ptr(), xy.as_ptr(), board_ids.len()) }, "a3_set_board");
        let intr = intrinsics.map(to_a3_intrinsics);
        let intr_ptr = intr.as_ref().map_or(std::ptr::null(), |i| i as *const A3Intrinsics);
        let mut cap = 64usize;
        let mut markers = vec![A3Marker::default(); cap];
        let mut poses = vec![A3Pose::default(); 2 * cap];
        let mut per = vec![0u32; 1];
        let mut found = 0usize;
        let rc = loop {
            let rc = unsafe {
                a3_detect_batch_pose(ctx.raw, p.bytes as *const c_void, A3_MEM_HOST, p.fmt, p.width, p.height, p.width as usize * p.bpp,
                                     p.width as usize * p.height as usize * p.bpp, 1, marker_size_mm, intr_ptr, markers.as_mut_ptr(),
                                     poses.as_mut_ptr(), cap, per.as_mut_ptr(), &mut found)
            };
            if rc == A3_ERR_CAPACITY && cap < MAX_MARKERS_PER_FRAME {
                cap *= 4;
                markers.resize(cap, A3Marker::default());
                poses.resize(2 * cap, A3Pose::default());
                continue;
            }
            break rc;
        };
        let mut board = A3BoardPose::default();
        let mut n = 0usize;
        let rc2 = if rc == A3_OK { unsafe { a3_get_board_poses(ctx.raw, &mut board, 1, &mut n) } } else { rc };
        unsafe { a3_set_board(ctx.raw, std::ptr::null(), std::ptr::null(), 0) }; // the shared context goes back to no board
        ctx.check(rc, "a3_detect_batch_pose");
        ctx.check(rc2, "a3_get_board_poses");
        let det = Detection { grey: None, candidates: vec![], homographies: vec![], markers: markers[..found].iter().map(marker_of).collect() };
        (det, board)
    }

    /// src/aruco.rs:52-121, same signature.  One frame = a batch of one.
    pub fn detect(&self, image: DynamicImage) -> Detection {
        self.detect_batch(std::slice::from_ref(&image)).pop().unwrap()
    }

    /// New (additive): many independent frames per call, all of one size -- what the GPU wants.  Results are in frame order;
    /// each `Detection` is what `detect` would have returned for that frame.
    pub fn detect_batch(&self, images: &[DynamicImage]) -> Vec<Detection> {
        if images.is_empty() {
            return Vec::new();
        }
        let populate = POPULATE.load(Ordering::Relaxed);
        if populate && images.len() > MAX_TAPPED_FRAMES {
            return images.chunks(MAX_TAPPED_FRAMES).flat_map(|c| self.detect_batch(c)).collect();
        }
        let slot = slot_for(self);
        let mut ctx = slot.lock().unwrap();
        let p = pack(images, &mut ctx.staging);
        ctx.check(unsafe { a3_set_debug_taps(ctx.raw, populate as c_int) }, "a3_set_debug_taps");
        let n = images.len();
        let mut markers = vec![A3Marker::default(); 64 * n];
        let mut per = vec![0u32; n];
        let mut found = 0usize;
        loop {
            let rc = unsafe {
                a3_detect_batch(ctx.raw, p.bytes as *const c_void, A3_MEM_HOST, p.fmt, p.width, p.height,
                                p.width as usize * p.bpp, p.width as usize * p.height as usize * p.bpp, n as u32,
                                markers.as_mut_ptr(), markers.len(), per.as_mut_ptr(), &mut found)
            };
            // the reference has no marker limit: a list that does not fit is grown and the batch re-run
            if rc == A3_ERR_CAPACITY && markers.len() < MAX_MARKERS_PER_FRAME * n {
                markers.resize(markers.len() * 4, A3Marker::default());
                continue;
            }
            ctx.check(rc, "a3_detect_batch");
            break;
        }
        let mut out = Vec::with_capacity(n);
        let mut pos = 0usize;
        for f in 0..n {
            let cnt = per[f] as usize;
            let mut det = Detection { grey: None, candidates: vec![], homographies: vec![], markers: markers[pos..pos + cnt].iter().map(marker_of).collect() };
            pos += cnt;
            if populate {
                fill_debug_outputs(&ctx, f as u32, p.width, p.height, self.config.homography_sample_size as u32, &mut det);
            }
            out.push(det);
        }
        out
    }

    /// New (additive): `detect` of one frame handed over as raw bytes in any layout the library takes (`fmt`: an A3_FMT_*), for the
    /// layouts `DynamicImage` cannot hold -- A3_FMT_YUYV8 / A3_FMT_UYVY8 straight from a V4L2 buffer, A3_FMT_BGRA8, or the luma plane
    /// of an NV12 / I420 buffer as A3_FMT_L8.  `row_stride` in bytes, 0 = tightly packed; `bytes` must hold `height` such rows (the last
    /// one may end with its pixels).  The Detection is what `detect` returns for the frame's grey levels; `Detector` gains no field.
    pub fn detect_raw(&self, bytes: &[u8], fmt: c_int, width: u32, height: u32, row_stride: usize) -> Detection {
        let bpp: usize = match fmt {
            A3_FMT_RGB8 => 3,
            A3_FMT_RGBA8 | A3_FMT_BGRA8 => 4,
            A3_FMT_YUYV8 | A3_FMT_UYVY8 => 2,
            A3_FMT_L8 => 1,
            _ => panic!("aruco3_hip: detect_raw: unknown pixel format {}", fmt),
        };
        let row = if row_stride == 0 { width as usize * bpp } else { row_stride };
        assert!(row >= width as usize * bpp, "aruco3_hip: detect_raw: row_stride smaller than a row");
        let need = if height == 0 { 0 } else { row * (height as usize - 1) + width as usize * bpp };
        assert!(bytes.len() >= need, "aruco3_hip: detect_raw: {} bytes given, the frame spans {}", bytes.len(), need);
        let populate = POPULATE.load(Ordering::Relaxed);
        let slot = slot_for(self);
        let ctx = slot.lock().unwrap();
        ctx.check(unsafe { a3_set_debug_taps(ctx.raw, populate as c_int) }, "a3_set_debug_taps");
        let mut markers = vec![A3Marker::default(); 64];
        let mut per = vec![0u32; 1];
        let mut found = 0usize;
        loop {
            let rc = unsafe {
                a3_detect_batch(ctx.raw, bytes.as_ptr() as *const c_void, A3_MEM_HOST, fmt, width, height, row, row * height as usize, 1,
                                markers.as_mut_ptr(), markers.len(), per.as_mut_ptr(), &mut found)
            };
            if rc == A3_ERR_CAPACITY && markers.len() < MAX_MARKERS_PER_FRAME {
                markers.resize(markers.len() * 4, A3Marker::default());
                continue;
            }
            ctx.check(rc, "a3_detect_batch");
            break;
        }
        let mut det = Detection { grey: None, candidates: vec![], homographies: vec![], markers: markers[..found].iter().map(marker_of).collect() };
        if populate && width != 0 && height != 0 {
            fill_debug_outputs(&ctx, 0, width, height, self.config.homography_sample_size as u32, &mut det);
        }
        det
    }

    /// New (additive): detect + both IPPE poses of every marker in one device pass (callers always solve the pose right after
    /// detect: examples/webcam_kamera.rs:56-71).  `intrinsics == None`: `solve_with_undistorted_points` with the frame size.
    pub fn detect_batch_with_pose(&self, images: &[DynamicImage], marker_size_mm: f32, intrinsics: Option<&CameraIntrinsics>)
        -> Vec<(Detection, Vec<(MarkerPose, MarkerPose)>)> {
        if images.is_empty() {
            return Vec::new();
        }
        let slot = slot_for(self);
        let mut ctx = slot.lock().unwrap();
        let p = pack(images, &mut ctx.staging);
        ctx.check(unsafe { a3_set_debug_taps(ctx.raw, 0) }, "a3_set_debug_taps");
        let n = images.len();
        let mut cap = 64 * n;
        let mut markers = vec![A3Marker::default(); cap];
        let mut poses = vec![A3Pose::default(); 2 * cap];
        let mut per = vec![0u32; n];
        let mut found = 0usize;
        let intr = intrinsics.map(to_a3_intrinsics);
        let intr_ptr = intr.as_ref().map_or(std::ptr::null(), |i| i as *const A3Intrinsics);
        loop {
            let rc = unsafe {
                a3_detect_batch_pose(ctx.raw, p.bytes as *const c_void, A3_MEM_HOST, p.fmt, p.width, p.height,
                                     p.width as usize * p.bpp, p.width as usize * p.height as usize * p.bpp, n as u32, marker_size_mm,
                                     intr_ptr, markers.as_mut_ptr(), poses.as_mut_ptr(), cap, per.as_mut_ptr(), &mut found)
            };
            // the reference has no marker limit: lists that do not fit are grown and the batch re-run (as in detect_batch)
            if rc == A3_ERR_CAPACITY && cap < MAX_MARKERS_PER_FRAME * n {
                cap *= 4;
                markers.resize(cap, A3Marker::default());
                poses.resize(2 * cap, A3Pose::default());
                continue;
            }
            ctx.check(rc, "a3_detect_batch_pose");
            break;
        }
        let mut out = Vec::with_capacity(n);
        let mut pos = 0usize;
        for f in 0..n {
            let cnt = per[f] as usize;
            let det = Detection { grey: None, candidates: vec![], homographies: vec![], markers: markers[pos..pos + cnt].iter().map(marker_of).collect() };
            let pp = (pos..pos + cnt).map(|i| (to_marker_pose(&poses[2 * i]), to_marker_pose(&poses[2 * i + 1]))).collect();
            pos += cnt;
            out.push((det, pp));
        }
        out
    }
}

// =====================================================================================================
// 3b. BatchQueue: several batches in flight, stepped in bursts (include/aruco3_hip.h, a3_order_after)
// =====================================================================================================

/// New (additive).  A capture / processing loop that must keep the GPU fed keeps `depth` batches in flight: `submit` hands a
/// batch over and returns at once, `collect` waits for the OLDEST batch in flight and returns its detections (markers only:
/// `Detection.grey` / `.candidates` / `.homographies` stay empty).  Inside, `depth` contexts of their own (not the registry's) are
/// used in rotation, each on a stream of its own, with the burst gates the header describes: before each submit context k calls
/// `a3_order_after` for the contexts k+1 .. depth-1, so the threshold kernels of one rotation run back to back after the previous
/// rotation's chains have drained and the contour / decode chains of the rotation run together.  Measured with a batch of its own per
/// context (round 5) a free-running rotation -- the same calls without `a3_order_after` -- is as fast within
/// 2 %, and depth 3 or 4 within 1 % of each other; the gates are kept because they give a rotation a quiet threshold phase and a quiet
/// chain phase, which is what a caller wants who runs something else (a collective, a copy) beside the detector.  Results never depend
/// on any of it.
/// The burst stepping is what the library does with these calls by itself (include/aruco3_hip.h, a3_order_after: a context that
/// declared gates holds its chain back behind its threshold kernel, the rotation's last context releases them) -- this type calls
/// nothing outside the public header, and `last_stepping()` reports what the library did with the batch just collected.
/// With fewer hardware queues than streams the batches overlap less (header, "Hardware queues").
pub struct BatchQueue {
    ctxs: Vec<HipCtx>,
    frames_in: Vec<usize>, // frames of the batch in flight on each context
    shape_in: Vec<(c_int, u32, u32, usize)>, // (fmt, width, height, bytes per pixel) of that batch, for the re-run of a marker-dense one
    last_stepping: u32,
    head: usize,           // context of the oldest batch in flight
    in_flight: usize,
    submitted: usize,
}

impl BatchQueue {
    pub fn new(detector: &Detector, depth: usize) -> BatchQueue {
        assert!(depth >= 1 && depth <= 8, "aruco3_hip: BatchQueue depth must be in 1..=8");
        let device = DEVICE.load(Ordering::Relaxed);
        let cfg = to_a3_config(&detector.config);
        let ctxs: Vec<HipCtx> = (0..depth).map(|_| HipCtx::create(device, &cfg, &detector.dictionary)).collect();
        BatchQueue { frames_in: vec![0; depth], shape_in: vec![(0, 0, 0, 0); depth], last_stepping: 0, ctxs, head: 0, in_flight: 0, submitted: 0 }
    }

    /// batches in flight
    pub fn len(&self) -> usize {
        self.in_flight
    }
    pub fn is_full(&self) -> bool {
        self.in_flight == self.ctxs.len()
    }
    /// a3_stats.stepping of the batch `collect` returned last (A3_STEP_* in bits 0-7)
    pub fn last_stepping(&self) -> u32 {
        self.last_stepping
    }

    /// Enqueue one batch (all frames of one size).  Panics if `depth` batches are already in flight: collect first.
    pub fn submit(&mut self, images: &[DynamicImage]) {
        assert!(!self.is_full(), "aruco3_hip: BatchQueue is full: collect() the oldest batch first");
        assert!(!images.is_empty(), "aruco3_hip: empty batch");
        let depth = self.ctxs.len();
        let k = self.submitted % depth;
        for m in k + 1..depth {
            // burst gate: this batch's threshold kernel starts once the batches in flight on the later contexts (the previous
            // rotation's) have drained.  A scheduling hint: a3_order_after never changes a result.
            let (this, other) = (self.ctxs[k].raw, self.ctxs[m].raw);
            self.ctxs[k].check(unsafe { a3_order_after(this, other) }, "a3_order_after");
        }
        let ctx = &mut self.ctxs[k];
        let p = pack(images, &mut ctx.staging); // pinned staging owned by the context: stays untouched until collect
        ctx.check(unsafe { a3_set_debug_taps(ctx.raw, 0) }, "a3_set_debug_taps");
        let n = images.len();
        let rc = unsafe {
            a3_detect_batch_submit(ctx.raw, p.bytes as *const c_void, A3_MEM_HOST, p.fmt, p.width, p.height, p.width as usize * p.bpp,
                                   p.width as usize * p.height as usize * p.bpp, n as u32, MAX_MARKERS_PER_FRAME.min(64) * n)
        };
        ctx.check(rc, "a3_detect_batch_submit");
        self.frames_in[k] = n;
        self.shape_in[k] = (p.fmt, p.width, p.height, p.bpp);
        self.submitted += 1;
        self.in_flight += 1;
    }

    /// Wait for the oldest batch in flight; one `Detection` per frame, in frame order.
    pub fn collect(&mut self) -> Vec<Detection> {
        assert!(self.in_flight > 0, "aruco3_hip: BatchQueue::collect with nothing in flight");
        let k = self.head;
        let ctx = &self.ctxs[k];
        let n = self.frames_in[k];
        let mut markers = vec![A3Marker::default(); 64 * n];
        let mut per = vec![0u32; n];
        let mut found = 0usize;
        let mut rc = unsafe { a3_detect_batch_collect(ctx.raw, markers.as_mut_ptr(), markers.len(), per.as_mut_ptr(), &mut found) };
        // the batch has left the queue whatever collect said (the library keeps no batch in flight after a failed collect)
        self.head = (self.head + 1) % self.ctxs.len();
        self.in_flight -= 1;
        let mut stats = A3Stats::default();
        if unsafe { a3_get_stats(ctx.raw, &mut stats) } == A3_OK {
            self.last_stepping = stats.stepping;
        }
        // The reference's marker Vec is unbounded (src/aruco.rs:75-113).  A frame with more markers than the list submitted for is
        // A3_ERR_CAPACITY: the frames are still in the context's pinned staging, so the batch is run again synchronously with a
        // list that grows, exactly as Detector::detect_batch does.
        while rc == A3_ERR_CAPACITY && markers.len() < MAX_MARKERS_PER_FRAME * n {
            markers.resize(markers.len() * 4, A3Marker::default());
            let (fmt, width, height, bpp) = self.shape_in[k];
            rc = unsafe {
                a3_detect_batch(ctx.raw, ctx.staging.as_ptr() as *const c_void, A3_MEM_HOST, fmt, width, height, width as usize * bpp,
                                width as usize * height as usize * bpp, n as u32, markers.as_mut_ptr(), markers.len(), per.as_mut_ptr(), &mut found)
            };
        }
        ctx.check(rc, "a3_detect_batch_collect");
        let mut out = Vec::with_capacity(n);
        let mut pos = 0usize;
        for f in 0..n {
            let cnt = per[f] as usize;
            out.push(Detection { grey: None, candidates: vec![], homographies: vec![], markers: markers[pos..pos + cnt].iter().map(marker_of).collect() });
            pos += cnt;
        }
        out
    }
}

// =====================================================================================================
// 4. Pose: the bodies of src/pose.rs:52-81 + README.md:34's `estimate_pose`
// =====================================================================================================

fn to_a3_intrinsics(c: &CameraIntrinsics) -> A3Intrinsics {
    A3Intrinsics { image_width: c.image_width, image_height: c.image_height, focal_x: c.focal_x, focal_y: c.focal_y,
                   principal_x: c.principal_x, principal_y: c.principal_y }
}

fn to_marker_pose(p: &A3Pose) -> MarkerPose {
    let r = &p.rotation;
    MarkerPose {
        error: p.error,
        rotation: na::Matrix3::new(r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8]), // row-major, like Matrix3::new
        translation: na::Vector3::new(p.translation[0], p.translation[1], p.translation[2]),
    }
}

/// The pose solvers are free functions with no detector to hang a context on: they share one small context of their own
/// (default config, empty dictionary -- the pose kernel reads neither).
fn pose_slot() -> &'static Mutex<HipCtx> {
    static POSE: OnceLock<Mutex<HipCtx>> = OnceLock::new();
    POSE.get_or_init(|| {
        let mut cfg = A3Config { threshold_window: 0, contour_simplification_epsilon: 0.0, min_side_length_factor: 0.0,
                                 min_corner_separation_factor: 0.0, homography_sample_size: 0, filter_high_bit_errors: 0 };
        unsafe { a3_default_config(&mut cfg) };
        let mut raw: *mut A3Ctx = std::ptr::null_mut();
        let rc = unsafe { a3_create(DEVICE.load(Ordering::Relaxed), &cfg, std::ptr::null(), 0, 1, 1, &mut raw) };
        if rc != A3_OK {
            panic!("aruco3_hip: a3_create (pose context) failed ({}): {}", rc, last_error(std::ptr::null()));
        }
        Mutex::new(HipCtx { raw, staging: PinnedBytes::empty() })
    })
}

/// Drop-in bodies for `pub mod pose` (src/pose.rs:52-81): same names, same arguments, same return order (lower error first).
pub mod pose_hip {
    use super::*;

    pub fn solve_with_intrinsics(image_points: &Vec<(u32, u32)>, marker_size_mm: f32, camera_intrinsics: &CameraIntrinsics)
        -> (MarkerPose, MarkerPose) {
        solve_pixels(image_points, marker_size_mm, Some(camera_intrinsics), (camera_intrinsics.image_width, camera_intrinsics.image_height))
    }

    pub fn solve_with_undistorted_points(image_points: &Vec<(u32, u32)>, marker_size_mm: f32, image_size: (u32, u32))
        -> (MarkerPose, MarkerPose) {
        solve_pixels(image_points, marker_size_mm, None, image_size)
    }

    pub fn solve_with_normalized_points(normalized_image_points: &Vec<(f32, f32)>, marker_size_mm: f32) -> (MarkerPose, MarkerPose) {
        assert!(normalized_image_points.len() == 4, "aruco3_hip: a marker has 4 corners");
        let pts: Vec<f32> = normalized_image_points.iter().flat_map(|&(x, y)| [x, y]).collect();
        let mut out = [A3Pose::default(); 2];
        let ctx = pose_slot().lock().unwrap();
        ctx.check(unsafe { a3_estimate_pose_normalized(ctx.raw, pts.as_ptr(), 1, marker_size_mm, out.as_mut_ptr()) },
                  "a3_estimate_pose_normalized");
        (to_marker_pose(&out[0]), to_marker_pose(&out[1]))
    }

    fn solve_pixels(image_points: &Vec<(u32, u32)>, marker_size_mm: f32, intr: Option<&CameraIntrinsics>, image_size: (u32, u32))
        -> (MarkerPose, MarkerPose) {
        assert!(image_points.len() == 4, "aruco3_hip: a marker has 4 corners");
        let xy: Vec<u32> = image_points.iter().flat_map(|&(x, y)| [x, y]).collect();
        let a3i = intr.map(to_a3_intrinsics);
        let intr_ptr = a3i.as_ref().map_or(std::ptr::null(), |i| i as *const A3Intrinsics);
        let mut out = [A3Pose::default(); 2];
        let ctx = pose_slot().lock().unwrap();
        ctx.check(unsafe { a3_estimate_pose(ctx.raw, xy.as_ptr(), 1, marker_size_mm, intr_ptr, image_size.0, image_size.1, out.as_mut_ptr()) },
                  "a3_estimate_pose");
        (to_marker_pose(&out[0]), to_marker_pose(&out[1]))
    }
}

/// README.md:34 -- `estimate_pose((1920, 1080), &d.corners, MARKER_SIZE_IN_MM, None)`.  The README names it, the source
/// never defined it; re-export it from src/lib.rs next to `Detector`.
pub fn estimate_pose(image_size: (u32, u32), corners: &Vec<(u32, u32)>, marker_size_mm: f32, intrinsics: Option<&CameraIntrinsics>)
    -> (MarkerPose, MarkerPose) {
    match intrinsics {
        Some(i) => pose_hip::solve_with_intrinsics(corners, marker_size_mm, i),
        None => pose_hip::solve_with_undistorted_points(corners, marker_size_mm, image_size),
    }
}

/// `ARDictionary::find_nearest` for many codes at once on the device (src/dictionaries.rs:160-196); the single-code method of
/// the reference stays as it is (a 1023-entry scan is not worth a launch).
pub fn find_nearest_batch(d: &Detector, bits: &[u64]) -> Vec<(usize, u8)> {
    let slot = slot_for(d);
    let ctx = slot.lock().unwrap();
    let mut idx = vec![0u32; bits.len().max(1)];
    let mut dist = vec![0u8; bits.len().max(1)];
    ctx.check(unsafe { a3_find_nearest(ctx.raw, bits.as_ptr(), bits.len(), idx.as_mut_ptr(), dist.as_mut_ptr()) }, "a3_find_nearest");
    (0..bits.len()).map(|i| (idx[i] as usize, dist[i])).collect()
}

/// New (additive): one camera calibrated on the device from views of a planar target (`a3_calibrate_cameras`; not in the
/// reference).  `views[i]` holds (board (x, y), pixel (u, v)) pairs; `flags` are A3_CALIB_* (without A3_CALIB_USE_INTRINSIC_GUESS).
/// Returns the camera's record and one record per view; the intrinsics go to `estimate_pose`, the lens to `Distortion`.
pub fn calibrate_camera(d: &Detector, views: &[Vec<((f32, f32), (f32, f32))>], image_size: (u32, u32), flags: u32)
                        -> (A3CalibResult, Vec<A3CalibView>) {
    let slot = slot_for(d);
    let ctx = slot.lock().unwrap();
    let mut offsets = vec![0u32];
    let (mut obj, mut img) = (Vec::new(), Vec::new());
    for v in views {
        for &((x, y), (u, w)) in v {
            obj.extend_from_slice(&[x, y]);
            img.extend_from_slice(&[u, w]);
        }
        offsets.push((obj.len() / 2) as u32);
    }
    let guess = A3Intrinsics { image_width: 0, image_height: 0, focal_x: 0.0, focal_y: 0.0, principal_x: 0.0, principal_y: 0.0 };
    let cam = A3CalibCamera { image_width: image_size.0, image_height: image_size.1, first_view: 0, n_views: views.len() as u32,
                              flags: flags & !A3_CALIB_USE_INTRINSIC_GUESS, max_iterations: 0, guess, guess_distortion: A3Distortion::default() };
    let mut res: A3CalibResult = unsafe { std::mem::zeroed() };   // (plain numbers: all-zero is a valid record)
    let mut out = vec![A3CalibView::default(); views.len()];
    ctx.check(unsafe {
        a3_calibrate_cameras(ctx.raw, &cam, 1, offsets.as_ptr(), views.len(), obj.as_ptr(), img.as_ptr(), &mut res, out.as_mut_ptr())
    }, "a3_calibrate_cameras");
    (res, out)
}

/// New (additive): the extrinsics of one camera rig solved on the device (`a3_calibrate_rigs`; not in the reference).  `cameras[c]`
/// holds camera c's known intrinsics and lens (fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6, what `calibrate_camera` returns);
/// `observations[i]` is (camera, frame, (board (x, y), pixel (u, v)) pairs): what that camera saw at that instant.  `flags` is 0
/// here (the extrinsic guess and A3_RIG_FIX_EXTRINSICS go through the raw call).  Returns the rig's record, one record per camera
/// (rig -> camera; the rig frame is camera 0's) and one per frame (board -> rig).
pub fn calibrate_rig(d: &Detector, cameras: &[[f64; 12]], n_frames: u32, observations: &[(u32, u32, Vec<((f32, f32), (f32, f32))>)])
                     -> (A3RigResult, Vec<A3RigCameraResult>, Vec<A3RigFrame>) {
    let slot = slot_for(d);
    let ctx = slot.lock().unwrap();
    let (mut obj, mut img, mut obs) = (Vec::new(), Vec::new(), Vec::new());
    for (camera, frame, pts) in observations {
        obs.push(A3RigObservation { camera: *camera, frame: *frame, first_point: (obj.len() / 2) as u32, n_points: pts.len() as u32 });
        for &((x, y), (u, w)) in pts {
            obj.extend_from_slice(&[x, y]);
            img.extend_from_slice(&[u, w]);
        }
    }
    let eye = [1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0];
    let cams: Vec<A3RigCamera> = cameras.iter().map(|a| A3RigCamera { a: *a, guess_rotation: eye, guess_translation: [0.0; 3] }).collect();
    let rig = A3Rig { first_camera: 0, n_cameras: cams.len() as u32, first_frame: 0, n_frames, first_obs: 0, n_obs: obs.len() as u32,
                      flags: 0, max_iterations: 0 };
    let mut res = A3RigResult::default();
    let mut cres = vec![A3RigCameraResult::default(); cams.len()];
    let mut frames = vec![A3RigFrame::default(); n_frames as usize];
    ctx.check(unsafe {
        a3_calibrate_rigs(ctx.raw, &rig, 1, cams.as_ptr(), cams.len(), obs.as_ptr(), obs.len(), obj.as_ptr(), img.as_ptr(), &mut res,
                          cres.as_mut_ptr(), frames.as_mut_ptr(), std::ptr::null_mut())
    }, "a3_calibrate_rigs");
    (res, cres, frames)
}

/// New (additive): hand-eye calibration solved on the device (`a3_calibrate_hand_eyes`; not in the reference).  `camera` holds the
/// known intrinsics and lens (fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6); `frames[f]` is (M_f as (rotation, translation), (board (x, y),
/// pixel (u, v)) pairs), with M_f = (gripper -> base)^-1 for a camera on the flange and gripper -> base for a fixed camera looking at
/// a board on the flange.  `flags` is 0 here (guesses and A3_HANDEYE_FIX_X go through the raw call).  Returns the problem's record
/// (X = gripper -> camera / base -> camera, Y = board -> base / board -> gripper) and one record per frame.
pub fn calibrate_hand_eye(d: &Detector, camera: &[f64; 12], frames: &[(([f64; 9], [f64; 3]), Vec<((f32, f32), (f32, f32))>)])
                          -> (A3HandEyeResult, Vec<A3HandEyeFrameResult>) {
    let slot = slot_for(d);
    let ctx = slot.lock().unwrap();
    let (mut obj, mut img, mut recs) = (Vec::new(), Vec::new(), Vec::new());
    for ((rotation, translation), pts) in frames {
        recs.push(A3HandEyeFrame { rotation: *rotation, translation: *translation, first_point: (obj.len() / 2) as u32, n_points: pts.len() as u32 });
        for &((x, y), (u, w)) in pts {
            obj.extend_from_slice(&[x, y]);
            img.extend_from_slice(&[u, w]);
        }
    }
    let problem = A3HandEyeProblem { first_frame: 0, n_frames: recs.len() as u32, a: *camera, ..Default::default() };
    let mut res = A3HandEyeResult::default();
    let mut fres = vec![A3HandEyeFrameResult::default(); recs.len()];
    ctx.check(unsafe {
        a3_calibrate_hand_eyes(ctx.raw, &problem, 1, recs.as_ptr(), recs.len(), obj.as_ptr(), img.as_ptr(), &mut res, fres.as_mut_ptr())
    }, "a3_calibrate_hand_eyes");
    (res, fres)
}

/// per-batch stage counters of the detector's last call
pub fn last_stats(d: &Detector) -> A3Stats {
    let slot = slot_for(d);
    let ctx = slot.lock().unwrap();
    let mut s = A3Stats::default();
    ctx.check(unsafe { a3_get_stats(ctx.raw, &mut s) }, "a3_get_stats");
    s
}
