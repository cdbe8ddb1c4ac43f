// Argument checks of the solver entry points (a3_calibrate_cameras, a3_calibrate_fisheye_cameras, a3_calibrate_rigs,
// a3_calibrate_hand_eyes, a3_build_marker_maps): all that stands between a caller's index arrays and the kernels that index with them.
// Host arithmetic on the public header's records only -- no HIP, no context -- so a plain C++ program can run every check
// (tests/solver_checks.cpp).  Each function returns the message of the FIRST check that fails, or nullptr, and fills what the staging
// needs; a range is bounded before anything is indexed with it.  `busy` (a submitted batch has not been collected) is the one check
// that needs the context: a3_api.hip evaluates it, and it is reported where it always was, behind the null checks.
// Every message is a whole string literal, so the library's read-only data holds each message as it reads: a shared helper returns a
// bool and its caller names the literal; the cameras' A3_MSG joins either entry point's name and the tail at compile time.
#pragma once
#include <algorithm>
#include <cmath>
#include <vector>

#include "../../include/aruco3_hip.h"

namespace a3 {

template <typename T> inline bool all_finite(const T* p, size_t n) {
    for (size_t i = 0; i < n; i++)
        if (!std::isfinite(p[i])) return false;
    return true;
}
template <typename T, size_t N> inline bool all_finite(const T (&a)[N]) { return all_finite(a, N); }

// the points [first, first + n) of the two point arrays, which the caller has bounded
inline bool points_finite(const float* object_xy, const float* image_xy, size_t first, size_t n) {
    return all_finite(object_xy + 2 * first, 2 * n) && all_finite(image_xy + 2 * first, 2 * n);
}

// claims [first, first + n) of an ownership map the caller has bounded the range by; false when another problem owns one of them
inline bool claim(std::vector<uint8_t>& owned, size_t first, size_t n = 1) {
    for (size_t i = first; i < first + n; i++) {
        if (owned[i]) return false;
        owned[i] = 1;
    }
    return true;
}

// both lens models: the fisheye model has one more flag and also checks the guess's coefficients it does not read
inline const char* check_cameras(bool fisheye, bool busy, const a3_calib_camera* cams, size_t n_cams, const uint32_t* view_offsets, size_t n_views,
                                 const float* object_xy, const float* image_xy, const a3_calib_result* results, size_t& n_pts) {
#define A3_MSG(tail) (fisheye ? "a3_calibrate_fisheye_cameras" tail : "a3_calibrate_cameras" tail)
    const uint32_t known_flags = fisheye ? 63u : 31u;
    const uint32_t guess_flag = fisheye ? (uint32_t)A3_FISHEYE_USE_INTRINSIC_GUESS : (uint32_t)A3_CALIB_USE_INTRINSIC_GUESS;
    if (!cams || !view_offsets || !results) return A3_MSG(": null argument");
    if (busy) return A3_MSG(": a submitted batch has not been collected");
    if (n_cams == 0 || n_cams > A3_CALIB_MAX_CAMERAS) return A3_MSG(": n_cams must be in 1..A3_CALIB_MAX_CAMERAS");
    if (n_views == 0 || n_views > A3_CALIB_MAX_CALL_VIEWS) return A3_MSG(": n_views must be in 1..A3_CALIB_MAX_CALL_VIEWS");
    if (view_offsets[0] != 0) return A3_MSG(": view_offsets[0] must be 0");
    for (size_t i = 0; i < n_views; i++) {
        if (view_offsets[i + 1] < view_offsets[i]) return A3_MSG(": view_offsets must not decrease");
        if (view_offsets[i + 1] - view_offsets[i] > A3_CALIB_MAX_POINTS) return A3_MSG(": a view has more than A3_CALIB_MAX_POINTS points");
    }
    n_pts = view_offsets[n_views];
    if (n_pts && (!object_xy || !image_xy)) return A3_MSG(": null point array");
    if (!points_finite(object_xy, image_xy, 0, n_pts)) return A3_MSG(": a point is not finite");
    std::vector<uint8_t> owned(n_views, 0);
    for (size_t c = 0; c < n_cams; c++) {
        const a3_calib_camera& cam = cams[c];
        if (cam.flags & ~known_flags) return A3_MSG(": unknown flags");
        if (cam.image_width == 0 || cam.image_height == 0 || cam.image_width > 65535 || cam.image_height > 65535)
            return A3_MSG(": image size must be in 1..65535");
        if (cam.max_iterations > A3_CALIB_MAX_ITERATIONS) return A3_MSG(": max_iterations above A3_CALIB_MAX_ITERATIONS");
        if (cam.n_views == 0 || cam.n_views > A3_CALIB_MAX_VIEWS) return A3_MSG(": a camera's n_views must be in 1..A3_CALIB_MAX_VIEWS");
        if ((uint64_t)cam.first_view + cam.n_views > n_views) return A3_MSG(": a camera's views lie past n_views");
        if (!claim(owned, cam.first_view, cam.n_views)) return A3_MSG(": two cameras share a view");
        if (cam.flags & guess_flag) {
            const a3_intrinsics& g = cam.guess;
            const a3_distortion& d = cam.guess_distortion;
            const float v[12] = {g.focal_x, g.focal_y, g.principal_x, g.principal_y, d.k1, d.k2, d.p1, d.p2, d.k3, d.k4, d.k5, d.k6};
            if (!all_finite(v)) return A3_MSG(": the guess is not finite");
            if (!(g.focal_x > 0.0f) || !(g.focal_y > 0.0f)) return A3_MSG(": the guess's focal lengths must be > 0");
            if (fisheye && (d.p1 != 0.0f || d.p2 != 0.0f || d.k5 != 0.0f || d.k6 != 0.0f))
                return A3_MSG(": the guess's lens reads k1 k2 k3 k4; p1, p2, k5 and k6 must be 0");
        }
    }
    return nullptr;
#undef A3_MSG
}

inline const char* check_rigs(bool busy, const a3_rig* rigs, size_t n_rigs, const a3_rig_camera* cameras, size_t n_cameras, const a3_rig_observation* obs,
                              size_t n_obs, const float* object_xy, const float* image_xy, const a3_rig_result* results,
                              const a3_rig_camera_result* camera_results, size_t& n_frames, size_t& n_pts) {
    if (!rigs || !cameras || !obs || !object_xy || !image_xy || !results || !camera_results) return "a3_calibrate_rigs: null argument";
    if (busy) return "a3_calibrate_rigs: a submitted batch has not been collected";
    if (n_rigs == 0 || n_rigs > A3_RIG_MAX_RIGS) return "a3_calibrate_rigs: n_rigs must be in 1..A3_RIG_MAX_RIGS";
    if (n_cameras == 0 || n_cameras > (size_t)A3_RIG_MAX_RIGS * A3_RIG_MAX_CAMERAS) return "a3_calibrate_rigs: n_cameras out of range";
    if (n_obs == 0 || n_obs > A3_RIG_MAX_CALL_OBSERVATIONS) return "a3_calibrate_rigs: n_obs must be in 1..A3_RIG_MAX_CALL_OBSERVATIONS";
    n_frames = n_pts = 0;
    for (size_t r = 0; r < n_rigs; r++) {
        const a3_rig& R = rigs[r];
        if (R.flags & ~3u) return "a3_calibrate_rigs: unknown flags";
        if (R.n_cameras < 2 || R.n_cameras > A3_RIG_MAX_CAMERAS) return "a3_calibrate_rigs: a rig's n_cameras must be in 2..A3_RIG_MAX_CAMERAS";
        if (R.max_iterations > A3_CALIB_MAX_ITERATIONS) return "a3_calibrate_rigs: max_iterations above A3_CALIB_MAX_ITERATIONS";
        if (R.n_frames == 0 || R.n_frames > A3_RIG_MAX_FRAMES) return "a3_calibrate_rigs: a rig's n_frames must be in 1..A3_RIG_MAX_FRAMES";
        if (R.n_obs == 0) return "a3_calibrate_rigs: a rig has no observations";
        if ((uint64_t)R.first_camera + R.n_cameras > n_cameras) return "a3_calibrate_rigs: a rig's cameras lie past n_cameras";
        if ((uint64_t)R.first_obs + R.n_obs > n_obs) return "a3_calibrate_rigs: a rig's observations lie past n_obs";
        if ((uint64_t)R.first_frame + R.n_frames > A3_RIG_MAX_CALL_FRAMES) return "a3_calibrate_rigs: a rig's frames lie past A3_RIG_MAX_CALL_FRAMES";
        n_frames = std::max(n_frames, (size_t)R.first_frame + R.n_frames);
    }
    std::vector<uint8_t> cam_owned(n_cameras, 0), frame_owned(n_frames, 0), obs_owned(n_obs, 0), seen(n_frames * A3_RIG_MAX_CAMERAS, 0);
    for (size_t r = 0; r < n_rigs; r++) {
        const a3_rig& R = rigs[r];
        for (size_t c = R.first_camera; c < (size_t)R.first_camera + R.n_cameras; c++) {
            if (!claim(cam_owned, c)) return "a3_calibrate_rigs: two rigs share a camera";
            if (!all_finite(cameras[c].a)) return "a3_calibrate_rigs: a camera's intrinsics are not finite";
            if (!(cameras[c].a[0] > 0.0) || !(cameras[c].a[1] > 0.0)) return "a3_calibrate_rigs: focal lengths must be > 0";
            if (R.flags && c > R.first_camera && (!all_finite(cameras[c].guess_rotation) || !all_finite(cameras[c].guess_translation)))
                return "a3_calibrate_rigs: the extrinsic guess is not finite";
        }
        if (!claim(frame_owned, R.first_frame, R.n_frames)) return "a3_calibrate_rigs: two rigs share a frame";
        for (size_t o = R.first_obs; o < (size_t)R.first_obs + R.n_obs; o++) {
            if (!claim(obs_owned, o)) return "a3_calibrate_rigs: two rigs share an observation";
            const a3_rig_observation& ob = obs[o];
            if (ob.camera < R.first_camera || ob.camera - R.first_camera >= R.n_cameras) return "a3_calibrate_rigs: an observation's camera lies outside its rig";
            if (ob.frame < R.first_frame || ob.frame - R.first_frame >= R.n_frames) return "a3_calibrate_rigs: an observation's frame lies outside its rig";
            if (ob.n_points > A3_CALIB_MAX_POINTS) return "a3_calibrate_rigs: an observation has more than A3_CALIB_MAX_POINTS points";
            if ((uint64_t)ob.first_point + ob.n_points > 0xffffffffull) return "a3_calibrate_rigs: an observation's points lie past 2^32";
            if (!claim(seen, (size_t)ob.frame * A3_RIG_MAX_CAMERAS + (ob.camera - R.first_camera))) return "a3_calibrate_rigs: two observations of one (camera, frame)";
            if (!points_finite(object_xy, image_xy, ob.first_point, ob.n_points)) return "a3_calibrate_rigs: a point is not finite";
            n_pts = std::max(n_pts, (size_t)ob.first_point + ob.n_points);
        }
    }
    return nullptr;
}

inline const char* check_hand_eyes(bool busy, const a3_handeye_problem* problems, size_t n_problems, const a3_handeye_frame* frames, size_t n_frames,
                                   const float* object_xy, const float* image_xy, const a3_handeye_result* results, size_t& n_pts) {
    if (!problems || !frames || !object_xy || !image_xy || !results) return "a3_calibrate_hand_eyes: null argument";
    if (busy) return "a3_calibrate_hand_eyes: a submitted batch has not been collected";
    if (n_problems == 0 || n_problems > A3_HANDEYE_MAX_PROBLEMS) return "a3_calibrate_hand_eyes: n_problems must be in 1..A3_HANDEYE_MAX_PROBLEMS";
    if (n_frames == 0 || n_frames > A3_HANDEYE_MAX_CALL_FRAMES) return "a3_calibrate_hand_eyes: n_frames must be in 1..A3_HANDEYE_MAX_CALL_FRAMES";
    std::vector<uint8_t> frame_owned(n_frames, 0);
    n_pts = 0;
    for (size_t r = 0; r < n_problems; r++) {
        const a3_handeye_problem& R = problems[r];
        if (R.flags & ~3u) return "a3_calibrate_hand_eyes: unknown flags";
        if (R.max_iterations > A3_CALIB_MAX_ITERATIONS) return "a3_calibrate_hand_eyes: max_iterations above A3_CALIB_MAX_ITERATIONS";
        if (R.n_frames == 0 || R.n_frames > A3_HANDEYE_MAX_FRAMES) return "a3_calibrate_hand_eyes: a problem's n_frames must be in 1..A3_HANDEYE_MAX_FRAMES";
        if ((uint64_t)R.first_frame + R.n_frames > n_frames) return "a3_calibrate_hand_eyes: a problem's frames lie past n_frames";
        if (!all_finite(R.a)) return "a3_calibrate_hand_eyes: the camera's intrinsics are not finite";
        if (!(R.a[0] > 0.0) || !(R.a[1] > 0.0)) return "a3_calibrate_hand_eyes: focal lengths must be > 0";
        if ((R.flags && (!all_finite(R.guess_x_rotation) || !all_finite(R.guess_x_translation))) ||
            ((R.flags & A3_HANDEYE_USE_GUESS) && (!all_finite(R.guess_y_rotation) || !all_finite(R.guess_y_translation))))
            return "a3_calibrate_hand_eyes: the guess is not finite";
        for (size_t f = R.first_frame; f < (size_t)R.first_frame + R.n_frames; f++) {
            if (!claim(frame_owned, f)) return "a3_calibrate_hand_eyes: two problems share a frame";
            const a3_handeye_frame& fr = frames[f];
            if (!all_finite(fr.rotation) || !all_finite(fr.translation)) return "a3_calibrate_hand_eyes: a frame's robot pose is not finite";
            if (fr.n_points > A3_CALIB_MAX_POINTS) return "a3_calibrate_hand_eyes: a frame has more than A3_CALIB_MAX_POINTS points";
            if ((uint64_t)fr.first_point + fr.n_points > 0xffffffffull) return "a3_calibrate_hand_eyes: a frame's points lie past 2^32";
            if (!points_finite(object_xy, image_xy, fr.first_point, fr.n_points)) return "a3_calibrate_hand_eyes: a point is not finite";
            n_pts = std::max(n_pts, (size_t)fr.first_point + fr.n_points);
        }
    }
    return nullptr;
}

// big_off[r]: where map r's reduced systems (two nmax x nmax, nmax = 6 (n_markers - 1), none with FIX_MAP) start; big_doubles: their sum
inline const char* check_marker_maps(bool busy, const a3_map* maps, size_t n_maps, const a3_map_marker* markers, size_t n_markers,
                                     const a3_map_observation* obs, size_t n_obs, const float* image_xy, const a3_map_result* results,
                                     const a3_map_marker_result* marker_results, size_t& n_frames, std::vector<uint64_t>& big_off,
                                     uint64_t& big_doubles) {
    if (!maps || !markers || !obs || !image_xy || !results || !marker_results) return "a3_build_marker_maps: null argument";
    if (busy) return "a3_build_marker_maps: a submitted batch has not been collected";
    if (n_maps == 0 || n_maps > A3_MAP_MAX_MAPS) return "a3_build_marker_maps: n_maps must be in 1..A3_MAP_MAX_MAPS";
    if (n_markers == 0 || n_markers > (size_t)A3_MAP_MAX_MAPS * A3_MAP_MAX_MARKERS) return "a3_build_marker_maps: n_markers out of range";
    if (n_obs == 0 || n_obs > A3_MAP_MAX_CALL_OBSERVATIONS) return "a3_build_marker_maps: n_obs must be in 1..A3_MAP_MAX_CALL_OBSERVATIONS";
    n_frames = 0;
    for (size_t r = 0; r < n_maps; r++) {
        const a3_map& R = maps[r];
        if (R.flags & ~3u) return "a3_build_marker_maps: unknown flags";
        if (R.n_markers < 1 || R.n_markers > A3_MAP_MAX_MARKERS) return "a3_build_marker_maps: a map's n_markers must be in 1..A3_MAP_MAX_MARKERS";
        if (R.max_iterations > A3_CALIB_MAX_ITERATIONS) return "a3_build_marker_maps: max_iterations above A3_CALIB_MAX_ITERATIONS";
        if (R.n_frames == 0 || R.n_frames > A3_MAP_MAX_FRAMES) return "a3_build_marker_maps: a map's n_frames must be in 1..A3_MAP_MAX_FRAMES";
        if (R.n_obs == 0) return "a3_build_marker_maps: a map has no observations";
        if ((uint64_t)R.first_marker + R.n_markers > n_markers) return "a3_build_marker_maps: a map's markers lie past n_markers";
        if ((uint64_t)R.first_obs + R.n_obs > n_obs) return "a3_build_marker_maps: a map's observations lie past n_obs";
        if ((uint64_t)R.first_frame + R.n_frames > A3_MAP_MAX_CALL_FRAMES) return "a3_build_marker_maps: a map's frames lie past A3_MAP_MAX_CALL_FRAMES";
        if (!all_finite(R.a)) return "a3_build_marker_maps: the camera's intrinsics are not finite";
        if (!(R.a[0] > 0.0) || !(R.a[1] > 0.0)) return "a3_build_marker_maps: focal lengths must be > 0";
        if (!std::isfinite(R.marker_length) || !(R.marker_length > 0.0f)) return "a3_build_marker_maps: marker_length must be finite and > 0";
        n_frames = std::max(n_frames, (size_t)R.first_frame + R.n_frames);
    }
    std::vector<uint8_t> marker_owned(n_markers, 0), frame_owned(n_frames, 0), obs_owned(n_obs, 0);
    big_off.assign(n_maps, 0);
    big_doubles = 0;
    for (size_t r = 0; r < n_maps; r++) {
        const a3_map& R = maps[r];
        for (size_t m = R.first_marker; m < (size_t)R.first_marker + R.n_markers; m++) {
            if (!claim(marker_owned, m)) return "a3_build_marker_maps: two maps share a marker";
            if (R.flags && m > R.first_marker && (!all_finite(markers[m].guess_rotation) || !all_finite(markers[m].guess_translation)))
                return "a3_build_marker_maps: the marker guess is not finite";
        }
        if (!claim(frame_owned, R.first_frame, R.n_frames)) return "a3_build_marker_maps: two maps share a frame";
        for (size_t o = R.first_obs; o < (size_t)R.first_obs + R.n_obs; o++) {
            if (!claim(obs_owned, o)) return "a3_build_marker_maps: two maps share an observation";
            const a3_map_observation& ob = obs[o];
            if (ob.marker < R.first_marker || ob.marker - R.first_marker >= R.n_markers) return "a3_build_marker_maps: an observation's marker lies outside its map";
            if (ob.frame < R.first_frame || ob.frame - R.first_frame >= R.n_frames) return "a3_build_marker_maps: an observation's frame lies outside its map";
            if (o > R.first_obs) {
                const a3_map_observation& pv = obs[o - 1];
                if (pv.frame == ob.frame && pv.marker == ob.marker) return "a3_build_marker_maps: two observations of one (marker, frame)";
                if (pv.frame > ob.frame || (pv.frame == ob.frame && pv.marker > ob.marker))
                    return "a3_build_marker_maps: a map's observations must be listed by frame, then by marker";
            }
            if (!all_finite(image_xy + 8 * o, 8)) return "a3_build_marker_maps: a corner is not finite";
        }
        const uint64_t nmax = (R.flags & A3_MAP_FIX_MAP) ? 0 : 6ull * (R.n_markers - 1);
        big_off[r] = big_doubles;
        big_doubles += 2 * nmax * nmax;
    }
    return nullptr;
}

}  // namespace a3
