// The argument checks of the solver entry points (aruco3_amd/csrc/a3_solve_check.h) on the smallest valid problem of each entry
// point and on one mutation of it at a time: prints "<entry point> <mutation>: <message>" per case, OK for a call that passes.
// tests/test_solver_checks.py compiles this with the address and undefined-behaviour sanitizers and compares every line.
#include <cmath>
#include <cstdio>
#include <functional>
#include <limits>

#include "../aruco3_amd/csrc/a3_solve_check.h"

namespace {

constexpr uint32_t kMax = 0xffffffffu;
const float kNanF = std::numeric_limits<float>::quiet_NaN();
const double kNan = std::numeric_limits<double>::quiet_NaN(), kInf = std::numeric_limits<double>::infinity();

void identity(double (&r)[9]) { r[0] = r[4] = r[8] = 1.0; }
void lens(double (&a)[12]) { a[0] = a[1] = 500.0; a[2] = 320.0; a[3] = 240.0; }

template <typename P> void run(const char* entry, const char* name, const std::function<void(P&)>& mutate = nullptr) {
    P p;
    if (mutate) mutate(p);
    const char* m = p.check();
    std::printf("%s %s: %s\n", entry, name, m ? m : "OK");
}

// 1 camera, 3 views of 4 points (a second camera record for the overlap)
struct Cameras {
    bool fisheye = false, busy = false;
    a3_calib_camera cams[2] = {};
    uint32_t off[4] = {0, 4, 8, 12};
    float obj[24] = {}, img[24] = {};
    a3_calib_result res[2];
    size_t n_cams = 1, n_views = 3;
    const a3_calib_camera* pc = cams;
    const uint32_t* po = off;
    const float *pobj = obj, *pimg = img;
    const a3_calib_result* pr = res;
    Cameras() {
        for (auto& c : cams) { c.image_width = 640; c.image_height = 480; c.n_views = 3; c.guess.focal_x = c.guess.focal_y = 500.0f; }
    }
    const char* check() {
        size_t n_pts = 0;
        return a3::check_cameras(fisheye, busy, pc, n_cams, po, n_views, pobj, pimg, pr, n_pts);
    }
};
struct Fisheye : Cameras { Fisheye() { fisheye = true; } };

template <typename P> void cameras(const char* e, uint32_t unknown_flag, uint32_t guess_flag) {
    using F = std::function<void(P&)>;
    run<P>(e, "valid");
    run<P>(e, "null_cams", F([](P& p) { p.pc = nullptr; }));
    run<P>(e, "null_offsets", F([](P& p) { p.po = nullptr; }));
    run<P>(e, "null_results", F([](P& p) { p.pr = nullptr; }));
    run<P>(e, "null_object", F([](P& p) { p.pobj = nullptr; }));
    run<P>(e, "null_image", F([](P& p) { p.pimg = nullptr; }));
    run<P>(e, "busy", F([](P& p) { p.busy = true; }));
    run<P>(e, "busy_null_results", F([](P& p) { p.busy = true; p.pr = nullptr; }));
    run<P>(e, "busy_n_cams_0", F([](P& p) { p.busy = true; p.n_cams = 0; }));
    run<P>(e, "n_cams_0", F([](P& p) { p.n_cams = 0; }));
    run<P>(e, "n_cams_1025", F([](P& p) { p.n_cams = 1025; }));
    run<P>(e, "n_views_0", F([](P& p) { p.n_views = 0; }));
    run<P>(e, "n_views_65537", F([](P& p) { p.n_views = 65537; }));
    run<P>(e, "offsets_0_not_0", F([](P& p) { p.off[0] = 1; }));
    run<P>(e, "offsets_decrease", F([](P& p) { p.off[2] = 3; }));
    run<P>(e, "view_4097_points", F([](P& p) { p.off[3] = 8 + 4097; p.pobj = p.pimg = nullptr; }));
    run<P>(e, "no_points_null_arrays", F([](P& p) { p.off[1] = p.off[2] = p.off[3] = 0; p.pobj = p.pimg = nullptr; }));
    run<P>(e, "nan_image_point", F([](P& p) { p.img[15] = kNanF; }));
    run<P>(e, "inf_object_point", F([](P& p) { p.obj[23] = std::numeric_limits<float>::infinity(); }));
    run<P>(e, "unknown_flag", F([=](P& p) { p.cams[0].flags = unknown_flag; }));
    run<P>(e, "unknown_flag_high", F([](P& p) { p.cams[0].flags = 128 | 1; }));
    run<P>(e, "image_width_0", F([](P& p) { p.cams[0].image_width = 0; }));
    run<P>(e, "image_height_70000", F([](P& p) { p.cams[0].image_height = 70000; }));
    run<P>(e, "max_iterations_1000", F([](P& p) { p.cams[0].max_iterations = 1000; }));
    run<P>(e, "max_iterations_1001", F([](P& p) { p.cams[0].max_iterations = 1001; }));
    run<P>(e, "camera_n_views_0", F([](P& p) { p.cams[0].n_views = 0; }));
    run<P>(e, "camera_n_views_4097", F([](P& p) { p.cams[0].n_views = 4097; }));
    run<P>(e, "camera_n_views_6", F([](P& p) { p.cams[0].n_views = 6; }));
    run<P>(e, "first_view_1", F([](P& p) { p.cams[0].first_view = 1; }));
    run<P>(e, "first_view_max_n_1", F([](P& p) { p.cams[0].first_view = kMax; p.cams[0].n_views = 1; }));
    run<P>(e, "first_view_max_n_max", F([](P& p) { p.cams[0].first_view = kMax; p.cams[0].n_views = kMax; }));
    run<P>(e, "two_cameras", F([](P& p) { p.n_cams = 2; p.cams[0].n_views = 2; p.cams[1].first_view = 2; p.cams[1].n_views = 1; }));
    run<P>(e, "overlap", F([](P& p) { p.n_cams = 2; p.cams[0].n_views = 2; p.cams[1].first_view = 1; p.cams[1].n_views = 2; }));
    run<P>(e, "view_not_owned", F([](P& p) { p.cams[0].n_views = 2; }));
    run<P>(e, "guess", F([=](P& p) { p.cams[0].flags = guess_flag; }));
    run<P>(e, "guess_focal_0", F([=](P& p) { p.cams[0].flags = guess_flag; p.cams[0].guess.focal_x = 0.0f; }));
    run<P>(e, "guess_nan_k3", F([=](P& p) { p.cams[0].flags = guess_flag; p.cams[0].guess_distortion.k3 = kNanF; }));
    run<P>(e, "guess_nan_k3_not_read", F([](P& p) { p.cams[0].guess_distortion.k3 = kNanF; p.cams[0].guess.focal_x = 0.0f; }));
    run<P>(e, "guess_p1", F([=](P& p) { p.cams[0].flags = guess_flag; p.cams[0].guess_distortion.p1 = 1e-3f; }));
    run<P>(e, "guess_p2", F([=](P& p) { p.cams[0].flags = guess_flag; p.cams[0].guess_distortion.p2 = 1e-3f; }));
    run<P>(e, "guess_k5", F([=](P& p) { p.cams[0].flags = guess_flag; p.cams[0].guess_distortion.k5 = 1e-3f; }));
    run<P>(e, "guess_k6", F([=](P& p) { p.cams[0].flags = guess_flag; p.cams[0].guess_distortion.k6 = 1e-3f; }));
    run<P>(e, "guess_p1_not_read", F([](P& p) { p.cams[0].guess_distortion.p1 = 1e-3f; }));
}

// 1 rig of 2 cameras, 2 frames, 4 observations of 4 points
struct Rigs {
    bool busy = false;
    a3_rig rigs[2] = {};
    a3_rig_camera cams[4] = {};
    a3_rig_observation obs[8] = {};
    float obj[32] = {}, img[32] = {};
    a3_rig_result res[2];
    a3_rig_camera_result cres[4];
    size_t n_rigs = 1, n_cameras = 2, n_obs = 4, n_frames = 0, n_pts = 0;
    const a3_rig* prigs = rigs;
    const a3_rig_camera* pcams = cams;
    const a3_rig_observation* pobs = obs;
    const float *pobj = obj, *pimg = img;
    const a3_rig_result* pres = res;
    const a3_rig_camera_result* pcres = cres;
    Rigs() {
        rigs[0] = {0, 2, 0, 2, 0, 4, 0, 0};
        rigs[1] = {2, 2, 2, 2, 4, 4, 0, 0};   // the same again, for the overlaps
        for (auto& c : cams) { lens(c.a); identity(c.guess_rotation); }
        for (uint32_t o = 0; o < 8; o++) obs[o] = {2 * (o / 4) + o % 2, 2 * (o / 4) + (o % 4) / 2, 4 * (o % 4), 4};
    }
    const char* check() { return a3::check_rigs(busy, prigs, n_rigs, pcams, n_cameras, pobs, n_obs, pobj, pimg, pres, pcres, n_frames, n_pts); }
};

void rigs() {
    using P = Rigs;
    using F = std::function<void(P&)>;
    const char* e = "a3_calibrate_rigs";
    const auto two = [](P& p) { p.n_rigs = 2; p.n_cameras = 4; p.n_obs = 8; };
    run<P>(e, "valid");
    run<P>(e, "two_rigs", F(two));
    run<P>(e, "null_rigs", F([](P& p) { p.prigs = nullptr; }));
    run<P>(e, "null_cams", F([](P& p) { p.pcams = nullptr; }));
    run<P>(e, "null_obs", F([](P& p) { p.pobs = nullptr; }));
    run<P>(e, "null_obj", F([](P& p) { p.pobj = nullptr; }));
    run<P>(e, "null_img", F([](P& p) { p.pimg = nullptr; }));
    run<P>(e, "null_res", F([](P& p) { p.pres = nullptr; }));
    run<P>(e, "null_cres", F([](P& p) { p.pcres = nullptr; }));
    run<P>(e, "busy", F([](P& p) { p.busy = true; }));
    run<P>(e, "busy_null_res", F([](P& p) { p.busy = true; p.pres = nullptr; }));
    run<P>(e, "busy_n_rigs_0", F([](P& p) { p.busy = true; p.n_rigs = 0; }));
    run<P>(e, "n_rigs_0", F([](P& p) { p.n_rigs = 0; }));
    run<P>(e, "n_rigs_1025", F([](P& p) { p.n_rigs = 1025; }));
    run<P>(e, "n_cameras_0", F([](P& p) { p.n_cameras = 0; }));
    run<P>(e, "n_cameras_8193", F([](P& p) { p.n_cameras = 8193; }));
    run<P>(e, "n_obs_0", F([](P& p) { p.n_obs = 0; }));
    run<P>(e, "n_obs_262145", F([](P& p) { p.n_obs = 262145; }));
    run<P>(e, "flags_4", F([](P& p) { p.rigs[0].flags = 4; }));
    run<P>(e, "rig_n_cameras_1", F([](P& p) { p.rigs[0].n_cameras = 1; }));
    run<P>(e, "rig_n_cameras_9", F([](P& p) { p.rigs[0].n_cameras = 9; }));
    run<P>(e, "max_iterations_1001", F([](P& p) { p.rigs[0].max_iterations = 1001; }));
    run<P>(e, "rig_n_frames_0", F([](P& p) { p.rigs[0].n_frames = 0; }));
    run<P>(e, "rig_n_frames_4097", F([](P& p) { p.rigs[0].n_frames = 4097; }));
    run<P>(e, "rig_n_obs_0", F([](P& p) { p.rigs[0].n_obs = 0; }));
    run<P>(e, "rig_n_obs_7", F([](P& p) { p.rigs[0].n_obs = 7; }));
    run<P>(e, "first_camera_1", F([](P& p) { p.rigs[0].first_camera = 1; }));
    run<P>(e, "first_camera_max_n_2", F([](P& p) { p.rigs[0].first_camera = kMax; }));
    run<P>(e, "first_camera_max_n_max", F([](P& p) { p.rigs[0].first_camera = kMax; p.rigs[0].n_cameras = kMax; }));
    run<P>(e, "first_frame_65535", F([](P& p) { p.rigs[0].first_frame = 65535; }));
    run<P>(e, "first_frame_max_n_1", F([](P& p) { p.rigs[0].first_frame = kMax; p.rigs[0].n_frames = 1; }));
    run<P>(e, "first_frame_max_n_max", F([](P& p) { p.rigs[0].first_frame = kMax; p.rigs[0].n_frames = kMax; }));
    run<P>(e, "first_obs_max_n_1", F([](P& p) { p.rigs[0].first_obs = kMax; p.rigs[0].n_obs = 1; }));
    run<P>(e, "first_obs_max_n_max", F([](P& p) { p.rigs[0].first_obs = kMax; p.rigs[0].n_obs = kMax; }));
    run<P>(e, "share_camera", F([=](P& p) { two(p); p.rigs[1].first_camera = 1; }));
    run<P>(e, "share_frame", F([=](P& p) { two(p); p.rigs[1].first_frame = 1; }));
    run<P>(e, "share_obs", F([=](P& p) { two(p); p.rigs[1].first_obs = 3; }));
    run<P>(e, "obs_camera_2", F([](P& p) { p.obs[0].camera = 2; }));
    run<P>(e, "obs_camera_max", F([](P& p) { p.obs[0].camera = kMax; }));
    run<P>(e, "obs_frame_3", F([](P& p) { p.obs[0].frame = 3; }));
    run<P>(e, "obs_frame_max", F([](P& p) { p.obs[0].frame = kMax; }));
    run<P>(e, "obs_camera_below_rig", F([=](P& p) { two(p); p.obs[4].camera = 1; }));
    run<P>(e, "obs_n_points_4097", F([](P& p) { p.obs[0].n_points = 4097; }));
    run<P>(e, "obs_first_point_max", F([](P& p) { p.obs[0].first_point = kMax; }));
    run<P>(e, "duplicate", F([](P& p) { p.obs[1].camera = p.obs[0].camera; p.obs[1].frame = p.obs[0].frame; }));
    run<P>(e, "focal_0", F([](P& p) { p.cams[1].a[0] = 0.0; }));
    run<P>(e, "nan_lens", F([](P& p) { p.cams[0].a[5] = kNan; }));
    run<P>(e, "nan_point", F([](P& p) { p.img[15] = kNanF; }));
    run<P>(e, "inf_guess_use", F([](P& p) { p.rigs[0].flags = A3_RIG_USE_EXTRINSIC_GUESS; p.cams[1].guess_translation[2] = kInf; }));
    run<P>(e, "inf_guess_fix", F([](P& p) { p.rigs[0].flags = A3_RIG_FIX_EXTRINSICS; p.cams[1].guess_translation[2] = kInf; }));
    run<P>(e, "inf_guess_not_read", F([](P& p) { p.cams[1].guess_translation[2] = kInf; }));
    run<P>(e, "inf_guess_first_camera", F([](P& p) { p.rigs[0].flags = A3_RIG_USE_EXTRINSIC_GUESS; p.cams[0].guess_rotation[0] = kInf; }));
}

// 1 problem of 3 frames of 4 points (a second problem for the overlap)
struct HandEyes {
    bool busy = false;
    a3_handeye_problem probs[2] = {};
    a3_handeye_frame frames[6] = {};
    float obj[48] = {}, img[48] = {};
    a3_handeye_result res[2];
    size_t n_problems = 1, n_frames = 3, n_pts = 0;
    const a3_handeye_problem* pprobs = probs;
    const a3_handeye_frame* pframes = frames;
    const float *pobj = obj, *pimg = img;
    const a3_handeye_result* pres = res;
    HandEyes() {
        for (uint32_t r = 0; r < 2; r++) {
            probs[r].first_frame = 3 * r;
            probs[r].n_frames = 3;
            lens(probs[r].a);
            identity(probs[r].guess_x_rotation);
            identity(probs[r].guess_y_rotation);
        }
        for (uint32_t f = 0; f < 6; f++) { identity(frames[f].rotation); frames[f].first_point = 4 * f; frames[f].n_points = 4; }
    }
    const char* check() { return a3::check_hand_eyes(busy, pprobs, n_problems, pframes, n_frames, pobj, pimg, pres, n_pts); }
};

void hand_eyes() {
    using P = HandEyes;
    using F = std::function<void(P&)>;
    const char* e = "a3_calibrate_hand_eyes";
    const auto two = [](P& p) { p.n_problems = 2; p.n_frames = 6; };
    run<P>(e, "valid");
    run<P>(e, "two_problems", F(two));
    run<P>(e, "null_probs", F([](P& p) { p.pprobs = nullptr; }));
    run<P>(e, "null_frames", F([](P& p) { p.pframes = nullptr; }));
    run<P>(e, "null_obj", F([](P& p) { p.pobj = nullptr; }));
    run<P>(e, "null_img", F([](P& p) { p.pimg = nullptr; }));
    run<P>(e, "null_res", F([](P& p) { p.pres = nullptr; }));
    run<P>(e, "busy", F([](P& p) { p.busy = true; }));
    run<P>(e, "busy_null_res", F([](P& p) { p.busy = true; p.pres = nullptr; }));
    run<P>(e, "busy_n_problems_0", F([](P& p) { p.busy = true; p.n_problems = 0; }));
    run<P>(e, "n_problems_0", F([](P& p) { p.n_problems = 0; }));
    run<P>(e, "n_problems_1025", F([](P& p) { p.n_problems = 1025; }));
    run<P>(e, "n_frames_0", F([](P& p) { p.n_frames = 0; }));
    run<P>(e, "n_frames_65537", F([](P& p) { p.n_frames = 65537; }));
    run<P>(e, "n_frames_2", F([](P& p) { p.n_frames = 2; }));
    run<P>(e, "flags_4", F([](P& p) { p.probs[0].flags = 4; }));
    run<P>(e, "max_iterations_1001", F([](P& p) { p.probs[0].max_iterations = 1001; }));
    run<P>(e, "problem_n_frames_0", F([](P& p) { p.probs[0].n_frames = 0; }));
    run<P>(e, "problem_n_frames_257", F([](P& p) { p.probs[0].n_frames = 257; }));
    run<P>(e, "problem_n_frames_2", F([](P& p) { p.probs[0].n_frames = 2; }));
    run<P>(e, "first_frame_1", F([](P& p) { p.probs[0].first_frame = 1; }));
    run<P>(e, "first_frame_max_n_1", F([](P& p) { p.probs[0].first_frame = kMax; p.probs[0].n_frames = 1; }));
    run<P>(e, "first_frame_max_n_max", F([](P& p) { p.probs[0].first_frame = kMax; p.probs[0].n_frames = kMax; }));
    run<P>(e, "share_frame", F([=](P& p) { two(p); p.probs[1].first_frame = 2; }));
    run<P>(e, "frame_n_points_4097", F([](P& p) { p.frames[0].n_points = 4097; }));
    run<P>(e, "frame_first_point_max", F([](P& p) { p.frames[0].first_point = kMax; }));
    run<P>(e, "focal_0", F([](P& p) { p.probs[0].a[1] = 0.0; }));
    run<P>(e, "nan_lens", F([](P& p) { p.probs[0].a[5] = kNan; }));
    run<P>(e, "nan_point", F([](P& p) { p.img[15] = kNanF; }));
    run<P>(e, "nan_robot", F([](P& p) { p.frames[1].rotation[4] = kNan; }));
    run<P>(e, "inf_robot", F([](P& p) { p.frames[2].translation[0] = kInf; }));
    run<P>(e, "skewed_robot", F([](P& p) { p.frames[0].rotation[1] += 0.01; }));
    run<P>(e, "inf_guess_x_use", F([](P& p) { p.probs[0].flags = A3_HANDEYE_USE_GUESS; p.probs[0].guess_x_translation[2] = kInf; }));
    run<P>(e, "inf_guess_x_fix", F([](P& p) { p.probs[0].flags = A3_HANDEYE_FIX_X; p.probs[0].guess_x_translation[2] = kInf; }));
    run<P>(e, "inf_guess_x_not_read", F([](P& p) { p.probs[0].guess_x_translation[2] = kInf; }));
    run<P>(e, "inf_guess_y_use", F([](P& p) { p.probs[0].flags = A3_HANDEYE_USE_GUESS; p.probs[0].guess_y_rotation[0] = kInf; }));
    run<P>(e, "inf_guess_y_fix_x_alone", F([](P& p) { p.probs[0].flags = A3_HANDEYE_FIX_X; p.probs[0].guess_y_rotation[0] = kInf; }));
}

// 1 map of 2 markers, 2 frames, 4 observations (a second map for the overlaps)
struct Maps {
    bool busy = false;
    a3_map maps[2] = {};
    a3_map_marker markers[4] = {};
    a3_map_observation obs[8] = {};
    float img[64] = {};
    a3_map_result res[2];
    a3_map_marker_result mres[4];
    size_t n_maps = 1, n_markers = 2, n_obs = 4, n_frames = 0;
    std::vector<uint64_t> big_off;
    uint64_t big_doubles = 0;
    const a3_map* pmaps = maps;
    const a3_map_marker* pmarkers = markers;
    const a3_map_observation* pobs = obs;
    const float* pimg = img;
    const a3_map_result* pres = res;
    const a3_map_marker_result* pmres = mres;
    Maps() {
        for (uint32_t r = 0; r < 2; r++) {
            a3_map& m = maps[r];
            m.first_marker = m.first_frame = 2 * r;
            m.n_markers = m.n_frames = 2;
            m.first_obs = 4 * r;
            m.n_obs = 4;
            lens(m.a);
            m.marker_length = 0.1f;
        }
        for (auto& m : markers) identity(m.guess_rotation);
        for (uint32_t o = 0; o < 8; o++) obs[o] = {2 * (o / 4) + o % 2, 2 * (o / 4) + (o % 4) / 2};   // by frame, then by marker
    }
    const char* check() {
        return a3::check_marker_maps(busy, pmaps, n_maps, pmarkers, n_markers, pobs, n_obs, pimg, pres, pmres, n_frames, big_off, big_doubles);
    }
};

void marker_maps() {
    using P = Maps;
    using F = std::function<void(P&)>;
    const char* e = "a3_build_marker_maps";
    const auto two = [](P& p) { p.n_maps = 2; p.n_markers = 4; p.n_obs = 8; };
    run<P>(e, "valid");
    run<P>(e, "two_maps", F(two));
    run<P>(e, "null_maps", F([](P& p) { p.pmaps = nullptr; }));
    run<P>(e, "null_markers", F([](P& p) { p.pmarkers = nullptr; }));
    run<P>(e, "null_obs", F([](P& p) { p.pobs = nullptr; }));
    run<P>(e, "null_img", F([](P& p) { p.pimg = nullptr; }));
    run<P>(e, "null_res", F([](P& p) { p.pres = nullptr; }));
    run<P>(e, "null_mres", F([](P& p) { p.pmres = nullptr; }));
    run<P>(e, "busy", F([](P& p) { p.busy = true; }));
    run<P>(e, "busy_null_res", F([](P& p) { p.busy = true; p.pres = nullptr; }));
    run<P>(e, "busy_n_maps_0", F([](P& p) { p.busy = true; p.n_maps = 0; }));
    run<P>(e, "n_maps_0", F([](P& p) { p.n_maps = 0; }));
    run<P>(e, "n_maps_1025", F([](P& p) { p.n_maps = 1025; }));
    run<P>(e, "n_markers_0", F([](P& p) { p.n_markers = 0; }));
    run<P>(e, "n_markers_131073", F([](P& p) { p.n_markers = 131073; }));
    run<P>(e, "n_obs_0", F([](P& p) { p.n_obs = 0; }));
    run<P>(e, "n_obs_262145", F([](P& p) { p.n_obs = 262145; }));
    run<P>(e, "flags_4", F([](P& p) { p.maps[0].flags = 4; }));
    run<P>(e, "map_n_markers_0", F([](P& p) { p.maps[0].n_markers = 0; }));
    run<P>(e, "map_n_markers_129", F([](P& p) { p.maps[0].n_markers = 129; }));
    run<P>(e, "max_iterations_1001", F([](P& p) { p.maps[0].max_iterations = 1001; }));
    run<P>(e, "map_n_frames_0", F([](P& p) { p.maps[0].n_frames = 0; }));
    run<P>(e, "map_n_frames_4097", F([](P& p) { p.maps[0].n_frames = 4097; }));
    run<P>(e, "map_n_obs_0", F([](P& p) { p.maps[0].n_obs = 0; }));
    run<P>(e, "map_n_obs_7", F([](P& p) { p.maps[0].n_obs = 7; }));
    run<P>(e, "first_marker_1", F([](P& p) { p.maps[0].first_marker = 1; }));
    run<P>(e, "first_marker_max_n_1", F([](P& p) { p.maps[0].first_marker = kMax; p.maps[0].n_markers = 1; }));
    run<P>(e, "first_marker_max_n_max", F([](P& p) { p.maps[0].first_marker = kMax; p.maps[0].n_markers = kMax; }));
    run<P>(e, "first_frame_65535", F([](P& p) { p.maps[0].first_frame = 65535; }));
    run<P>(e, "first_frame_max_n_1", F([](P& p) { p.maps[0].first_frame = kMax; p.maps[0].n_frames = 1; }));
    run<P>(e, "first_frame_max_n_max", F([](P& p) { p.maps[0].first_frame = kMax; p.maps[0].n_frames = kMax; }));
    run<P>(e, "first_obs_max_n_1", F([](P& p) { p.maps[0].first_obs = kMax; p.maps[0].n_obs = 1; }));
    run<P>(e, "first_obs_max_n_max", F([](P& p) { p.maps[0].first_obs = kMax; p.maps[0].n_obs = kMax; }));
    run<P>(e, "marker_length_0", F([](P& p) { p.maps[0].marker_length = 0.0f; }));
    run<P>(e, "marker_length_nan", F([](P& p) { p.maps[0].marker_length = kNanF; }));
    run<P>(e, "focal_0", F([](P& p) { p.maps[0].a[0] = 0.0; }));
    run<P>(e, "nan_lens", F([](P& p) { p.maps[0].a[5] = kNan; }));
    run<P>(e, "share_marker", F([=](P& p) { two(p); p.maps[1].first_marker = 1; }));
    run<P>(e, "share_frame", F([=](P& p) { two(p); p.maps[1].first_frame = 1; }));
    run<P>(e, "share_obs", F([=](P& p) { two(p); p.maps[1].first_obs = 3; }));
    run<P>(e, "obs_marker_2", F([](P& p) { p.obs[0].marker = 2; }));
    run<P>(e, "obs_marker_max", F([](P& p) { p.obs[0].marker = kMax; }));
    run<P>(e, "obs_frame_3", F([](P& p) { p.obs[0].frame = 3; }));
    run<P>(e, "obs_frame_max", F([](P& p) { p.obs[0].frame = kMax; }));
    run<P>(e, "duplicate", F([](P& p) { p.obs[1] = p.obs[0]; }));
    run<P>(e, "out_of_order", F([](P& p) { std::swap(p.obs[0].frame, p.obs[2].frame); }));
    run<P>(e, "markers_out_of_order", F([](P& p) { std::swap(p.obs[0].marker, p.obs[1].marker); }));
    run<P>(e, "nan_corner", F([](P& p) { p.img[7] = kNanF; }));
    run<P>(e, "inf_guess_use", F([](P& p) { p.maps[0].flags = A3_MAP_USE_GUESS; p.markers[1].guess_translation[2] = kInf; }));
    run<P>(e, "inf_guess_fix", F([](P& p) { p.maps[0].flags = A3_MAP_FIX_MAP; p.markers[1].guess_translation[2] = kInf; }));
    run<P>(e, "inf_guess_not_read", F([](P& p) { p.markers[1].guess_translation[2] = kInf; }));
    run<P>(e, "inf_guess_first_marker", F([](P& p) { p.maps[0].flags = A3_MAP_USE_GUESS; p.markers[0].guess_rotation[0] = kInf; }));
}

// what the staging reads from a valid call
void outputs() {
    Rigs r;
    r.n_rigs = 2; r.n_cameras = 4; r.n_obs = 8;
    r.check();
    std::printf("outputs rigs: n_frames %zu n_pts %zu\n", r.n_frames, r.n_pts);
    HandEyes h;
    h.check();
    std::printf("outputs hand_eyes: n_pts %zu\n", h.n_pts);
    Maps m;
    m.n_maps = 2; m.n_markers = 4; m.n_obs = 8;
    m.maps[1].flags = A3_MAP_FIX_MAP | A3_MAP_USE_GUESS;
    m.check();
    std::printf("outputs maps: n_frames %zu big_off %llu %llu big_doubles %llu\n", m.n_frames, (unsigned long long)m.big_off[0],
                (unsigned long long)m.big_off[1], (unsigned long long)m.big_doubles);
}

}  // namespace

int main() {
    cameras<Cameras>("a3_calibrate_cameras", 32, A3_CALIB_USE_INTRINSIC_GUESS);
    cameras<Fisheye>("a3_calibrate_fisheye_cameras", 64, A3_FISHEYE_USE_INTRINSIC_GUESS);
    rigs();
    hand_eyes();
    marker_maps();
    outputs();
    return 0;
}
