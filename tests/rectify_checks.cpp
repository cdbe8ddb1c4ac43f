// The argument check of an a3_rectify (aruco3_amd/csrc/a3_rectify_check.h) on a valid record and on one mutation of it at a time, for
// both callers: a3_rectify_frames must give the messages it always gave, a3_set_rectification the same text behind its own name, and
// the first failing check decides.  Exits 0 and prints "ok: <n> checks" when every message is the expected one.
// tests/test_rectified_detection.py compiles this with the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstring>
#include <functional>
#include <limits>
#include <string>

#include "../aruco3_amd/csrc/a3_rectify_check.h"

namespace {

const float kNan = std::numeric_limits<float>::quiet_NaN(), kInf = std::numeric_limits<float>::infinity();
int g_checks = 0, g_failed = 0;

a3_rectify valid() {
    a3_rectify r{};
    r.src = a3_intrinsics{32, 16, 40.0f, 40.0f, 16.0f, 8.0f};
    r.dst = a3_intrinsics{24, 12, 30.0f, 30.0f, 12.0f, 6.0f};
    r.distortion.model = A3_DIST_RATIONAL;
    r.distortion.k1 = -0.2f;
    r.rotation[0] = r.rotation[4] = r.rotation[8] = 1.0f;
    return r;
}

struct Strides { size_t bpp = 3, src_row = 96, src_frame = 96 * 16, dst_row = 72, dst_frame = 72 * 12; };

// `frames_msg`: what a3_rectify_frames says (nullptr: accepted); `prefixed`: whether that text already starts with the entry point's
// name, which the setter replaces by its own -- else the setter puts its name in front
void expect(const char* name, const std::function<void(a3_rectify&, Strides&)>& mutate, const char* frames_msg, bool prefixed) {
    a3_rectify r = valid();
    Strides s;
    if (mutate) mutate(r, s);
    const char* got = a3::check_rectify(false, r, s.bpp, s.src_row, s.src_frame, s.dst_row, s.dst_frame);
    g_checks++;
    if ((got == nullptr) != (frames_msg == nullptr) || (got && std::strcmp(got, frames_msg) != 0)) {
        std::printf("FAILED a3_rectify_frames %s: got \"%s\", expected \"%s\"\n", name, got ? got : "OK", frames_msg ? frames_msg : "OK");
        g_failed++;
    }
    // the setter has no frames: bpp 1 and tightly packed strides, as a3_api.hip calls it
    const size_t sw = r.src.image_width, sh = r.src.image_height, dw = r.dst.image_width, dh = r.dst.image_height;
    const char* set = a3::check_rectify(true, r, 1, sw, sw * sh, dw, dw * dh);
    std::string want;
    const bool about_strides = frames_msg && std::strstr(frames_msg, "stride") != nullptr;
    if (frames_msg && !about_strides)
        want = std::string("a3_set_rectification: ") + (prefixed ? frames_msg + std::strlen("a3_rectify_frames: ") : frames_msg);
    g_checks++;
    if ((set == nullptr) != want.empty() || (set && want != set)) {
        std::printf("FAILED a3_set_rectification %s: got \"%s\", expected \"%s\"\n", name, set ? set : "OK", want.empty() ? "OK" : want.c_str());
        g_failed++;
    }
}

}  // namespace

int main() {
    using R = a3_rectify;
    using S = Strides;
    const char* SIZE = "a3_rectify_frames: an image size of 0, above 65535 or of 2^30 pixels and more";
    const char* ROW = "a3_rectify_frames: row stride smaller than a row";
    const char* FRAME = "a3_rectify_frames: frame stride smaller than a frame";
    const char* FINITE = "a3_rectify_frames: an intrinsic is not finite";
    const char* FOCAL = "a3_rectify_frames: focal lengths must be > 0";
    const char* COEFF = "a3_rectify.distortion: a coefficient is not finite";
    const char* FISHEYE = "a3_rectify.distortion: model A3_DIST_FISHEYE reads k1 k2 k3 k4; p1 p2 k5 k6 must be 0";
    expect("valid", nullptr, nullptr, false);
    for (int which = 0; which < 2; which++) {
        auto img = [which](R& r) -> a3_intrinsics& { return which ? r.dst : r.src; };
        auto big = [](S& s) { s.src_row = s.dst_row = (size_t)1 << 20; s.src_frame = s.dst_frame = (size_t)1 << 40; };
        expect("width_0", [&](R& r, S& s) { img(r).image_width = 0; big(s); }, SIZE, true);
        expect("height_0", [&](R& r, S& s) { img(r).image_height = 0; big(s); }, SIZE, true);
        expect("width_65536", [&](R& r, S& s) { img(r).image_width = 65536; big(s); }, SIZE, true);
        expect("height_65536", [&](R& r, S& s) { img(r).image_height = 65536; big(s); }, SIZE, true);
        expect("2^30_pixels", [&](R& r, S& s) { img(r).image_width = img(r).image_height = 32768; big(s); }, SIZE, true);
        expect("65535_x_16384", [&](R& r, S& s) { img(r).image_width = 65535; img(r).image_height = 16384; big(s); }, nullptr, false);
        expect("row_stride_short", [&](R&, S& s) { (which ? s.dst_row : s.src_row) -= 1; }, ROW, true);
        expect("frame_stride_short", [&](R&, S& s) { (which ? s.dst_frame : s.src_frame) -= 1; }, FRAME, true);
        expect("row_stride_padded", [&](R&, S& s) { (which ? s.dst_row : s.src_row) += 4; }, FRAME, true);   // (the frame no longer holds its rows)
        expect("focal_x_nan", [&](R& r, S&) { img(r).focal_x = kNan; }, FINITE, true);
        expect("focal_y_inf", [&](R& r, S&) { img(r).focal_y = kInf; }, FINITE, true);
        expect("principal_x_inf", [&](R& r, S&) { img(r).principal_x = -kInf; }, FINITE, true);
        expect("principal_y_nan", [&](R& r, S&) { img(r).principal_y = kNan; }, FINITE, true);
        expect("focal_x_0", [&](R& r, S&) { img(r).focal_x = 0.0f; }, FOCAL, true);
        expect("focal_y_negative", [&](R& r, S&) { img(r).focal_y = -40.0f; }, FOCAL, true);
    }
    expect("src_before_dst", [](R& r, S&) { r.src.focal_x = 0.0f; r.dst.image_width = 0; }, FOCAL, true);
    expect("image_before_reserved", [](R& r, S&) { r.dst.focal_y = kNan; r.reserved[0] = 1; }, FINITE, true);
    for (int k = 0; k < 3; k++) expect("reserved", [k](R& r, S&) { r.reserved[k] = 1; }, "a3_rectify.reserved must be 0", false);
    expect("model_2", [](R& r, S&) { r.distortion.model = 2; }, "a3_rectify.distortion.model: unknown model", false);
    expect("model_4", [](R& r, S&) { r.distortion.model = 4; }, "a3_rectify.distortion.model: unknown model", false);
    expect("reserved_before_model", [](R& r, S&) { r.distortion.model = 2; r.reserved[2] = 9; }, "a3_rectify.reserved must be 0", false);
    float a3_distortion::* const coeffs[8] = {&a3_distortion::k1, &a3_distortion::k2, &a3_distortion::p1, &a3_distortion::p2,
                                              &a3_distortion::k3, &a3_distortion::k4, &a3_distortion::k5, &a3_distortion::k6};
    for (auto c : coeffs) {
        expect("coefficient_nan", [c](R& r, S&) { r.distortion.*c = kNan; }, COEFF, false);
        expect("coefficient_inf_fisheye", [c](R& r, S&) { r.distortion.model = A3_DIST_FISHEYE; r.distortion.*c = kInf; }, COEFF, false);
        expect("coefficient_nan_not_read", [c](R& r, S&) { r.distortion.model = A3_DIST_NONE; r.distortion.*c = kNan; }, nullptr, false);
    }
    expect("fisheye", [](R& r, S&) { r.distortion.model = A3_DIST_FISHEYE; r.distortion.k3 = 0.01f; r.distortion.k4 = -0.002f; }, nullptr, false);
    expect("fisheye_p1", [](R& r, S&) { r.distortion.model = A3_DIST_FISHEYE; r.distortion.p1 = 1e-3f; }, FISHEYE, false);
    expect("fisheye_p2", [](R& r, S&) { r.distortion.model = A3_DIST_FISHEYE; r.distortion.p2 = 1e-3f; }, FISHEYE, false);
    expect("fisheye_k5", [](R& r, S&) { r.distortion.model = A3_DIST_FISHEYE; r.distortion.k5 = 1e-3f; }, FISHEYE, false);
    expect("fisheye_k6", [](R& r, S&) { r.distortion.model = A3_DIST_FISHEYE; r.distortion.k6 = 1e-3f; }, FISHEYE, false);
    expect("iterations_not_read", [](R& r, S&) { r.distortion.iterations = 0; r.distortion.max_residual_px = kNan; }, nullptr, false);
    for (int k = 0; k < 9; k++) expect("rotation_inf", [k](R& r, S&) { r.rotation[k] = kInf; }, "a3_rectify.rotation: an entry is not finite", false);
    expect("rotation_not_orthonormal", [](R& r, S&) { r.rotation[1] = 5.0f; }, nullptr, false);
    if (g_failed) return 1;
    std::printf("ok: %d checks\n", g_checks);
    return 0;
}
