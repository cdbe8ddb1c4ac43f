// Argument checks of an a3_rectify, shared by a3_rectify_frames and a3_set_rectification: everything that stands between a caller's
// record and k_rectify, which indexes the frames with its sizes.  Host arithmetic on the public header's records only -- no HIP, no
// context -- so a plain C++ program can run every check (tests/rectify_checks.cpp).  check_rectify returns the message of the FIRST
// check that fails, or nullptr; the order of the checks and, for a3_rectify_frames, every message are what that entry point always
// gave.  The setter's messages are the same text behind its own name.  Every message is a whole string literal (as a3_solve_check.h).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/aruco3_hip.h"
#include "a3_format.h"

namespace a3 {

#define A3_RECT_MSG(tail) (setter ? "a3_set_rectification: " tail : "a3_rectify_frames: " tail)
#define A3_RECT_REC(tail) (setter ? "a3_set_rectification: " tail : tail)

// one image of the record (src or dst) with the strides its frames have; bpp: bytes per pixel
inline const char* check_rectify_image(bool setter, const a3_intrinsics& k, size_t bpp, size_t row_stride, size_t frame_stride) {
    if (k.image_width == 0 || k.image_height == 0 || k.image_width > 65535 || k.image_height > 65535 ||
        (uint64_t)k.image_width * k.image_height >= (1ull << 30))
        return A3_RECT_MSG("an image size of 0, above 65535 or of 2^30 pixels and more");
    if (row_stride < (size_t)k.image_width * bpp) return A3_RECT_MSG("row stride smaller than a row");
    if (frame_stride / k.image_height < row_stride) return A3_RECT_MSG("frame stride smaller than a frame");
    const float v[4] = {k.focal_x, k.focal_y, k.principal_x, k.principal_y};
    for (float x : v)
        if (!std::isfinite(x)) return A3_RECT_MSG("an intrinsic is not finite");
    if (!(k.focal_x > 0.0f) || !(k.focal_y > 0.0f)) return A3_RECT_MSG("focal lengths must be > 0");
    return nullptr;
}

// setter: a3_set_rectification, which has no frames yet -- it passes bpp 1 and tightly packed strides, so the stride checks cannot
// fail there; the detect call checks the strides of its own frames (stage_input)
// src_bpp / dst_bpp: bytes per pixel of the source frames and of what the call writes -- the same but for a packed 4:2:2 source, whose
// rectified frames are the luma view (a3_format.h: format_bpp, format_rectified_bpp)
inline const char* check_rectify_as(bool setter, const a3_rectify& r, size_t src_bpp, size_t dst_bpp, size_t src_row_stride, size_t src_frame_stride,
                                    size_t dst_row_stride, size_t dst_frame_stride) {
    if (const char* m = check_rectify_image(setter, r.src, src_bpp, src_row_stride, src_frame_stride)) return m;
    if (const char* m = check_rectify_image(setter, r.dst, dst_bpp, dst_row_stride, dst_frame_stride)) return m;
    if (r.reserved[0] || r.reserved[1] || r.reserved[2]) return A3_RECT_REC("a3_rectify.reserved must be 0");
    const a3_distortion& d = r.distortion;
    if (d.model != A3_DIST_NONE && d.model != A3_DIST_RATIONAL && d.model != A3_DIST_FISHEYE) return A3_RECT_REC("a3_rectify.distortion.model: unknown model");
    if (d.model != A3_DIST_NONE) {   // the coefficients of a model that has some: all finite, and the fisheye model reads k1 k2 k3 k4 only
        const float k[8] = {d.k1, d.k2, d.p1, d.p2, d.k3, d.k4, d.k5, d.k6};
        for (float v : k)
            if (!std::isfinite(v)) return A3_RECT_REC("a3_rectify.distortion: a coefficient is not finite");
        if (d.model == A3_DIST_FISHEYE && (d.p1 != 0.0f || d.p2 != 0.0f || d.k5 != 0.0f || d.k6 != 0.0f))
            return A3_RECT_REC("a3_rectify.distortion: model A3_DIST_FISHEYE reads k1 k2 k3 k4; p1 p2 k5 k6 must be 0");
    }
    for (float v : r.rotation)
        if (!std::isfinite(v)) return A3_RECT_REC("a3_rectify.rotation: an entry is not finite");
    return nullptr;
}
inline const char* check_rectify(bool setter, const a3_rectify& r, size_t bpp, size_t src_row_stride, size_t src_frame_stride, size_t dst_row_stride,
                                 size_t dst_frame_stride) {
    return check_rectify_as(setter, r, bpp, bpp, src_row_stride, src_frame_stride, dst_row_stride, dst_frame_stride);
}
// a3_rectify_frames on frames of format fmt (a valid one): the format's own rule first, then the record with the format's pixel sizes
inline const char* check_rectify_frames_fmt(const a3_rectify& r, int fmt, size_t src_row_stride, size_t src_frame_stride, size_t dst_row_stride,
                                            size_t dst_frame_stride) {
    if (format_width_error(fmt, r.src.image_width)) return "a3_rectify_frames: 4:2:2 frames have an even width";
    return check_rectify_as(false, r, format_bpp(fmt), format_rectified_bpp(fmt), src_row_stride, src_frame_stride, dst_row_stride, dst_frame_stride);
}

#undef A3_RECT_MSG
#undef A3_RECT_REC

}  // namespace a3
