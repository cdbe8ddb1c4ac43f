// Argument checks of the reduction (a3_reduce_frames, a3_set_reduction): everything that stands between a caller's arguments and
// k_reduce_frames, which indexes the frames with its sizes.  Host arithmetic on the public header's records only -- no HIP, no context --
// so a plain C++ program can run every check (tests/reduce_checks.cpp).  Each function returns the message of the FIRST check that
// fails, or nullptr.  Every message is a whole string literal (as a3_rectify_check.h).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/aruco3_hip.h"
#include "a3_format.h"

namespace a3 {

// bytes per pixel of an A3_FMT_*, 0 for none (a3_format.h)
inline size_t reduce_bpp(int fmt) { return format_bpp(fmt); }

// the record of a3_set_reduction
inline const char* check_reduction(const a3_reduction& r) {
    if (r.factor < 2 || r.factor > 4) return "a3_set_reduction: factor must be 2, 3 or 4";
    if (r.reserved[0] || r.reserved[1] || r.reserved[2]) return "a3_set_reduction: a3_reduction.reserved must be 0";
    return nullptr;
}

// frames of width x height reduced by factor: the reduced size must be one a3_detect_batch takes as a frame size, and not empty
inline const char* check_reduced_size(bool detect, uint32_t width, uint32_t height, uint32_t factor) {
    const uint32_t w = width / factor, h = height / factor;
    if (w == 0 || h == 0)
        return detect ? "a3_detect_batch: with a reduction set the frames must hold at least one block (a3_set_reduction)"
                      : "a3_reduce_frames: a reduced width or height of 0";
    if (w > 65535 || h > 65535 || (uint64_t)w * h >= (1ull << 30))
        return detect ? "a3_detect_batch: reduced image dimensions above 65535 (or 2^30 pixels) are not supported"
                      : "a3_reduce_frames: a reduced size above 65535 or of 2^30 pixels and more";
    return nullptr;
}

// a3_reduce_frames, behind its null-pointer test; the strides are as the caller gave them (0 is no default here)
inline const char* check_reduce_frames(const void* src, int src_memory, int fmt, uint32_t width, uint32_t height, size_t src_row_stride,
                                       size_t src_frame_stride, uint32_t n_frames, uint32_t factor, const void* dst, int dst_memory,
                                       size_t dst_row_stride, size_t dst_frame_stride) {
    if (n_frames == 0 || n_frames > 65535) return "a3_reduce_frames: n_frames must be in 1..65535";
    const size_t bpp = reduce_bpp(fmt);
    if (bpp == 0) return "a3_reduce_frames: unknown pixel format";
    if (format_width_error(fmt, width)) return "a3_reduce_frames: 4:2:2 frames have an even width";
    if ((src_memory != A3_MEM_HOST && src_memory != A3_MEM_DEVICE) || (dst_memory != A3_MEM_HOST && dst_memory != A3_MEM_DEVICE))
        return "a3_reduce_frames: memory must be A3_MEM_HOST or A3_MEM_DEVICE";
    if (factor < 2 || factor > 4) return "a3_reduce_frames: factor must be 2, 3 or 4";
    if (const char* m = check_reduced_size(false, width, height, factor)) return m;
    const size_t w = width / factor, h = height / factor;
    if (src_row_stride / bpp < width || dst_row_stride < w) return "a3_reduce_frames: row stride smaller than a row";
    if (src_frame_stride / height < src_row_stride || dst_frame_stride / h < dst_row_stride) return "a3_reduce_frames: frame stride smaller than a frame";
    // the byte ranges the call reads and writes (the last frame and row end with their pixels)
    const uintptr_t s0 = reinterpret_cast<uintptr_t>(src), d0 = reinterpret_cast<uintptr_t>(dst);
    const uint64_t s_len = (uint64_t)src_frame_stride * (n_frames - 1) + (uint64_t)src_row_stride * (height - 1) + (uint64_t)width * bpp;
    const uint64_t d_len = (uint64_t)dst_frame_stride * (n_frames - 1) + (uint64_t)dst_row_stride * (h - 1) + w;
    if (s0 < d0 + d_len && d0 < s0 + s_len) return "a3_reduce_frames: src and dst overlap";
    return nullptr;
}

}  // namespace a3
