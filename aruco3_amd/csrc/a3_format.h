// The one description of a pixel format (an A3_FMT_* of include/aruco3_hip.h): whether the value names one, how many bytes a pixel
// takes in all stride arithmetic, where a packed 4:2:2 pixel keeps its luma, which widths the format has, and the fewest bytes a row and
// a frame span.  Host arithmetic on the public header only -- no HIP, no context -- so a plain C++ program can run every function
// (tests/format_checks.cpp); a3_api.hip, a3_reduce_check.h and a3_rectify_check.h ask here instead of spelling the formats out.
// The kernels that are templates on the format take their bytes per pixel from format_bpp too (k_threshold_k1.h's RawRow<FMT>,
// k_rectify), and their launchers name the formats in one place, a3_launch.h's with_format.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/aruco3_hip.h"

namespace a3 {

// packed 4:2:2 (Y0 U Y1 V / U Y0 V Y1): two bytes per pixel, one of them the pixel's luma, which is its grey level as it stands
constexpr bool format_is_422(int fmt) { return fmt == A3_FMT_YUYV8 || fmt == A3_FMT_UYVY8; }

// bytes a pixel takes in a row (all stride arithmetic), 0 for a value that names no format -- 4 (the library's own grey plane tag)
// among them
constexpr size_t format_bpp(int fmt) {
    return fmt == A3_FMT_RGB8 ? 3 : fmt == A3_FMT_L8 ? 1 : (fmt == A3_FMT_RGBA8 || fmt == A3_FMT_BGRA8) ? 4 : format_is_422(fmt) ? 2 : 0;
}
constexpr bool format_valid(int fmt) { return format_bpp(fmt) != 0; }

// the byte of pixel x's format_bpp() bytes that is its grey level, for the formats that keep one (L8: 0, YUYV8: 0, UYVY8: 1); -1 for the
// colour formats, whose grey level is luma_of their three channels, and for an invalid value
constexpr int format_luma_offset(int fmt) { return fmt == A3_FMT_L8 || fmt == A3_FMT_YUYV8 ? 0 : fmt == A3_FMT_UYVY8 ? 1 : -1; }

// bytes per pixel of the plane a3_rectify_frames writes for a source of this format: the input's format, but for 4:2:2 the luma view
constexpr size_t format_rectified_bpp(int fmt) { return format_is_422(fmt) ? 1 : format_bpp(fmt); }

// a width the format cannot have -> its message, else nullptr: a 4:2:2 row is made of pixel pairs that share their chroma
constexpr const char* format_width_error(int fmt, uint32_t width) {
    return format_is_422(fmt) && (width & 1u) ? "4:2:2 frames have an even width" : nullptr;
}

// the fewest bytes a row of `width` pixels spans, and a frame of `height` such rows `row_stride` apart (its last row ends with its
// pixels); 0 for an invalid format or an empty image
constexpr size_t format_min_row_bytes(int fmt, uint32_t width) { return (size_t)width * format_bpp(fmt); }
constexpr size_t format_min_frame_bytes(int fmt, uint32_t width, uint32_t height, size_t row_stride) {
    return height == 0 || !format_valid(fmt) ? 0 : row_stride * (height - 1) + format_min_row_bytes(fmt, width);
}

}  // namespace a3
