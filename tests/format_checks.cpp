// The one host description of a pixel format (aruco3_amd/csrc/a3_format.h) on every value of the public enum and on the values that
// name no format, and what a3_reduce_check.h and a3_rectify_check.h make of a packed 4:2:2 call: the odd width, the row stride one byte
// short, the smallest strides that pass, the luma view's one byte per pixel on the rectified side.  Prints "value NAME <n>" for the
// header's constants (tests/test_pixel_formats.py compares them with the Python and Rust bindings), exits 0 and prints "ok: <n> checks"
// when everything holds.  tests/test_pixel_formats.py compiles this with the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstring>
#include <initializer_list>

#include "../aruco3_amd/csrc/a3_format.h"
#include "../aruco3_amd/csrc/a3_rectify_check.h"
#include "../aruco3_amd/csrc/a3_reduce_check.h"

namespace {

int g_checks = 0, g_failed = 0;
unsigned char g_src[1 << 16], g_dst[1 << 16];   // (never read or written: the checks compare addresses)

void same(const char* name, const char* got, const char* want) {
    g_checks++;
    if ((got == nullptr) != (want == nullptr) || (got && std::strcmp(got, want) != 0)) {
        std::printf("FAILED %s: got \"%s\", expected \"%s\"\n", name, got ? got : "OK", want ? want : "OK");
        g_failed++;
    }
}
void equal(const char* name, long long got, long long want) {
    g_checks++;
    if (got != want) {
        std::printf("FAILED %s: got %lld, expected %lld\n", name, got, want);
        g_failed++;
    }
}

struct Fmt { const char* name; int value; int bpp, luma, rect_bpp; bool is422; };

a3_rectify rect(uint32_t sw, uint32_t sh, uint32_t dw, uint32_t dh) {
    a3_rectify r{};
    r.src.image_width = sw; r.src.image_height = sh; r.src.focal_x = r.src.focal_y = 50.0f;
    r.dst = r.src; r.dst.image_width = dw; r.dst.image_height = dh;
    r.rotation[0] = r.rotation[4] = r.rotation[8] = 1.0f;
    return r;
}

}  // namespace

int main() {
    static_assert(A3_FMT_RGB8 == 0 && A3_FMT_RGBA8 == 1 && A3_FMT_L8 == 2 && A3_FMT_BGRA8 == 3, "the four formats keep their values");
    static_assert(A3_FMT_YUYV8 == 5 && A3_FMT_UYVY8 == 6, "the packed 4:2:2 formats");
    std::printf("value A3_ABI_VERSION %d\n", (int)A3_ABI_VERSION);
    const Fmt fmts[] = {{"A3_FMT_RGB8", A3_FMT_RGB8, 3, -1, 3, false}, {"A3_FMT_RGBA8", A3_FMT_RGBA8, 4, -1, 4, false},
                        {"A3_FMT_L8", A3_FMT_L8, 1, 0, 1, false},      {"A3_FMT_BGRA8", A3_FMT_BGRA8, 4, -1, 4, false},
                        {"A3_FMT_YUYV8", A3_FMT_YUYV8, 2, 0, 1, true}, {"A3_FMT_UYVY8", A3_FMT_UYVY8, 2, 1, 1, true}};
    for (const Fmt& f : fmts) {
        std::printf("value %s %d\n", f.name, f.value);
        equal("valid", a3::format_valid(f.value), 1);
        equal("bpp", (long long)a3::format_bpp(f.value), f.bpp);
        equal("reduce_bpp", (long long)a3::reduce_bpp(f.value), f.bpp);
        equal("luma_offset", a3::format_luma_offset(f.value), f.luma);
        equal("rectified_bpp", (long long)a3::format_rectified_bpp(f.value), f.rect_bpp);
        equal("is_422", a3::format_is_422(f.value), f.is422);
        // the even-width rule: 4:2:2 only, with its own message
        same("width_even", a3::format_width_error(f.value, 640), nullptr);
        same("width_0", a3::format_width_error(f.value, 0), nullptr);
        same("width_odd", a3::format_width_error(f.value, 641), f.is422 ? "4:2:2 frames have an even width" : nullptr);
        same("width_1", a3::format_width_error(f.value, 1), f.is422 ? "4:2:2 frames have an even width" : nullptr);
        // the minimum row and frame bytes: the last row ends with its pixels
        equal("min_row", (long long)a3::format_min_row_bytes(f.value, 640), 640LL * f.bpp);
        equal("min_frame_packed", (long long)a3::format_min_frame_bytes(f.value, 640, 480, 640u * f.bpp), 640LL * f.bpp * 480);
        equal("min_frame_padded", (long long)a3::format_min_frame_bytes(f.value, 640, 480, 4096), 4096LL * 479 + 640LL * f.bpp);
        equal("min_frame_one_row", (long long)a3::format_min_frame_bytes(f.value, 6, 1, 1 << 20), 6LL * f.bpp);
        equal("min_frame_empty", (long long)a3::format_min_frame_bytes(f.value, 6, 0, 64), 0);
        equal("min_frame_65535", (long long)a3::format_min_frame_bytes(f.value, 65534, 16384, (size_t)65534 * f.bpp), 65534LL * f.bpp * 16384);
    }
    // 4 is the library's own grey plane tag: unassigned in the public enum and refused, as is everything else
    for (int bad : {4, 7, 8, 9, -1, 255, 256, -2147483647 - 1, 2147483647}) {
        equal("invalid", a3::format_valid(bad), 0);
        equal("invalid_bpp", (long long)a3::format_bpp(bad), 0);
        equal("invalid_luma", a3::format_luma_offset(bad), -1);
        equal("invalid_422", a3::format_is_422(bad), 0);
        equal("invalid_frame", (long long)a3::format_min_frame_bytes(bad, 8, 8, 64), 0);
        same("invalid_width", a3::format_width_error(bad, 3), nullptr);
        same("reduce_invalid", a3::check_reduce_frames(g_src, A3_MEM_HOST, bad, 32, 16, 128, 128 * 16, 1, 2, g_dst, A3_MEM_HOST, 16, 128),
             "a3_reduce_frames: unknown pixel format");
    }

    // a3_reduce_frames on 4:2:2: 32 x 16 pixels are 64 bytes a row
    for (int fmt : {(int)A3_FMT_YUYV8, (int)A3_FMT_UYVY8}) {
        auto reduce = [&](uint32_t w, uint32_t h, size_t row, size_t frame, uint32_t factor, size_t drow, size_t dframe) {
            return a3::check_reduce_frames(g_src, A3_MEM_HOST, fmt, w, h, row, frame, 2, factor, g_dst, A3_MEM_DEVICE, drow, dframe);
        };
        same("reduce_422_valid", reduce(32, 16, 64, 64 * 16, 2, 16, 128), nullptr);
        same("reduce_422_factor_3", reduce(32, 16, 64, 64 * 16, 3, 10, 50), nullptr);
        same("reduce_422_odd_width", reduce(33, 16, 66, 66 * 16, 2, 16, 128), "a3_reduce_frames: 4:2:2 frames have an even width");
        same("reduce_422_row_2w-1", reduce(32, 16, 63, 64 * 16, 2, 16, 128), "a3_reduce_frames: row stride smaller than a row");
        same("reduce_422_row_w", reduce(32, 16, 32, 64 * 16, 2, 16, 128), "a3_reduce_frames: row stride smaller than a row");
        same("reduce_422_row_padded", reduce(32, 16, 65, 65 * 16, 2, 16, 128), nullptr);
        same("reduce_422_frame_short", reduce(32, 16, 64, 64 * 16 - 1, 2, 16, 128), "a3_reduce_frames: frame stride smaller than a frame");
        same("reduce_422_fmt_before_width", a3::check_reduce_frames(g_src, A3_MEM_HOST, fmt, 33, 16, 66, 66 * 16, 0, 2, g_dst, A3_MEM_HOST, 16, 128),
             "a3_reduce_frames: n_frames must be in 1..65535");
        same("reduce_422_width_before_memory", a3::check_reduce_frames(g_src, 7, fmt, 33, 16, 66, 66 * 16, 1, 2, g_dst, A3_MEM_HOST, 16, 128),
             "a3_reduce_frames: 4:2:2 frames have an even width");

        // a3_rectify_frames on 4:2:2: the source takes 2 bytes per pixel, what is written 1 (the luma view)
        const a3_rectify r = rect(32, 16, 24, 12);
        same("rectify_422_valid", a3::check_rectify_frames_fmt(r, fmt, 64, 64 * 16, 24, 24 * 12), nullptr);
        same("rectify_422_src_row_2w-1", a3::check_rectify_frames_fmt(r, fmt, 63, 64 * 16, 24, 24 * 12), "a3_rectify_frames: row stride smaller than a row");
        same("rectify_422_src_frame_short", a3::check_rectify_frames_fmt(r, fmt, 64, 64 * 16 - 1, 24, 24 * 12), "a3_rectify_frames: frame stride smaller than a frame");
        same("rectify_422_dst_row_short", a3::check_rectify_frames_fmt(r, fmt, 64, 64 * 16, 23, 24 * 12), "a3_rectify_frames: row stride smaller than a row");
        same("rectify_422_dst_frame_short", a3::check_rectify_frames_fmt(r, fmt, 64, 64 * 16, 24, 24 * 12 - 1), "a3_rectify_frames: frame stride smaller than a frame");
        same("rectify_422_odd_src_width", a3::check_rectify_frames_fmt(rect(33, 16, 24, 12), fmt, 66, 66 * 16, 24, 24 * 12),
             "a3_rectify_frames: 4:2:2 frames have an even width");
        same("rectify_422_odd_dst_width", a3::check_rectify_frames_fmt(rect(32, 16, 23, 12), fmt, 64, 64 * 16, 23, 23 * 12), nullptr);   // (the view is a plane)
    }
    // the other formats: what is written has the input's format
    {
        const a3_rectify r = rect(32, 16, 24, 12);
        same("rectify_rgb_valid", a3::check_rectify_frames_fmt(r, A3_FMT_RGB8, 96, 96 * 16, 72, 72 * 12), nullptr);
        same("rectify_rgb_dst_row_short", a3::check_rectify_frames_fmt(r, A3_FMT_RGB8, 96, 96 * 16, 71, 72 * 12), "a3_rectify_frames: row stride smaller than a row");
        same("rectify_rgb_odd_width", a3::check_rectify_frames_fmt(rect(33, 16, 24, 12), A3_FMT_RGB8, 99, 99 * 16, 72, 72 * 12), nullptr);
        same("rectify_same_as_before", a3::check_rectify(false, r, 3, 96, 96 * 16, 72, 72 * 12), nullptr);
    }
    if (g_failed) return 1;
    std::printf("ok: %d checks\n", g_checks);
    return 0;
}
