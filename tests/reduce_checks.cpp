// The argument checks of the reduction (aruco3_amd/csrc/a3_reduce_check.h) on a valid call and on one mutation of it at a time: every
// input error of a3_reduce_frames with its message, the first failing check deciding, every boundary that passes, and the setter's
// record.  Exits 0 and prints "ok: <n> checks" when every message is the expected one.
// tests/test_reduced_detection.py compiles this with the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstring>
#include <functional>

#include "../aruco3_amd/csrc/a3_reduce_check.h"

namespace {

int g_checks = 0, g_failed = 0;
unsigned char g_src[1 << 16], g_dst[1 << 16];   // (never read or written: the checks compare addresses)

struct Call {
    const void* src = g_src; int src_memory = A3_MEM_HOST, fmt = A3_FMT_RGB8; uint32_t width = 33, height = 17;
    size_t src_row = 99, src_frame = 99 * 17; uint32_t n_frames = 2, factor = 2; const void* dst = g_dst; int dst_memory = A3_MEM_DEVICE;
    size_t dst_row = 16, dst_frame = 16 * 8;
};

void same(const char* name, const char* got, const char* want) {
    g_checks++;
    if ((got == nullptr) != (want == nullptr) || (got && std::strcmp(got, want) != 0)) {
        std::printf("FAILED %s: got \"%s\", expected \"%s\"\n", name, got ? got : "OK", want ? want : "OK");
        g_failed++;
    }
}

void expect(const char* name, const std::function<void(Call&)>& mutate, const char* want) {
    Call c;
    if (mutate) mutate(c);
    same(name, a3::check_reduce_frames(c.src, c.src_memory, c.fmt, c.width, c.height, c.src_row, c.src_frame, c.n_frames, c.factor, c.dst, c.dst_memory,
                                       c.dst_row, c.dst_frame), want);
}

}  // namespace

int main() {
    using C = Call;
    const char* FRAMES = "a3_reduce_frames: n_frames must be in 1..65535";
    const char* FMT = "a3_reduce_frames: unknown pixel format";
    const char* MEM = "a3_reduce_frames: memory must be A3_MEM_HOST or A3_MEM_DEVICE";
    const char* FACTOR = "a3_reduce_frames: factor must be 2, 3 or 4";
    const char* EMPTY = "a3_reduce_frames: a reduced width or height of 0";
    const char* BIG = "a3_reduce_frames: a reduced size above 65535 or of 2^30 pixels and more";
    const char* ROW = "a3_reduce_frames: row stride smaller than a row";
    const char* FRAME = "a3_reduce_frames: frame stride smaller than a frame";
    const char* OVERLAP = "a3_reduce_frames: src and dst overlap";
    auto big = [](C& c) { c.src_row = (size_t)1 << 24; c.src_frame = (size_t)1 << 44; c.dst_row = (size_t)1 << 20; c.dst_frame = (size_t)1 << 40; c.n_frames = 1; };
    expect("valid", nullptr, nullptr);
    // every error
    expect("n_frames_0", [](C& c) { c.n_frames = 0; }, FRAMES);
    expect("n_frames_65536", [](C& c) { c.n_frames = 65536; }, FRAMES);
    expect("fmt_-1", [](C& c) { c.fmt = -1; }, FMT);
    expect("fmt_4", [](C& c) { c.fmt = 4; }, FMT);
    expect("src_memory", [](C& c) { c.src_memory = 2; }, MEM);
    expect("dst_memory", [](C& c) { c.dst_memory = -1; }, MEM);
    expect("factor_0", [](C& c) { c.factor = 0; }, FACTOR);
    expect("factor_1", [](C& c) { c.factor = 1; }, FACTOR);
    expect("factor_5", [](C& c) { c.factor = 5; }, FACTOR);
    expect("width_1", [](C& c) { c.width = 1; }, EMPTY);
    expect("height_0", [](C& c) { c.height = 0; }, EMPTY);
    expect("height_below_factor", [](C& c) { c.factor = 4; c.height = 3; c.dst_row = 8; c.dst_frame = 0; }, EMPTY);
    expect("reduced_width_65536", [&](C& c) { big(c); c.width = 2 * 65536; }, BIG);
    expect("reduced_height_65536", [&](C& c) { big(c); c.factor = 4; c.height = 4 * 65536; }, BIG);
    expect("reduced_2^30_pixels", [&](C& c) { big(c); c.width = c.height = 2 * 32768; }, BIG);
    expect("src_row_short", [](C& c) { c.src_row = 98; }, ROW);
    expect("dst_row_short", [](C& c) { c.dst_row = 15; }, ROW);
    expect("src_frame_short", [](C& c) { c.src_frame -= 1; }, FRAME);
    expect("dst_frame_short", [](C& c) { c.dst_frame -= 1; }, FRAME);
    expect("src_row_padded", [](C& c) { c.src_row += 1; }, FRAME);   // (the frame no longer holds its rows)
    expect("dst_inside_src", [](C& c) { c.dst = g_src + 100; }, OVERLAP);
    expect("src_inside_dst", [](C& c) { c.src = g_dst + 255; }, OVERLAP);
    expect("dst_is_src", [](C& c) { c.dst = c.src; c.dst_memory = c.src_memory; }, OVERLAP);
    expect("src_ends_in_dst", [](C& c) { c.dst = g_src + 2 * 99 * 17 - 1; }, OVERLAP);
    // the first failing check decides, in the order above
    expect("frames_before_fmt", [](C& c) { c.n_frames = 0; c.fmt = 9; }, FRAMES);
    expect("fmt_before_memory", [](C& c) { c.fmt = 9; c.src_memory = 5; }, FMT);
    expect("memory_before_factor", [](C& c) { c.dst_memory = 5; c.factor = 9; }, MEM);
    expect("factor_before_size", [](C& c) { c.factor = 1; c.width = 0; }, FACTOR);
    expect("size_before_strides", [](C& c) { c.width = 1; c.src_row = 0; }, EMPTY);
    expect("row_before_frame", [](C& c) { c.dst_row = 1; c.src_frame = 1; }, ROW);
    expect("frame_before_overlap", [](C& c) { c.dst_frame = 1; c.dst = c.src; }, FRAME);
    // every boundary that passes
    expect("factor_2", [](C& c) { c.factor = 2; }, nullptr);
    expect("factor_3", [](C& c) { c.factor = 3; }, nullptr);
    expect("factor_4", [](C& c) { c.factor = 4; }, nullptr);
    expect("n_frames_1", [](C& c) { c.n_frames = 1; }, nullptr);
    expect("n_frames_65535", [&](C& c) { c.n_frames = 65535; c.src = reinterpret_cast<const void*>((uintptr_t)1 << 40); c.dst = reinterpret_cast<const void*>((uintptr_t)1 << 50); }, nullptr);
    expect("reduced_size_1", [](C& c) { c.factor = 4; c.width = 7; c.height = 4; c.src_row = 21; c.src_frame = 84; c.dst_row = 1; c.dst_frame = 1; }, nullptr);
    expect("reduced_width_65535", [&](C& c) { big(c); c.fmt = A3_FMT_L8; c.width = 2 * 65535 + 1; c.src = reinterpret_cast<const void*>((uintptr_t)1 << 50); }, nullptr);
    expect("reduced_65535_x_16384", [&](C& c) { big(c); c.fmt = A3_FMT_L8; c.width = 2 * 65535; c.height = 2 * 16384; c.src = reinterpret_cast<const void*>((uintptr_t)1 << 50); }, nullptr);
    expect("strides_equal_a_row", [](C& c) { c.src_row = 99; c.src_frame = 99 * 17; c.dst_row = 16; c.dst_frame = 128; }, nullptr);
    expect("l8_row", [](C& c) { c.fmt = A3_FMT_L8; c.src_row = 33; c.src_frame = 33 * 17; }, nullptr);
    expect("bgra_row", [](C& c) { c.fmt = A3_FMT_BGRA8; c.src_row = 132; c.src_frame = 132 * 17; }, nullptr);
    expect("bgra_row_short", [](C& c) { c.fmt = A3_FMT_BGRA8; c.src_row = 131; c.src_frame = 132 * 17; }, ROW);
    expect("dst_right_behind_src", [](C& c) { c.dst = g_src + 99 * 17 * 2; }, nullptr);
    expect("src_right_behind_dst", [](C& c) { c.src = g_dst + 256; }, nullptr);
    // the setter's record
    auto rec = [](uint32_t f, uint32_t r0 = 0, uint32_t r1 = 0, uint32_t r2 = 0) { a3_reduction r{}; r.factor = f; r.reserved[0] = r0; r.reserved[1] = r1; r.reserved[2] = r2; return r; };
    for (uint32_t f = 2; f <= 4; f++) same("set_factor", a3::check_reduction(rec(f)), nullptr);
    for (uint32_t f : {0u, 1u, 5u, 0xFFFFFFFFu}) same("set_factor_bad", a3::check_reduction(rec(f)), "a3_set_reduction: factor must be 2, 3 or 4");
    same("set_reserved_0", a3::check_reduction(rec(2, 1)), "a3_set_reduction: a3_reduction.reserved must be 0");
    same("set_reserved_1", a3::check_reduction(rec(3, 0, 1)), "a3_set_reduction: a3_reduction.reserved must be 0");
    same("set_reserved_2", a3::check_reduction(rec(4, 0, 0, 1)), "a3_set_reduction: a3_reduction.reserved must be 0");
    same("set_factor_before_reserved", a3::check_reduction(rec(7, 1)), "a3_set_reduction: factor must be 2, 3 or 4");
    // the detect call's size check
    same("detect_block", a3::check_reduced_size(true, 3, 9, 4), "a3_detect_batch: with a reduction set the frames must hold at least one block (a3_set_reduction)");
    same("detect_ok", a3::check_reduced_size(true, 4, 4, 4), nullptr);
    if (g_failed) return 1;
    std::printf("ok: %d checks\n", g_checks);
    return 0;
}
