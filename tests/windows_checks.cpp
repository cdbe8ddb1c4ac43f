// The argument checks and the index arithmetic of detection with several threshold windows (aruco3_amd/csrc/a3_windows_check.h): every
// refusal of a3_set_threshold_windows with its message, the first failing check deciding, every boundary that passes, the plane index
// and the merged tables' capacity.  Exits 0 and prints "ok: <n> checks" when every answer is the expected one.
// tests/test_multiwindow.py compiles this with the address and undefined-behaviour sanitizers.
#include <cstdio>
#include <cstring>
#include <initializer_list>
#include <vector>

#include "../aruco3_amd/csrc/a3_windows_check.h"

namespace {

int g_checks = 0, g_failed = 0;

void same(const char* name, const char* got, const char* want) {
    g_checks++;
    if ((got == nullptr) != (want == nullptr) || (got && std::strcmp(got, want) != 0)) {
        std::printf("FAILED %s: got \"%s\", expected \"%s\"\n", name, got ? got : "OK", want ? want : "OK");
        g_failed++;
    }
}
void equal(const char* name, uint64_t got, uint64_t want) {
    g_checks++;
    if (got != want) {
        std::printf("FAILED %s: got %llu, expected %llu\n", name, (unsigned long long)got, (unsigned long long)want);
        g_failed++;
    }
}
const char* set(std::initializer_list<uint32_t> radii, bool busy = false) {
    const std::vector<uint32_t> r(radii);   // (exactly the radii: a read past them is the sanitizer's to find)
    return a3::check_threshold_windows(busy, r.data(), r.size());
}

constexpr const char* kBusy = "a3_set_threshold_windows: a submitted batch has not been collected";
constexpr const char* kMany = "a3_set_threshold_windows: more than A3_MAX_THRESHOLD_WINDOWS (4) windows";
constexpr const char* kZero = "a3_set_threshold_windows: a radius must be > 0 (imageproc asserts block_radius > 0)";
constexpr const char* kHuge = "a3_set_threshold_windows: a radius must be at most 2^31 - 1 (the threshold kernels take it as a signed 32-bit int)";
constexpr const char* kRange = "a3_set_threshold_windows: in a set of two or more every radius must be in 1..31";
constexpr const char* kOrder = "a3_set_threshold_windows: the radii must be strictly ascending";

}  // namespace

int main() {
    static_assert(A3_MAX_THRESHOLD_WINDOWS == 4, "the header's limit");
    // off
    same("off_null", a3::check_threshold_windows(false, nullptr, 0), nullptr);
    same("off_null_n", a3::check_threshold_windows(false, nullptr, 3), nullptr);
    const uint32_t one = 7;
    same("off_n0", a3::check_threshold_windows(false, &one, 0), nullptr);
    // one window: the single-window path's range
    for (uint32_t w : {1u, 7u, 12u, 31u, 32u, 1000u, 0x7FFFFFFFu}) same("one_ok", set({w}), nullptr);
    same("one_zero", set({0}), kZero);
    same("one_huge", set({0x80000000u}), kHuge);
    same("one_huge_max", set({0xFFFFFFFFu}), kHuge);
    // sets
    same("two_ok", set({7, 15}), nullptr);
    same("three_ok", set({3, 7, 15}), nullptr);
    same("four_ok", set({1, 2, 30, 31}), nullptr);
    same("edges_ok", set({1, 31}), nullptr);
    same("five", set({1, 2, 3, 4, 5}), kMany);
    same("five_before_zero", set({0, 2, 3, 4, 5}), kMany);
    same("set_zero_first", set({0, 7}), kZero);
    same("set_zero_last", set({3, 7, 0}), kZero);
    same("set_zero_before_range", set({40, 0}), kZero);
    same("set_32", set({7, 32}), kRange);
    same("set_32_first", set({32, 33}), kRange);
    same("set_huge", set({7, 0x80000000u}), kRange);
    same("set_range_before_order", set({32, 7}), kRange);
    same("equal", set({7, 7}), kOrder);
    same("descending", set({15, 7}), kOrder);
    same("descending_late", set({3, 7, 15, 14}), kOrder);
    same("equal_late", set({3, 7, 7}), kOrder);
    // a batch in flight: refused whatever the arguments, off included
    same("busy", set({3, 7, 15}, true), kBusy);
    same("busy_bad", set({0}, true), kBusy);
    same("busy_off", a3::check_threshold_windows(true, nullptr, 0), kBusy);
    // planes
    same("planes_ok", a3::check_window_planes(16383, 4), nullptr);
    same("planes_edge", a3::check_window_planes(21845, 3), nullptr);
    same("planes_over", a3::check_window_planes(21846, 3), "a3_detect_batch: frames x threshold windows above 65535 (split the batch)");
    same("planes_over_4", a3::check_window_planes(16384, 4), "a3_detect_batch: frames x threshold windows above 65535 (split the batch)");
    same("planes_one", a3::check_window_planes(65535, 1), nullptr);
    same("planes_none", a3::check_window_planes(0, 4), nullptr);
    same("planes_wrap", a3::check_window_planes(0xFFFFFFFFu, 4), "a3_detect_batch: frames x threshold windows above 65535 (split the batch)");
    // the plane index: window-major, a bijection onto 0 .. n * K - 1
    for (uint32_t n : {1u, 3u, 7u}) {
        for (uint32_t K : {2u, 3u, 4u}) {
            std::vector<int> seen(n * K, 0);
            for (uint32_t k = 0; k < K; k++)
                for (uint32_t f = 0; f < n; f++) {
                    const uint32_t p = a3::window_plane(k, f, n);
                    equal("plane_in_range", p < n * K, 1);
                    if (p < n * K) seen[p]++;
                    equal("plane_window_major", p, k * n + f);
                }
            for (int s : seen) equal("plane_once", (uint64_t)s, 1);
        }
    }
    equal("plane_3_batch", a3::window_plane(2, 1, 3), 7);
    // the merged capacity: K planes' tables, up to the format's limit
    equal("cap_default", a3::merged_cand_capacity(3, 1024), 3072);
    equal("cap_two", a3::merged_cand_capacity(2, 1024), 2048);
    equal("cap_lds_edge", a3::merged_cand_capacity(3, 2048), 6144);
    equal("cap_big", a3::merged_cand_capacity(2, 4096), 8192);
    equal("cap_at_limit", a3::merged_cand_capacity(4, 16384), 65536);
    equal("cap_clamped", a3::merged_cand_capacity(4, 24576), 65536);
    equal("cap_clamped_2", a3::merged_cand_capacity(2, 49152), 65536);
    equal("cap_full", a3::merged_cand_capacity(4, 65536), 65536);
    equal("cap_no_wrap", a3::merged_cand_capacity(4, 0x40000000u), 65536);
    for (uint32_t K : {2u, 3u, 4u})
        for (uint32_t c : {1u, 1024u, 2048u, 4096u, 6144u, 12288u, 24576u, 49152u, 65536u}) {
            const uint32_t m = a3::merged_cand_capacity(K, c);
            equal("cap_holds_planes_or_limit", m == K * c || (m == A3_MAX_CANDIDATES_PER_FRAME && (uint64_t)K * c > m), 1);
        }
    if (g_failed) return 1;
    std::printf("ok: %d checks\n", g_checks);
    return 0;
}
