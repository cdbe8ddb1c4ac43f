// The threshold stage's host decisions (aruco3_amd/csrc/a3_threshold_plan.h) as a stand-alone program: which path a radius takes at
// every class boundary, and what the ring kernel's plan promises for every radius 8..31, format and load form -- the LDS a wave asks
// for stays inside its share of the CU's, a burst holds at least one row, and the plan counts eight waves per CU exactly where the
// kernel's __launch_bounds__ asks for two per SIMD.  Then the planner itself on the table standard input holds, one row
// "n W H R format fast" per line (format: an A3_FMT_* value; R 1..7 asks plan_k1, 8..31 plan_ring), answered by
// "plan n W H R format fast strips_x strips_y rows_per_wave flush_rows lds_bytes": tests/test_threshold_plan.py sends every shape the
// GPU tests rely on and compares the answers with tests/threshold_util.py's mirrors.  Exits 0 and prints "ok: <n> checks" last when
// every answer is the expected one; the test compiles this with the address and undefined-behaviour sanitizers.
#include <cstdio>

#include "../aruco3_amd/csrc/a3_threshold_plan.h"

namespace {

int g_checks = 0, g_failed = 0;

void check(bool ok, const char* what, long long a = 0, long long b = 0, long long c = 0) {
    g_checks++;
    if (!ok) {
        std::printf("FAILED %s (%lld, %lld, %lld)\n", what, a, b, c);
        g_failed++;
    }
}

void path_checks() {
    using a3::ThresholdPath;
    const struct { uint32_t radius; ThresholdPath path; } want[] = {
        {0u, ThresholdPath::Brute}, {1u, ThresholdPath::K1}, {7u, ThresholdPath::K1}, {8u, ThresholdPath::Ring}, {15u, ThresholdPath::Ring},
        {16u, ThresholdPath::Ring}, {31u, ThresholdPath::Ring}, {32u, ThresholdPath::Separable}, {128u, ThresholdPath::Separable},
        {129u, ThresholdPath::Brute}, {0x7FFFFFFFu, ThresholdPath::Brute}};
    for (const auto& w : want) {
        check(a3::threshold_path(w.radius) == w.path, "threshold_path", w.radius);
        const bool plain = w.path == ThresholdPath::Separable || w.path == ThresholdPath::Brute;
        check(a3::threshold_writes_grey_plane(w.radius) == plain, "threshold_writes_grey_plane", w.radius);
    }
}

void ring_invariants() {
    const int formats[] = {A3_FMT_RGB8, A3_FMT_RGBA8, A3_FMT_L8, A3_FMT_BGRA8, A3_FMT_YUYV8, A3_FMT_UYVY8};
    for (int R = 8; R <= 31; R++)
        for (int fmt : formats)
            for (int fast = 0; fast < 2; fast++) {
                // (a full-size batch: the strips are taller than any burst, so flush_rows is what the LDS leaves room for)
                const a3::RingPlan p = a3::plan_ring(1920, 1080, 256, R, fmt, fast != 0);
                const int waves = a3::ring_waves(R, fast != 0, fmt);
                check(p.NB == 2 * R + 1 - a3::ring_reg_rows(R, fast != 0, fmt) && p.NB >= 1, "ring: NB", R, fmt, fast);
                check((p.NB <= a3::kRingLdsRows8) == (waves == 2), "ring: two waves per SIMD exactly where NB <= kRingLdsRows8", R, fmt, fast);
                // ... and that line is where the LDS draws it: eight waves' rings, each with one parked row, the load queue's rows and the
                // allocation granule, fit a CU exactly up to kRingLdsRows8 rows of ring
                check((8 * (p.NB * 1024 + (1 + a3::T_PF) * 128 + 64) <= a3::kLdsBytes) == (waves == 2), "ring: eight waves' LDS fits exactly where two per SIMD are asked for", R, fmt, fast);
                check(p.WPC == a3::kSIMDs * waves, "ring: the plan's waves per CU are the launch bounds'", R, fmt, fast);
                check(p.per_wave == a3::kLdsBytes / p.WPC - 64, "ring: a wave's share of the LDS", R, fmt, fast);
                check(p.lds_bytes <= (size_t)p.per_wave, "ring: the LDS bytes stay inside the wave's share", R, fmt, fast);
                check(p.park_room >= 1 && p.flush_rows >= 1 && p.flush_rows <= p.park_room, "ring: a burst has room", R, fmt, fast);
                check(p.lds_bytes == (size_t)p.NB * 1024 + (size_t)(p.flush_rows + a3::T_PF) * 128, "ring: LDS bytes", R, fmt, fast);
            }
}

// the table on standard input; a row that is not six numbers in range ends the program with a failure
void planner_table() {
    long long n, W, H, R, fmt, fast;
    int got;
    while ((got = std::scanf("%lld %lld %lld %lld %lld %lld", &n, &W, &H, &R, &fmt, &fast)) == 6) {
        const bool ok = n >= 1 && n <= 65535 && W >= 1 && W <= 65535 && H >= 1 && H <= 65535 && R >= 1 && R <= 31 && a3::format_valid((int)fmt) && (fast == 0 || fast == 1);
        check(ok, "table row out of range", n, W, H);
        if (!ok) return;
        if (R <= 7) {
            const a3::K1Plan p = a3::plan_k1((int)W, (int)H, (uint32_t)n, (int)R);
            std::printf("plan %lld %lld %lld %lld %lld %lld %d %d %d %d %zu\n", n, W, H, R, fmt, fast, p.s.strips_x, p.s.strips_y, p.s.rows_per_wave, p.flush_rows, p.lds_bytes);
        } else {
            const a3::RingPlan p = a3::plan_ring((int)W, (int)H, (uint32_t)n, (int)R, (int)fmt, fast != 0);
            std::printf("plan %lld %lld %lld %lld %lld %lld %d %d %d %d %zu\n", n, W, H, R, fmt, fast, p.s.strips_x, p.s.strips_y, p.s.rows_per_wave, p.flush_rows, p.lds_bytes);
        }
    }
    check(got == EOF, "table row is not six numbers");
}

}  // namespace

int main() {
    path_checks();
    ring_invariants();
    planner_table();
    if (g_failed) {
        std::printf("%d of %d checks FAILED\n", g_failed, g_checks);
        return 1;
    }
    std::printf("ok: %d checks\n", g_checks);
    return 0;
}
