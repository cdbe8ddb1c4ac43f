// a3_threshold_plan.h -- what the host decides for a threshold launch: which of the four paths a window takes, how the frames are cut
// into strips (one wave each), and how much LDS a wave of the two fused kernels parks its result bits in.  Host arithmetic only -- no
// HIP, no context -- so a plain C++ program can run every function (tests/threshold_plan_checks.cpp, which also holds
// tests/threshold_util.py's mirrors against it).  The constants here are the ones the kernels (k_threshold_k1.h, k_threshold_big.hip)
// and their launchers share.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>

#include "a3_format.h"

namespace a3 {

// ---- the lanes of a wave (both fused kernels) ----
// Pixels per lane and row: 256 VGPRs (the ring of row sums alone is 120), two waves per SIMD.  8 pixels per lane (144 VGPRs, three
// waves per SIMD) was built to see whether occupancy was what kept the kernel (stores off) 0.025 ms above the bare reads of
// tools/micro/readbench.hip.  It was not: 0.293 ms against 0.286 with stores off, 0.343 against 0.324 with them (docs/HISTORY.md
// A.1); the difference to the microbenchmark is the 5 % of halo rows and the feeder lanes.
constexpr int T_LPX = 16;
constexpr int T_PF = 3;              // rows of loads in flight per lane
constexpr int T_WAVES = 2;           // K1's waves per SIMD (__launch_bounds__); every resident wave's LDS parking area must fit the CU
constexpr int T_OUT = 62 * T_LPX;    // K1's output columns per wave (lanes 0 and 63 only feed their neighbours)
constexpr int kCUs = 256, kSIMDs = 4, kLdsBytes = 160 * 1024;   // the chip: CUs, SIMDs per CU, LDS per CU

// ---- which path a window takes ----
// K1: the register-resident kernel, radii 1..7.  Beyond 7 its packed 16-bit arithmetic ends -- (2R+1)^2 * 256 no longer fits a u16
// from R = 8 on (289 * 256 = 73 984).  Ring: radii 8..31, the grey ring in registers + LDS and 32-bit sums (k_threshold_big.hip).
// Separable: radii 32..128, a grey plane and a u16 plane of row sums (2R+1 <= 257 values of at most 255).  Brute: what is left, radius
// 0 and radii above 128, work per pixel growing with the window's area.
enum class ThresholdPath { K1, Ring, Separable, Brute };
constexpr ThresholdPath threshold_path(uint32_t radius) {
    return radius == 0 || radius > 128 ? ThresholdPath::Brute
         : radius <= 7 ? ThresholdPath::K1 : radius <= 31 ? ThresholdPath::Ring : ThresholdPath::Separable;
}
// this window's path reads a grey plane (and, separable, a plane of row sums) that the caller provides; the fused kernels need neither
constexpr bool threshold_writes_grey_plane(uint32_t radius) {
    return threshold_path(radius) == ThresholdPath::Separable || threshold_path(radius) == ThresholdPath::Brute;
}

// ---- strips ----
// Rows per wave.  Every wave also reads and converts 2R rows outside its strip, so strips should be tall; but the chip holds
// wave_slots waves at once and a launch runs in whole rounds of that many, so the number of strips should fill the last round.
// Model: time ~ rounds x (rows per strip + 2R); take the best strip count (at least 16 rows per strip, the smaller count on a tie).
// 256 frames of 1920x1080, R = 7: 2 column strips x 4 strips of 270 rows = 2048 waves = exactly one round of two waves per SIMD.
// (Strips of ONE row for a single small frame -- 480 waves of one 15-row block instead of 30 waves of two -- were tried in round 5:
// 23.0 us against 16.8 for one 640x480 frame; a wave's fixed costs outweigh the block saved.  The model stays at >= 16 rows.)
struct StripPlan { int strips_x, strips_y, rows_per_wave; };
inline StripPlan plan_strips(int W, int H, uint32_t n_frames, int R, int out_cols, long long wave_slots) {
    const int strips_x = (W + out_cols - 1) / out_cols;
    const long long cols = (long long)strips_x * n_frames;
    int best_sy = 1; double best_cost = 1e300;
    for (int sy = 1; sy <= std::max(1, H / 16); sy++) {
        const int rows = (H + sy - 1) / sy;
        const long long waves = cols * ((H + rows - 1) / rows);
        const double cost = (double)((waves + wave_slots - 1) / wave_slots) * (rows + 2 * R);
        if (cost < best_cost - 1e-9) { best_cost = cost; best_sy = sy; }
    }
    const int rows_per_wave = (H + best_sy - 1) / best_sy;
    return {strips_x, (H + rows_per_wave - 1) / rows_per_wave, rows_per_wave};
}
// workgroups (of one wave) of a launch: every strip of a frame on one XCD, frames dealt over the 8 XCDs (strip_of, k_threshold_k1.h)
inline unsigned strip_grid(const StripPlan& s, uint32_t n_frames) { return 8u * ((n_frames + 7u) / 8u) * (unsigned)(s.strips_x * s.strips_y); }

// ---- K1 (radii 1..7) ----
// rows of results a wave parks in LDS before it writes them out: 128 (+ the row loop's unroll) rows x 64 lanes x 2 bytes = 18 KB per
// wave, and every resident wave's parking area must fit the CU's LDS (4 x T_WAVES waves)
constexpr int kFlushRows = 128;
constexpr int k1_unroll(int R) { return ((2 * R + 1 + T_PF - 1) / T_PF) * T_PF; }   // the window's rows, a multiple of the load queue
static_assert((kFlushRows + k1_unroll(7)) * 128 * kSIMDs * T_WAVES <= kLdsBytes, "the parked rows fit the LDS");
struct K1Plan { StripPlan s; int flush_rows; size_t lds_bytes; };
inline K1Plan plan_k1(int W, int H, uint32_t n_frames, int R) {
    const StripPlan s = plan_strips(W, H, n_frames, R, T_OUT, (long long)kCUs * kSIMDs * T_WAVES);
    const int flush_rows = std::min(kFlushRows, s.rows_per_wave);
    return {s, flush_rows, (size_t)(flush_rows + k1_unroll(R)) * 128};
}

// ---- the ring kernel (radii 8..31) ----
// The ring's split.  RA rows (the youngest) in registers, NB = 2R + 1 - RA in LDS.  Two waves per SIMD -- eight per CU -- are worth a
// factor 1.8 (measured: 0.41 against 0.72 ms for radius 16), and eight waves fit a CU's LDS with at most 19 KB of ring each: up to radius
// 18 the split is R | R + 1; beyond, as long as the registers hold the rest without scratch (115 + 4 RA VGPRs for RGB with vector loads,
// 12 more for four-byte pixels, 25 fewer for L8, ~40 more with per-pixel loads), the LDS part stays at 19 rows and the register part
// grows (1.26-1.45 x of window 7); the largest radii fall back to R | R + 1 and one wave per SIMD (2.4-2.6 x).
constexpr int kRingLdsRows8 = 19;
constexpr int ring_reg_rows(int R, bool fast, int fmt) {   // (the limits: the largest radius whose instantiation needs no scratch)
    // packed 4:2:2 has 8 raw dwords per row in flight: between L8's 4 and RGB8's 12
    const int last8 = !fast ? 19 : (fmt == A3_FMT_L8 ? 28 : (format_is_422(fmt) ? 27 : (fmt == A3_FMT_RGB8 ? 26 : 24)));
    return R + 1 <= kRingLdsRows8 ? R : (R <= last8 ? 2 * R + 1 - kRingLdsRows8 : R);
}
constexpr int ring_lds_rows(int R, bool fast, int fmt) { return 2 * R + 1 - ring_reg_rows(R, fast, fmt); }
// waves per SIMD (__launch_bounds__): two while the ring's LDS part is at most 19 KB per wave, else one
constexpr int ring_waves(int R, bool fast, int fmt) { return ring_lds_rows(R, fast, fmt) <= kRingLdsRows8 ? 2 : 1; }
// apron lanes on either side of a wave and the output columns left to it
constexpr int ring_halo_lanes(int R) { return R > 15 ? 2 : 1; }
constexpr int ring_out_cols(int R) { return (64 - 2 * ring_halo_lanes(R)) * T_LPX; }
// NB KB of ring + (flush_rows + T_PF) rows of parked result bits per wave, in the wave's share of the LDS less the allocation granule.
// park_room: the rows of bits that share holds; below 1 the launcher refuses (cannot happen: 19 KB + 4 rows fit an eighth, 32 KB + 60
// rows a quarter).
struct RingPlan { StripPlan s; int NB, WPC, per_wave, park_room, flush_rows; size_t lds_bytes; };
inline RingPlan plan_ring(int W, int H, uint32_t n_frames, int R, int fmt, bool fast) {
    const int NB = ring_lds_rows(R, fast, fmt), WPC = kSIMDs * ring_waves(R, fast, fmt);
    const StripPlan s = plan_strips(W, H, n_frames, R, ring_out_cols(R), (long long)kCUs * WPC);
    const int per_wave = kLdsBytes / WPC - 64, park_room = (per_wave - NB * 1024) / 128 - T_PF;
    const int flush_rows = std::max(1, std::min({kFlushRows, s.rows_per_wave, park_room}));
    return {s, NB, WPC, per_wave, park_room, flush_rows, (size_t)NB * 1024 + (size_t)(flush_rows + T_PF) * 128};
}

}  // namespace a3
