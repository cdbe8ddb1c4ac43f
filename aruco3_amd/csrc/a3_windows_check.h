// Argument checks and index arithmetic of detection with several threshold windows (a3_set_threshold_windows): everything that stands
// between a caller's radii and the K threshold launches, the n * K planes of the contour stage and k_merge_candidates, which indexes the
// per-plane and the merged candidate tables with the sizes below.  Host arithmetic on plain values -- no HIP, no context -- so a plain
// C++ program can run every check (tests/windows_checks.cpp).  Each check returns the message of the FIRST test that fails, or nullptr.
// Every message is a whole string literal (as a3_reduce_check.h).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/aruco3_hip.h"

namespace a3 {

constexpr uint32_t kWindowSetMaxRadius = 31;   // the largest radius of the fused one-pass threshold kernels, which need no grey plane

// a3_set_threshold_windows(ctx, radii, n), behind its null-context test; busy: a submitted batch has not been collected.
// NULL radii or n = 0 switch the setting off and pass.
inline const char* check_threshold_windows(bool busy, const uint32_t* radii, size_t n) {
    if (busy) return "a3_set_threshold_windows: a submitted batch has not been collected";
    if (!radii || n == 0) return nullptr;
    if (n > A3_MAX_THRESHOLD_WINDOWS) return "a3_set_threshold_windows: more than A3_MAX_THRESHOLD_WINDOWS (4) windows";
    for (size_t k = 0; k < n; k++)
        if (radii[k] == 0) return "a3_set_threshold_windows: a radius must be > 0 (imageproc asserts block_radius > 0)";
    if (n == 1)
        return radii[0] > 0x7FFFFFFFu ? "a3_set_threshold_windows: a radius must be at most 2^31 - 1 (the threshold kernels take it as a signed 32-bit int)"
                                      : nullptr;
    for (size_t k = 0; k < n; k++)
        if (radii[k] > kWindowSetMaxRadius) return "a3_set_threshold_windows: in a set of two or more every radius must be in 1..31";
    for (size_t k = 1; k < n; k++)
        if (radii[k] <= radii[k - 1]) return "a3_set_threshold_windows: the radii must be strictly ascending";
    return nullptr;
}

// A batch of n frames under K windows is n * K planes to the front half and the contour stage; their number stays where a plain batch's
// frame count stays (65535: a3_detect_batch's own limit).
inline const char* check_window_planes(uint32_t n_frames, uint32_t n_windows) {
    if ((uint64_t)n_frames * n_windows > 65535u) return "a3_detect_batch: frames x threshold windows above 65535 (split the batch)";
    return nullptr;
}

// plane (k, f) of a batch of n frames: window-major, so window k's planes are one contiguous batch of n frames to its threshold launch
constexpr uint32_t window_plane(uint32_t k, uint32_t f, uint32_t n_frames) { return k * n_frames + f; }

// Slots per frame of the merged tables (pre_xy, fin_xy, work, outs, proj) when every plane's table has plane_cand slots: all K planes'
// candidates fit by construction, up to the format's limit (a3_marker.candidate_index is 16 bits).  The merged tables so have no
// capacity of their own to overflow: a plane that outgrows plane_cand raises kErrCandTable in the contour stage and the batch is re-run
// with larger per-plane tables (and with them larger merged ones); a frame whose K planes together hold more than the limit raises the
// same flag in k_merge_candidates with the sum as the fullest frame's count, which the verdict turns into A3_ERR_LIMIT.
constexpr uint32_t merged_cand_capacity(uint32_t n_windows, uint32_t plane_cand) {
    return (uint64_t)n_windows * plane_cand > A3_MAX_CANDIDATES_PER_FRAME ? (uint32_t)A3_MAX_CANDIDATES_PER_FRAME : n_windows * plane_cand;
}

}  // namespace a3
