// Argument checks of boards, planar (a3_set_board) and 3-D (a3_set_board3d): the validity test of one marker's eight or twelve floats,
// each call's own refusals, and the refusals of the settings that need a plane while a 3-D board is set (a3_set_charuco,
// a3_set_board_recovery, a3_recover_markers: a homography places the chessboard and the missing markers).  Host arithmetic on plain values -- no HIP, no context -- so a plain C++
// program can run every check (tests/board3d_checks.cpp).  Each check returns the message of the FIRST test that fails, or nullptr.
// Every message is a whole string literal (as a3_windows_check.h).
#pragma once
#include <cmath>
#include <cstddef>
#include <cstdint>

#include "../../include/aruco3_hip.h"

namespace a3 {

constexpr double kBoardSquareTol = 1e-3;   // relative to the side, for both kinds of board (SQUARE_TOL of aruco3_amd/board.py)

// One planar marker: corners X0..X3 (x, y each) in the order top-left, top-right, bottom-right, bottom-left with y up.  In f64 on the
// floats, with e_k = X_(k+1) - X_k and s = |e_0|: all finite; s > 0; every | |e_k| - s | <= tol s; every |e_k . e_(k+1)| <= tol s^2;
// e_0 x e_1 < 0 (the winding).
inline const char* check_board_marker(const float c[8]) {
    for (int k = 0; k < 8; k++)
        if (!std::isfinite(c[k])) return "a3_set_board: a corner is not finite";
    double ex[4], ey[4];
    for (int k = 0; k < 4; k++) { ex[k] = (double)c[2 * ((k + 1) & 3)] - c[2 * k]; ey[k] = (double)c[2 * ((k + 1) & 3) + 1] - c[2 * k + 1]; }
    const double s = std::sqrt(ex[0] * ex[0] + ey[0] * ey[0]);
    if (!(s > 0.0)) return "a3_set_board: a marker has no size";
    for (int k = 0; k < 4; k++) {
        const int k1 = (k + 1) & 3;
        if (std::fabs(std::sqrt(ex[k] * ex[k] + ey[k] * ey[k]) - s) > kBoardSquareTol * s)
            return "a3_set_board: a marker's sides differ (its corners must form a square)";
        if (std::fabs(ex[k] * ex[k1] + ey[k] * ey[k1]) > kBoardSquareTol * s * s)
            return "a3_set_board: a marker's corners are not at right angles (they must form a square)";
    }
    if (!(ex[0] * ey[1] - ey[0] * ex[1] < 0.0))
        return "a3_set_board: a marker is wound the wrong way (corner order top-left, top-right, bottom-right, bottom-left with y up)";
    return nullptr;
}

// a3_set_board(ctx, ids, corners_xy, n), behind its null-context test.  n = 0 clears the board and passes.  The ids (in the dictionary,
// no repeats) and each marker are checked by the setters' shared loop.
inline const char* check_board_call(const uint32_t* ids, const float* corners_xy, size_t n) {
    if (n > A3_BOARD_MAX_MARKERS) return "a3_set_board: more than A3_BOARD_MAX_MARKERS markers";
    if (n && (!ids || !corners_xy)) return "a3_set_board: null ids or corners";
    return nullptr;
}

// One 3-D marker: corners X0..X3 (x, y, z each) in the order top-left, top-right, bottom-right, bottom-left as seen from the printed side.
// In f64 on the floats, with e_k = X_(k+1) - X_k and s = |e_0|: all finite; s > 0; every | |e_k| - s | <= tol s; every
// |e_k . e_(k+1)| <= tol s^2; |X2 - (X1 + X3 - X0)| <= tol s (planar, and a parallelogram).
inline const char* check_board3d_marker(const float c[12]) {
    for (int k = 0; k < 12; k++)
        if (!std::isfinite(c[k])) return "a3_set_board3d: a corner is not finite";
    double e[4][3];
    for (int k = 0; k < 4; k++)
        for (int j = 0; j < 3; j++) e[k][j] = (double)c[3 * ((k + 1) & 3) + j] - (double)c[3 * k + j];
    auto dot = [](const double a[3], const double b[3]) { return (a[0] * b[0] + a[1] * b[1]) + a[2] * b[2]; };
    const double s = std::sqrt(dot(e[0], e[0]));
    if (!(s > 0.0)) return "a3_set_board3d: a marker has no size";
    for (int k = 0; k < 4; k++) {
        const int k1 = (k + 1) & 3;
        if (std::fabs(std::sqrt(dot(e[k], e[k])) - s) > kBoardSquareTol * s)
            return "a3_set_board3d: a marker's sides differ (its corners must form a square)";
        if (std::fabs(dot(e[k], e[k1])) > kBoardSquareTol * s * s)
            return "a3_set_board3d: a marker's corners are not at right angles (they must form a square)";
    }
    double g[3];
    for (int j = 0; j < 3; j++) g[j] = (double)c[6 + j] - (((double)c[3 + j] + (double)c[9 + j]) - (double)c[j]);
    if (std::sqrt(dot(g, g)) > kBoardSquareTol * s) return "a3_set_board3d: a marker's corners do not lie in one plane (they must form a square)";
    return nullptr;
}

// a3_set_board3d(ctx, ids, corners_xyz, n), behind its null-context test; busy: a submitted batch has not been collected.  n = 0 clears
// the board and passes.  The ids and each marker: as a3_set_board's.
inline const char* check_board3d_call(bool busy, const uint32_t* ids, const float* corners_xyz, size_t n) {
    if (busy) return "a3_set_board3d: a submitted batch has not been collected";
    if (n > A3_BOARD_MAX_MARKERS) return "a3_set_board3d: more than A3_BOARD_MAX_MARKERS markers";
    if (n && (!ids || !corners_xyz)) return "a3_set_board3d: null ids or corners";
    return nullptr;
}

// the settings that need a plane, asked for while the board that is set is (board3d) a 3-D one; clearing them always passes
inline const char* check_charuco_board_kind(bool board3d, size_t n_corners) {
    return board3d && n_corners ? "a3_set_charuco: the board is a 3-D board (a3_set_board3d); ChArUco needs a planar one (a3_set_board)" : nullptr;
}
inline const char* check_recovery_board_kind(bool board3d, uint32_t mode) {
    return board3d && mode ? "a3_set_board_recovery: the board is a 3-D board (a3_set_board3d); recovery needs a planar one (a3_set_board)" : nullptr;
}
inline const char* check_recover_markers_board_kind(bool board3d) {
    return board3d ? "a3_recover_markers: the board is a 3-D board (a3_set_board3d); recovery needs a planar one (a3_set_board)" : nullptr;
}

}  // namespace a3
