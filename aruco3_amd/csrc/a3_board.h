// a3_board.h -- the board-pose pieces of include/aruco3_hip.h (a3_set_board) shared by k_board_pose (k_board.hip) and the ChArUco corner
// pose (k_charuco.hip): board slots, the start's IPPE, the per-corner residual / Jacobian sums, the LDL^T step and the Cayley update.
// Built with -ffp-contract=off: the same inputs give the same bits in either kernel.
#pragma once
#include <cmath>

#include "a3_common.h"
#include "a3_ippe.h"
#include "a3_launch.h"

namespace a3 {

constexpr uint16_t kNoSlot = 0xFFFF;
constexpr int kBoardCache = 4;   // corners per lane held in registers (lane l: l, l + 64, l + 128, l + 192)

struct BoardSlot {   // per board marker, built by a3_set_board (host, float)
    float x[4], y[4];
    float side, cs, sn, cx, cy, pad[3];
};
static_assert(sizeof(BoardSlot) == 64, "BoardSlot is 64 bytes");

struct BoardArgs {
    const a3_marker* markers;     // batch: the compacted marker list; nullptr: stand-alone (ids / pts)
    const uint32_t* ids;          // stand-alone: n ids
    const float* pts;             // stand-alone: 8 float corners per marker, pixels
    const float* refined;         // batch with refinement: 8 floats per marker (nullable)
    const unsigned int* n_dev;    // batch: markers produced
    const uint32_t* per_frame;    // batch: markers per frame
    uint32_t n, n_frames;         // batch: marker capacity; stand-alone: marker count (one frame)
    const uint16_t* slot_of;      // n_codes entries, kNoSlot: not on the board
    uint32_t n_codes;
    const BoardSlot* slots;
    int has_intr;
    float iw, ih, fx, fy, cx, cy;
    a3_board_pose* out;
};

// the kernels' view of a marker source and the board's tables (a3_launch.h); intr == nullptr: normalised by the image size
inline BoardArgs board_args(const MarkerSrc& m, const BoardTables& t, const a3_intrinsics* intr, uint32_t W, uint32_t H) {
    BoardArgs a{};
    a.markers = m.markers; a.ids = m.ids; a.pts = m.pts; a.refined = m.corners; a.n_dev = m.n_dev; a.per_frame = m.per_frame;
    a.n = m.n; a.n_frames = m.n_frames; a.slot_of = t.slot_of; a.n_codes = t.n_codes; a.slots = reinterpret_cast<const BoardSlot*>(t.slots);
    a.has_intr = intr ? 1 : 0; a.iw = (float)W; a.ih = (float)H;
    if (intr) { a.fx = intr->focal_x; a.fy = intr->focal_y; a.cx = intr->principal_x; a.cy = intr->principal_y; }
    return a;
}

struct BoardAcc {
    float h[21], g[6], cost, pix;
};

__device__ __forceinline__ uint32_t board_slot(const BoardArgs& a, uint32_t m) {
    const uint32_t id = a.markers ? a.markers[m].id : a.ids[m];
    return id < a.n_codes ? (uint32_t)a.slot_of[id] : (uint32_t)kNoSlot;
}

// image corner k of marker m in pixels (refined, integer, or the caller's floats)
__device__ __forceinline__ void board_image_px(const BoardArgs& a, uint32_t m, int k, float* x, float* y) {
    if (a.refined) { *x = a.refined[8 * (size_t)m + 2 * k]; *y = a.refined[8 * (size_t)m + 2 * k + 1]; }
    else if (a.markers) { *x = (float)a.markers[m].corners[2 * k]; *y = (float)a.markers[m].corners[2 * k + 1]; }
    else { *x = a.pts[8 * (size_t)m + 2 * k]; *y = a.pts[8 * (size_t)m + 2 * k + 1]; }
}

// as k_pose normalises (modes 0 / 1, 3 / 4)
__device__ __forceinline__ void board_normalise(const BoardArgs& a, float x, float y, float* u, float* v) {
    if (a.has_intr) { *u = (x - a.cx) / a.fx; *v = (y - a.cy) / a.fy; }
    else { *u = x / a.iw; *v = y / a.ih; }
}

__device__ __forceinline__ bool board_dup(const uint32_t* s_dup, uint32_t slot) { return (s_dup[slot >> 5] >> (slot & 31)) & 1u; }

// corner c of the frame (marker first + c / 4, corner c % 4): board point and normalised image point; false when not used
__device__ __forceinline__ bool board_corner(const BoardArgs& a, const uint32_t* s_dup, uint32_t first, uint32_t c, float* bx, float* by,
                                             float* mx, float* my) {
    const uint32_t m = first + (c >> 2);
    const int k = (int)(c & 3u);
    const uint32_t slot = board_slot(a, m);
    if (slot == kNoSlot || board_dup(s_dup, slot)) return false;
    *bx = a.slots[slot].x[k]; *by = a.slots[slot].y[k];
    float x, y;
    board_image_px(a, m, k, &x, &y);
    board_normalise(a, x, y, mx, my);
    return true;
}

__device__ __forceinline__ void board_accum(BoardAcc& s, const float R[9], const float t[3], float bx, float by, float mx, float my,
                                            float sx, float sy) {
    const float qx = R[0] * bx + R[1] * by, qy = R[3] * bx + R[4] * by, qz = R[6] * bx + R[7] * by;
    const float px = qx + t[0], py = qy + t[1], pz = qz + t[2];
    const float zz = pz > 1e-5f ? pz : 1e-5f;
    const float u = px / zz, v = py / zz;
    const float a = 1.0f / zz, a2 = 2.0f * a;
    const float ru = u - mx, rv = v - my;
    const float ju[6] = {-(a2 * u) * qy, a2 * (qz + u * qx), -a2 * qy, a, 0.0f, -(a * u)};
    const float jv[6] = {-a2 * (qz + v * qy), (a2 * v) * qx, a2 * qx, 0.0f, a, -(a * v)};
    int idx = 0;
    for (int r = 0; r < 6; r++) {
        for (int c = r; c < 6; c++) { s.h[idx] += ju[r] * ju[c] + jv[r] * jv[c]; idx++; }
        s.g[r] += ju[r] * ru + jv[r] * rv;
    }
    s.cost += ru * ru + rv * rv;
    const float eu = ru * sx, ev = rv * sy;
    s.pix += eu * eu + ev * ev;
}

__device__ __forceinline__ float wave_sum_f(float v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t wave_sum_u(uint32_t v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// (J^T J + lambda diag(J^T J)) d = -J^T r by LDL^T; false when a pivot is not positive and finite
__device__ __forceinline__ bool board_solve(const float h[21], const float g[6], float lambda, float d[6]) {
    float A[6][6];
    int idx = 0;
    for (int r = 0; r < 6; r++)
        for (int c = r; c < 6; c++) { A[r][c] = h[idx]; A[c][r] = h[idx]; idx++; }
    for (int r = 0; r < 6; r++) A[r][r] = A[r][r] + lambda * A[r][r];
    float L[6][6], D[6];
    for (int j = 0; j < 6; j++) {
        for (int i = j; i < 6; i++) {
            float s = A[i][j];
            for (int k = 0; k < j; k++) s = s - L[i][k] * L[j][k] * D[k];
            if (i == j) {
                if (!(s > 0.0f) || !isfinite(s)) return false;
                D[j] = s;
                L[j][j] = 1.0f;
            } else L[i][j] = s / D[j];
        }
    }
    float y[6];
    for (int i = 0; i < 6; i++) {
        float s = -g[i];
        for (int k = 0; k < i; k++) s = s - L[i][k] * y[k];
        y[i] = s;
    }
    for (int i = 5; i >= 0; i--) {
        float s = y[i] / D[i];
        for (int k = i + 1; k < 6; k++) s = s - L[k][i] * d[k];
        d[i] = s;
    }
    return true;
}

// R <- cay(w) R
__device__ __forceinline__ void board_cayley(const float w[3], const float R[9], float Rn[9]) {
    const float n2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const float k = 2.0f / (1.0f + n2);
    const float W[9] = {0.0f, -w[2], w[1], w[2], 0.0f, -w[0], -w[1], w[0], 0.0f};
    float C[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const float w2 = w[r] * w[c] - (r == c ? n2 : 0.0f);
            C[3 * r + c] = (r == c ? 1.0f : 0.0f) + k * (W[3 * r + c] + w2);
        }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Rn[3 * r + c] = (C[3 * r] * R[c] + C[3 * r + 1] * R[3 + c]) + C[3 * r + 2] * R[6 + c];
}

__device__ __forceinline__ bool pose_finite(const a3_pose& p) {
    bool ok = true;
    for (int q = 0; q < 9; q++) ok = ok && isfinite(p.rotation[q]);
    for (int q = 0; q < 3; q++) ok = ok && isfinite(p.translation[q]);
    return ok;
}

// IPPE of marker m of the frame (normalised as the per-marker poses), with that marker's board side
__device__ __forceinline__ void board_ippe(const BoardArgs& a, uint32_t m, float side, a3_pose* p0, a3_pose* p1) {
    float pts[8];
    for (int k = 0; k < 4; k++) {
        float x, y;
        board_image_px(a, m, k, &x, &y);
        board_normalise(a, x, y, &pts[2 * k], &pts[2 * k + 1]);
    }
    solve_normalized(pts, side, p0, p1);
}

// Levenberg-Marquardt from (R, t) as the contract states it; evaluate(R, t, acc) sums one state over the caller's correspondences
// (wave-uniform result).  -> evaluations; `s` holds the final state's sums.
template <typename Eval>
__device__ __forceinline__ uint32_t board_lm(Eval&& evaluate, float R[9], float t[3], BoardAcc& s) {
    evaluate(R, t, s);
    uint32_t evals = 1;
    float lambda = 1e-3f;
    while (evals < A3_BOARD_MAX_EVALS && s.cost > 0.0f) {
        float d[6];
        if (!board_solve(s.h, s.g, lambda, d)) { lambda = lambda * 10.0f; evals++; continue; }
        float Rn[9], tn[3];
        board_cayley(d, R, Rn);
        for (int r = 0; r < 3; r++) tn[r] = t[r] + d[3 + r];
        BoardAcc s2;
        evaluate(Rn, tn, s2);
        evals++;
        if (s2.cost < s.cost) {
            const float rel = (s.cost - s2.cost) / s.cost;
            for (int q = 0; q < 9; q++) R[q] = Rn[q];
            for (int q = 0; q < 3; q++) t[q] = tn[q];
            s = s2;
            lambda = lambda / 10.0f;
            if (rel < A3_BOARD_REL_TOL) break;
        } else lambda = lambda * 10.0f;
    }
    return evals;
}

}  // namespace a3
