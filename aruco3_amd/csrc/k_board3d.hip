// k_board3d.hip -- one pose per frame of a board whose markers are not coplanar (a3_set_board3d; a3_get_board_poses /
// a3_estimate_board_pose serve it as they serve a planar board).  Not part of the reference: an extension stated in
// include/aruco3_hip.h and restated on the CPU by tests/board3d_oracle.c (a3o_board3d_pose), in the same order of operations.
//
// The shape is k_board_pose's (k_board.hip): one workgroup of two waves per frame, one wave per IPPE start; the frame's markers are a
// contiguous run of the device-resident marker list; duplicate board ids are found with an LDS bitmap over the board slots; a lane
// caches the first kBoardCache corners it owns in registers and re-reads the rest (marker id -> slot -> board corner, image corner)
// on every evaluation; every sum ends in an xor butterfly, so the solve state and the control flow are wave-uniform.  What differs:
// a corner has three board coordinates (Board3Slot), the start carries the marker's IPPE pose through the marker's own frame
// (e_x, e_y, e_z, c) instead of an in-plane rotation, and the sums take q = R (X, Y, Z) (board3_accum).
#include <algorithm>
#include <cmath>

#include "a3_board3d.h"
#include "a3_common.h"
#include "a3_launch.h"

namespace a3 {

__global__ __launch_bounds__(128) void k_board3d_pose(BoardArgs a) {
    __shared__ uint32_t s_seen[A3_BOARD_MAX_MARKERS / 32], s_dup[A3_BOARD_MAX_MARKERS / 32];
    __shared__ float s_res[2][16];   // per start: R (9), t (3), cost, pixel cost, evaluations (as bits)
    const uint32_t f = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const Board3Slot* const slots = board3_slots(a);
    // ---- the frame's run of the marker list (both waves) ----
    uint32_t first = 0, cnt = a.n;
    if (a.markers) {
        uint32_t before = 0;
        for (uint32_t g = (uint32_t)lane; g < f; g += 64) before += a.per_frame[g];
        first = wave_sum_u(before);
        const uint32_t limit = min(a.n, *a.n_dev);
        cnt = first >= limit ? 0u : min(a.per_frame[f], limit - first);
    }
    if (threadIdx.x < A3_BOARD_MAX_MARKERS / 32) { s_seen[threadIdx.x] = 0; s_dup[threadIdx.x] = 0; }
    __syncthreads();
    if (wave == 0)
        for (uint32_t i = (uint32_t)lane; i < cnt; i += 64) {
            const uint32_t slot = board_slot(a, first + i);
            if (slot == kNoSlot) continue;
            const uint32_t bit = 1u << (slot & 31);
            if (atomicOr(&s_seen[slot >> 5], bit) & bit) atomicOr(&s_dup[slot >> 5], bit);
        }
    __syncthreads();
    // ---- counts and the start marker: the largest image quad whose IPPE poses are finite, then the lowest slot (both waves) ----
    uint32_t used = 0, rejected = 0, best_i = 0;
    unsigned long long best_key = 0;
    for (uint32_t i = (uint32_t)lane; i < cnt; i += 64) {
        const uint32_t slot = board_slot(a, first + i);
        if (slot == kNoSlot) continue;
        if (board_dup(s_dup, slot)) { rejected++; continue; }
        used++;
        float x[4], y[4];
        for (int k = 0; k < 4; k++) board_image_px(a, first + i, k, &x[k], &y[k]);
        float s = 0.0f;
        for (int k = 0; k < 4; k++) { const int k1 = (k + 1) & 3; s = s + (x[k] * y[k1] - x[k1] * y[k]); }
        const float area = 0.5f * fabsf(s);
        const unsigned long long key = ((unsigned long long)__float_as_uint(area) << 32) | (unsigned long long)(0xFFFFu - slot);
        if (key > best_key) {
            a3_pose q0, q1;
            board_ippe(a, first + i, slots[slot].side, &q0, &q1);
            if (pose_finite(q0) && pose_finite(q1)) { best_key = key; best_i = i; }
        }
    }
    used = wave_sum_u(used);
    rejected = wave_sum_u(rejected);
    unsigned long long top = best_key;
    for (int o = 32; o >= 1; o >>= 1) { const unsigned long long v = __shfl_xor(top, o); top = v > top ? v : top; }
    if (top) {   // (uniform over the workgroup)
        const unsigned long long owners = __ballot(best_key == top);
        const uint32_t mi = first + (uint32_t)__shfl((int)best_i, (int)__builtin_ctzll(owners));
        const Board3Slot& bs = slots[0xFFFFu - (uint32_t)(top & 0xFFFFu)];
        a3_pose p[2];
        board_ippe(a, mi, bs.side, &p[0], &p[1]);
        const a3_pose& pm = wave ? p[1] : p[0];
        const float sx = a.has_intr ? a.fx : a.iw, sy = a.has_intr ? a.fy : a.ih;
        // ---- the lane's cached corners ----
        float cb[kBoardCache][3], cmx[kBoardCache], cmy[kBoardCache];
        bool cok[kBoardCache];
        for (int j = 0; j < kBoardCache; j++) {
            const uint32_t c = (uint32_t)lane + 64u * (uint32_t)j;
            cok[j] = c < 4 * cnt && board3_corner(a, s_dup, first, c, cb[j], &cmx[j], &cmy[j]);
        }
        auto evaluate = [&](const float R[9], const float t[3], BoardAcc& s) {
            for (int q = 0; q < 21; q++) s.h[q] = 0.0f;
            for (int q = 0; q < 6; q++) s.g[q] = 0.0f;
            s.cost = 0.0f; s.pix = 0.0f;
            for (int j = 0; j < kBoardCache; j++)
                if (cok[j]) board3_accum(s, R, t, cb[j], cmx[j], cmy[j], sx, sy);
            for (uint32_t c = (uint32_t)lane + 64u * kBoardCache; c < 4 * cnt; c += 64) {
                float b[3], mx, my;
                if (board3_corner(a, s_dup, first, c, b, &mx, &my)) board3_accum(s, R, t, b, mx, my, sx, sy);
            }
            for (int q = 0; q < 21; q++) s.h[q] = wave_sum_f(s.h[q]);
            for (int q = 0; q < 6; q++) s.g[q] = wave_sum_f(s.g[q]);
            s.cost = wave_sum_f(s.cost);
            s.pix = wave_sum_f(s.pix);
        };
        // ---- this wave's start, carried through the start marker's frame into the board's, then Levenberg-Marquardt ----
        float R[9], t[3];
        const float* Rm = pm.rotation;
        for (int r = 0; r < 3; r++)
            for (int j = 0; j < 3; j++) R[3 * r + j] = (Rm[3 * r] * bs.ex[j] + Rm[3 * r + 1] * bs.ey[j]) + Rm[3 * r + 2] * bs.ez[j];
        for (int r = 0; r < 3; r++) t[r] = pm.translation[r] - ((R[3 * r] * bs.c[0] + R[3 * r + 1] * bs.c[1]) + R[3 * r + 2] * bs.c[2]);
        BoardAcc s;
        const uint32_t evals = board_lm(evaluate, R, t, s);
        if (lane == 0) {
            for (int q = 0; q < 9; q++) s_res[wave][q] = R[q];
            for (int q = 0; q < 3; q++) s_res[wave][9 + q] = t[q];
            s_res[wave][12] = s.cost; s_res[wave][13] = s.pix; s_res[wave][14] = __uint_as_float(evals);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        a3_board_pose rec{};
        rec.markers_used = used;
        rec.markers_rejected = rejected;
        if (top) {
            const int k = s_res[1][12] < s_res[0][12] ? 1 : 0;   // (ties: the first IPPE pose)
            const float nc = (float)(4u * used);
            rec.status = A3_BOARD_OK;
            rec.iterations = __float_as_uint(s_res[k][14]);
            rec.rms_px = sqrtf(s_res[k][13] / nc);
            rec.alt_rms_px = sqrtf(s_res[1 - k][13] / nc);
            for (int q = 0; q < 9; q++) rec.rotation[q] = s_res[k][q];
            for (int q = 0; q < 3; q++) rec.translation[q] = s_res[k][9 + q];
        }
        a.out[f] = rec;
    }
}

size_t board3d_slot_bytes() { return sizeof(Board3Slot); }

// (the contract's float arithmetic; tests/board3d_oracle.c a3o_board3d_slot)
void board3d_slot_from(const float xyz[12], void* out) {
    Board3Slot s{};
    for (int k = 0; k < 4; k++) { s.x[k] = xyz[3 * k]; s.y[k] = xyz[3 * k + 1]; s.z[k] = xyz[3 * k + 2]; }
    const float d[3] = {s.x[1] - s.x[0], s.y[1] - s.y[0], s.z[1] - s.z[0]};
    s.side = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    for (int j = 0; j < 3; j++) s.ex[j] = d[j] / s.side;
    const float v[3] = {s.x[0] - s.x[3], s.y[0] - s.y[3], s.z[0] - s.z[3]};
    const float k = (v[0] * s.ex[0] + v[1] * s.ex[1]) + v[2] * s.ex[2];
    float w[3];
    for (int j = 0; j < 3; j++) w[j] = v[j] - k * s.ex[j];
    const float wn = sqrtf((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    for (int j = 0; j < 3; j++) s.ey[j] = w[j] / wn;
    s.ez[0] = s.ex[1] * s.ey[2] - s.ex[2] * s.ey[1];
    s.ez[1] = s.ex[2] * s.ey[0] - s.ex[0] * s.ey[2];
    s.ez[2] = s.ex[0] * s.ey[1] - s.ex[1] * s.ey[0];
    s.c[0] = 0.25f * ((s.x[0] + s.x[1]) + (s.x[2] + s.x[3]));
    s.c[1] = 0.25f * ((s.y[0] + s.y[1]) + (s.y[2] + s.y[3]));
    s.c[2] = 0.25f * ((s.z[0] + s.z[1]) + (s.z[2] + s.z[3]));
    *reinterpret_cast<Board3Slot*>(out) = s;
}

hipError_t launch_board3d_pose(hipStream_t st, const BoardPoseLaunch& b) {
    if (b.board.slot_kind != kBoardSlots3D) return hipErrorInvalidValue;   // (planar BoardSlot records are half the size)
    if (b.m.n_frames == 0) return hipSuccess;
    BoardArgs a = board_args(b.m, b.board, b.intr, b.W, b.H);
    a.out = b.out;
    hipLaunchKernelGGL(k_board3d_pose, dim3(b.m.n_frames), dim3(128), 0, st, a);
    return hipGetLastError();
}

}  // namespace a3
