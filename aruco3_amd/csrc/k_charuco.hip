// k_charuco.hip -- ChArUco chessboard corners and their board pose (a3_set_charuco / a3_get_charuco_corners / a3_get_charuco_poses /
// a3_interpolate_charuco).  Not part of the reference: an extension stated in include/aruco3_hip.h and restated on the CPU by
// tests/charuco_oracle.c, which these kernels match bit for bit.
//
// Three launches, all behind the marker list of a batch (or a stand-alone call's caller markers, one frame):
//   k_charuco_interp   one workgroup per frame: the frame's run of the marker list (the sum of per_frame before it, as k_board_pose),
//                      the duplicate rule on an LDS bitmap, one homography per used marker (one lane each, kept in LDS by board slot),
//                      then one lane per chessboard corner; the reported corners are compacted in id order by ballot prefix sums into
//                      the frame's own slot array (frame f: slots f * n_corners ...), with the frame's count -- no atomics, no races;
//   k_charuco_refine   one wave per reported corner, four per workgroup (grid: corner quads x frames): the frame's output offset is
//                      the sum of the counts before it; the wave refines its corner (a3_subpix.h) and writes the record at offset +
//                      rank, so the records come out ordered by (frame, id); the workgroup of the last frame also writes the total;
//   k_charuco_pose     two waves per frame, one per IPPE start, as k_board_pose: the start from the board markers, then the
//                      Levenberg-Marquardt of a3_board.h over the frame's records.
// Per-frame slot arrays and a second launch, rather than a prefix over frames inside k_charuco_interp: the refinement wants one wave
// per corner anyway, and that launch can take the frame offsets once every frame's count is final.
#include <algorithm>
#include <cmath>

#include "a3_board.h"
#include "a3_common.h"
#include "a3_launch.h"
#include "a3_subpix.h"
#include "a3_undistort.h"

namespace a3 {

constexpr uint32_t kNoAdj = 0xFFFFFFFFu;

struct CharucoArgs {
    const float* cxy;             // 2 floats per chessboard corner, board units
    const uint32_t* adj;          // 4 adjacent marker ids per corner, kNoAdj = none
    uint32_t nc;                  // chessboard corners
    uint32_t W, H, min_markers, refine;
    PixelSrc src;                 // what the refinement samples
    a3_charuco_corner* slots;     // n_frames x nc: each frame's reported corners, id order
    uint32_t* counts;             // n_frames + 1: reported corners per frame, then the total
    a3_charuco_corner* out;       // the records, ordered by (frame, id)
    float* und;                   // nullable: 2 floats per record, the undistorted pixel corner (pose batches with a distortion)
    UndistortParams up;
};

// imageproc's from_control_points from board marker corners `from` to image corners `to`, the decode stage's LU (k_decode.hip
// solve_projection, whose `to` is fixed there) -> the f32 matrix h0 .. h7 (h8 = 1); false when singular or without an inverse
__device__ bool charuco_homography(const float* from, const float* to, float h[8]) {
    double A[8][8], b[8];
    for (int i = 0; i < 4; i++) {
        const double xf = from[2 * i], yf = from[2 * i + 1], x = to[2 * i], y = to[2 * i + 1];
        A[2 * i][0] = 0.0; A[2 * i][1] = 0.0; A[2 * i][2] = 0.0; A[2 * i][3] = -xf; A[2 * i][4] = -yf; A[2 * i][5] = -1.0;
        A[2 * i][6] = y * xf; A[2 * i][7] = y * yf;
        A[2 * i + 1][0] = xf; A[2 * i + 1][1] = yf; A[2 * i + 1][2] = 1.0; A[2 * i + 1][3] = 0.0; A[2 * i + 1][4] = 0.0; A[2 * i + 1][5] = 0.0;
        A[2 * i + 1][6] = -x * xf; A[2 * i + 1][7] = -x * yf;
        b[2 * i] = -y; b[2 * i + 1] = x;
    }
#pragma unroll
    for (int i = 0; i < 8; i++) {
        int piv = i; double best = fabs(A[i][i]);
#pragma unroll
        for (int r = i + 1; r < 8; r++) { const double v = fabs(A[r][i]); if (v > best) { best = v; piv = r; } }
        double diag = A[i][i];
#pragma unroll
        for (int r = i + 1; r < 8; r++) diag = piv == r ? A[r][i] : diag;
        if (diag == 0.0) continue;
#pragma unroll
        for (int r = i + 1; r < 8; r++) {
            const bool sw = piv == r;
#pragma unroll
            for (int c = 0; c < 8; c++) { const double x = A[i][c], y = A[r][c]; A[i][c] = sw ? y : x; A[r][c] = sw ? x : y; }
            const double x = b[i], y = b[r]; b[i] = sw ? y : x; b[r] = sw ? x : y;
        }
        const double inv_diag = 1.0 / diag;
#pragma unroll
        for (int r = i + 1; r < 8; r++) A[r][i] *= inv_diag;
#pragma unroll
        for (int c = i + 1; c < 8; c++) {
            const double pr = -A[i][c];
#pragma unroll
            for (int r = i + 1; r < 8; r++) A[r][c] = pr * A[r][i] + A[r][c];
        }
    }
#pragma unroll
    for (int i = 0; i < 7; i++) {
        const double coeff = -b[i];
#pragma unroll
        for (int r = i + 1; r < 8; r++) b[r] = coeff * A[r][i] + b[r];
    }
    bool singular = false;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        const double diag = A[i][i];
        if (diag == 0.0) singular = true;
        const double coeff = b[i] / diag;
        b[i] = coeff;
        const double nc = -coeff;
#pragma unroll
        for (int r = 0; r < i; r++) b[r] = nc * A[r][i] + b[r];
    }
    if (singular) return false;
    for (int i = 0; i < 8; i++) h[i] = (float)b[i];
    const float t00 = h[0], t01 = h[1], t02 = h[2], t10 = h[3], t11 = h[4], t12 = h[5], t20 = h[6], t21 = h[7], t22 = 1.0f;
    const float m00 = t11 * t22 - t12 * t21;
    const float m01 = t10 * t22 - t12 * t20;
    const float m02 = t10 * t21 - t11 * t20;
    const float det = t00 * m00 - t01 * m01 + t02 * m02;
    return !(fabsf(det) < 1e-10f);
}

// the frame's run of the marker list: first index and count (every lane of every wave gets the same)
__device__ __forceinline__ void charuco_frame_run(const BoardArgs& a, uint32_t f, int lane, uint32_t* first, uint32_t* cnt) {
    *first = 0; *cnt = a.n;
    if (a.markers) {
        uint32_t before = 0;
        for (uint32_t g = (uint32_t)lane; g < f; g += 64) before += a.per_frame[g];
        *first = wave_sum_u(before);
        const uint32_t limit = min(a.n, *a.n_dev);
        *cnt = *first >= limit ? 0u : min(a.per_frame[f], limit - *first);
    }
}

__global__ __launch_bounds__(256) void k_charuco_interp(BoardArgs a, CharucoArgs c, RefineParams p) {
    __shared__ uint32_t s_seen[A3_BOARD_MAX_MARKERS / 32], s_dup[A3_BOARD_MAX_MARKERS / 32];
    __shared__ float s_h[A3_BOARD_MAX_MARKERS][8];      // homography of the slot's marker
    __shared__ uint32_t s_mi[A3_BOARD_MAX_MARKERS];     // the slot's marker (index into the marker list); kNoAdj: none with a homography
    __shared__ uint32_t s_wave[4];
    const uint32_t f = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint32_t first, cnt;
    charuco_frame_run(a, f, lane, &first, &cnt);
    if (tid < A3_BOARD_MAX_MARKERS / 32) { s_seen[tid] = 0; s_dup[tid] = 0; }
    for (int s = tid; s < A3_BOARD_MAX_MARKERS; s += 256) s_mi[s] = kNoAdj;
    __syncthreads();
    for (uint32_t i = (uint32_t)tid; i < cnt; i += 256) {
        const uint32_t slot = board_slot(a, first + i);
        if (slot == kNoSlot) continue;
        const uint32_t bit = 1u << (slot & 31);
        if (atomicOr(&s_seen[slot >> 5], bit) & bit) atomicOr(&s_dup[slot >> 5], bit);
    }
    __syncthreads();
    for (uint32_t i = (uint32_t)tid; i < cnt; i += 256) {   // (a slot not duplicated belongs to one marker: one writer)
        const uint32_t slot = board_slot(a, first + i);
        if (slot == kNoSlot || board_dup(s_dup, slot)) continue;
        float from[8], to[8], h[8];
        for (int k = 0; k < 4; k++) {
            from[2 * k] = a.slots[slot].x[k]; from[2 * k + 1] = a.slots[slot].y[k];
            board_image_px(a, first + i, k, &to[2 * k], &to[2 * k + 1]);
        }
        if (charuco_homography(from, to, h)) {
            for (int q = 0; q < 8; q++) s_h[slot][q] = h[q];
            s_mi[slot] = first + i;
        }
    }
    __syncthreads();
    uint32_t running = 0;
    for (uint32_t base = 0; base < c.nc; base += 256) {   // (uniform over the workgroup: the barriers below are safe)
        const uint32_t k = base + (uint32_t)tid;
        bool keep = false;
        a3_charuco_corner rec{};
        if (k < c.nc) {
            const float X = c.cxy[2 * k], Y = c.cxy[2 * k + 1];
            float sx = 0.0f, sy = 0.0f;
            uint32_t used = 0, slots[4];
            for (int j = 0; j < 4; j++) {
                const uint32_t id = c.adj[4 * k + j];
                if (id == kNoAdj || id >= a.n_codes) continue;
                const uint32_t slot = a.slot_of[id];
                if (slot == kNoSlot || s_mi[slot] == kNoAdj) continue;
                const float* h = s_h[slot];
                const float den = (h[6] * X + h[7] * Y) + 1.0f;
                sx = sx + ((h[0] * X + h[1] * Y) + h[2]) / den;
                sy = sy + ((h[3] * X + h[4] * Y) + h[5]) / den;
                slots[used++] = slot;
            }
            if (used >= c.min_markers) {   // (min_markers >= 1)
                const float ix = sx / (float)used, iy = sy / (float)used;
                if (ix >= 0.0f && ix <= (float)(c.W - 1) && iy >= 0.0f && iy <= (float)(c.H - 1)) {   // (false for NaN)
                    keep = true;
                    rec.frame = f; rec.id = k;
                    rec.x = ix; rec.y = iy; rec.interp_x = ix; rec.interp_y = iy;
                    rec.markers_used = used;
                    if (c.refine) {
                        float d = __builtin_inff();
                        for (uint32_t j = 0; j < used; j++)
                            for (int q = 0; q < 4; q++) {
                                float x, y;
                                board_image_px(a, s_mi[slots[j]], q, &x, &y);
                                const float dx = x - ix, dy = y - iy;
                                const float dist = sqrtf(dx * dx + dy * dy);
                                if (dist < d) d = dist;
                            }
                        rec.window = (uint32_t)refine_window(p, d);
                    }
                }
            }
        }
        const unsigned long long m = __ballot(keep);
        if (lane == 0) s_wave[wave] = (uint32_t)__popcll(m);
        __syncthreads();
        uint32_t off = running;
        for (int q = 0; q < wave; q++) off += s_wave[q];
        if (keep) c.slots[(size_t)f * c.nc + off + (uint32_t)__popcll(m & ((1ull << lane) - 1ull))] = rec;
        running += (s_wave[0] + s_wave[1]) + (s_wave[2] + s_wave[3]);
        __syncthreads();   // (s_wave is rewritten by the next round)
    }
    if (tid == 0) c.counts[f] = running;
}

__global__ __launch_bounds__(256) void k_charuco_refine(CharucoArgs c, RefineParams p, uint32_t n_frames) {
    __shared__ uint8_t s_tile[4][kRefineTile * kRefineTile];
    __shared__ float s_g[4][2 * kRefineMaxWin + 1];
    const uint32_t f = blockIdx.y;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t before = 0;
    for (uint32_t g = (uint32_t)lane; g < f; g += 64) before += c.counts[g];
    before = wave_sum_u(before);
    const uint32_t cnt = c.counts[f];
    if (blockIdx.x == 0 && f == n_frames - 1 && threadIdx.x == 0) c.counts[n_frames] = before + cnt;
    if (blockIdx.x * 4u >= cnt) return;   // (uniform over the workgroup)
    const uint32_t k = blockIdx.x * 4u + (uint32_t)wave;
    const bool live = k < cnt;
    a3_charuco_corner rec{};
    if (live) rec = c.slots[(size_t)f * c.nc + k];
    if (c.refine) {
        const int w = (int)rec.window;
        const int T = 4 * w + 6;
        const int ox = (int)floorf(rec.interp_x) - 2 * w - 2, oy = (int)floorf(rec.interp_y) - 2 * w - 2;
        if (live) subpix_load_tile(c.src, c.src.base + (size_t)f * c.src.frame_stride, c.W, c.H, T, ox, oy, p, w, lane, s_tile[wave], s_g[wave]);
        __syncthreads();
        if (live) {
            const float2 q = subpix_iterate(s_tile[wave], T, ox, oy, s_g[wave], w, rec.interp_x, rec.interp_y, p, p.min_shift * p.min_shift, lane);
            rec.x = q.x; rec.y = q.y;
        }
    }
    if (live && lane == 0) {
        const size_t r = (size_t)before + k;
        c.out[r] = rec;
        if (c.und) {
            float x, y, res;
            undistort_corner(c.up, rec.x, rec.y, &x, &y, &res);
            c.und[2 * r] = x; c.und[2 * r + 1] = y;
        }
    }
}

// Two waves per frame, one per IPPE start: the start exactly as k_board_pose takes it, then a3_board.h's LM over the frame's records.
__global__ __launch_bounds__(128) void k_charuco_pose(BoardArgs a, CharucoArgs c, a3_charuco_pose* out) {
    __shared__ uint32_t s_seen[A3_BOARD_MAX_MARKERS / 32], s_dup[A3_BOARD_MAX_MARKERS / 32];
    __shared__ float s_res[2][16];   // per start: R (9), t (3), cost, pixel cost, evaluations (as bits)
    const uint32_t f = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    uint32_t first, cnt;
    charuco_frame_run(a, f, lane, &first, &cnt);
    uint32_t roff = 0;   // the frame's records
    for (uint32_t g = (uint32_t)lane; g < f; g += 64) roff += c.counts[g];
    roff = wave_sum_u(roff);
    const uint32_t ncorn = c.counts[f];
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
    // ---- the start marker: the largest image quad whose IPPE poses are finite, then the lowest slot ----
    uint32_t best_i = 0;
    unsigned long long best_key = 0;
    for (uint32_t i = (uint32_t)lane; i < cnt; i += 64) {
        const uint32_t slot = board_slot(a, first + i);
        if (slot == kNoSlot || board_dup(s_dup, slot)) continue;
        float x[4], y[4];
        for (int k = 0; k < 4; k++) board_image_px(a, first + i, k, &x[k], &y[k]);
        float s = 0.0f;
        for (int k = 0; k < 4; k++) { const int k1 = (k + 1) & 3; s = s + (x[k] * y[k1] - x[k1] * y[k]); }
        const float area = 0.5f * fabsf(s);
        const unsigned long long key = ((unsigned long long)__float_as_uint(area) << 32) | (unsigned long long)(0xFFFFu - slot);
        if (key > best_key) {
            a3_pose q0, q1;
            board_ippe(a, first + i, a.slots[slot].side, &q0, &q1);
            if (pose_finite(q0) && pose_finite(q1)) { best_key = key; best_i = i; }
        }
    }
    unsigned long long top = best_key;
    for (int o = 32; o >= 1; o >>= 1) { const unsigned long long v = __shfl_xor(top, o); top = v > top ? v : top; }
    const bool solve = top && ncorn >= 4;   // (uniform over the workgroup)
    if (solve) {
        const unsigned long long owners = __ballot(best_key == top);
        const uint32_t mi = first + (uint32_t)__shfl((int)best_i, (int)__builtin_ctzll(owners));
        const BoardSlot& bs = a.slots[0xFFFFu - (uint32_t)(top & 0xFFFFu)];
        a3_pose pp[2];
        board_ippe(a, mi, bs.side, &pp[0], &pp[1]);
        const a3_pose& pm = wave ? pp[1] : pp[0];
        const float sx = a.has_intr ? a.fx : a.iw, sy = a.has_intr ? a.fy : a.ih;
        // the record r of the frame: board point and normalised image point
        auto corner = [&](uint32_t r, float* bx, float* by, float* mx, float* my) {
            const a3_charuco_corner& rec = c.out[roff + r];
            *bx = c.cxy[2 * rec.id]; *by = c.cxy[2 * rec.id + 1];
            const float x = c.und ? c.und[2 * ((size_t)roff + r)] : rec.x, y = c.und ? c.und[2 * ((size_t)roff + r) + 1] : rec.y;
            board_normalise(a, x, y, mx, my);
        };
        float cbx[kBoardCache], cby[kBoardCache], cmx[kBoardCache], cmy[kBoardCache];
        for (int j = 0; j < kBoardCache; j++) {
            const uint32_t r = (uint32_t)lane + 64u * (uint32_t)j;
            if (r < ncorn) corner(r, &cbx[j], &cby[j], &cmx[j], &cmy[j]);
        }
        auto evaluate = [&](const float R[9], const float t[3], BoardAcc& s) {
            for (int q = 0; q < 21; q++) s.h[q] = 0.0f;
            for (int q = 0; q < 6; q++) s.g[q] = 0.0f;
            s.cost = 0.0f; s.pix = 0.0f;
            for (int j = 0; j < kBoardCache; j++)
                if ((uint32_t)lane + 64u * (uint32_t)j < ncorn) board_accum(s, R, t, cbx[j], cby[j], cmx[j], cmy[j], sx, sy);
            for (uint32_t r = (uint32_t)lane + 64u * kBoardCache; r < ncorn; r += 64) {
                float bx, by, mx, my;
                corner(r, &bx, &by, &mx, &my);
                board_accum(s, R, t, bx, by, mx, my, sx, sy);
            }
            for (int q = 0; q < 21; q++) s.h[q] = wave_sum_f(s.h[q]);
            for (int q = 0; q < 6; q++) s.g[q] = wave_sum_f(s.g[q]);
            s.cost = wave_sum_f(s.cost);
            s.pix = wave_sum_f(s.pix);
        };
        float R[9], t[3];
        const float* Rm = pm.rotation;
        for (int r = 0; r < 3; r++) {
            R[3 * r] = Rm[3 * r] * bs.cs - Rm[3 * r + 1] * bs.sn;
            R[3 * r + 1] = Rm[3 * r] * bs.sn + Rm[3 * r + 1] * bs.cs;
            R[3 * r + 2] = Rm[3 * r + 2];
        }
        for (int r = 0; r < 3; r++) t[r] = pm.translation[r] - (R[3 * r] * bs.cx + R[3 * r + 1] * bs.cy);
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
        a3_charuco_pose rec{};
        rec.corners_used = ncorn;
        if (solve) {
            const int k = s_res[1][12] < s_res[0][12] ? 1 : 0;   // (ties: the first IPPE pose)
            const float nc = (float)ncorn;
            rec.status = A3_BOARD_OK;
            rec.iterations = __float_as_uint(s_res[k][14]);
            rec.rms_px = sqrtf(s_res[k][13] / nc);
            rec.alt_rms_px = sqrtf(s_res[1 - k][13] / nc);
            for (int q = 0; q < 9; q++) rec.rotation[q] = s_res[k][q];
            for (int q = 0; q < 3; q++) rec.translation[q] = s_res[k][9 + q];
        }
        out[f] = rec;
    }
}

hipError_t launch_charuco_corners(hipStream_t st, const CharucoCornersLaunch& l) {
    const uint32_t n_frames = l.m.n_frames, nc = l.board.nc;
    const a3_intrinsics* const intr = l.intr; const a3_distortion* const dist = l.dist;
    if (n_frames == 0 || nc == 0) return hipSuccess;
    const BoardArgs a = board_args(l.m, l.board, nullptr, 0, 0);
    CharucoArgs c{};
    c.cxy = l.board.cxy; c.adj = l.board.adj; c.nc = nc; c.W = l.W; c.H = l.H; c.min_markers = l.min_markers; c.refine = l.refine; c.src = l.src;
    c.slots = l.slots_tmp; c.counts = l.counts; c.out = l.out;
    if (l.und && intr && dist) {
        c.und = l.und;
        c.up = UndistortParams{intr->focal_x, intr->focal_y, intr->principal_x, intr->principal_y, dist->k1, dist->k2, dist->p1, dist->p2,
                               dist->k3, dist->k4, dist->k5, dist->k6, dist->max_residual_px, dist->iterations, dist->model};
    }
    const RefineParams& p = *reinterpret_cast<const RefineParams*>(l.params);
    hipLaunchKernelGGL(k_charuco_interp, dim3(n_frames), dim3(256), 0, st, a, c, p);
    hipLaunchKernelGGL(k_charuco_refine, dim3((nc + 3) / 4, n_frames), dim3(256), 0, st, c, p, n_frames);
    return hipGetLastError();
}

hipError_t launch_charuco_pose(hipStream_t st, const CharucoPoseLaunch& l) {
    if (l.m.n_frames == 0) return hipSuccess;
    const BoardArgs a = board_args(l.m, l.board, l.intr, l.W, l.H);
    CharucoArgs c{};
    c.cxy = l.board.cxy; c.nc = l.board.nc; c.counts = const_cast<uint32_t*>(l.counts); c.out = const_cast<a3_charuco_corner*>(l.recs); c.und = const_cast<float*>(l.und);
    hipLaunchKernelGGL(k_charuco_pose, dim3(l.m.n_frames), dim3(128), 0, st, a, c, l.out);
    return hipGetLastError();
}

}  // namespace a3
