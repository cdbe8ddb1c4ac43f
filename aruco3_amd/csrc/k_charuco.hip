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
//   k_charuco_pose     a3_board.h's board_pose_body with the record model (CharucoRecords): the start from the board markers as
//                      k_board_pose takes it, then the Levenberg-Marquardt over the frame's records.
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

__global__ __launch_bounds__(256) void k_charuco_interp(BoardArgs a, CharucoArgs c, RefineParams p) {
    __shared__ uint32_t s_seen[A3_BOARD_MAX_MARKERS / 32], s_dup[A3_BOARD_MAX_MARKERS / 32];
    __shared__ float s_h[A3_BOARD_MAX_MARKERS][8];      // homography of the slot's marker
    __shared__ uint32_t s_mi[A3_BOARD_MAX_MARKERS];     // the slot's marker (index into the marker list); kNoAdj: none with a homography
    __shared__ uint32_t s_wave[4];
    const uint32_t f = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    uint32_t first, cnt;
    board_frame_run(a.markers != nullptr, a.per_frame, a.n, a.n_dev, f, lane, &first, &cnt);
    for (int s = tid; s < A3_BOARD_MAX_MARKERS; s += 256) s_mi[s] = kNoAdj;
    board_mark_duplicates(s_seen, s_dup, cnt, true, (uint32_t)tid, 256u, [&](uint32_t i) { return board_slot(a, first + i); });
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

// The record model of a3_board.h's board_pose_body: the start marker as k_board_pose takes it, the correspondences the frame's records
// (chessboard corner id -> board point; the undistorted corner where the batch has one), solved when there are four or more.
struct CharucoRecords {
    using Slot = BoardSlot;
    using Record = a3_charuco_pose;
    using Corr = BoardCorr;
    const CharucoArgs& c;
    uint32_t roff = 0, ncorn = 0;   // the frame's records: the sum of the counts before it, its count
    __device__ static const BoardSlot* slots(const BoardArgs& a) { return a.slots; }
    __device__ void bind(const BoardArgs&, uint32_t f, int lane, uint32_t, uint32_t, const uint32_t*) {
        for (uint32_t g = (uint32_t)lane; g < f; g += 64) roff += c.counts[g];
        roff = wave_sum_u(roff);
        ncorn = c.counts[f];
    }
    __device__ uint32_t count() const { return ncorn; }
    __device__ bool corner(const BoardArgs& a, uint32_t r, BoardCorr& o) const {
        const a3_charuco_corner& rec = c.out[roff + r];
        o.bx = c.cxy[2 * rec.id]; o.by = c.cxy[2 * rec.id + 1];
        const float x = c.und ? c.und[2 * ((size_t)roff + r)] : rec.x, y = c.und ? c.und[2 * ((size_t)roff + r) + 1] : rec.y;
        board_normalise(a, x, y, &o.mx, &o.my);
        return true;
    }
    __device__ static void accum(BoardAcc& s, const float R[9], const float t[3], const BoardCorr& o, float sx, float sy) {
        board_accum(s, R, t, o.bx, o.by, o.mx, o.my, sx, sy);
    }
    __device__ static void start(const BoardSlot& bs, const a3_pose& pm, float R[9], float t[3]) { board_planar_start(bs, pm, R, t); }
    __device__ bool solves(bool top) const { return top && ncorn >= 4; }
    __device__ float denominator(const BoardStart&) const { return (float)ncorn; }
    __device__ void counts(a3_charuco_pose& rec, const BoardStart&) const { rec.corners_used = ncorn; }
};

__global__ __launch_bounds__(128) void k_charuco_pose(BoardArgs a, CharucoArgs c, a3_charuco_pose* out) { board_pose_body(a, CharucoRecords{c}, out); }

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
