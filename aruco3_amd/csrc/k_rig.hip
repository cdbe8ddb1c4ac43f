// k_rig.hip -- camera rig calibration (a3_calibrate_rigs).  Not part of the reference: an extension stated in include/aruco3_hip.h and
// restated on the CPU by tests/rig_oracle.c (a3o_calibrate_rigs), which this kernel matches bit for bit.
//
// One workgroup of four waves per rig; every phase runs inside the one launch, separated by barriers.  Per-observation work (step 1) goes
// to one wave (observations w, w + 4, ...), per-frame work to one wave (frame f to wave f mod 4).  An observation's sums run in point
// order: the lanes write the rows of up to 64 points into the wave's LDS, then each lane owns up to two of the 91 block entries and adds
// the rows in order (aug_block of a3_solve.h, where the pose start, pose_from_h, lives too).  The Schur complement over the extrinsics (order 6 (C - 1) <= 42) has one
// thread per entry, each summing over the frames in frame order; its LDL^T runs column by column on wave 0, one lane per row, every
// entry in the contract's order; the covariance's unit-vector solves take one lane each.  Blocks, poses and the frames' Schur
// vectors live in device scratch: kRigObsDoubles per observation, kRigFrameDoubles per frame, and a table [frame][8] of the USED
// observation of every (frame, camera).
#include <cmath>

#include "a3_common.h"
#include "a3_launch.h"
#include "a3_rig.h"

namespace a3 {

constexpr int kRigThreads = 256, kRigWaves = 4;
constexpr int kRigRowStride = 2 * kRigAug;   // doubles per point in LDS: the u row, then the v row
constexpr int kRigMaxC = A3_RIG_MAX_CAMERAS, kRigMaxN = 6 * (A3_RIG_MAX_CAMERAS - 1);
constexpr uint32_t kRigNone = 0xffffffffu;
// per-observation scratch: blocks (2 slots), P (step 1's pose; the homography before it), step 1's cost
constexpr int kObsBlk = 0, kObsP = 2 * kRigEntries, kObsCost = kObsP + 12;
constexpr size_t kRigObsDoubles = 200;
static_assert(kObsCost + 1 <= (int)kRigObsDoubles, "observation scratch");
// per-frame scratch: poses (2 slots), the frame's sums (2 slots of 28), y_i = V^-1 W[i] and y_g (6 each), the final slot
constexpr int kFrPose = 0, kFrVg = 24, kFrY = kFrVg + 56, kFrCur = kFrY + 6 * (kRigMaxN + 1);
constexpr size_t kRigFrameDoubles = 344;
static_assert(kFrCur + 1 <= (int)kRigFrameDoubles, "frame scratch");
static_assert(64 * kRigRowStride >= 64 + 64 + 8 + 8 && 64 * kRigRowStride >= 64 * 2 * kHomAug, "the homography works in the row buffer");

struct RigArgs {
    const a3_rig* rigs;
    const a3_rig_camera* cams;
    const a3_rig_observation* obs;
    const float* obj;
    const float* img;
    uint32_t* tab;
    double* oscr;
    double* fscr;
    a3_rig_result* res;
    a3_rig_camera_result* cres;
    a3_rig_frame* frames;
    a3_rig_observation_result* ores;
};

// one observation's 91 block entries at (a, E, T), G = E . T -> out (wave-level): aug_block (a3_solve.h) over rig_row
__device__ __forceinline__ void obs_block(const double a[12], const double* E, const double* T, const double* G, const float* __restrict__ obj,
                                          const float* __restrict__ img, uint32_t p0, uint32_t np, double* rows, int lane, double* out) {
    aug_block<kRigAug>([&](double X, double Y, double ou, double ov, double* au, double* av) { rig_row(a, E, T, G, X, Y, ou, ov, au, av); }, obj, img, p0,
                       np, rows, lane, out);
}

// the blocks of frame f (call index) at (s_E, T) into `slot`, then the frame's sums (wave-level)
__device__ __forceinline__ void frame_eval(const RigArgs& g, uint32_t f, uint32_t C, uint32_t c0, const double* s_a, const double* s_E, const double* T,
                                           int slot, double* rows, int lane) {
    for (uint32_t c = 0; c < C; c++) {
        const uint32_t o = g.tab[(size_t)f * kRigMaxC + c];
        if (o == kRigNone) continue;
        double a[12], E[12], G[12];
#pragma unroll
        for (int q = 0; q < 12; q++) { a[q] = s_a[c * 12 + q]; E[q] = s_E[c * 12 + q]; }
        pose_mul(E, T, G);
        const a3_rig_observation ob = g.obs[o];
        obs_block(a, E, T, G, g.obj, g.img, ob.first_point, ob.n_points, rows, lane, g.oscr + (size_t)o * kRigObsDoubles + kObsBlk + slot * kRigEntries);
    }
    if (lane < 28) {
        double s = 0.0;
        for (uint32_t c = 0; c < C; c++) {
            const uint32_t o = g.tab[(size_t)f * kRigMaxC + c];
            if (o != kRigNone) s = s + g.oscr[(size_t)o * kRigObsDoubles + kObsBlk + slot * kRigEntries + kRigFrameTri + lane];
        }
        g.fscr[(size_t)f * kRigFrameDoubles + kFrVg + slot * 28 + lane] = s;
    }
    wave_sync();
}

// LDL^T of the n x n matrix in A (row stride kRigMaxN) on one wave, lane r the entry (j + r, j) of column j: every entry's arithmetic is
// ldl_n's.  -> false on a bad pivot
__device__ __forceinline__ bool ldl_wave(double* A, int n, double* D, int lane, int* flag) {
    if (lane == 0) *flag = 0;
    wave_sync();
    for (int j = 0; j < n; j++) {
        const int i = j + lane;
        double s = 0.0;
        if (i < n) {
            s = A[i * kRigMaxN + j];
            for (int k = 0; k < j; k++) s = s - A[i * kRigMaxN + k] * A[j * kRigMaxN + k] * D[k];
        }
        if (lane == 0) {
            if (!(s > 0.0) || !fin(s)) *flag = 1;
            D[j] = s;
        }
        wave_sync();
        if (*flag) break;
        if (lane > 0 && i < n) A[i * kRigMaxN + j] = s / D[j];
        wave_sync();
    }
    return *flag == 0;
}

__global__ __launch_bounds__(kRigThreads) void k_rig(RigArgs g) {
    __shared__ double s_rows[kRigWaves][64 * kRigRowStride];
    __shared__ double s_wv[kRigWaves][8];
    __shared__ double s_S[kRigMaxN * kRigMaxN], s_X[kRigMaxN * kRigMaxN];
    __shared__ double s_a[kRigMaxC * 12], s_E[2][kRigMaxC * 12], s_U[kRigMaxC * 27];
    __shared__ double s_rhs[kRigMaxN], s_D[kRigMaxN], s_de[kRigMaxN], s_std[kRigMaxN];
    __shared__ double s_cost, s_lambda;
    __shared__ int s_best[kRigMaxC * kRigMaxC];
    __shared__ int s_status, s_stop, s_bad, s_skip, s_cur, s_sums, s_iter, s_conv, s_cov, s_flag;
    __shared__ uint32_t s_fu, s_ou, s_np;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const a3_rig R = g.rigs[blockIdx.x];
    const uint32_t C = R.n_cameras, c0 = R.first_camera, f0 = R.first_frame, F = R.n_frames, o0 = R.first_obs, NO = R.n_obs;
    const bool fix = (R.flags & A3_RIG_FIX_EXTRINSICS) != 0, guess = fix || (R.flags & A3_RIG_USE_EXTRINSIC_GUESS) != 0;
    const int maxit = R.max_iterations ? (int)R.max_iterations : A3_CALIB_DEFAULT_ITERATIONS;
    const int n = fix ? 0 : 6 * ((int)C - 1);
    double* rows = s_rows[wave];
    double* wv = s_wv[wave];

    for (uint32_t i = (uint32_t)tid; i < F * kRigMaxC; i += kRigThreads) g.tab[(size_t)f0 * kRigMaxC + i] = kRigNone;
    for (uint32_t i = (uint32_t)tid; i < C * 12; i += kRigThreads) s_a[i] = g.cams[c0 + i / 12].a[i % 12];
    if (tid == 0) {
        s_status = A3_RIG_OK;
        s_stop = 0; s_bad = 0; s_skip = 0; s_cur = 0; s_sums = 1; s_iter = 0; s_conv = fix ? 1 : 0; s_cov = 0;
        s_lambda = 1e-3;
        s_cost = 0.0;
    }
    __syncthreads();
    // ---- 1. per observation: homography, pose start, pose LM ----
    for (uint32_t j = (uint32_t)wave; j < NO; j += kRigWaves) {
        const uint32_t o = o0 + j;
        const a3_rig_observation ob = g.obs[o];
        const uint32_t p0 = ob.first_point, np = ob.n_points;
        double* os = g.oscr + (size_t)o * kRigObsDoubles;
        uint32_t st = A3_RIG_OBS_TOO_FEW_POINTS;
        if (np >= 4) st = view_homography(g.obj, g.img, p0, np, rows, wv, lane, os + kObsP) ? A3_RIG_OBS_USED : A3_RIG_OBS_DEGENERATE;
        if (lane == 0) {
            a3_rig_observation_result* rec = &g.ores[o];
            rec->status = st;
            rec->points = np;
            rec->rms_px = 0.0f;
            rec->reserved = 0;
            if (st == A3_RIG_OBS_USED) g.tab[(size_t)ob.frame * kRigMaxC + (ob.camera - c0)] = o;
        }
        if (st != A3_RIG_OBS_USED) continue;
        double a[12];
#pragma unroll
        for (int q = 0; q < 12; q++) a[q] = s_a[(ob.camera - c0) * 12 + q];
        const double* H = os + kObsP;
        double m[3][3], T[12];
#pragma unroll
        for (int c = 0; c < 3; c++) {
            m[c][0] = (H[c] - a[2] * H[6 + c]) / a[0];
            m[c][1] = (H[3 + c] - a[3] * H[6 + c]) / a[1];
            m[c][2] = H[6 + c];
        }
        pose_from_h(m, T, T + 9);
        const double ID[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
        wave_sync();   // (every lane has read H before the blocks and P go over this scratch)
        // (the pose-only LM loop stays this kernel's own: behind a shared function it compiles to other code)
        double* cur = os + kObsBlk;
        double* oth = cur + kRigEntries;
        obs_block(a, ID, T, T, g.obj, g.img, p0, np, rows, lane, cur);
        double cost = cur[kRigEntries - 1];
        int evals = 1;
        double lambda = 1e-3;
        while (evals < A3_CALIB_POSE_EVALS && cost > 0.0) {
            double L[6][6], D[6];
            if (!ldl6_at<6, kRigAug>(cur, lambda, L, D)) { lambda = lambda * 10.0; evals++; continue; }
            double b[6], d[6], Tn[12];
#pragma unroll
            for (int q = 0; q < 6; q++) b[q] = -cur[tri_index(6 + q, 12, kRigAug)];
            ldl6_solve(L, D, b, d);
            pose_update(T, d, Tn);
            obs_block(a, ID, Tn, Tn, g.obj, g.img, p0, np, rows, lane, oth);
            evals++;
            const double c2 = oth[kRigEntries - 1];
            if (c2 < cost) {
                const double rel = (cost - c2) / cost;
#pragma unroll
                for (int q = 0; q < 12; q++) T[q] = Tn[q];
                double* s = cur; cur = oth; oth = s;
                cost = c2;
                lambda = lambda / 10.0;
                if (rel < A3_CALIB_REL_TOL) break;
            } else lambda = lambda * 10.0;
        }
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 12; q++) os[kObsP + q] = T[q];
            os[kObsCost] = cost;
        }
        wave_sync();
    }
    __syncthreads();
    // ---- counts; 2. the start ----
    for (uint32_t j = (uint32_t)tid; j < F; j += kRigThreads) {
        a3_rig_frame* fr = &g.frames[f0 + j];
        uint32_t nu = 0, np = 0;
        for (uint32_t c = 0; c < C; c++) {
            const uint32_t o = g.tab[(size_t)(f0 + j) * kRigMaxC + c];
            if (o != kRigNone) { nu++; np += g.obs[o].n_points; }
        }
        fr->status = nu ? A3_RIG_FRAME_USED : A3_RIG_FRAME_UNUSED;
        fr->obs_used = nu;
        fr->points_used = np;
        fr->rms_px = 0.0f;
        for (int q = 0; q < 9; q++) { fr->rotation[q] = 0.0; fr->rotation_f[q] = 0.0f; }
        for (int q = 0; q < 3; q++) { fr->translation[q] = 0.0; fr->translation_f[q] = 0.0f; }
    }
    if (tid < kRigMaxC * kRigMaxC) {
        const uint32_t c = (uint32_t)tid / kRigMaxC, b = (uint32_t)tid % kRigMaxC;
        int best = -1;
        double bs = 0.0;
        if (c < C && b < C && c != b)
            for (uint32_t j = 0; j < F; j++) {
                const uint32_t oc = g.tab[(size_t)(f0 + j) * kRigMaxC + c], ob = g.tab[(size_t)(f0 + j) * kRigMaxC + b];
                if (oc == kRigNone || ob == kRigNone) continue;
                const double s = g.oscr[(size_t)oc * kRigObsDoubles + kObsCost] / (double)g.obs[oc].n_points +
                                 g.oscr[(size_t)ob * kRigObsDoubles + kObsCost] / (double)g.obs[ob].n_points;
                if (best < 0 || s < bs) { best = (int)j; bs = s; }
            }
        s_best[tid] = best;
    }
    if (tid >= 64 && tid < 64 + (int)C) {   // the camera's counts (wave 1)
        const uint32_t c = (uint32_t)tid - 64;
        uint32_t nu = 0, np = 0;
        for (uint32_t j = 0; j < F; j++) {
            const uint32_t o = g.tab[(size_t)(f0 + j) * kRigMaxC + c];
            if (o != kRigNone) { nu++; np += g.obs[o].n_points; }
        }
        g.cres[c0 + c].obs_used = nu;
        g.cres[c0 + c].points_used = np;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t fu = 0, ou = 0, np = 0;
        for (uint32_t j = 0; j < F; j++) {
            const a3_rig_frame* fr = &g.frames[f0 + j];
            if (fr->obs_used) fu++;
            ou += fr->obs_used;
            np += fr->points_used;
        }
        s_fu = fu; s_ou = ou; s_np = np;
        for (uint32_t c = 0; c < C; c++)
            for (int q = 0; q < 12; q++) {
                double v = q == 0 || q == 4 || q == 8 ? 1.0 : 0.0;
                if (guess && c >= 1) v = q < 9 ? g.cams[c0 + c].guess_rotation[q] : g.cams[c0 + c].guess_translation[q - 9];
                s_E[0][c * 12 + q] = v;
                s_E[1][c * 12 + q] = q == 0 || q == 4 || q == 8 ? 1.0 : 0.0;
            }
        uint32_t reached = 1u;
        for (bool found = true; found;) {
            found = false;
            for (uint32_t c = 1; c < C && !found; c++) {
                if (reached >> c & 1u) continue;
                for (uint32_t b = 0; b < C && !found; b++) {
                    if (!(reached >> b & 1u) || s_best[c * kRigMaxC + b] < 0) continue;
                    if (!guess) {
                        const uint32_t f = f0 + (uint32_t)s_best[c * kRigMaxC + b];
                        const double* Pc = g.oscr + (size_t)g.tab[(size_t)f * kRigMaxC + c] * kRigObsDoubles + kObsP;
                        const double* Pb = g.oscr + (size_t)g.tab[(size_t)f * kRigMaxC + b] * kRigObsDoubles + kObsP;
                        double P[12], Eb[12], X[12], Y[12], O[12];
#pragma unroll
                        for (int q = 0; q < 12; q++) { P[q] = Pb[q]; Eb[q] = s_E[0][b * 12 + q]; }
                        pose_inv(P, X);
                        pose_mul(X, Eb, Y);
#pragma unroll
                        for (int q = 0; q < 12; q++) P[q] = Pc[q];
                        pose_mul(P, Y, O);
#pragma unroll
                        for (int q = 0; q < 12; q++) s_E[0][c * 12 + q] = O[q];
                    }
                    reached |= 1u << c;
                    found = true;
                }
            }
        }
        if (!fix && reached != (1u << C) - 1u) s_status = A3_RIG_NOT_CONNECTED;
    }
    __syncthreads();
    if (s_status == A3_RIG_OK) {
        // the frames' start and their blocks
        for (uint32_t j = (uint32_t)wave; j < F; j += kRigWaves) {
            const uint32_t f = f0 + j;
            int bc = -1;
            double bs = 0.0;
            for (uint32_t c = 0; c < C; c++) {
                const uint32_t o = g.tab[(size_t)f * kRigMaxC + c];
                if (o == kRigNone) continue;
                const double s = g.oscr[(size_t)o * kRigObsDoubles + kObsCost] / (double)g.obs[o].n_points;
                if (bc < 0 || s < bs) { bc = (int)c; bs = s; }
            }
            if (bc < 0) continue;
            const double* Pp = g.oscr + (size_t)g.tab[(size_t)f * kRigMaxC + (uint32_t)bc] * kRigObsDoubles + kObsP;
            double Ec[12], P[12], X[12], T[12];
#pragma unroll
            for (int q = 0; q < 12; q++) { Ec[q] = s_E[0][bc * 12 + q]; P[q] = Pp[q]; }
            pose_inv(Ec, X);
            pose_mul(X, P, T);
            double* fs = g.fscr + (size_t)f * kRigFrameDoubles;
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < 12; q++) fs[kFrPose + q] = T[q];
                fs[kFrCur] = 0.0;
            }
            frame_eval(g, f, C, c0, s_a, s_E[0], T, 0, rows, lane);
        }
        __syncthreads();
        if (tid == 0) {
            double cost = 0.0;
            for (uint32_t j = 0; j < F; j++)
                if (g.frames[f0 + j].obs_used) cost = cost + g.fscr[(size_t)(f0 + j) * kRigFrameDoubles + kFrVg + 27];
            s_cost = cost;
            if (!fin(cost)) s_status = A3_RIG_NOT_FINITE;
            if (cost == 0.0) { s_stop = 1; s_conv = 1; }
        }
        __syncthreads();
    }
    if (s_status == A3_RIG_OK && fix) {
        // ---- 3. every frame alone ----
        for (uint32_t j = (uint32_t)wave; j < F; j += kRigWaves) {
            const uint32_t f = f0 + j;
            if (!g.frames[f].obs_used) continue;
            double* fs = g.fscr + (size_t)f * kRigFrameDoubles;
            double T[12];
#pragma unroll
            for (int q = 0; q < 12; q++) T[q] = fs[kFrPose + q];
            double c1 = fs[kFrVg + 27], lam = 1e-3;
            int it = 0, cv = 0, fc = 0;
            bool stop = false;
            if (c1 == 0.0) { stop = true; cv = 1; }
            while (!stop) {
                const double* vg = fs + kFrVg + fc * 28;
                double L[6][6], D[6], b[6], d[6], Tn[12];
                if (!ldl6_at<0, 7>(vg, lam, L, D)) {
                    lam = lam * 10.0;
                    it = it + 1;
                    if (it >= maxit) stop = true;
                    continue;
                }
#pragma unroll
                for (int q = 0; q < 6; q++) b[q] = -vg[tri_index(q, 6, 7)];
                ldl6_solve(L, D, b, d);
                pose_update(T, d, Tn);
                frame_eval(g, f, C, c0, s_a, s_E[0], Tn, 1 - fc, rows, lane);
                const double c2 = fs[kFrVg + (1 - fc) * 28 + 27];
                it = it + 1;
                if (c2 < c1) {
                    const double rel = (c1 - c2) / c1;
                    fc = 1 - fc;
#pragma unroll
                    for (int q = 0; q < 12; q++) T[q] = Tn[q];
                    c1 = c2;
                    lam = lam / 10.0;
                    if (rel < A3_CALIB_REL_TOL || c2 == 0.0) { cv = 1; stop = true; }
                } else lam = lam * 10.0;
                if (it >= maxit) stop = true;
            }
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < 12; q++) fs[kFrPose + fc * 12 + q] = T[q];
                fs[kFrCur] = (double)fc;
                atomicMax(&s_iter, it);
                if (!cv) atomicAnd(&s_conv, 0);
            }
            wave_sync();
        }
        __syncthreads();
        if (tid == 0) {
            double cost = 0.0;
            for (uint32_t j = 0; j < F; j++) {
                const double* fs = g.fscr + (size_t)(f0 + j) * kRigFrameDoubles;
                if (g.frames[f0 + j].obs_used) cost = cost + fs[kFrVg + (fs[kFrCur] != 0.0 ? 28 : 0) + 27];
            }
            s_cost = cost;
        }
        __syncthreads();
    }
    if (s_status == A3_RIG_OK && !fix) {
        // ---- 3. joint LM; its last pass (s_cov) is step 4's undamped Schur complement ----
        const int ne = (n + 1) * (n + 2) / 2 - 1;   // the triangle of S with the right-hand side as column n, less the corner
        while (true) {
            __syncthreads();
            if (tid == 0 && s_stop) { s_cov = 1; s_lambda = 0.0; }
            __syncthreads();
            const int cur = s_cur, cov = s_cov;
            const double lambda = s_lambda;
            if (s_sums && tid >= 27 && tid < 27 * (int)C) {
                const uint32_t c = (uint32_t)tid / 27;
                const int e = tid % 27;
                int i = 0, k = 0;
                if (e < 21) tri_ik(e, 6, &i, &k);
                const int idx = e < 21 ? tri_index(i, k, kRigAug) : tri_index(e - 21, 12, kRigAug);
                double s = 0.0;
                for (uint32_t j = 0; j < F; j++) {
                    const uint32_t o = g.tab[(size_t)(f0 + j) * kRigMaxC + c];
                    if (o != kRigNone) s = s + g.oscr[(size_t)o * kRigObsDoubles + kObsBlk + cur * kRigEntries + idx];
                }
                s_U[c * 27 + e] = s;
            }
            for (uint32_t j = (uint32_t)wave; j < F; j += kRigWaves) {
                const uint32_t f = f0 + j;
                if (!g.frames[f].obs_used) continue;
                double* fs = g.fscr + (size_t)f * kRigFrameDoubles;
                const double* vg = fs + kFrVg + cur * 28;
                double L[6][6], D[6];
                if (!ldl6_at<0, 7>(vg, lambda, L, D)) {
                    if (lane == 0) s_bad = 1;
                    continue;
                }
                if (lane <= n) {
                    const uint32_t o = lane < n ? g.tab[(size_t)f * kRigMaxC + (uint32_t)(lane / 6 + 1)] : 0u;
                    if (o != kRigNone) {
                        const double* blk = g.oscr + (size_t)o * kRigObsDoubles + kObsBlk + cur * kRigEntries;
                        double b[6], y[6];
#pragma unroll
                        for (int m = 0; m < 6; m++) b[m] = lane < n ? blk[tri_index(lane % 6, 6 + m, kRigAug)] : vg[tri_index(m, 6, 7)];
                        ldl6_solve(L, D, b, y);
#pragma unroll
                        for (int m = 0; m < 6; m++) fs[kFrY + lane * 6 + m] = y[m];
                    }
                }
            }
            __syncthreads();
            if (!s_bad)
                for (int e = tid; e < ne; e += kRigThreads) {
                    int i, k;
                    tri_ik(e, n + 1, &i, &k);
                    const uint32_t ci = (uint32_t)(i / 6 + 1), ck = k < n ? (uint32_t)(k / 6 + 1) : ci;
                    double s;
                    if (k < n) {
                        s = ci == ck ? s_U[ci * 27 + tri_index(i % 6, k % 6, 6)] : 0.0;
                        if (i == k) s = s + lambda * s;
                    } else s = -s_U[ci * 27 + 21 + i % 6];
                    const int wi = tri_index(i % 6, 6, kRigAug);
                    for (uint32_t j = 0; j < F; j++) {
                        const uint32_t f = f0 + j;
                        const uint32_t oi = g.tab[(size_t)f * kRigMaxC + ci], ok = g.tab[(size_t)f * kRigMaxC + ck];
                        if (oi == kRigNone || ok == kRigNone) continue;
                        const double* w = g.oscr + (size_t)oi * kRigObsDoubles + kObsBlk + cur * kRigEntries + wi;
                        const double* y = g.fscr + (size_t)f * kRigFrameDoubles + kFrY + k * 6;
                        double t = 0.0;
#pragma unroll
                        for (int m = 0; m < 6; m++) t = t + w[m] * y[m];
                        s = k < n ? s - t : s + t;
                    }
                    if (k < n) { s_S[i * kRigMaxN + k] = s; s_S[k * kRigMaxN + i] = s; }
                    else s_rhs[i] = s;
                }
            __syncthreads();
            if (wave == 0) {
                bool bad = s_bad != 0;
                if (!bad) bad = !ldl_wave(s_S, n, s_D, lane, &s_flag);
                if (cov) {
                    if (lane < n) {
                        double dv = __builtin_inf();
                        if (!bad) {
                            const double sigma2 = s_cost / (double)(2ll * s_np - n - 6ll * s_fu);
                            double* x = s_X + lane * kRigMaxN;
                            for (int q = 0; q < n; q++) x[q] = q == lane ? 1.0 : 0.0;
                            ldl_n_solve<kRigMaxN>(s_S, n, s_D, x, x);
                            dv = sqrt(sigma2 * x[lane]);
                        }
                        s_std[lane] = dv;
                    }
                } else if (lane == 0) {
                    if (!bad) {
                        ldl_n_solve<kRigMaxN>(s_S, n, s_D, s_rhs, s_de);
                        for (uint32_t c = 1; c < C; c++) {
                            double E[12], d[6], En[12];
#pragma unroll
                            for (int q = 0; q < 12; q++) E[q] = s_E[cur][c * 12 + q];
#pragma unroll
                            for (int q = 0; q < 6; q++) d[q] = s_de[6 * (c - 1) + q];
                            pose_update(E, d, En);
#pragma unroll
                            for (int q = 0; q < 12; q++) s_E[1 - cur][c * 12 + q] = En[q];
                        }
                    }
                    s_bad = 0;
                    s_skip = bad ? 1 : 0;
                    s_sums = 0;
                    if (bad) {
                        s_lambda = lambda * 10.0;
                        s_iter = s_iter + 1;
                        if (s_iter >= maxit) s_stop = 1;
                    }
                }
            }
            __syncthreads();
            if (cov) break;
            if (s_skip) continue;
            for (uint32_t j = (uint32_t)wave; j < F; j += kRigWaves) {
                const uint32_t f = f0 + j;
                if (!g.frames[f].obs_used) continue;
                double* fs = g.fscr + (size_t)f * kRigFrameDoubles;
                const double* vg = fs + kFrVg + cur * 28;
                double L[6][6], D[6], b[6], d[6], sm[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                ldl6_at<0, 7>(vg, lambda, L, D);
                for (int k = 0; k < n; k++) {
                    const uint32_t o = g.tab[(size_t)f * kRigMaxC + (uint32_t)(k / 6 + 1)];
                    if (o == kRigNone) continue;
                    const double* w = g.oscr + (size_t)o * kRigObsDoubles + kObsBlk + cur * kRigEntries + tri_index(k % 6, 6, kRigAug);
                    const double dk = s_de[k];
#pragma unroll
                    for (int q = 0; q < 6; q++) sm[q] = sm[q] + w[q] * dk;
                }
#pragma unroll
                for (int q = 0; q < 6; q++) b[q] = -vg[tri_index(q, 6, 7)] - sm[q];
                ldl6_solve(L, D, b, d);
                double T[12], Tn[12];
#pragma unroll
                for (int q = 0; q < 12; q++) T[q] = fs[kFrPose + cur * 12 + q];
                pose_update(T, d, Tn);
                if (lane == 0) {
#pragma unroll
                    for (int q = 0; q < 12; q++) fs[kFrPose + (1 - cur) * 12 + q] = Tn[q];
                }
                frame_eval(g, f, C, c0, s_a, s_E[1 - cur], Tn, 1 - cur, rows, lane);
            }
            __syncthreads();
            if (tid == 0) {
                double c2 = 0.0;
                for (uint32_t j = 0; j < F; j++)
                    if (g.frames[f0 + j].obs_used) c2 = c2 + g.fscr[(size_t)(f0 + j) * kRigFrameDoubles + kFrVg + (1 - cur) * 28 + 27];
                const double cost = s_cost;
                s_iter = s_iter + 1;
                if (c2 < cost) {
                    const double rel = (cost - c2) / cost;
                    s_cur = 1 - cur;
                    s_cost = c2;
                    s_lambda = lambda / 10.0;
                    s_sums = 1;
                    if (rel < A3_CALIB_REL_TOL || c2 == 0.0) { s_conv = 1; s_stop = 1; }
                } else s_lambda = lambda * 10.0;
                if (s_iter >= maxit) s_stop = 1;
            }
        }
        __syncthreads();
        const int cur = s_cur;
        for (uint32_t j = (uint32_t)tid; j < F; j += kRigThreads) g.fscr[(size_t)(f0 + j) * kRigFrameDoubles + kFrCur] = (double)cur;
        __syncthreads();
    }
    // ---- 4. results ----
    const bool ok = s_status == A3_RIG_OK;
    if (tid == 0) {
        a3_rig_result* r = &g.res[blockIdx.x];
        r->status = (uint32_t)s_status;
        r->frames_used = s_fu;
        r->obs_used = s_ou;
        r->points_used = s_np;
        r->iterations = ok ? (uint32_t)s_iter : 0u;
        r->converged = ok ? (uint32_t)s_conv : 0u;
        r->rms_px = ok && s_np ? sqrt(s_cost / (double)s_np) : 0.0;
    }
    if (tid < (int)C) {
        const uint32_t c = (uint32_t)tid;
        a3_rig_camera_result* cr = &g.cres[c0 + c];
        const double* Ec = s_E[fix ? 0 : s_cur] + c * 12;
        double cc = 0.0;
        if (ok)
            for (uint32_t j = 0; j < F; j++) {
                const uint32_t o = g.tab[(size_t)(f0 + j) * kRigMaxC + c];
                if (o == kRigNone) continue;
                const int fc = g.fscr[(size_t)(f0 + j) * kRigFrameDoubles + kFrCur] != 0.0 ? 1 : 0;
                cc = cc + g.oscr[(size_t)o * kRigObsDoubles + kObsBlk + fc * kRigEntries + kRigEntries - 1];
            }
        for (int q = 0; q < 9; q++) { cr->rotation[q] = ok ? Ec[q] : 0.0; cr->rotation_f[q] = ok ? (float)Ec[q] : 0.0f; }
        for (int q = 0; q < 3; q++) { cr->translation[q] = ok ? Ec[9 + q] : 0.0; cr->translation_f[q] = ok ? (float)Ec[9 + q] : 0.0f; }
        for (int q = 0; q < 6; q++) cr->std_dev[q] = ok && c >= 1 && !fix ? s_std[6 * (c - 1) + q] : 0.0;
        cr->rms_px = ok && cr->points_used ? sqrt(cc / (double)cr->points_used) : 0.0;
    }
    if (ok)
        for (uint32_t j = (uint32_t)tid; j < F; j += kRigThreads) {
            const uint32_t f = f0 + j;
            a3_rig_frame* fr = &g.frames[f];
            if (!fr->obs_used) continue;
            const double* fs = g.fscr + (size_t)f * kRigFrameDoubles;
            const int fc = fs[kFrCur] != 0.0 ? 1 : 0;
            fr->rms_px = (float)sqrt(fs[kFrVg + fc * 28 + 27] / (double)fr->points_used);
            for (int q = 0; q < 9; q++) { fr->rotation[q] = fs[kFrPose + fc * 12 + q]; fr->rotation_f[q] = (float)fs[kFrPose + fc * 12 + q]; }
            for (int q = 0; q < 3; q++) { fr->translation[q] = fs[kFrPose + fc * 12 + 9 + q]; fr->translation_f[q] = (float)fs[kFrPose + fc * 12 + 9 + q]; }
            for (uint32_t c = 0; c < C; c++) {
                const uint32_t o = g.tab[(size_t)f * kRigMaxC + c];
                if (o != kRigNone)
                    g.ores[o].rms_px = (float)sqrt(g.oscr[(size_t)o * kRigObsDoubles + kObsBlk + fc * kRigEntries + kRigEntries - 1] / (double)g.ores[o].points);
            }
        }
}

size_t rig_obs_bytes() { return kRigObsDoubles * sizeof(double); }
size_t rig_frame_bytes() { return kRigFrameDoubles * sizeof(double); }
size_t rig_table_bytes() { return kRigMaxC * sizeof(uint32_t); }

hipError_t launch_rig(hipStream_t st, const RigLaunch& r) {
    if (r.n_rigs == 0) return hipSuccess;
    const RigArgs g{r.rigs, r.cams, r.obs, r.obj, r.img, r.tab, r.oscr, r.fscr, r.res, r.cres, r.frames, r.ores};
    hipLaunchKernelGGL(k_rig, dim3(r.n_rigs), dim3(kRigThreads), 0, st, g);
    return hipGetLastError();
}

}  // namespace a3
