// k_map.hip -- marker maps (a3_build_marker_maps).  Not part of the reference: an extension stated in include/aruco3_hip.h and restated
// on the CPU by tests/map_oracle.c (a3o_build_marker_maps), which this kernel matches bit for bit.
//
// One workgroup of eight waves per map; every phase runs inside the one launch, separated by barriers (the k_rig scheme).  Step 1 and
// every block evaluation go to one wave per observation / frame; the start's rounds take one thread per frame (a) and per marker (b),
// each running its hypotheses in the contract's order.  The reduced system over the markers (order n = 6 x the reached markers but the
// first, up to 762) lives in device scratch, column-major so that a column's rows are contiguous: one thread per entry builds it,
// summing over the frames in frame order and touching only the blocks of marker pairs a frame sees together; its LDL^T runs column by
// column over the whole workgroup, one thread per row; the solve keeps one running row sum per thread and publishes one unknown per
// barrier, which is the contract's order (ascending forward, descending backward); the covariance's unit-vector solves take one
// thread each on a second n x n scratch.  Blocks, candidates, poses and the frames' vectors live in device scratch: kMapObsDoubles
// per observation, kMapFrameDoubles per frame, kMapMarkerDoubles per marker, and two tables (a frame's first observation, a marker's
// observations in order).  No atomics on shared addresses but the rig's iteration maximum: every result is reproducible.  Step 1's
// pose start is pose_from_h (a3_solve.h).
#include <cmath>

#include "a3_common.h"
#include "a3_launch.h"
#include "a3_map.h"

namespace a3 {

constexpr int kMapThreads = 512, kMapWaves = 8;
constexpr int kMapMaxM = A3_MAP_MAX_MARKERS, kMapMaxN = 6 * (A3_MAP_MAX_MARKERS - 1);
constexpr int kMapRows = 144;   // doubles per wave: four points' rows of 13 (u, v), or the homography's rows, matrix and vectors
// per-observation scratch: blocks (2 slots), step 1's candidates and their costs, y_o,k, whether it takes part
constexpr int kMoBlk = 0, kMoP = 2 * kRigEntries, kMoC = kMoP + 24, kMoY = kMoC + 2, kMoAct = kMoY + 36;
constexpr size_t kMapObsDoubles = 248;
static_assert(kMoAct + 1 <= (int)kMapObsDoubles, "observation scratch");
// per-frame scratch: poses (2 slots; in the start the frame's two candidates), the frame's sums (2 slots of 28), y_g, the final slot,
// the reached markers it was located from (0: not located), the two candidates' costs
constexpr int kMfPose = 0, kMfVg = 24, kMfYg = kMfVg + 56, kMfCur = kMfYg + 6, kMfLoc = kMfCur + 1, kMfK = kMfLoc + 1;
constexpr size_t kMapFrameDoubles = 96;
static_assert(kMfK + 2 <= (int)kMapFrameDoubles, "frame scratch");
// per-marker scratch: U_m and g_m (27), the deviations (6)
constexpr int kMmU = 0, kMmStd = 27;
constexpr size_t kMapMarkerDoubles = 40;
static_assert(4 * 2 * kRigAug <= kMapRows && 64 + 64 + 8 + 8 <= kMapRows && 4 * 2 * kHomAug <= kMapRows, "the wave's row buffer");

struct MapArgs {
    const a3_map* maps;
    const a3_map_marker* markers;
    const a3_map_observation* obs;
    const float* img;
    const uint64_t* big_off;   // per map: where its two n x n matrices start in `big` (doubles)
    uint32_t* fo;              // per frame of the call: its first observation
    uint32_t* ml;              // per map, over its observation range: the observations sorted by marker, in order
    double* oscr;
    double* fscr;
    double* mscr;
    double* big;
    a3_map_result* res;
    a3_map_marker_result* mres;
    a3_map_frame* frames;
    a3_map_observation_result* ores;
};

// one observation's 91 block entries at (a, E, T), G = E . T -> out (wave-level): one chunk of aug_block (a3_solve.h) over rig_row, the
// four object points from sq.  aug_block takes its points __restrict__: sq is the map's s_sq in LDS, which is written before a barrier
// and never while a block is evaluated.
__device__ __forceinline__ void map_block(const double a[12], const double* E, const double* T, const double* G, const float* sq,
                                          const float* __restrict__ img, double* rows, int lane, double* out) {
    aug_block<kRigAug>([&](double X, double Y, double ou, double ov, double* au, double* av) { rig_row(a, E, T, G, X, Y, ou, ov, au, av); }, sq, img, 0, 4,
                       rows, lane, out);
}

// the pose LM of step 1 on columns 6-12 with E the identity (wave-level): T in / out -> the cost; the blocks go over blk[2][91]
__device__ __forceinline__ double map_pose_lm(const double a[12], const float* sq, const float* __restrict__ img, double T[12], double* blk, double* rows,
                                              int lane) {
    const double ID[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    double* cur = blk;
    double* oth = blk + kRigEntries;
    map_block(a, ID, T, T, sq, img, rows, lane, cur);
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
        map_block(a, ID, Tn, Tn, sq, img, rows, lane, oth);
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
    return cost;
}

struct MapView {   // what the wave-level helpers need of one map
    const MapArgs* g;
    const double* a;      // LDS: the camera
    const float* sq;      // LDS: the object points
    uint32_t m0, f0, F, o0, NO;
    __device__ __forceinline__ uint32_t fbeg(uint32_t f) const { return g->fo[f]; }
    __device__ __forceinline__ uint32_t fend(uint32_t f) const { return f + 1 < f0 + F ? g->fo[f + 1] : o0 + NO; }
};

// the blocks of frame f (call index) at (M, T) into `slot`, then the frame's sums (wave-level); M: the markers' poses in LDS
__device__ __forceinline__ void map_frame_eval(const MapView& v, uint32_t f, const double* M, const double* T, int slot, double* rows, int lane) {
    const MapArgs& g = *v.g;
    const uint32_t ob = v.fbeg(f), oe = v.fend(f);
    double a[12];
#pragma unroll
    for (int q = 0; q < 12; q++) a[q] = v.a[q];
    for (uint32_t o = ob; o < oe; o++) {
        if (g.oscr[(size_t)o * kMapObsDoubles + kMoAct] == 0.0) continue;
        double Mm[12], G[12];
        const double* mp = M + (size_t)(g.obs[o].marker - v.m0) * 12;
#pragma unroll
        for (int q = 0; q < 12; q++) Mm[q] = mp[q];
        pose_mul(T, Mm, G);
        map_block(a, T, Mm, G, v.sq, g.img + 8 * (size_t)o, rows, lane, g.oscr + (size_t)o * kMapObsDoubles + kMoBlk + slot * kRigEntries);
    }
    if (lane < 28) {
        const int idx = map_frame_tri(lane);
        double s = 0.0;
        for (uint32_t o = ob; o < oe; o++)
            if (g.oscr[(size_t)o * kMapObsDoubles + kMoAct] != 0.0) s = s + g.oscr[(size_t)o * kMapObsDoubles + kMoBlk + slot * kRigEntries + idx];
        g.fscr[(size_t)f * kMapFrameDoubles + kMfVg + slot * 28 + lane] = s;
    }
    wave_sync();
}

// LDL^T of the n x n matrix in S (column-major, lower triangle: entry (i, j), i >= j, at S[j n + i]) over the workgroup, thread r the
// rows j + r and j + r + kMapThreads of column j: every entry's arithmetic is the contract's.  -> false on a bad pivot
__device__ __forceinline__ bool map_ldl(double* S, int n, double* D, int tid, int* flag) {
    if (tid == 0) *flag = 0;
    __syncthreads();
    for (int j = 0; j < n; j++) {
        double s[2] = {0.0, 0.0};
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int i = j + tid + r * kMapThreads;
            if (i < n) {
                double t = S[(size_t)j * n + i];
                for (int k = 0; k < j; k++) t = t - S[(size_t)k * n + i] * S[(size_t)k * n + j] * D[k];
                s[r] = t;
            }
        }
        if (tid == 0) {
            if (!(s[0] > 0.0) || !fin(s[0])) *flag = 1;
            D[j] = s[0];
        }
        __syncthreads();
        if (*flag) break;
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int i = j + tid + r * kMapThreads;
            if (i < n && i > j) S[(size_t)j * n + i] = s[r] / D[j];
        }
        __syncthreads();
    }
    __syncthreads();
    return *flag == 0;
}

// x <- (L D L^T)^-1 x over the workgroup (x in LDS): thread r keeps the running sums of rows r and r + kMapThreads; one unknown becomes
// final per barrier, forward in ascending and backward in descending order
__device__ __forceinline__ void map_solve(const double* S, int n, const double* D, double* x, int tid) {
    double s[2];
#pragma unroll
    for (int r = 0; r < 2; r++) s[r] = tid + r * kMapThreads < n ? x[tid + r * kMapThreads] : 0.0;
    __syncthreads();
    for (int k = 0; k < n; k++) {
        if ((k & (kMapThreads - 1)) == tid) x[k] = k >= kMapThreads ? s[1] : s[0];
        __syncthreads();
        const double xk = x[k];
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int i = tid + r * kMapThreads;
            if (i > k && i < n) s[r] = s[r] - S[(size_t)k * n + i] * xk;
        }
    }
    __syncthreads();
#pragma unroll
    for (int r = 0; r < 2; r++) {
        const int i = tid + r * kMapThreads;
        if (i < n) s[r] = x[i] / D[i];
    }
    __syncthreads();
    for (int k = n - 1; k >= 0; k--) {
        if ((k & (kMapThreads - 1)) == tid) x[k] = k >= kMapThreads ? s[1] : s[0];
        __syncthreads();
        const double xk = x[k];
#pragma unroll
        for (int r = 0; r < 2; r++) {
            const int i = tid + r * kMapThreads;
            if (i < k) s[r] = s[r] - S[(size_t)i * n + k] * xk;
        }
    }
    __syncthreads();
}

__global__ __launch_bounds__(kMapThreads) void k_map(MapArgs g) {
    __shared__ double s_rows[kMapWaves][kMapRows];
    __shared__ double s_wv[kMapWaves][8];
    __shared__ double s_M[2][kMapMaxM * 12];
    __shared__ double s_D[kMapMaxN], s_x[kMapMaxN];
    __shared__ double s_a[12];
    __shared__ float s_sq[8];
    __shared__ double s_cost, s_lambda;
    __shared__ int s_reached[kMapMaxM], s_ua[kMapMaxM], s_pos[kMapMaxM];
    __shared__ uint32_t s_mo[kMapMaxM + 1];
    __shared__ int s_status, s_stop, s_bad, s_skip, s_cur, s_sums, s_iter, s_conv, s_cov, s_flag, s_changed, s_nu;
    __shared__ uint32_t s_fu, s_ou, s_mu;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const a3_map R = g.maps[blockIdx.x];
    const uint32_t M = R.n_markers, m0 = R.first_marker, f0 = R.first_frame, F = R.n_frames, o0 = R.first_obs, NO = R.n_obs;
    const bool fix = (R.flags & A3_MAP_FIX_MAP) != 0, guess = fix || (R.flags & A3_MAP_USE_GUESS) != 0;
    const int maxit = R.max_iterations ? (int)R.max_iterations : A3_CALIB_DEFAULT_ITERATIONS;
    double* rows = s_rows[wave];
    double* wv = s_wv[wave];
    const MapView v{&g, s_a, s_sq, m0, f0, F, o0, NO};

    // ---- tables and the start's state ----
    for (uint32_t j = (uint32_t)tid; j < F; j += kMapThreads) {   // a frame's first observation: the first whose frame is not below it
        uint32_t lo = 0, hi = NO;
        while (lo < hi) {
            const uint32_t mid = (lo + hi) >> 1;
            if (g.obs[o0 + mid].frame < f0 + j) lo = mid + 1; else hi = mid;
        }
        g.fo[f0 + j] = o0 + lo;
        g.fscr[(size_t)(f0 + j) * kMapFrameDoubles + kMfLoc] = 0.0;
        g.fscr[(size_t)(f0 + j) * kMapFrameDoubles + kMfCur] = 0.0;
    }
    if (tid < (int)M) {
        uint32_t c = 0;
        for (uint32_t j = 0; j < NO; j++) c += g.obs[o0 + j].marker == m0 + (uint32_t)tid ? 1u : 0u;
        s_pos[tid] = (int)c;
        s_reached[tid] = fix || tid == 0 ? 1 : 0;
    }
    for (uint32_t i = (uint32_t)tid; i < M * 12; i += kMapThreads) {
        const uint32_t m = i / 12, q = i % 12;
        double val = q == 0 || q == 4 || q == 8 ? 1.0 : 0.0;
        if (guess && m >= 1) val = q < 9 ? g.markers[m0 + m].guess_rotation[q] : g.markers[m0 + m].guess_translation[q - 9];
        s_M[0][i] = val;
        s_M[1][i] = val;
    }
    if (tid < 12) s_a[tid] = g.maps[blockIdx.x].a[tid];
    if (tid == 0) {
        const float h = R.marker_length * 0.5f;
        s_sq[0] = -h; s_sq[1] = h; s_sq[2] = h; s_sq[3] = h; s_sq[4] = h; s_sq[5] = -h; s_sq[6] = -h; s_sq[7] = -h;
        s_status = A3_MAP_OK;
        s_stop = 0; s_bad = 0; s_skip = 0; s_cur = 0; s_sums = 1; s_iter = 0; s_conv = fix ? 1 : 0; s_cov = 0; s_nu = 0;
        s_lambda = 1e-3;
        s_cost = 0.0;
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t q = 0;
        for (uint32_t m = 0; m < M; m++) { s_mo[m] = q; q += (uint32_t)s_pos[m]; }
        s_mo[M] = q;
    }
    __syncthreads();
    if (tid < (int)M) {
        uint32_t q = o0 + s_mo[tid];
        for (uint32_t j = 0; j < NO; j++)
            if (g.obs[o0 + j].marker == m0 + (uint32_t)tid) g.ml[q++] = o0 + j;
    }
    __syncthreads();
    // ---- 1. per observation: homography, both planar candidates, each through the pose LM ----
    for (uint32_t j = (uint32_t)wave; j < NO; j += kMapWaves) {
        const uint32_t o = o0 + j;
        const float* im = g.img + 8 * (size_t)o;
        double* os = g.oscr + (size_t)o * kMapObsDoubles;
        const bool used = view_homography(s_sq, im, 0, 4, rows, wv, lane, os + kMoP);
        double c0 = 0.0, c1 = 0.0;
        if (used) {
            double a[12];
#pragma unroll
            for (int q = 0; q < 12; q++) a[q] = s_a[q];
            const double* H = os + kMoP;
            double m[3][3], T[12];
#pragma unroll
            for (int c = 0; c < 3; c++) {
                m[c][0] = (H[c] - a[2] * H[6 + c]) / a[0];
                m[c][1] = (H[3 + c] - a[3] * H[6 + c]) / a[1];
                m[c][2] = H[6 + c];
            }
            pose_from_h(m, T, T + 9);
            wave_sync();   // (every lane has read H before the candidates go over this scratch)
            c0 = map_pose_lm(a, s_sq, im, T, os + kMoBlk, rows, lane);
            double Q[12];
            pose_flip(T, Q);
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < 12; q++) os[kMoP + q] = T[q];
                os[kMoC] = c0;
            }
            wave_sync();
            c1 = map_pose_lm(a, s_sq, im, Q, os + kMoBlk, rows, lane);
            if (lane == 0) {
#pragma unroll
                for (int q = 0; q < 12; q++) os[kMoP + 12 + q] = Q[q];
                os[kMoC + 1] = c1;
            }
        }
        if (lane == 0) {
            a3_map_observation_result* rec = &g.ores[o];
            rec->status = used ? A3_MAP_OBS_USED : A3_MAP_OBS_DEGENERATE;
            rec->rms_px = 0.0f;
            rec->start_rms_px[0] = used ? (float)sqrt(c0 / 4.0) : 0.0f;
            rec->start_rms_px[1] = used ? (float)sqrt(c1 / 4.0) : 0.0f;
            os[kMoAct] = 0.0;
        }
        wave_sync();
    }
    // ---- 2. the start, in rounds ----
    while (true) {
        __syncthreads();
        if (tid == 0) s_changed = 0;
        __syncthreads();
        for (uint32_t j = (uint32_t)tid; j < F; j += kMapThreads) {   // a: locate frames
            const uint32_t f = f0 + j;
            double* fs = g.fscr + (size_t)f * kMapFrameDoubles;
            const uint32_t ob = v.fbeg(f), oe = v.fend(f);
            int cnt = 0;
            for (uint32_t o = ob; o < oe; o++)
                if (g.ores[o].status == A3_MAP_OBS_USED && s_reached[g.obs[o].marker - m0]) cnt++;
            if (cnt == 0 || (double)cnt == fs[kMfLoc]) continue;
            bool have = false;
            double bc = 0.0, alt = 0.0;
            uint32_t bo = 0;
            int bk = 0;
            for (uint32_t o = ob; o < oe; o++) {
                if (g.ores[o].status != A3_MAP_OBS_USED || !s_reached[g.obs[o].marker - m0]) continue;
                double Mm[12], X[12], k0 = 0.0, k1 = 0.0;
                const double* mp = s_M[0] + (size_t)(g.obs[o].marker - m0) * 12;
#pragma unroll
                for (int q = 0; q < 12; q++) Mm[q] = mp[q];
                pose_inv(Mm, X);
#pragma unroll 1
                for (int c = 0; c < 2; c++) {
                    double P[12], T[12], cs = 0.0;
                    const double* pp = g.oscr + (size_t)o * kMapObsDoubles + kMoP + 12 * c;
#pragma unroll
                    for (int q = 0; q < 12; q++) P[q] = pp[q];
                    pose_mul(P, X, T);
                    for (uint32_t p = ob; p < oe; p++) {
                        if (g.ores[p].status != A3_MAP_OBS_USED || !s_reached[g.obs[p].marker - m0]) continue;
                        double Mq[12], G[12];
                        const double* mq = s_M[0] + (size_t)(g.obs[p].marker - m0) * 12;
#pragma unroll
                        for (int q = 0; q < 12; q++) Mq[q] = mq[q];
                        pose_mul(T, Mq, G);
                        cs = cs + map_cost(s_a, G, s_sq, g.img + 8 * (size_t)p);
                    }
                    if (c == 0) k0 = cs; else k1 = cs;
                }
                if (!have || k0 < bc) { have = true; bc = k0; alt = k1; bo = o; bk = 0; }
                if (k1 < bc) { bc = k1; alt = k0; bo = o; bk = 1; }
            }
            {   // (the chosen hypothesis and its mirror again: the same expressions, the same bits)
                double Mm[12], X[12], P[12], T[12];
                const double* mp = s_M[0] + (size_t)(g.obs[bo].marker - m0) * 12;
#pragma unroll
                for (int q = 0; q < 12; q++) Mm[q] = mp[q];
                pose_inv(Mm, X);
#pragma unroll 1
                for (int c = 0; c < 2; c++) {
                    const double* pp = g.oscr + (size_t)bo * kMapObsDoubles + kMoP + 12 * (c == 0 ? bk : 1 - bk);
#pragma unroll
                    for (int q = 0; q < 12; q++) P[q] = pp[q];
                    pose_mul(P, X, T);
#pragma unroll
                    for (int q = 0; q < 12; q++) fs[kMfPose + 12 * c + q] = T[q];
                }
                fs[kMfK] = bc;
                fs[kMfK + 1] = alt;
                fs[kMfLoc] = (double)cnt;
                s_changed = 1;
            }
        }
        __syncthreads();
        if (tid >= 1 && tid < (int)M && !s_reached[tid]) {   // b: reach markers
            const uint32_t qb = o0 + s_mo[tid], qe = o0 + s_mo[tid + 1];
            bool have = false;
            int nh = 0, bh = 0;
            double bc = 0.0;
            uint32_t bo = 0;
            for (uint32_t qo = qb; qo < qe && nh < A3_MAP_START_OBSERVATIONS; qo++) {
                const uint32_t o = g.ml[qo];
                const double* fso = g.fscr + (size_t)g.obs[o].frame * kMapFrameDoubles;
                if (g.ores[o].status != A3_MAP_OBS_USED || fso[kMfLoc] == 0.0) continue;
                nh++;
#pragma unroll 1
                for (int h = 0; h < 4; h++) {   // the frame's candidate h / 2, the observation's h % 2
                    double Tf[12], X[12], P[12], Mh[12], cs = 0.0;
                    const double* pp = g.oscr + (size_t)o * kMapObsDoubles + kMoP + 12 * (h % 2);
#pragma unroll
                    for (int q = 0; q < 12; q++) { Tf[q] = fso[kMfPose + 12 * (h / 2) + q]; P[q] = pp[q]; }
                    pose_inv(Tf, X);
                    pose_mul(X, P, Mh);
                    for (uint32_t qp = qb; qp < qe; qp++) {
                        const uint32_t p = g.ml[qp];
                        const double* fsp = g.fscr + (size_t)g.obs[p].frame * kMapFrameDoubles;
                        if (g.ores[p].status != A3_MAP_OBS_USED || fsp[kMfLoc] == 0.0) continue;
                        double kk[2];
#pragma unroll
                        for (int c = 0; c < 2; c++) {
                            double Tp[12], G[12];
#pragma unroll
                            for (int q = 0; q < 12; q++) Tp[q] = fsp[kMfPose + 12 * c + q];
                            pose_mul(Tp, Mh, G);
                            kk[c] = fsp[kMfK + c] + map_cost(s_a, G, s_sq, g.img + 8 * (size_t)p);
                        }
                        cs = cs + (kk[1] < kk[0] ? kk[1] : kk[0]);
                    }
                    if (!have || cs < bc) { have = true; bc = cs; bo = o; bh = h; }
                }
            }
            if (have) {
                if (!guess) {
                    double Tf[12], X[12], P[12], Mh[12];
                    const double* fso = g.fscr + (size_t)g.obs[bo].frame * kMapFrameDoubles;
                    const double* pp = g.oscr + (size_t)bo * kMapObsDoubles + kMoP + 12 * (bh % 2);
#pragma unroll
                    for (int q = 0; q < 12; q++) { Tf[q] = fso[kMfPose + 12 * (bh / 2) + q]; P[q] = pp[q]; }
                    pose_inv(Tf, X);
                    pose_mul(X, P, Mh);
#pragma unroll
                    for (int q = 0; q < 12; q++) { s_M[0][tid * 12 + q] = Mh[q]; s_M[1][tid * 12 + q] = Mh[q]; }
                }
                s_reached[tid] = 1;
                s_changed = 1;
            }
        }
        __syncthreads();
        if (!s_changed) break;
    }
    // ---- counts ----
    for (uint32_t j = (uint32_t)tid; j < NO; j += kMapThreads) {
        const uint32_t o = o0 + j;
        if (g.ores[o].status != A3_MAP_OBS_USED) continue;
        if (s_reached[g.obs[o].marker - m0]) g.oscr[(size_t)o * kMapObsDoubles + kMoAct] = 1.0;
        else g.ores[o].status = A3_MAP_OBS_UNREACHED;
    }
    __syncthreads();
    if (tid < (int)M) {
        a3_map_marker_result* mr = &g.mres[m0 + tid];
        uint32_t seen = 0, nu = 0;
        for (uint32_t q = o0 + s_mo[tid]; q < o0 + s_mo[tid + 1]; q++) {
            const uint32_t st = g.ores[g.ml[q]].status;
            if (st == A3_MAP_OBS_USED) nu++;
            if (st != A3_MAP_OBS_DEGENERATE) seen++;
        }
        mr->status = !seen ? A3_MAP_MARKER_UNSEEN : s_reached[tid] ? A3_MAP_MARKER_USED : A3_MAP_MARKER_UNREACHED;
        mr->obs_used = nu;
        for (int q = 0; q < 9; q++) { mr->rotation[q] = 0.0; mr->rotation_f[q] = 0.0f; }
        for (int q = 0; q < 3; q++) { mr->translation[q] = 0.0; mr->translation_f[q] = 0.0f; }
        for (int q = 0; q < 6; q++) mr->std_dev[q] = 0.0;
        for (int q = 0; q < 12; q++) mr->corners[q] = 0.0;
        mr->rms_px = 0.0;
    }
    for (uint32_t j = (uint32_t)tid; j < F; j += kMapThreads) {
        const uint32_t f = f0 + j;
        a3_map_frame* fr = &g.frames[f];
        uint32_t nu = 0;
        for (uint32_t o = v.fbeg(f); o < v.fend(f); o++)
            if (g.ores[o].status == A3_MAP_OBS_USED) nu++;
        fr->status = g.fscr[(size_t)f * kMapFrameDoubles + kMfLoc] != 0.0 ? A3_MAP_FRAME_USED : A3_MAP_FRAME_UNUSED;
        fr->obs_used = nu;
        fr->rms_px = 0.0f;
        fr->reserved = 0;
        for (int q = 0; q < 9; q++) { fr->rotation[q] = 0.0; fr->rotation_f[q] = 0.0f; }
        for (int q = 0; q < 3; q++) { fr->translation[q] = 0.0; fr->translation_f[q] = 0.0f; }
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t fu = 0, ou = 0, mu = 0;
        int nu = 0;
        for (uint32_t j = 0; j < F; j++) {
            if (g.frames[f0 + j].status == A3_MAP_FRAME_USED) fu++;
            ou += g.frames[f0 + j].obs_used;
        }
        for (uint32_t m = 0; m < M; m++) {
            s_pos[m] = -1;
            if (g.mres[m0 + m].status != A3_MAP_MARKER_USED) continue;
            mu++;
            if (m >= 1 && !fix) { s_pos[m] = nu; s_ua[nu++] = (int)m; }
        }
        s_fu = fu; s_ou = ou; s_mu = mu; s_nu = nu;
        if (!fix && (nu == 0 || g.mres[m0].status != A3_MAP_MARKER_USED)) s_status = A3_MAP_NOT_CONNECTED;
    }
    __syncthreads();
    const int nu = s_nu, n = 6 * nu;
    const uint32_t N = 4u * s_ou;
    double* S = g.big + g.big_off[blockIdx.x];
    double* X = S + (size_t)n * n;
    if (s_status == A3_MAP_OK) {
        for (uint32_t j = (uint32_t)wave; j < F; j += kMapWaves) {
            const uint32_t f = f0 + j;
            const double* fs = g.fscr + (size_t)f * kMapFrameDoubles;
            if (fs[kMfLoc] == 0.0) continue;
            double T[12];
#pragma unroll
            for (int q = 0; q < 12; q++) T[q] = fs[kMfPose + q];
            map_frame_eval(v, f, s_M[0], T, 0, rows, lane);
        }
        __syncthreads();
        if (tid == 0) {
            double cost = 0.0;
            for (uint32_t j = 0; j < F; j++) {
                const double* fs = g.fscr + (size_t)(f0 + j) * kMapFrameDoubles;
                if (fs[kMfLoc] != 0.0) cost = cost + fs[kMfVg + 27];
            }
            s_cost = cost;
            if (!fin(cost)) s_status = A3_MAP_NOT_FINITE;
            if (cost == 0.0) { s_stop = 1; s_conv = 1; }
        }
        __syncthreads();
    }
    if (s_status == A3_MAP_OK && fix) {
        // ---- 3. every frame alone ----
        for (uint32_t j = (uint32_t)wave; j < F; j += kMapWaves) {
            const uint32_t f = f0 + j;
            double* fs = g.fscr + (size_t)f * kMapFrameDoubles;
            if (fs[kMfLoc] == 0.0) continue;
            double T[12];
#pragma unroll
            for (int q = 0; q < 12; q++) T[q] = fs[kMfPose + q];
            double c1 = fs[kMfVg + 27], lam = 1e-3;
            int it = 0, cv = 0, fc = 0;
            bool stop = false;
            if (c1 == 0.0) { stop = true; cv = 1; }
            while (!stop) {
                const double* vg = fs + kMfVg + fc * 28;
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
                map_frame_eval(v, f, s_M[0], Tn, 1 - fc, rows, lane);
                const double c2 = fs[kMfVg + (1 - fc) * 28 + 27];
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
                for (int q = 0; q < 12; q++) fs[kMfPose + fc * 12 + q] = T[q];
                fs[kMfCur] = (double)fc;
                atomicMax(&s_iter, it);
                if (!cv) atomicAnd(&s_conv, 0);
            }
            wave_sync();
        }
        __syncthreads();
        if (tid == 0) {
            double cost = 0.0;
            for (uint32_t j = 0; j < F; j++) {
                const double* fs = g.fscr + (size_t)(f0 + j) * kMapFrameDoubles;
                if (fs[kMfLoc] != 0.0) cost = cost + fs[kMfVg + (fs[kMfCur] != 0.0 ? 28 : 0) + 27];
            }
            s_cost = cost;
        }
        __syncthreads();
    }
    if (s_status == A3_MAP_OK && !fix) {
        // ---- 3. joint LM; its last pass (s_cov) is step 4's undamped reduced system ----
        while (true) {
            __syncthreads();
            if (tid == 0 && s_stop) { s_cov = 1; s_lambda = 0.0; }
            __syncthreads();
            const int cur = s_cur, cov = s_cov;
            const double lambda = s_lambda;
            if (s_sums)
                for (int t = tid; t < nu * 27; t += kMapThreads) {
                    const int u = t / 27, e = t % 27;
                    int i = 0, k = 0;
                    if (e < 21) tri_ik(e, 6, &i, &k);
                    const int idx = e < 21 ? tri_index(6 + i, 6 + k, kRigAug) : tri_index(6 + (e - 21), 12, kRigAug);
                    double s = 0.0;
                    for (uint32_t q = o0 + s_mo[s_ua[u]]; q < o0 + s_mo[s_ua[u] + 1]; q++) {
                        const double* os = g.oscr + (size_t)g.ml[q] * kMapObsDoubles;
                        if (os[kMoAct] != 0.0) s = s + os[kMoBlk + cur * kRigEntries + idx];
                    }
                    g.mscr[(size_t)(m0 + (uint32_t)s_ua[u]) * kMapMarkerDoubles + kMmU + e] = s;
                }
            for (uint32_t j = (uint32_t)wave; j < F; j += kMapWaves) {
                const uint32_t f = f0 + j;
                double* fs = g.fscr + (size_t)f * kMapFrameDoubles;
                if (fs[kMfLoc] == 0.0) continue;
                const double* vg = fs + kMfVg + cur * 28;
                double L[6][6], D[6];
                if (!ldl6_at<0, 7>(vg, lambda, L, D)) {
                    if (lane == 0) s_bad = 1;
                    continue;
                }
                const uint32_t ob = v.fbeg(f), cnt = v.fend(f) - ob;
                for (uint32_t t = (uint32_t)lane; t <= 6 * cnt; t += 64) {
                    double b[6], y[6];
                    if (t < 6 * cnt) {
                        const uint32_t o = ob + t / 6;
                        const int k = (int)(t % 6);
                        double* os = g.oscr + (size_t)o * kMapObsDoubles;
                        if (os[kMoAct] == 0.0 || g.obs[o].marker == m0) continue;
                        const double* blk = os + kMoBlk + cur * kRigEntries;
#pragma unroll
                        for (int q = 0; q < 6; q++) b[q] = blk[tri_index(q, 6 + k, kRigAug)];
                        ldl6_solve(L, D, b, y);
#pragma unroll
                        for (int q = 0; q < 6; q++) os[kMoY + k * 6 + q] = y[q];
                    } else {
#pragma unroll
                        for (int q = 0; q < 6; q++) b[q] = vg[tri_index(q, 6, 7)];
                        ldl6_solve(L, D, b, y);
#pragma unroll
                        for (int q = 0; q < 6; q++) fs[kMfYg + q] = y[q];
                    }
                }
            }
            __syncthreads();
            if (!s_bad)
                for (int e = tid; e < n * (n + 1); e += kMapThreads) {
                    const int i = e / (n + 1), k = e % (n + 1);
                    if (k < i) continue;
                    const int ui = s_ua[i / 6], uk = k < n ? s_ua[k / 6] : ui;
                    const double* U = g.mscr + (size_t)(m0 + (uint32_t)ui) * kMapMarkerDoubles + kMmU;
                    double s;
                    if (k < n) {
                        s = ui == uk ? U[tri_index(i % 6, k % 6, 6)] : 0.0;
                        if (i == k) s = s + lambda * s;
                    } else s = -U[21 + i % 6];
                    for (uint32_t qi = o0 + s_mo[ui]; qi < o0 + s_mo[ui + 1]; qi++) {
                        const uint32_t oi = g.ml[qi];
                        const double* osi = g.oscr + (size_t)oi * kMapObsDoubles;
                        if (osi[kMoAct] == 0.0) continue;
                        const uint32_t f = g.obs[oi].frame;
                        const double* y = nullptr;
                        if (k == n) y = g.fscr + (size_t)f * kMapFrameDoubles + kMfYg;
                        else if (uk == ui) y = osi + kMoY + (k % 6) * 6;
                        else
                            for (uint32_t p = v.fbeg(f); p < v.fend(f); p++)
                                if (g.obs[p].marker == m0 + (uint32_t)uk && g.oscr[(size_t)p * kMapObsDoubles + kMoAct] != 0.0)
                                    y = g.oscr + (size_t)p * kMapObsDoubles + kMoY + (k % 6) * 6;
                        if (!y) continue;
                        const double* blk = osi + kMoBlk + cur * kRigEntries;
                        double t = 0.0;
#pragma unroll
                        for (int q = 0; q < 6; q++) t = t + blk[tri_index(q, 6 + i % 6, kRigAug)] * y[q];
                        s = k < n ? s - t : s + t;
                    }
                    if (k < n) S[(size_t)i * n + k] = s;
                    else s_x[i] = s;
                }
            __syncthreads();
            bool bad = s_bad != 0;
            if (!bad) bad = !map_ldl(S, n, s_D, tid, &s_flag);
            if (cov) {
                const long long dof = 2ll * N - n - 6ll * s_fu;
                const double sigma2 = s_cost / (double)dof;
                for (int t = tid; t < n; t += kMapThreads) {
                    double dv = __builtin_inf();
                    if (!bad && dof > 0) {
                        for (int i = 0; i < n; i++) {
                            double s = i == t ? 1.0 : 0.0;
                            for (int k = 0; k < i; k++) s = s - S[(size_t)k * n + i] * X[(size_t)k * n + t];
                            X[(size_t)i * n + t] = s;
                        }
                        for (int i = n - 1; i >= 0; i--) {
                            double s = X[(size_t)i * n + t] / s_D[i];
                            for (int k = n - 1; k > i; k--) s = s - S[(size_t)i * n + k] * X[(size_t)k * n + t];
                            X[(size_t)i * n + t] = s;
                        }
                        dv = sqrt(sigma2 * X[(size_t)t * n + t]);
                    }
                    g.mscr[(size_t)(m0 + (uint32_t)s_ua[t / 6]) * kMapMarkerDoubles + kMmStd + t % 6] = dv;
                }
                __syncthreads();
                break;
            }
            if (!bad) {
                map_solve(S, n, s_D, s_x, tid);
                if (tid < nu) {
                    const int m = s_ua[tid];
                    double E[12], d[6], En[12];
#pragma unroll
                    for (int q = 0; q < 12; q++) E[q] = s_M[cur][m * 12 + q];
#pragma unroll
                    for (int q = 0; q < 6; q++) d[q] = s_x[6 * tid + q];
                    pose_update(E, d, En);
#pragma unroll
                    for (int q = 0; q < 12; q++) s_M[1 - cur][m * 12 + q] = En[q];
                }
            }
            __syncthreads();
            if (tid == 0) {
                s_bad = 0;
                s_skip = bad ? 1 : 0;
                s_sums = 0;
                if (bad) {
                    s_lambda = lambda * 10.0;
                    s_iter = s_iter + 1;
                    if (s_iter >= maxit) s_stop = 1;
                }
            }
            __syncthreads();
            if (s_skip) continue;
            for (uint32_t j = (uint32_t)wave; j < F; j += kMapWaves) {
                const uint32_t f = f0 + j;
                double* fs = g.fscr + (size_t)f * kMapFrameDoubles;
                if (fs[kMfLoc] == 0.0) continue;
                const double* vg = fs + kMfVg + cur * 28;
                double L[6][6], D[6], b[6], d[6], sm[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                ldl6_at<0, 7>(vg, lambda, L, D);
                for (uint32_t o = v.fbeg(f); o < v.fend(f); o++) {
                    const double* os = g.oscr + (size_t)o * kMapObsDoubles;
                    if (os[kMoAct] == 0.0 || g.obs[o].marker == m0) continue;
                    const int u = s_pos[g.obs[o].marker - m0];
                    const double* blk = os + kMoBlk + cur * kRigEntries;
                    for (int k = 0; k < 6; k++) {
                        const double dk = s_x[6 * u + k];
#pragma unroll
                        for (int q = 0; q < 6; q++) sm[q] = sm[q] + blk[tri_index(q, 6 + k, kRigAug)] * dk;
                    }
                }
#pragma unroll
                for (int q = 0; q < 6; q++) b[q] = -vg[tri_index(q, 6, 7)] - sm[q];
                ldl6_solve(L, D, b, d);
                double T[12], Tn[12];
#pragma unroll
                for (int q = 0; q < 12; q++) T[q] = fs[kMfPose + cur * 12 + q];
                pose_update(T, d, Tn);
                if (lane == 0) {
#pragma unroll
                    for (int q = 0; q < 12; q++) fs[kMfPose + (1 - cur) * 12 + q] = Tn[q];
                }
                map_frame_eval(v, f, s_M[1 - cur], Tn, 1 - cur, rows, lane);
            }
            __syncthreads();
            if (tid == 0) {
                double c2 = 0.0;
                for (uint32_t j = 0; j < F; j++) {
                    const double* fs = g.fscr + (size_t)(f0 + j) * kMapFrameDoubles;
                    if (fs[kMfLoc] != 0.0) c2 = c2 + fs[kMfVg + (1 - cur) * 28 + 27];
                }
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
        for (uint32_t j = (uint32_t)tid; j < F; j += kMapThreads) g.fscr[(size_t)(f0 + j) * kMapFrameDoubles + kMfCur] = (double)cur;
        __syncthreads();
    }
    // ---- 4. results ----
    const bool ok = s_status == A3_MAP_OK;
    if (tid == 0) {
        a3_map_result* r = &g.res[blockIdx.x];
        r->status = (uint32_t)s_status;
        r->markers_used = s_mu;
        r->frames_used = s_fu;
        r->obs_used = s_ou;
        r->iterations = ok ? (uint32_t)s_iter : 0u;
        r->converged = ok ? (uint32_t)s_conv : 0u;
        r->rms_px = ok && N ? sqrt(s_cost / (double)N) : 0.0;
    }
    if (ok && tid < (int)M && g.mres[m0 + tid].status == A3_MAP_MARKER_USED) {
        a3_map_marker_result* mr = &g.mres[m0 + tid];
        const double* Mm = s_M[fix ? 0 : s_cur] + tid * 12;
        double cc = 0.0;
        for (uint32_t q = o0 + s_mo[tid]; q < o0 + s_mo[tid + 1]; q++) {
            const uint32_t o = g.ml[q];
            const double* os = g.oscr + (size_t)o * kMapObsDoubles;
            if (os[kMoAct] == 0.0) continue;
            const int fc = g.fscr[(size_t)g.obs[o].frame * kMapFrameDoubles + kMfCur] != 0.0 ? 1 : 0;
            cc = cc + os[kMoBlk + fc * kRigEntries + kRigEntries - 1];
        }
        for (int q = 0; q < 9; q++) { mr->rotation[q] = Mm[q]; mr->rotation_f[q] = (float)Mm[q]; }
        for (int q = 0; q < 3; q++) { mr->translation[q] = Mm[9 + q]; mr->translation_f[q] = (float)Mm[9 + q]; }
        for (int q = 0; q < 6; q++) mr->std_dev[q] = s_pos[tid] >= 0 ? g.mscr[(size_t)(m0 + tid) * kMapMarkerDoubles + kMmStd + q] : 0.0;
        mr->rms_px = mr->obs_used ? sqrt(cc / (double)(4u * mr->obs_used)) : 0.0;
        for (int j = 0; j < 4; j++)
            for (int r = 0; r < 3; r++)
                mr->corners[3 * j + r] = (Mm[3 * r] * (double)s_sq[2 * j] + Mm[3 * r + 1] * (double)s_sq[2 * j + 1]) + Mm[9 + r];
    }
    if (ok)
        for (uint32_t j = (uint32_t)tid; j < F; j += kMapThreads) {
            const uint32_t f = f0 + j;
            a3_map_frame* fr = &g.frames[f];
            if (fr->status != A3_MAP_FRAME_USED) continue;
            const double* fs = g.fscr + (size_t)f * kMapFrameDoubles;
            const int fc = fs[kMfCur] != 0.0 ? 1 : 0;
            fr->rms_px = (float)sqrt(fs[kMfVg + fc * 28 + 27] / (double)(4u * fr->obs_used));
            for (int q = 0; q < 9; q++) { fr->rotation[q] = fs[kMfPose + fc * 12 + q]; fr->rotation_f[q] = (float)fs[kMfPose + fc * 12 + q]; }
            for (int q = 0; q < 3; q++) { fr->translation[q] = fs[kMfPose + fc * 12 + 9 + q]; fr->translation_f[q] = (float)fs[kMfPose + fc * 12 + 9 + q]; }
            for (uint32_t o = v.fbeg(f); o < v.fend(f); o++) {
                const double* os = g.oscr + (size_t)o * kMapObsDoubles;
                if (os[kMoAct] != 0.0) g.ores[o].rms_px = (float)sqrt(os[kMoBlk + fc * kRigEntries + kRigEntries - 1] / 4.0);
            }
        }
}

size_t map_obs_bytes() { return kMapObsDoubles * sizeof(double); }
size_t map_frame_bytes() { return kMapFrameDoubles * sizeof(double); }
size_t map_marker_bytes() { return kMapMarkerDoubles * sizeof(double); }

hipError_t launch_map(hipStream_t st, const MapLaunch& m) {
    if (m.n_maps == 0) return hipSuccess;
    const MapArgs g{m.maps, m.markers, m.obs, m.img, m.big_off, m.fo, m.ml, m.oscr, m.fscr, m.mscr, m.big, m.res, m.mres, m.frames, m.ores};
    hipLaunchKernelGGL(k_map, dim3(m.n_maps), dim3(kMapThreads), 0, st, g);
    return hipGetLastError();
}

}  // namespace a3
