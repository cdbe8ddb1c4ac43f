// k_handeye.hip -- hand-eye calibration by reprojection error (a3_calibrate_hand_eyes).  Not part of the reference: an extension stated
// in include/aruco3_hip.h and restated on the CPU by tests/handeye_oracle.c (a3o_calibrate_hand_eyes), which this kernel matches bit for
// bit.
//
// One workgroup of four waves per problem, on the structure of k_rig; every phase runs inside the one launch, separated by barriers.
// Per-frame work (step 1's homography and pose LM, every evaluation of a frame's 91-entry block) goes to one wave (frames w, w + 4,
// ...): the lanes write the rows of up to 64 points into the wave's LDS, then each lane owns up to two of the 91 entries and adds the
// rows in point order (aug_block, a3_solve.h; step 1's pose start is its pose_from_h).  The start's pair sums take one thread per frame i (the partial over j > i in order), thread 0 adds the
// partials in i order and solves the charts and the translation.  The 91 sums over the frames take one thread each, in frame order;
// the damped 12 x 12 system, its LDL^T and the covariance are thread 0's.  Blocks, step 1's poses and the pair partials live in device
// scratch, kHeFrameDoubles per frame.  A shared flag is read into a register and a barrier passed before thread 0 may change it, so
// that every barrier is reached by all threads.
#include <cmath>

#include "a3_common.h"
#include "a3_launch.h"
#include "a3_handeye.h"

namespace a3 {

constexpr int kHeThreads = 256, kHeWaves = 4;
constexpr int kHeRowStride = 2 * kRigAug;   // doubles per point in LDS: the u row, then the v row
// per-frame scratch: blocks (2 slots), P (step 1's pose; the homography before it), step 1's cost, the frame's pair partial
constexpr int kHeBlk = 0, kHeP = 2 * kRigEntries, kHeCost = kHeP + 12, kHePart = kHeCost + 1;
constexpr size_t kHeFrameDoubles = 208;
static_assert(kHePart + 10 <= (int)kHeFrameDoubles, "frame scratch");
static_assert(64 * kHeRowStride >= 64 + 64 + 8 + 8 && 64 * kHeRowStride >= 64 * 2 * kHomAug, "the homography works in the row buffer");
static_assert(A3_HANDEYE_MAX_FRAMES <= kHeThreads, "one thread per frame in the pair sums");

struct HeArgs {
    const a3_handeye_problem* probs;
    const a3_handeye_frame* frames;
    const float* obj;
    const float* img;
    double* fscr;
    a3_handeye_result* res;
    a3_handeye_frame_result* fres;
};

__device__ __forceinline__ void frame_pose(const a3_handeye_frame* fr, double* M) {
#pragma unroll
    for (int q = 0; q < 9; q++) M[q] = fr->rotation[q];
#pragma unroll
    for (int q = 0; q < 3; q++) M[9 + q] = fr->translation[q];
}

// the blocks of the problem's USED frames at (X, Y) into `slot` (wave w takes frames w, w + 4, ...)
__device__ __forceinline__ void frames_eval(const HeArgs& g, uint32_t f0, uint32_t F, const double* s_a, const double* sX, const double* sY, int slot,
                                            double* rows, int wave, int lane) {
    for (uint32_t j = (uint32_t)wave; j < F; j += kHeWaves) {
        const uint32_t f = f0 + j;
        if (g.fres[f].status != A3_HANDEYE_FRAME_USED) continue;
        double a[12], X[12], Y[12], M[12], Ep[12], G[12];
#pragma unroll
        for (int q = 0; q < 12; q++) { a[q] = s_a[q]; X[q] = sX[q]; Y[q] = sY[q]; }
        frame_pose(&g.frames[f], M);
        pose_mul(X, M, Ep);
        pose_mul(Ep, Y, G);
        aug_block<kRigAug>([&](double Xc, double Yc, double ou, double ov, double* au, double* av) { he_row(a, X, M, Y, Ep, G, Xc, Yc, ou, ov, au, av); }, g.obj,
                 g.img, g.frames[f].first_point, g.frames[f].n_points, rows, lane, g.fscr + (size_t)f * kHeFrameDoubles + kHeBlk + slot * kRigEntries);
    }
}

// the free part of S damped by lambda -> LDL^T in A (row stride 12), D; false on a bad pivot
__device__ inline bool he_system(const double* S, int n, int off, double lambda, double* A, double* D) {
    for (int i = 0; i < n; i++)
        for (int k = i; k < n; k++) { const double v = S[tri_index(off + i, off + k, kRigAug)]; A[i * 12 + k] = v; A[k * 12 + i] = v; }
    for (int i = 0; i < n; i++) A[i * 12 + i] = A[i * 12 + i] + lambda * A[i * 12 + i];
    return ldl_n<12>(A, n, D);
}

__global__ __launch_bounds__(kHeThreads) void k_handeye(HeArgs g) {
    __shared__ double s_rows[kHeWaves][64 * kHeRowStride];
    __shared__ double s_wv[kHeWaves][8];
    __shared__ double s_S[2][kRigEntries];
    __shared__ double s_X[2][12], s_Y[2][12], s_a[12];
    __shared__ double s_A[144], s_D[12], s_b[12], s_d[12], s_e[12], s_x[12], s_std[12];
    __shared__ double s_cost, s_lambda;
    __shared__ int s_status, s_stop, s_skip, s_cur, s_iter, s_conv;
    __shared__ uint32_t s_fu, s_np, s_pairs;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const a3_handeye_problem* R = &g.probs[blockIdx.x];
    const uint32_t f0 = R->first_frame, F = R->n_frames;
    const bool fixx = (R->flags & A3_HANDEYE_FIX_X) != 0, guess = (R->flags & A3_HANDEYE_USE_GUESS) != 0;
    const int maxit = R->max_iterations ? (int)R->max_iterations : A3_CALIB_DEFAULT_ITERATIONS;
    const int n = fixx ? 6 : 12, off = fixx ? 6 : 0;
    double* rows = s_rows[wave];
    double* wv = s_wv[wave];

    if (tid < 12) { s_a[tid] = R->a[tid]; s_std[tid] = 0.0; }
    if (tid == 0) {
        s_status = A3_HANDEYE_OK;
        s_stop = 0; s_skip = 0; s_cur = 0; s_iter = 0; s_conv = 0;
        s_lambda = 1e-3;
        s_cost = 0.0;
        s_pairs = 0u;
    }
    __syncthreads();
    // ---- 1. per frame: homography, pose start, pose LM ----
    for (uint32_t j = (uint32_t)wave; j < F; j += kHeWaves) {
        const uint32_t f = f0 + j;
        const uint32_t p0 = g.frames[f].first_point, np = g.frames[f].n_points;
        double* os = g.fscr + (size_t)f * kHeFrameDoubles;
        uint32_t st = A3_HANDEYE_FRAME_TOO_FEW_POINTS;
        if (np >= 4) st = view_homography(g.obj, g.img, p0, np, rows, wv, lane, os + kHeP) ? A3_HANDEYE_FRAME_USED : A3_HANDEYE_FRAME_DEGENERATE;
        a3_handeye_frame_result* rec = &g.fres[f];
        if (st != A3_HANDEYE_FRAME_USED) {
            if (lane == 0) {
                rec->status = st;
                rec->points = np;
                rec->rms_px = 0.0f;
                rec->reserved = 0;
                for (int q = 0; q < 9; q++) { rec->rotation[q] = 0.0; rec->rotation_f[q] = 0.0f; }
                for (int q = 0; q < 3; q++) { rec->translation[q] = 0.0; rec->translation_f[q] = 0.0f; }
            }
            continue;
        }
        double a[12];
#pragma unroll
        for (int q = 0; q < 12; q++) a[q] = s_a[q];
        const double* H = os + kHeP;
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
        double* cur = os + kHeBlk;
        double* oth = cur + kRigEntries;
        aug_block<kRigAug>([&](double Xc, double Yc, double ou, double ov, double* au, double* av) { rig_row(a, ID, T, T, Xc, Yc, ou, ov, au, av); }, g.obj, g.img,
                 p0, np, rows, lane, cur);
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
            aug_block<kRigAug>([&](double Xc, double Yc, double ou, double ov, double* au, double* av) { rig_row(a, ID, Tn, Tn, Xc, Yc, ou, ov, au, av); }, g.obj,
                     g.img, p0, np, rows, lane, oth);
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
            for (int q = 0; q < 12; q++) os[kHeP + q] = T[q];
            os[kHeCost] = cost;
            rec->status = st;
            rec->points = np;
            rec->rms_px = 0.0f;
            rec->reserved = 0;
            for (int q = 0; q < 9; q++) { rec->rotation[q] = T[q]; rec->rotation_f[q] = (float)T[q]; }
            for (int q = 0; q < 3; q++) { rec->translation[q] = T[9 + q]; rec->translation_f[q] = (float)T[9 + q]; }
        }
        wave_sync();
    }
    __syncthreads();
    if (tid == 0) {
        uint32_t fu = 0, np = 0;
        for (uint32_t j = 0; j < F; j++)
            if (g.fres[f0 + j].status == A3_HANDEYE_FRAME_USED) { fu++; np += g.frames[f0 + j].n_points; }
        s_fu = fu; s_np = np;
        if (fu < 3) s_status = A3_HANDEYE_TOO_FEW_FRAMES;
        for (int q = 0; q < 12; q++) {
            const double id = q == 0 || q == 4 || q == 8 ? 1.0 : 0.0;
            s_X[0][q] = fixx || guess ? (q < 9 ? R->guess_x_rotation[q] : R->guess_x_translation[q - 9]) : id;
            s_Y[0][q] = guess ? (q < 9 ? R->guess_y_rotation[q] : R->guess_y_translation[q - 9]) : id;
        }
    }
    __syncthreads();
    // ---- 2. the start: pair sums (one thread per frame i), charts, translation, Y ----
    int st = s_status;
    const bool start = st == A3_HANDEYE_OK && !(fixx || guess);
    for (int pass = 0; pass < 2; pass++) {
        const bool run = start && st == A3_HANDEYE_OK;
        const int ns = pass == 0 ? 10 : 9;
        if (run)
            for (uint32_t i = (uint32_t)tid; i < F; i += kHeThreads) {
                double part[10], A[12], B[12], Mi[12], Mj[12], Pi[12], Pj[12], RX[9], qa[4], qb[4];
                uint32_t cnt = 0;
#pragma unroll
                for (int e = 0; e < 10; e++) part[e] = 0.0;
#pragma unroll
                for (int q = 0; q < 9; q++) RX[q] = s_X[0][q];
                if (g.fres[f0 + i].status == A3_HANDEYE_FRAME_USED) {
                    frame_pose(&g.frames[f0 + i], Mi);
                    for (int q = 0; q < 12; q++) Pi[q] = g.fscr[(size_t)(f0 + i) * kHeFrameDoubles + kHeP + q];
                    for (uint32_t j = i + 1; j < F; j++) {
                        if (g.fres[f0 + j].status != A3_HANDEYE_FRAME_USED) continue;
                        frame_pose(&g.frames[f0 + j], Mj);
                        for (int q = 0; q < 12; q++) Pj[q] = g.fscr[(size_t)(f0 + j) * kHeFrameDoubles + kHeP + q];
                        if (!he_pair(Pi, Pj, Mi, Mj, A, B, qa, qb)) continue;
                        cnt++;
                        if (pass == 0) he_pair_rot(qa, qb, part);
                        else he_pair_tr(A, B, RX, part);
                    }
                }
                for (int e = 0; e < ns; e++) g.fscr[(size_t)(f0 + i) * kHeFrameDoubles + kHePart + e] = part[e];
                if (pass == 0 && cnt) atomicAdd(&s_pairs, cnt);
            }
        __syncthreads();
        if (run && tid == 0) {
            double sum[10];
            for (int e = 0; e < ns; e++) sum[e] = 0.0;
            for (uint32_t i = 0; i < F; i++)
                for (int e = 0; e < ns; e++) sum[e] = sum[e] + g.fscr[(size_t)(f0 + i) * kHeFrameDoubles + kHePart + e];
            if (pass == 0) {
                double q[4], RX[9];
                if (s_pairs == 0u || !he_charts(sum, q)) s_status = A3_HANDEYE_NO_MOTION;
                else {
                    he_quat_rot(q, RX);
                    for (int e = 0; e < 9; e++) s_X[0][e] = RX[e];
                }
            } else {
                double t[3];
                if (!he_solve3(sum, sum + 6, t)) s_status = A3_HANDEYE_NO_MOTION;
                else
                    for (int e = 0; e < 3; e++) s_X[0][9 + e] = t[e];
            }
        }
        __syncthreads();
        st = s_status;
    }
    if (st == A3_HANDEYE_OK && !guess && tid == 0) {
        int bf = -1;
        double bs = 0.0;
        for (uint32_t j = 0; j < F; j++) {
            if (g.fres[f0 + j].status != A3_HANDEYE_FRAME_USED) continue;
            const double s = g.fscr[(size_t)(f0 + j) * kHeFrameDoubles + kHeCost] / (double)g.frames[f0 + j].n_points;
            if (bf < 0 || s < bs) { bf = (int)j; bs = s; }
        }
        double M[12], Mi[12], X[12], Xi[12], P[12], Z[12], Y[12];
        frame_pose(&g.frames[f0 + (uint32_t)bf], M);
        for (int q = 0; q < 12; q++) { X[q] = s_X[0][q]; P[q] = g.fscr[(size_t)(f0 + (uint32_t)bf) * kHeFrameDoubles + kHeP + q]; }
        pose_inv(M, Mi);
        pose_inv(X, Xi);
        pose_mul(Xi, P, Z);
        pose_mul(Mi, Z, Y);
        for (int q = 0; q < 12; q++) s_Y[0][q] = Y[q];
    }
    __syncthreads();
    // ---- 3. joint LM over (w, t) of X and of Y ----
    if (st == A3_HANDEYE_OK) frames_eval(g, f0, F, s_a, s_X[0], s_Y[0], 0, rows, wave, lane);
    __syncthreads();
    if (st == A3_HANDEYE_OK && tid < kRigEntries) {
        double s = 0.0;
        for (uint32_t j = 0; j < F; j++)
            if (g.fres[f0 + j].status == A3_HANDEYE_FRAME_USED) s = s + g.fscr[(size_t)(f0 + j) * kHeFrameDoubles + kHeBlk + tid];
        s_S[0][tid] = s;
    }
    __syncthreads();
    if (st == A3_HANDEYE_OK && tid == 0) {
        const double cost = s_S[0][kRigEntries - 1];
        s_cost = cost;
        if (!fin(cost)) s_status = A3_HANDEYE_NOT_FINITE;
        if (cost == 0.0) { s_stop = 1; s_conv = 1; }
    }
    __syncthreads();
    st = s_status;
    if (st == A3_HANDEYE_OK) {
        while (true) {
            const int stop = s_stop, cur = s_cur;
            __syncthreads();
            if (stop) break;
            if (tid == 0) {
                const double lambda = s_lambda;
                if (!he_system(s_S[cur], n, off, lambda, s_A, s_D)) {
                    s_skip = 1;
                    s_lambda = lambda * 10.0;
                    s_iter = s_iter + 1;
                    if (s_iter >= maxit) s_stop = 1;
                } else {
                    s_skip = 0;
                    for (int i = 0; i < n; i++) s_b[i] = -s_S[cur][tri_index(off + i, 12, kRigAug)];
                    ldl_n_solve<12>(s_A, n, s_D, s_b, s_d);
                    double T[12], d[6], Tn[12];
                    for (int q = 0; q < 12; q++) T[q] = s_X[cur][q];
                    if (fixx) {
                        for (int q = 0; q < 12; q++) Tn[q] = T[q];
                    } else {
                        for (int q = 0; q < 6; q++) d[q] = s_d[q];
                        pose_update(T, d, Tn);
                    }
                    for (int q = 0; q < 12; q++) s_X[1 - cur][q] = Tn[q];
                    for (int q = 0; q < 12; q++) T[q] = s_Y[cur][q];
                    for (int q = 0; q < 6; q++) d[q] = s_d[n - 6 + q];
                    pose_update(T, d, Tn);
                    for (int q = 0; q < 12; q++) s_Y[1 - cur][q] = Tn[q];
                }
            }
            __syncthreads();
            if (!s_skip) {
                frames_eval(g, f0, F, s_a, s_X[1 - cur], s_Y[1 - cur], 1 - cur, rows, wave, lane);
                __syncthreads();
                if (tid < kRigEntries) {
                    double s = 0.0;
                    for (uint32_t j = 0; j < F; j++)
                        if (g.fres[f0 + j].status == A3_HANDEYE_FRAME_USED)
                            s = s + g.fscr[(size_t)(f0 + j) * kHeFrameDoubles + kHeBlk + (1 - cur) * kRigEntries + tid];
                    s_S[1 - cur][tid] = s;
                }
                __syncthreads();
                if (tid == 0) {
                    const double c2 = s_S[1 - cur][kRigEntries - 1], cost = s_cost, lambda = s_lambda;
                    s_iter = s_iter + 1;
                    if (c2 < cost) {
                        const double rel = (cost - c2) / cost;
                        s_cur = 1 - cur;
                        s_cost = c2;
                        s_lambda = lambda / 10.0;
                        if (rel < A3_CALIB_REL_TOL || c2 == 0.0) { s_conv = 1; s_stop = 1; }
                    } else s_lambda = lambda * 10.0;
                    if (s_iter >= maxit) s_stop = 1;
                }
            }
            __syncthreads();
        }
        // ---- 4. the deviations ----
        if (tid == 0) {
            const bool bad = !he_system(s_S[s_cur], n, off, 0.0, s_A, s_D);
            const double sigma2 = s_cost / (double)(2ll * s_np - n);
            for (int i = 0; i < n; i++) {
                double dv = __builtin_inf();
                if (!bad) {
                    for (int k = 0; k < n; k++) s_e[k] = k == i ? 1.0 : 0.0;
                    ldl_n_solve<12>(s_A, n, s_D, s_e, s_x);
                    dv = sqrt(sigma2 * s_x[i]);
                }
                s_std[off + i] = dv;
            }
        }
        __syncthreads();
    }
    // ---- results ----
    const bool ok = st == A3_HANDEYE_OK;
    const int cur = s_cur;
    if (tid == 0) {
        a3_handeye_result* r = &g.res[blockIdx.x];
        r->status = (uint32_t)st;
        r->frames_used = s_fu;
        r->points_used = s_np;
        r->pairs_used = s_pairs;
        r->iterations = ok ? (uint32_t)s_iter : 0u;
        r->converged = ok ? (uint32_t)s_conv : 0u;
        r->rms_px = ok ? sqrt(s_cost / (double)s_np) : 0.0;
        for (int q = 0; q < 9; q++) {
            r->x_rotation[q] = ok ? s_X[cur][q] : 0.0; r->x_rotation_f[q] = ok ? (float)s_X[cur][q] : 0.0f;
            r->y_rotation[q] = ok ? s_Y[cur][q] : 0.0; r->y_rotation_f[q] = ok ? (float)s_Y[cur][q] : 0.0f;
        }
        for (int q = 0; q < 3; q++) {
            r->x_translation[q] = ok ? s_X[cur][9 + q] : 0.0; r->x_translation_f[q] = ok ? (float)s_X[cur][9 + q] : 0.0f;
            r->y_translation[q] = ok ? s_Y[cur][9 + q] : 0.0; r->y_translation_f[q] = ok ? (float)s_Y[cur][9 + q] : 0.0f;
        }
        for (int q = 0; q < 12; q++) r->std_dev[q] = ok ? s_std[q] : 0.0;
    }
    if (ok)
        for (uint32_t j = (uint32_t)tid; j < F; j += kHeThreads) {
            a3_handeye_frame_result* rec = &g.fres[f0 + j];
            if (rec->status == A3_HANDEYE_FRAME_USED)
                rec->rms_px = (float)sqrt(g.fscr[(size_t)(f0 + j) * kHeFrameDoubles + kHeBlk + cur * kRigEntries + kRigEntries - 1] / (double)rec->points);
        }
}

size_t handeye_frame_bytes() { return kHeFrameDoubles * sizeof(double); }

hipError_t launch_handeye(hipStream_t st, const a3_handeye_problem* probs, uint32_t n_probs, const a3_handeye_frame* frames, const float* obj,
                          const float* img, double* fscr, a3_handeye_result* res, a3_handeye_frame_result* fres) {
    if (n_probs == 0) return hipSuccess;
    const HeArgs g{probs, frames, obj, img, fscr, res, fres};
    hipLaunchKernelGGL(k_handeye, dim3(n_probs), dim3(kHeThreads), 0, st, g);
    return hipGetLastError();
}

}  // namespace a3
