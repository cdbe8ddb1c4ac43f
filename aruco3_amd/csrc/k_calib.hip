// k_calib.hip -- camera calibration (a3_calibrate_cameras).  Not part of the reference: an extension stated in include/aruco3_hip.h and
// restated on the CPU by tests/calib_oracle.c (a3o_calibrate), which this kernel matches bit for bit.
//
// One workgroup of four waves per camera: the homographies, the initialisation, the per-view pose starts, the joint Levenberg-Marquardt
// and the covariance all run inside the one launch, their phases separated by barriers.  Per-view work goes to one wave (views w, w + 4,
// ...).  A view's sums run in point order: the lanes write the augmented rows of up to 64 points into the wave's LDS, then each lane owns
// up to three of the 190 block entries and adds the rows in order -- deterministic sums with three accumulators per lane instead of 190.
// Camera-level sums run over the views in view order, one lane of wave 0 per entry; the <= 12 x 12 Schur system is solved by one lane.
// Per-view blocks, poses and Schur terms live in a device scratch buffer of kCalViewDoubles per view.  The block accumulator
// (aug_block), the pose start (pose_from_h) and the small solves are a3_solve.h's, shared with the other solver kernels.
#include <cmath>

#include "a3_common.h"
#include "a3_launch.h"
#include "a3_calib.h"

namespace a3 {

constexpr int kCalThreads = 256, kCalWaves = 4;
constexpr int kRowStride = 2 * kCalAug;   // doubles per point in LDS: the u row, then the v row
// per-view scratch: blocks (2 slots), poses (2 slots: R 9, t 3), Schur terms (<= 78 + 12), homography
constexpr int kOffBlk = 0, kOffPose = 2 * kCalEntries, kOffCon = kOffPose + 24, kOffH = kOffCon + 90;
constexpr size_t kCalViewDoubles = 504;
static_assert(kOffH + 9 <= (int)kCalViewDoubles, "view scratch");

struct CalibArgs {
    const a3_calib_camera* cams;
    const uint32_t* view_off;
    const float* obj;
    const float* img;
    double* scratch;
    a3_calib_result* res;
    a3_calib_view* views;
};

__device__ __forceinline__ bool cal_free(uint32_t flags, int i) {
    if (i == 2 || i == 3) return !(flags & A3_CALIB_FIX_PRINCIPAL_POINT);
    if (i == 6 || i == 7) return !(flags & A3_CALIB_ZERO_TANGENT_DIST);
    if (i == 8) return !(flags & A3_CALIB_FIX_K3);
    if (i >= 9) return (flags & A3_CALIB_RATIONAL_MODEL) != 0;
    return true;
}

// one view's 190 block entries at (a, R, t) -> out (wave-level): aug_block (a3_solve.h) over calib_row
__device__ __forceinline__ void view_block(const double a[12], const double R[9], const double t[3], const float* __restrict__ obj, const float* __restrict__ img,
                           uint32_t p0, uint32_t np, double* rows, int lane, double* out) {
    aug_block<kCalAug>([&](double X, double Y, double ou, double ov, double* au, double* av) { calib_row(a, R, t, X, Y, ou, ov, au, av); }, obj, img, p0,
                       np, rows, lane, out);
}

// step 4's per-view Schur terms at `lambda` from block slot `slot` (wave-level, every USED view of the wave); a bad pivot sets *bad
__device__ void schur_terms(const CalibArgs& g, uint32_t v0, uint32_t nv, int slot, int nf, const int* s_free, double lambda, int wave, int lane,
                            int* bad) {
    const int nt = nf * (nf + 1) / 2;
    for (uint32_t j = (uint32_t)wave; j < nv; j += kCalWaves) {
        const uint32_t v = v0 + j;
        if (g.views[v].status != A3_CALIB_VIEW_USED) continue;
        double* sv = g.scratch + (size_t)v * kCalViewDoubles;
        const double* blk = sv + kOffBlk + slot * kCalEntries;
        double L[6][6], D[6];
        if (!ldl6_at<12, kCalAug>(blk, lambda, L, D)) {
            if (lane == 0) *bad = 1;
            continue;
        }
        if (lane <= nf) {
            double b[6], y[6];
            const int fc = lane < nf ? s_free[lane] : 0;
#pragma unroll
            for (int m = 0; m < 6; m++) b[m] = lane < nf ? blk[tri_index(fc, 12 + m, kCalAug)] : blk[tri_index(12 + m, 18, kCalAug)];
            ldl6_solve(L, D, b, y);
            for (int k = lane < nf ? lane : 0; k < nf; k++) {
                const int fk = s_free[k];
                double s = 0.0;
#pragma unroll
                for (int m = 0; m < 6; m++) s = s + blk[tri_index(fk, 12 + m, kCalAug)] * y[m];
                sv[kOffCon + (lane < nf ? tri_index(lane, k, nf) : nt + k)] = s;
            }
        }
    }
}

// S (+ lambda on U's diagonal) and its right-hand side from the camera sums and the views' terms (wave 0)
__device__ void schur_matrix(const CalibArgs& g, uint32_t v0, uint32_t nv, int nf, const double* s_U, double lambda, int lane, double* s_S,
                             double* s_rhs) {
    const int nt = nf * (nf + 1) / 2, ne = nt + nf;
    for (int e = lane; e < ne; e += 64) {
        int c = 0, k = 0;
        if (e < nt) tri_ik(e, nf, &c, &k);
        double s = e < nt ? s_U[e] : -s_U[e];
        if (e < nt && c == k) s = s + lambda * s;
        for (uint32_t j = 0; j < nv; j++) {
            const uint32_t v = v0 + j;
            if (g.views[v].status != A3_CALIB_VIEW_USED) continue;
            const double t = g.scratch[(size_t)v * kCalViewDoubles + kOffCon + e];
            s = e < nt ? s - t : s + t;
        }
        if (e < nt) { s_S[c * 12 + k] = s; s_S[k * 12 + c] = s; }
        else s_rhs[e - nt] = s;
    }
}

// U = sum of the views' intrinsic blocks and g_a (free entries), from block slot `slot` (wave 0)
__device__ void camera_sums(const CalibArgs& g, uint32_t v0, uint32_t nv, int slot, int nf, const int* s_free, int lane, double* s_U) {
    const int nt = nf * (nf + 1) / 2, ne = nt + nf;
    for (int e = lane; e < ne; e += 64) {
        int idx;
        if (e < nt) {
            int c, k;
            tri_ik(e, nf, &c, &k);
            idx = tri_index(s_free[c], s_free[k], kCalAug);
        } else idx = tri_index(s_free[e - nt], 18, kCalAug);
        double s = 0.0;
        for (uint32_t j = 0; j < nv; j++) {
            const uint32_t v = v0 + j;
            if (g.views[v].status != A3_CALIB_VIEW_USED) continue;
            s = s + g.scratch[(size_t)v * kCalViewDoubles + kOffBlk + slot * kCalEntries + idx];
        }
        s_U[e] = s;
    }
}

__global__ __launch_bounds__(kCalThreads) void k_calibrate(CalibArgs g) {
    __shared__ double s_rows[kCalWaves][64 * kRowStride];
    __shared__ double s_wv[kCalWaves][8];
    __shared__ double s_a[12], s_an[12], s_da[12], s_rhs[12], s_D[12], s_x[12], s_b[12], s_S[144], s_U[90];
    __shared__ double s_cost, s_lambda;
    __shared__ int s_free[12];
    __shared__ int s_nf, s_status, s_stop, s_bad, s_skip, s_cur, s_sums, s_iter, s_conv, s_maxit;
    __shared__ uint32_t s_vu, s_np;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const a3_calib_camera C = g.cams[blockIdx.x];
    const uint32_t v0 = C.first_view, nv = C.n_views;
    double* rows = s_rows[wave];
    double* wv = s_wv[wave];

    if (tid == 0) {
        int nf = 0;
        for (int i = 0; i < 12; i++)
            if (cal_free(C.flags, i)) s_free[nf++] = i;
        s_nf = nf;
        s_status = A3_CALIB_OK;
        s_stop = 0; s_bad = 0; s_skip = 0; s_cur = 0; s_sums = 1; s_iter = 0; s_conv = 0;
        s_maxit = C.max_iterations ? (int)C.max_iterations : A3_CALIB_DEFAULT_ITERATIONS;
        s_lambda = 1e-3;
    }
    // ---- 1. homographies ----
    for (uint32_t j = (uint32_t)wave; j < nv; j += kCalWaves) {
        const uint32_t v = v0 + j, p0 = g.view_off[v], np = g.view_off[v + 1] - p0;
        double* sv = g.scratch + (size_t)v * kCalViewDoubles;
        uint32_t st = A3_CALIB_VIEW_TOO_FEW_POINTS;
        if (np >= 4) st = view_homography(g.obj, g.img, p0, np, rows, wv, lane, sv + kOffH) ? A3_CALIB_VIEW_USED : A3_CALIB_VIEW_DEGENERATE;
        if (lane == 0) {
            a3_calib_view* rec = &g.views[v];
            rec->status = st;
            rec->points = np;
            rec->rms_px = 0.0f;
            for (int q = 0; q < 9; q++) rec->rotation[q] = 0.0f;
            for (int q = 0; q < 3; q++) rec->translation[q] = 0.0f;
        }
    }
    __syncthreads();
    const int nf = s_nf;
    // ---- 2. counts and the start ----
    if (tid == 0) {
        uint32_t vu = 0, n = 0;
        for (uint32_t j = 0; j < nv; j++)
            if (g.views[v0 + j].status == A3_CALIB_VIEW_USED) { vu++; n += g.views[v0 + j].points; }
        s_vu = vu;
        s_np = n;
        double a[12] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
        if (vu == 0 || 2ll * n - nf - 6ll * vu <= 0) s_status = A3_CALIB_TOO_FEW;
        else if (C.flags & A3_CALIB_USE_INTRINSIC_GUESS) {
            const a3_distortion& d = C.guess_distortion;
            a[0] = C.guess.focal_x; a[1] = C.guess.focal_y; a[2] = C.guess.principal_x; a[3] = C.guess.principal_y;
            a[4] = d.k1; a[5] = d.k2; a[6] = d.p1; a[7] = d.p2; a[8] = d.k3; a[9] = d.k4; a[10] = d.k5; a[11] = d.k6;
            if (C.flags & A3_CALIB_ZERO_TANGENT_DIST) { a[6] = 0.0; a[7] = 0.0; }
            if (!(C.flags & A3_CALIB_RATIONAL_MODEL)) { a[9] = 0.0; a[10] = 0.0; a[11] = 0.0; }
        } else {
            const double cx = ((double)C.image_width - 1.0) * 0.5, cy = ((double)C.image_height - 1.0) * 0.5;
            double A00 = 0.0, A01 = 0.0, A11 = 0.0, b0 = 0.0, b1 = 0.0;
            for (uint32_t j = 0; j < nv; j++) {
                if (g.views[v0 + j].status != A3_CALIB_VIEW_USED) continue;
                const double* H = g.scratch + (size_t)(v0 + j) * kCalViewDoubles + kOffH;
                double h0 = H[0] - H[6] * cx, h1 = H[3] - H[6] * cy, h2 = H[6];
                double w0 = H[1] - H[7] * cx, w1 = H[4] - H[7] * cy, w2 = H[7];
                double d10 = (h0 + w0) * 0.5, d11 = (h1 + w1) * 0.5, d12 = (h2 + w2) * 0.5;
                double d20 = (h0 - w0) * 0.5, d21 = (h1 - w1) * 0.5, d22 = (h2 - w2) * 0.5;
                const double n0 = 1.0 / sqrt((h0 * h0 + h1 * h1) + h2 * h2), n1 = 1.0 / sqrt((w0 * w0 + w1 * w1) + w2 * w2);
                const double n2 = 1.0 / sqrt((d10 * d10 + d11 * d11) + d12 * d12), n3 = 1.0 / sqrt((d20 * d20 + d21 * d21) + d22 * d22);
                h0 = h0 * n0; h1 = h1 * n0; h2 = h2 * n0;
                w0 = w0 * n1; w1 = w1 * n1; w2 = w2 * n1;
                d10 = d10 * n2; d11 = d11 * n2; d12 = d12 * n2;
                d20 = d20 * n3; d21 = d21 * n3; d22 = d22 * n3;
                const double ra = h0 * w0, rb = h1 * w1, rc = -(h2 * w2);
                const double qa = d10 * d20, qb = d11 * d21, qc = -(d12 * d22);
                A00 = A00 + ra * ra; A00 = A00 + qa * qa;
                A01 = A01 + ra * rb; A01 = A01 + qa * qb;
                A11 = A11 + rb * rb; A11 = A11 + qb * qb;
                b0 = b0 + ra * rc; b0 = b0 + qa * qc;
                b1 = b1 + rb * rc; b1 = b1 + qb * qc;
            }
            const double det = A00 * A11 - A01 * A01;
            const double s0 = (A11 * b0 - A01 * b1) / det, s1 = (A00 * b1 - A01 * b0) / det;
            const double fx = sqrt(1.0 / fabs(s0)), fy = sqrt(1.0 / fabs(s1));
            if (!(det > 1e-9 * (A00 * A11)) || !(fx > 0.0) || !fin(fx) || !(fy > 0.0) || !fin(fy)) s_status = A3_CALIB_NO_INIT;
            a[0] = fx; a[1] = fy; a[2] = cx; a[3] = cy;
        }
        for (int i = 0; i < 12; i++) s_a[i] = a[i];
    }
    __syncthreads();
    if (s_status == A3_CALIB_OK) {
        double a[12];
        for (int i = 0; i < 12; i++) a[i] = s_a[i];
        // ---- 3. per-view pose start and pose-only LM ----
        for (uint32_t j = (uint32_t)wave; j < nv; j += kCalWaves) {
            const uint32_t v = v0 + j;
            if (g.views[v].status != A3_CALIB_VIEW_USED) continue;
            const uint32_t p0 = g.view_off[v], np = g.view_off[v + 1] - p0;
            double* sv = g.scratch + (size_t)v * kCalViewDoubles;
            const double* H = sv + kOffH;
            double m[3][3], R[9], t[3];
            for (int c = 0; c < 3; c++) {
                m[c][0] = (H[c] - a[2] * H[6 + c]) / a[0];
                m[c][1] = (H[3 + c] - a[3] * H[6 + c]) / a[1];
                m[c][2] = H[6 + c];
            }
            pose_from_h(m, R, t);
            // (the pose-only LM loop stays this kernel's own: behind a shared function it compiles to other code)
            double* cur = sv + kOffBlk;
            double* oth = cur + kCalEntries;
            view_block(a, R, t, g.obj, g.img, p0, np, rows, lane, cur);
            double cost = cur[kCalEntries - 1];
            int evals = 1;
            double lambda = 1e-3;
            while (evals < A3_CALIB_POSE_EVALS && cost > 0.0) {
                double L[6][6], D[6];
                if (!ldl6_at<12, kCalAug>(cur, lambda, L, D)) { lambda = lambda * 10.0; evals++; continue; }
                double b[6], d[6];
#pragma unroll
                for (int q = 0; q < 6; q++) b[q] = -cur[tri_index(12 + q, 18, kCalAug)];
                ldl6_solve(L, D, b, d);
                double Rn[9], tn[3];
                cayley_d(d, R, Rn);
                for (int q = 0; q < 3; q++) tn[q] = t[q] + d[3 + q];
                view_block(a, Rn, tn, g.obj, g.img, p0, np, rows, lane, oth);
                evals++;
                const double c2 = oth[kCalEntries - 1];
                if (c2 < cost) {
                    const double rel = (cost - c2) / cost;
                    for (int q = 0; q < 9; q++) R[q] = Rn[q];
                    for (int q = 0; q < 3; q++) t[q] = tn[q];
                    double* s = cur; cur = oth; oth = s;
                    cost = c2;
                    lambda = lambda / 10.0;
                    if (rel < A3_CALIB_REL_TOL) break;
                } else lambda = lambda * 10.0;
            }
            if (lane == 0) {
                for (int q = 0; q < 9; q++) sv[kOffPose + q] = R[q];
                for (int q = 0; q < 3; q++) sv[kOffPose + 9 + q] = t[q];
            }
            wave_sync();
        }
        __syncthreads();
        // ---- 4. joint LM ----
        for (uint32_t j = (uint32_t)wave; j < nv; j += kCalWaves) {
            const uint32_t v = v0 + j;
            if (g.views[v].status != A3_CALIB_VIEW_USED) continue;
            const uint32_t p0 = g.view_off[v], np = g.view_off[v + 1] - p0;
            double* sv = g.scratch + (size_t)v * kCalViewDoubles;
            double R[9], t[3];
            for (int q = 0; q < 9; q++) R[q] = sv[kOffPose + q];
            for (int q = 0; q < 3; q++) t[q] = sv[kOffPose + 9 + q];
            view_block(a, R, t, g.obj, g.img, p0, np, rows, lane, sv + kOffBlk);
        }
        __syncthreads();
        if (tid == 0) {
            double cost = 0.0;
            for (uint32_t j = 0; j < nv; j++)
                if (g.views[v0 + j].status == A3_CALIB_VIEW_USED) cost = cost + g.scratch[(size_t)(v0 + j) * kCalViewDoubles + kOffBlk + kCalEntries - 1];
            s_cost = cost;
            if (!fin(cost)) s_status = A3_CALIB_NOT_FINITE;
            if (cost == 0.0) { s_stop = 1; s_conv = 1; }
        }
        __syncthreads();
    }
    if (s_status == A3_CALIB_OK) {
        while (true) {
            __syncthreads();
            if (s_stop) break;
            const int cur = s_cur;
            const double lambda = s_lambda;
            if (s_sums && wave == 0) camera_sums(g, v0, nv, cur, nf, s_free, lane, s_U);
            __syncthreads();
            schur_terms(g, v0, nv, cur, nf, s_free, lambda, wave, lane, &s_bad);
            __syncthreads();
            if (wave == 0 && !s_bad) schur_matrix(g, v0, nv, nf, s_U, lambda, lane, s_S, s_rhs);
            __syncthreads();
            if (tid == 0) {
                bool bad = s_bad != 0;
                if (!bad) bad = !ldl_n<12>(s_S, nf, s_D);
                if (!bad) {
                    ldl_n_solve<12>(s_S, nf, s_D, s_rhs, s_da);
                    for (int i = 0; i < 12; i++) s_an[i] = s_a[i];
                    for (int c = 0; c < nf; c++) s_an[s_free[c]] = s_a[s_free[c]] + s_da[c];
                }
                s_bad = 0;
                s_skip = bad ? 1 : 0;
                s_sums = 0;
                if (bad) {
                    s_lambda = lambda * 10.0;
                    s_iter = s_iter + 1;
                    if (s_iter >= s_maxit) s_stop = 1;
                }
            }
            __syncthreads();
            if (s_skip) continue;
            double an[12];
            for (int i = 0; i < 12; i++) an[i] = s_an[i];
            for (uint32_t j = (uint32_t)wave; j < nv; j += kCalWaves) {
                const uint32_t v = v0 + j;
                if (g.views[v].status != A3_CALIB_VIEW_USED) continue;
                const uint32_t p0 = g.view_off[v], np = g.view_off[v + 1] - p0;
                double* sv = g.scratch + (size_t)v * kCalViewDoubles;
                const double* blk = sv + kOffBlk + cur * kCalEntries;
                double L[6][6], D[6];
                ldl6_at<12, kCalAug>(blk, lambda, L, D);
                double b[6], d[6];
#pragma unroll
                for (int q = 0; q < 6; q++) {
                    double s = 0.0;
                    for (int k = 0; k < nf; k++) s = s + blk[tri_index(s_free[k], 12 + q, kCalAug)] * s_da[k];
                    b[q] = -blk[tri_index(12 + q, 18, kCalAug)] - s;
                }
                ldl6_solve(L, D, b, d);
                const double* pose = sv + kOffPose + cur * 12;
                double R[9], t[3], Rn[9], tn[3];
                for (int q = 0; q < 9; q++) R[q] = pose[q];
                for (int q = 0; q < 3; q++) t[q] = pose[9 + q];
                cayley_d(d, R, Rn);
                for (int q = 0; q < 3; q++) tn[q] = t[q] + d[3 + q];
                double* npose = sv + kOffPose + (1 - cur) * 12;
                if (lane == 0) {
                    for (int q = 0; q < 9; q++) npose[q] = Rn[q];
                    for (int q = 0; q < 3; q++) npose[9 + q] = tn[q];
                }
                view_block(an, Rn, tn, g.obj, g.img, p0, np, rows, lane, sv + kOffBlk + (1 - cur) * kCalEntries);
            }
            __syncthreads();
            if (tid == 0) {
                double c2 = 0.0;
                for (uint32_t j = 0; j < nv; j++)
                    if (g.views[v0 + j].status == A3_CALIB_VIEW_USED)
                        c2 = c2 + g.scratch[(size_t)(v0 + j) * kCalViewDoubles + kOffBlk + (1 - cur) * kCalEntries + kCalEntries - 1];
                const double cost = s_cost;
                s_iter = s_iter + 1;
                if (c2 < cost) {
                    const double rel = (cost - c2) / cost;
                    s_cur = 1 - cur;
                    for (int i = 0; i < 12; i++) s_a[i] = s_an[i];
                    s_cost = c2;
                    s_lambda = lambda / 10.0;
                    s_sums = 1;
                    if (rel < A3_CALIB_REL_TOL || c2 == 0.0) { s_conv = 1; s_stop = 1; }
                } else s_lambda = lambda * 10.0;
                if (s_iter >= s_maxit) s_stop = 1;
            }
        }
        // ---- 5. covariance: the undamped Schur complement at the final state ----
        __syncthreads();
        const int cur = s_cur;
        if (s_sums && wave == 0) camera_sums(g, v0, nv, cur, nf, s_free, lane, s_U);
        __syncthreads();
        schur_terms(g, v0, nv, cur, nf, s_free, 0.0, wave, lane, &s_bad);
        __syncthreads();
        if (wave == 0 && !s_bad) schur_matrix(g, v0, nv, nf, s_U, 0.0, lane, s_S, s_rhs);
        __syncthreads();
        if (tid == 0) {
            const bool pd = !s_bad && ldl_n<12>(s_S, nf, s_D);
            const double sigma2 = s_cost / (double)(2ll * s_np - nf - 6ll * s_vu);
            for (int i = 0; i < nf; i++) {
                double diag = __builtin_inf();
                if (pd) {
                    for (int k = 0; k < nf; k++) s_b[k] = k == i ? 1.0 : 0.0;
                    ldl_n_solve<12>(s_S, nf, s_D, s_b, s_x);
                    diag = sqrt(sigma2 * s_x[i]);
                }
                s_rhs[i] = diag;   // (s_rhs is free now: the deviations of the free parameters)
            }
        }
        __syncthreads();
    }
    // ---- outputs ----
    const bool ok = s_status == A3_CALIB_OK;
    if (tid == 0) {   // (field by field into global memory: a local record would live in scratch)
        a3_calib_result* r = &g.res[blockIdx.x];
        r->status = (uint32_t)s_status;
        r->views_used = s_vu;
        r->points_used = s_np;
        r->iterations = ok ? (uint32_t)s_iter : 0u;
        r->converged = ok ? (uint32_t)s_conv : 0u;
        r->reserved = 0;
        r->fx = ok ? s_a[0] : 0.0; r->fy = ok ? s_a[1] : 0.0; r->cx = ok ? s_a[2] : 0.0; r->cy = ok ? s_a[3] : 0.0;
        for (int i = 0; i < 8; i++) r->dist[i] = ok ? s_a[4 + i] : 0.0;
        for (int i = 0; i < 12; i++) r->std_dev[i] = 0.0;
        if (ok)
            for (int c = 0; c < nf; c++) r->std_dev[s_free[c]] = s_rhs[c];
        r->rms_px = ok ? sqrt(s_cost / (double)s_np) : 0.0;
        r->intrinsics.image_width = ok ? C.image_width : 0u;
        r->intrinsics.image_height = ok ? C.image_height : 0u;
        r->intrinsics.focal_x = (float)r->fx; r->intrinsics.focal_y = (float)r->fy;
        r->intrinsics.principal_x = (float)r->cx; r->intrinsics.principal_y = (float)r->cy;
        r->distortion.model = ok ? (uint32_t)A3_DIST_RATIONAL : 0u;
        r->distortion.iterations = ok ? 20u : 0u;
        r->distortion.k1 = (float)r->dist[0]; r->distortion.k2 = (float)r->dist[1]; r->distortion.p1 = (float)r->dist[2];
        r->distortion.p2 = (float)r->dist[3]; r->distortion.k3 = (float)r->dist[4]; r->distortion.k4 = (float)r->dist[5];
        r->distortion.k5 = (float)r->dist[6]; r->distortion.k6 = (float)r->dist[7];
        r->distortion.max_residual_px = ok ? 0.1f : 0.0f;
        r->reserved2 = 0;
    }
    if (ok) {
        const int cur = s_cur;
        for (uint32_t j = (uint32_t)wave; j < nv; j += kCalWaves) {
            const uint32_t v = v0 + j;
            if (lane != 0 || g.views[v].status != A3_CALIB_VIEW_USED) continue;
            const double* sv = g.scratch + (size_t)v * kCalViewDoubles;
            a3_calib_view* rec = &g.views[v];
            rec->rms_px = (float)sqrt(sv[kOffBlk + cur * kCalEntries + kCalEntries - 1] / (double)rec->points);
            for (int q = 0; q < 9; q++) rec->rotation[q] = (float)sv[kOffPose + cur * 12 + q];
            for (int q = 0; q < 3; q++) rec->translation[q] = (float)sv[kOffPose + cur * 12 + 9 + q];
        }
    }
}

size_t calib_view_bytes() { return kCalViewDoubles * sizeof(double); }

hipError_t launch_calibrate(hipStream_t st, const CalibLaunch& c) {
    if (c.n_cams == 0) return hipSuccess;
    const CalibArgs g{c.cams, c.view_off, c.obj, c.img, c.scratch, c.res, c.views};
    hipLaunchKernelGGL(k_calibrate, dim3(c.n_cams), dim3(kCalThreads), 0, st, g);
    return hipGetLastError();
}

}  // namespace a3
