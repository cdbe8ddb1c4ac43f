// k_calib_fisheye.hip -- fisheye camera calibration (a3_calibrate_fisheye_cameras).  Not part of the reference: an extension stated in
// include/aruco3_hip.h and restated on the CPU by tests/fisheye_calib_oracle.c (a3o_calibrate_fisheye), which this kernel matches bit
// for bit.
//
// k_calibrate's shape (k_calib.hip): one workgroup of four waves per camera, every phase inside the one launch, separated by barriers.
// Per-view work goes to one wave (views w, w + 4, ...).  A view's sums run in point order: the lanes write the augmented rows of up to
// 64 points into the wave's LDS, then each lane owns up to two of the 120 block entries and adds the rows in order.  The start undistorts
// a view's image points a lane each and compacts the kept ones in point order (a ballot and a prefix count) into a device scratch of 4
// floats per point, which view_homography (a3_calib.h) reads as it reads the caller's arrays.  Camera-level sums run over the views in
// view order, one lane of wave 0 per entry; the <= 8 x 8 Schur system is solved by one lane.  Per-view blocks, poses and Schur terms
// live in a device scratch buffer of kFeViewDoubles per view.  The block accumulator (aug_block), the pose start (pose_from_h) and the
// small solves are a3_solve.h's, shared with the other solver kernels.
#include <cmath>

#include "a3_common.h"
#include "a3_launch.h"
#include "a3_fisheye_calib.h"

namespace a3 {

constexpr int kFeThreads = 256, kFeWaves = 4;
constexpr int kFeRowStride = 2 * kFeAug;   // doubles per point in LDS: the u row, then the v row
// per-view scratch: blocks (2 slots), poses (2 slots: R 9, t 3), Schur terms (<= 36 + 8), homography
constexpr int kFeOffBlk = 0, kFeOffPose = 2 * kFeEntries, kFeOffCon = kFeOffPose + 24, kFeOffH = kFeOffCon + 44;
constexpr size_t kFeViewDoubles = 320;
static_assert(kFeOffH + 9 <= (int)kFeViewDoubles, "view scratch");
static_assert(64 * kFeRowStride >= 64 * 2 * kHomAug && 64 * kFeRowStride >= 64 + 64 + 8 + 8, "view_homography's use of the rows");

struct FisheyeCalibArgs {
    const a3_calib_camera* cams;
    const uint32_t* view_off;
    const float* obj;
    const float* img;
    double* scratch;
    float* start_obj;   // the start's compacted board points and normalised image points, 2 floats per point each
    float* start_img;
    a3_calib_result* res;
    a3_calib_view* views;
};

__device__ __forceinline__ bool fe_free(uint32_t flags, int i) {
    if (i == 2 || i == 3) return !(flags & A3_FISHEYE_FIX_PRINCIPAL_POINT);
    if (i >= 4) return !(flags & ((uint32_t)A3_FISHEYE_FIX_K1 << (i - 4)));
    return true;
}

// where parameter i (fx fy cx cy k1 k2 k3 k4) sits in a3_calib_result.std_dev and, less 4, in .dist
__device__ __forceinline__ int fe_out_index(int i) { return i < 6 ? i : i + 2; }

__device__ __forceinline__ bool fe_ldl6(const double* blk, double lambda, double L[6][6], double D[6]) {
    return ldl6_at<kFePose, kFeAug>(blk, lambda, L, D);
}

// one view's 120 block entries at (a, R, t) -> out (wave-level): aug_block (a3_solve.h) over fisheye_row
__device__ __forceinline__ void fe_view_block(const double a[8], const double R[9], const double t[3], const float* __restrict__ obj,
                                              const float* __restrict__ img, uint32_t p0, uint32_t np, double* rows, int lane, double* out) {
    aug_block<kFeAug>([&](double X, double Y, double ou, double ov, double* au, double* av) { fisheye_row(a, R, t, X, Y, ou, ov, au, av); }, obj, img,
                      p0, np, rows, lane, out);
}

// step 2's kept points of one view, compacted in point order into start_obj / start_img at the view's own offset (wave-level) -> how many
__device__ __forceinline__ uint32_t fe_start_points(const FisheyeCalibArgs& g, const double a[8], uint32_t p0, uint32_t np, int lane) {
    uint32_t nk = 0;
    for (uint32_t c0 = 0; c0 < np; c0 += 64) {
        const uint32_t cnt = min(64u, np - c0);
        const size_t p = (size_t)p0 + c0 + (uint32_t)lane;
        bool keep = false;
        double x = 0.0, y = 0.0;
        if ((uint32_t)lane < cnt) keep = fe_start_point(a, (double)g.img[2 * p], (double)g.img[2 * p + 1], &x, &y);
        const uint64_t mask = __builtin_amdgcn_ballot_w64(keep);
        if (keep) {
            const size_t o = (size_t)p0 + nk + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));   // (o <= p: inside the view's range)
            g.start_obj[2 * o] = g.obj[2 * p];
            g.start_obj[2 * o + 1] = g.obj[2 * p + 1];
            g.start_img[2 * o] = (float)x;
            g.start_img[2 * o + 1] = (float)y;
        }
        nk += (uint32_t)__popcll(mask);
    }
    wave_sync();
    return nk;
}

// steps 4 / 5's per-view Schur terms at `lambda` from block slot `slot` (wave-level, every USED view of the wave); a bad pivot sets *bad
__device__ void fe_schur_terms(const FisheyeCalibArgs& g, uint32_t v0, uint32_t nv, int slot, int nf, const int* s_free, double lambda, int wave,
                               int lane, int* bad) {
    const int nt = nf * (nf + 1) / 2;
    for (uint32_t j = (uint32_t)wave; j < nv; j += kFeWaves) {
        const uint32_t v = v0 + j;
        if (g.views[v].status != A3_CALIB_VIEW_USED) continue;
        double* sv = g.scratch + (size_t)v * kFeViewDoubles;
        const double* blk = sv + kFeOffBlk + slot * kFeEntries;
        double L[6][6], D[6];
        if (!fe_ldl6(blk, lambda, L, D)) {
            if (lane == 0) *bad = 1;
            continue;
        }
        if (lane <= nf) {
            double b[6], y[6];
            const int fc = lane < nf ? s_free[lane] : 0;
#pragma unroll
            for (int m = 0; m < 6; m++) b[m] = lane < nf ? blk[tri_index(fc, kFePose + m, kFeAug)] : blk[tri_index(kFePose + m, kFeRes, kFeAug)];
            ldl6_solve(L, D, b, y);
            for (int k = lane < nf ? lane : 0; k < nf; k++) {
                const int fk = s_free[k];
                double s = 0.0;
#pragma unroll
                for (int m = 0; m < 6; m++) s = s + blk[tri_index(fk, kFePose + m, kFeAug)] * y[m];
                sv[kFeOffCon + (lane < nf ? tri_index(lane, k, nf) : nt + k)] = s;
            }
        }
    }
}

// S (+ lambda on U's diagonal) and its right-hand side from the camera sums and the views' terms (wave 0)
__device__ void fe_schur_matrix(const FisheyeCalibArgs& g, uint32_t v0, uint32_t nv, int nf, const double* s_U, double lambda, int lane, double* s_S,
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
            const double t = g.scratch[(size_t)v * kFeViewDoubles + kFeOffCon + e];
            s = e < nt ? s - t : s + t;
        }
        if (e < nt) { s_S[c * 8 + k] = s; s_S[k * 8 + c] = s; }
        else s_rhs[e - nt] = s;
    }
}

// U = sum of the views' intrinsic blocks and g_a (free entries), from block slot `slot` (wave 0)
__device__ void fe_camera_sums(const FisheyeCalibArgs& g, uint32_t v0, uint32_t nv, int slot, int nf, const int* s_free, int lane, double* s_U) {
    const int nt = nf * (nf + 1) / 2, ne = nt + nf;
    for (int e = lane; e < ne; e += 64) {
        int idx;
        if (e < nt) {
            int c, k;
            tri_ik(e, nf, &c, &k);
            idx = tri_index(s_free[c], s_free[k], kFeAug);
        } else idx = tri_index(s_free[e - nt], kFeRes, kFeAug);
        double s = 0.0;
        for (uint32_t j = 0; j < nv; j++) {
            const uint32_t v = v0 + j;
            if (g.views[v].status != A3_CALIB_VIEW_USED) continue;
            s = s + g.scratch[(size_t)v * kFeViewDoubles + kFeOffBlk + slot * kFeEntries + idx];
        }
        s_U[e] = s;
    }
}

__global__ __launch_bounds__(kFeThreads) void k_calibrate_fisheye(FisheyeCalibArgs g) {
    __shared__ double s_rows[kFeWaves][64 * kFeRowStride];
    __shared__ double s_wv[kFeWaves][8];
    __shared__ double s_a[8], s_an[8], s_da[8], s_rhs[8], s_D[8], s_x[8], s_b[8], s_S[64], s_U[44];
    __shared__ double s_cost, s_lambda;
    __shared__ int s_free[8];
    __shared__ int s_nf, s_status, s_stop, s_bad, s_skip, s_cur, s_sums, s_iter, s_conv, s_maxit;
    __shared__ uint32_t s_vu, s_np;

    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const a3_calib_camera C = g.cams[blockIdx.x];
    const uint32_t v0 = C.first_view, nv = C.n_views;
    double* rows = s_rows[wave];
    double* wv = s_wv[wave];

    // ---- 1. the start ----
    if (tid == 0) {
        int nf = 0;
        for (int i = 0; i < 8; i++)
            if (fe_free(C.flags, i)) s_free[nf++] = i;
        s_nf = nf;
        s_status = A3_CALIB_OK;
        s_stop = 0; s_bad = 0; s_skip = 0; s_cur = 0; s_sums = 1; s_iter = 0; s_conv = 0;
        s_maxit = C.max_iterations ? (int)C.max_iterations : A3_CALIB_DEFAULT_ITERATIONS;
        s_lambda = 1e-3;
        if (C.flags & A3_FISHEYE_USE_INTRINSIC_GUESS) {
            const a3_distortion& d = C.guess_distortion;
            s_a[0] = C.guess.focal_x; s_a[1] = C.guess.focal_y; s_a[2] = C.guess.principal_x; s_a[3] = C.guess.principal_y;
            s_a[4] = d.k1; s_a[5] = d.k2; s_a[6] = d.k3; s_a[7] = d.k4;
        } else {
            const double W = (double)C.image_width, H = (double)C.image_height;
            const double f = (W > H ? W : H) / 3.141592653589793;
            s_a[0] = f; s_a[1] = f; s_a[2] = (W - 1.0) * 0.5; s_a[3] = (H - 1.0) * 0.5;
            s_a[4] = 0.0; s_a[5] = 0.0; s_a[6] = 0.0; s_a[7] = 0.0;
        }
    }
    __syncthreads();
    const int nf = s_nf;
    double a[8];
    for (int i = 0; i < 8; i++) a[i] = s_a[i];
    // ---- 2. per view: the start's points, the homography board -> normalised plane ----
    for (uint32_t j = (uint32_t)wave; j < nv; j += kFeWaves) {
        const uint32_t v = v0 + j, p0 = g.view_off[v], np = g.view_off[v + 1] - p0;
        double* sv = g.scratch + (size_t)v * kFeViewDoubles;
        uint32_t st = A3_CALIB_VIEW_TOO_FEW_POINTS;
        if (np >= 4) {
            const uint32_t nk = fe_start_points(g, a, p0, np, lane);
            st = A3_CALIB_VIEW_DEGENERATE;
            // view_homography takes its arrays as read-only __restrict__ inputs, which these were not a moment ago: the pointers go
            // through a vector register, so that no read of them can become a scalar load (the scalar cache does not see vector stores)
            const float* so = g.start_obj;
            const float* si = g.start_img;
            asm volatile("" : "+v"(so), "+v"(si));
            if (nk >= 4 && view_homography(so, si, p0, nk, rows, wv, lane, sv + kFeOffH)) st = A3_CALIB_VIEW_USED;
        }
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
    if (tid == 0) {
        uint32_t vu = 0, n = 0;
        for (uint32_t j = 0; j < nv; j++)
            if (g.views[v0 + j].status == A3_CALIB_VIEW_USED) { vu++; n += g.views[v0 + j].points; }
        s_vu = vu;
        s_np = n;
        if (vu == 0 || 2ll * n - nf - 6ll * vu <= 0) s_status = A3_CALIB_TOO_FEW;
    }
    __syncthreads();
    if (s_status == A3_CALIB_OK) {
        // ---- the pose start and the pose-only LM ----
        for (uint32_t j = (uint32_t)wave; j < nv; j += kFeWaves) {
            const uint32_t v = v0 + j;
            if (g.views[v].status != A3_CALIB_VIEW_USED) continue;
            const uint32_t p0 = g.view_off[v], np = g.view_off[v + 1] - p0;
            double* sv = g.scratch + (size_t)v * kFeViewDoubles;
            const double* H = sv + kFeOffH;   // board -> normalised plane, taken as it is
            double m[3][3], R[9], t[3];
            for (int c = 0; c < 3; c++) { m[c][0] = H[c]; m[c][1] = H[3 + c]; m[c][2] = H[6 + c]; }
            pose_from_h(m, R, t);
            // (the pose-only LM loop stays this kernel's own: behind a shared function it compiles to other code)
            double* cur = sv + kFeOffBlk;
            double* oth = cur + kFeEntries;
            fe_view_block(a, R, t, g.obj, g.img, p0, np, rows, lane, cur);
            double cost = cur[kFeEntries - 1];
            int evals = 1;
            double lambda = 1e-3;
            while (evals < A3_CALIB_POSE_EVALS && cost > 0.0) {
                double L[6][6], D[6];
                if (!fe_ldl6(cur, lambda, L, D)) { lambda = lambda * 10.0; evals++; continue; }
                double b[6], d[6];
#pragma unroll
                for (int q = 0; q < 6; q++) b[q] = -cur[tri_index(kFePose + q, kFeRes, kFeAug)];
                ldl6_solve(L, D, b, d);
                double Rn[9], tn[3];
                cayley_d(d, R, Rn);
                for (int q = 0; q < 3; q++) tn[q] = t[q] + d[3 + q];
                fe_view_block(a, Rn, tn, g.obj, g.img, p0, np, rows, lane, oth);
                evals++;
                const double c2 = oth[kFeEntries - 1];
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
                for (int q = 0; q < 9; q++) sv[kFeOffPose + q] = R[q];
                for (int q = 0; q < 3; q++) sv[kFeOffPose + 9 + q] = t[q];
            }
            wave_sync();
        }
        __syncthreads();
        // ---- 3. the blocks at the start of the joint LM ----
        for (uint32_t j = (uint32_t)wave; j < nv; j += kFeWaves) {
            const uint32_t v = v0 + j;
            if (g.views[v].status != A3_CALIB_VIEW_USED) continue;
            const uint32_t p0 = g.view_off[v], np = g.view_off[v + 1] - p0;
            double* sv = g.scratch + (size_t)v * kFeViewDoubles;
            double R[9], t[3];
            for (int q = 0; q < 9; q++) R[q] = sv[kFeOffPose + q];
            for (int q = 0; q < 3; q++) t[q] = sv[kFeOffPose + 9 + q];
            fe_view_block(a, R, t, g.obj, g.img, p0, np, rows, lane, sv + kFeOffBlk);
        }
        __syncthreads();
        if (tid == 0) {
            double cost = 0.0;
            for (uint32_t j = 0; j < nv; j++)
                if (g.views[v0 + j].status == A3_CALIB_VIEW_USED) cost = cost + g.scratch[(size_t)(v0 + j) * kFeViewDoubles + kFeOffBlk + kFeEntries - 1];
            s_cost = cost;
            if (!fin(cost)) s_status = A3_CALIB_NOT_FINITE;
            if (cost == 0.0) { s_stop = 1; s_conv = 1; }
        }
        __syncthreads();
    }
    if (s_status == A3_CALIB_OK) {
        // ---- 4. joint LM ----
        while (true) {
            __syncthreads();
            if (s_stop) break;
            const int cur = s_cur;
            const double lambda = s_lambda;
            if (s_sums && wave == 0) fe_camera_sums(g, v0, nv, cur, nf, s_free, lane, s_U);
            __syncthreads();
            fe_schur_terms(g, v0, nv, cur, nf, s_free, lambda, wave, lane, &s_bad);
            __syncthreads();
            if (wave == 0 && !s_bad) fe_schur_matrix(g, v0, nv, nf, s_U, lambda, lane, s_S, s_rhs);
            __syncthreads();
            if (tid == 0) {
                bool bad = s_bad != 0;
                if (!bad) bad = !ldl_n<8>(s_S, nf, s_D);
                if (!bad) {
                    ldl_n_solve<8>(s_S, nf, s_D, s_rhs, s_da);
                    for (int i = 0; i < 8; i++) s_an[i] = s_a[i];
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
            double an[8];
            for (int i = 0; i < 8; i++) an[i] = s_an[i];
            for (uint32_t j = (uint32_t)wave; j < nv; j += kFeWaves) {
                const uint32_t v = v0 + j;
                if (g.views[v].status != A3_CALIB_VIEW_USED) continue;
                const uint32_t p0 = g.view_off[v], np = g.view_off[v + 1] - p0;
                double* sv = g.scratch + (size_t)v * kFeViewDoubles;
                const double* blk = sv + kFeOffBlk + cur * kFeEntries;
                double L[6][6], D[6];
                fe_ldl6(blk, lambda, L, D);
                double b[6], d[6];
#pragma unroll
                for (int q = 0; q < 6; q++) {
                    double s = 0.0;
                    for (int k = 0; k < nf; k++) s = s + blk[tri_index(s_free[k], kFePose + q, kFeAug)] * s_da[k];
                    b[q] = -blk[tri_index(kFePose + q, kFeRes, kFeAug)] - s;
                }
                ldl6_solve(L, D, b, d);
                const double* pose = sv + kFeOffPose + cur * 12;
                double R[9], t[3], Rn[9], tn[3];
                for (int q = 0; q < 9; q++) R[q] = pose[q];
                for (int q = 0; q < 3; q++) t[q] = pose[9 + q];
                cayley_d(d, R, Rn);
                for (int q = 0; q < 3; q++) tn[q] = t[q] + d[3 + q];
                double* npose = sv + kFeOffPose + (1 - cur) * 12;
                if (lane == 0) {
                    for (int q = 0; q < 9; q++) npose[q] = Rn[q];
                    for (int q = 0; q < 3; q++) npose[9 + q] = tn[q];
                }
                fe_view_block(an, Rn, tn, g.obj, g.img, p0, np, rows, lane, sv + kFeOffBlk + (1 - cur) * kFeEntries);
            }
            __syncthreads();
            if (tid == 0) {
                double c2 = 0.0;
                for (uint32_t j = 0; j < nv; j++)
                    if (g.views[v0 + j].status == A3_CALIB_VIEW_USED)
                        c2 = c2 + g.scratch[(size_t)(v0 + j) * kFeViewDoubles + kFeOffBlk + (1 - cur) * kFeEntries + kFeEntries - 1];
                const double cost = s_cost;
                s_iter = s_iter + 1;
                if (c2 < cost) {
                    const double rel = (cost - c2) / cost;
                    s_cur = 1 - cur;
                    for (int i = 0; i < 8; i++) s_a[i] = s_an[i];
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
        if (s_sums && wave == 0) fe_camera_sums(g, v0, nv, cur, nf, s_free, lane, s_U);
        __syncthreads();
        fe_schur_terms(g, v0, nv, cur, nf, s_free, 0.0, wave, lane, &s_bad);
        __syncthreads();
        if (wave == 0 && !s_bad) fe_schur_matrix(g, v0, nv, nf, s_U, 0.0, lane, s_S, s_rhs);
        __syncthreads();
        if (tid == 0) {
            const bool pd = !s_bad && ldl_n<8>(s_S, nf, s_D);
            const double sigma2 = s_cost / (double)(2ll * s_np - nf - 6ll * s_vu);
            for (int i = 0; i < nf; i++) {
                double diag = __builtin_inf();
                if (pd) {
                    for (int k = 0; k < nf; k++) s_b[k] = k == i ? 1.0 : 0.0;
                    ldl_n_solve<8>(s_S, nf, s_D, s_b, s_x);
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
        for (int i = 0; i < 8; i++) r->dist[i] = 0.0;
        for (int i = 4; i < 8; i++) r->dist[fe_out_index(i) - 4] = ok ? s_a[i] : 0.0;
        for (int i = 0; i < 12; i++) r->std_dev[i] = 0.0;
        if (ok)
            for (int c = 0; c < nf; c++) r->std_dev[fe_out_index(s_free[c])] = s_rhs[c];
        r->rms_px = ok ? sqrt(s_cost / (double)s_np) : 0.0;
        r->intrinsics.image_width = ok ? C.image_width : 0u;
        r->intrinsics.image_height = ok ? C.image_height : 0u;
        r->intrinsics.focal_x = (float)r->fx; r->intrinsics.focal_y = (float)r->fy;
        r->intrinsics.principal_x = (float)r->cx; r->intrinsics.principal_y = (float)r->cy;
        r->distortion.model = ok ? (uint32_t)A3_DIST_FISHEYE : 0u;
        r->distortion.iterations = ok ? 20u : 0u;
        r->distortion.k1 = (float)r->dist[0]; r->distortion.k2 = (float)r->dist[1]; r->distortion.p1 = 0.0f; r->distortion.p2 = 0.0f;
        r->distortion.k3 = (float)r->dist[4]; r->distortion.k4 = (float)r->dist[5]; r->distortion.k5 = 0.0f; r->distortion.k6 = 0.0f;
        r->distortion.max_residual_px = ok ? 0.1f : 0.0f;
        r->reserved2 = 0;
    }
    if (ok) {
        const int cur = s_cur;
        for (uint32_t j = (uint32_t)wave; j < nv; j += kFeWaves) {
            const uint32_t v = v0 + j;
            if (lane != 0 || g.views[v].status != A3_CALIB_VIEW_USED) continue;
            const double* sv = g.scratch + (size_t)v * kFeViewDoubles;
            a3_calib_view* rec = &g.views[v];
            rec->rms_px = (float)sqrt(sv[kFeOffBlk + cur * kFeEntries + kFeEntries - 1] / (double)rec->points);
            for (int q = 0; q < 9; q++) rec->rotation[q] = (float)sv[kFeOffPose + cur * 12 + q];
            for (int q = 0; q < 3; q++) rec->translation[q] = (float)sv[kFeOffPose + cur * 12 + 9 + q];
        }
    }
}

size_t fisheye_calib_view_bytes() { return kFeViewDoubles * sizeof(double); }

hipError_t launch_calibrate_fisheye(hipStream_t st, const CalibLaunch& c) {
    if (c.n_cams == 0) return hipSuccess;
    const FisheyeCalibArgs g{c.cams, c.view_off, c.obj, c.img, c.scratch, c.start_obj, c.start_img, c.res, c.views};
    hipLaunchKernelGGL(k_calibrate_fisheye, dim3(c.n_cams), dim3(kFeThreads), 0, st, g);
    return hipGetLastError();
}

}  // namespace a3
