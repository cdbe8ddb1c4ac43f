// a3_solve.h -- the solver skeleton that the calibration kernels share (k_calibrate and k_calibrate_fisheye in k_calib.hip, k_rig, k_map,
// k_handeye), each piece written once: the triangle indexing, the 6 x 6 and n x n LDL^T, the Cayley pose update, the wave-level block
// accumulator (aug_block) and the pose start from a homography (pose_from_h), all in f64.  What differs between the kernels -- the row
// of a point, the width of the augmented sum, where the pose columns sit -- comes in as a functor or a template parameter.  The
// pose-only Levenberg-Marquardt loop is not here: moved behind a function it compiles to other code in every one of the kernels, so
// each keeps its loop and stays instruction for instruction what it was.  Every expression is written in the contract's order and the tests' oracles (tests/*_oracle.c)
// restate each one in the same order; the library is built with -ffp-contract=off, so nothing is fused.
// The CPU counterpart of this header, which those oracles share, is tests/solve_oracle.h.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace a3 {

// index of (i, k), i <= k, in the row-by-row upper triangle of an n x n matrix
__device__ __forceinline__ int tri_index(int i, int k, int n) { return i * n - (i * (i - 1)) / 2 + (k - i); }

// (i, k) of entry e of that triangle
__device__ __forceinline__ void tri_ik(int e, int n, int* i, int* k) {
    int r = 0;
    while (e >= n - r) { e -= n - r; r++; }
    *i = r;
    *k = r + e;
}

__device__ __forceinline__ bool fin(double v) { return v - v == 0.0; }

__device__ __forceinline__ void wave_sync() { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); }

// LDL^T of V + lambda diag(V), V the 6 x 6 block at columns OFF .. OFF + 5 of the upper triangle of an AUG x AUG sum: L below the
// diagonal, D; false on a pivot that is not positive and finite
template <int OFF, int AUG>
__device__ __forceinline__ bool ldl6_at(const double* blk, double lambda, double L[6][6], double D[6]) {
    double A[6][6];
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = r; c < 6; c++) { const double v = blk[tri_index(OFF + r, OFF + c, AUG)]; A[r][c] = v; A[c][r] = v; }
#pragma unroll
    for (int r = 0; r < 6; r++) A[r][r] = A[r][r] + lambda * A[r][r];
    bool ok = true;
#pragma unroll
    for (int j = 0; j < 6; j++) {
#pragma unroll
        for (int i = j; i < 6; i++) {
            double s = A[i][j];
#pragma unroll
            for (int k = 0; k < j; k++) s = s - L[i][k] * L[j][k] * D[k];
            if (i == j) {
                ok = ok && s > 0.0 && fin(s);
                D[j] = s;
                L[j][j] = 1.0;
            } else L[i][j] = s / D[j];
        }
    }
    return ok;
}

__device__ __forceinline__ void ldl6_solve(const double L[6][6], const double D[6], const double b[6], double x[6]) {
    double y[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        double s = b[i];
#pragma unroll
        for (int k = 0; k < i; k++) s = s - L[i][k] * y[k];
        y[i] = s;
    }
#pragma unroll
    for (int i = 5; i >= 0; i--) {
        double s = y[i] / D[i];
#pragma unroll
        for (int k = i + 1; k < 6; k++) s = s - L[k][i] * x[k];
        x[i] = s;
    }
}

// LDL^T of the n x n matrix in A (row stride S, lower triangle read), L written below the diagonal; false on a bad pivot
template <int S>
__device__ inline bool ldl_n(double* A, int n, double* D) {
    for (int j = 0; j < n; j++)
        for (int i = j; i < n; i++) {
            double s = A[i * S + j];
            for (int k = 0; k < j; k++) s = s - A[i * S + k] * A[j * S + k] * D[k];
            if (i == j) {
                if (!(s > 0.0) || !fin(s)) return false;
                D[j] = s;
            } else A[i * S + j] = s / D[j];
        }
    return true;
}

template <int S>
__device__ inline void ldl_n_solve(const double* A, int n, const double* D, const double* b, double* x) {
    for (int i = 0; i < n; i++) {
        double s = b[i];
        for (int k = 0; k < i; k++) s = s - A[i * S + k] * x[k];
        x[i] = s;
    }
    for (int i = n - 1; i >= 0; i--) {
        double s = x[i] / D[i];
        for (int k = i + 1; k < n; k++) s = s - A[k * S + i] * x[k];
        x[i] = s;
    }
}

// R <- cay(w) R, a pose's rotation update in f64
__device__ __forceinline__ void cayley_d(const double w[3], const double R[9], double Rn[9]) {
    const double n2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double k = 2.0 / (1.0 + n2);
    const double W[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    double C[9];
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) {
            const double w2 = w[r] * w[c] - (r == c ? n2 : 0.0);
            C[3 * r + c] = (r == c ? 1.0 : 0.0) + k * (W[3 * r + c] + w2);
        }
#pragma unroll
    for (int r = 0; r < 3; r++)
#pragma unroll
        for (int c = 0; c < 3; c++) Rn[3 * r + c] = (C[3 * r] * R[c] + C[3 * r + 1] * R[3 + c]) + C[3 * r + 2] * R[6 + c];
}

// poses are 12 doubles: R (9, row-major), t (3).  R <- cay(w) R, t <- t + dt
__device__ __forceinline__ void pose_update(const double* T, const double d[6], double* Tn) {
    cayley_d(d, T, Tn);
#pragma unroll
    for (int q = 0; q < 3; q++) Tn[9 + q] = T[9 + q] + d[3 + q];
}

// the upper triangle of the AUG x AUG sum over points p0 .. p0 + np - 1 of their two augmented rows -> out (wave-level);
// row(X, Y, u, v, au, av) writes one point's rows of AUG.  The sums run in point order: the lanes write the rows of up to 64 points
// into `rows` (64 x 2 AUG doubles of the wave's LDS), then each lane owns up to (entries + 63) / 64 of the entries and adds the rows in
// order -- deterministic sums with two or three accumulators per lane.  Inlined: what the row functor captures (the intrinsics, the
// poses) stays in registers; a call would pass it through scratch memory.
template <int AUG, class Row>
__device__ __forceinline__ void aug_block(Row row, const float* __restrict__ obj, const float* __restrict__ img, uint32_t p0, uint32_t np, double* rows,
                                          int lane, double* out) {
    constexpr int kEntries = AUG * (AUG + 1) / 2, kAcc = (kEntries + 63) / 64, kStride = 2 * AUG;
    int ei[kAcc], ek[kAcc];
    double acc[kAcc];
#pragma unroll
    for (int q = 0; q < kAcc; q++) {
        acc[q] = 0.0;
        ei[q] = 0;
        ek[q] = 0;
        if (lane + 64 * q < kEntries) tri_ik(lane + 64 * q, AUG, &ei[q], &ek[q]);
    }
    for (uint32_t c0 = 0; c0 < np; c0 += 64) {
        const uint32_t cnt = min(64u, np - c0);
        if ((uint32_t)lane < cnt) {
            const size_t p = (size_t)p0 + c0 + (uint32_t)lane;
            row((double)obj[2 * p], (double)obj[2 * p + 1], (double)img[2 * p], (double)img[2 * p + 1], rows + lane * kStride,
                rows + lane * kStride + AUG);
        }
        wave_sync();
        for (uint32_t j = 0; j < cnt; j++) {
            const double* u = rows + j * kStride;
            const double* v = u + AUG;
#pragma unroll
            for (int q = 0; q < kAcc; q++) {
                acc[q] = acc[q] + u[ei[q]] * u[ek[q]];
                acc[q] = acc[q] + v[ei[q]] * v[ek[q]];
            }
        }
        wave_sync();
    }
#pragma unroll
    for (int q = 0; q < kAcc; q++)
        if (lane + 64 * q < kEntries) out[lane + 64 * q] = acc[q];
    wave_sync();
}

// the pose start (R, t) from m = (h1 h2 h3)^T, the columns of a board -> normalised-plane homography as rows: r1 along h1, r2 the part
// of h2 across it, r3 their cross product, t = 2 h3 / (|h1| + |h2|).  A pose kept as 12 doubles passes (T, T + 9).
// The callers form m: K^-1 H for an image homography, H as it is for one onto the normalised plane.
__device__ __forceinline__ void pose_from_h(const double m[3][3], double* R, double* t) {
    const double n0 = sqrt((m[0][0] * m[0][0] + m[0][1] * m[0][1]) + m[0][2] * m[0][2]);
    const double r00 = m[0][0] / n0, r01 = m[0][1] / n0, r02 = m[0][2] / n0;
    const double dd = (r00 * m[1][0] + r01 * m[1][1]) + r02 * m[1][2];
    const double e0 = m[1][0] - dd * r00, e1 = m[1][1] - dd * r01, e2 = m[1][2] - dd * r02;
    const double ne = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
    const double r10 = e0 / ne, r11 = e1 / ne, r12 = e2 / ne;
    const double n1 = sqrt((m[1][0] * m[1][0] + m[1][1] * m[1][1]) + m[1][2] * m[1][2]);
    const double den = n0 + n1;
    R[0] = r00; R[1] = r10; R[2] = r01 * r12 - r02 * r11;
    R[3] = r01; R[4] = r11; R[5] = r02 * r10 - r00 * r12;
    R[6] = r02; R[7] = r12; R[8] = r00 * r11 - r01 * r10;
    t[0] = (2.0 * m[2][0]) / den; t[1] = (2.0 * m[2][1]) / den; t[2] = (2.0 * m[2][2]) / den;
}

}  // namespace a3
