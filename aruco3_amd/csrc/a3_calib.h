// a3_calib.h -- the per-point and per-view pieces of the camera calibration of include/aruco3_hip.h (a3_calibrate_cameras): the
// projection with its 18 Jacobian columns, the homography rows, the 6 x 6 LDL^T and the Cayley update, all in f64.  k_calibrate
// (k_calib.hip) is the only user.  Every expression is written in the contract's order and tests/calib_oracle.c restates each one
// in the same order; the library is built with -ffp-contract=off, so nothing is fused.
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

namespace a3 {

constexpr int kCalAug = 19;        // 18 Jacobian columns (12 intrinsics, then w and t) + the residual
constexpr int kCalEntries = 190;   // upper triangle of the 19 x 19 augmented sum
constexpr int kHomAug = 9;         // 8 homography columns + the right-hand side
constexpr int kHomEntries = 45;

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

// the two augmented rows of one point: intrinsics a (fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6), pose (R, t), board point (X, Y, 0) seen at
// (ou, ov).  au / av: 19 values each (columns 0-11 intrinsics, 12-14 w, 15-17 t, 18 the residual).
__device__ __forceinline__ void calib_row(const double a[12], const double R[9], const double t[3], double X, double Y, double ou, double ov,
                                          double* au, double* av) {
    const double fx = a[0], fy = a[1], cx = a[2], cy = a[3];
    const double k1 = a[4], k2 = a[5], p1 = a[6], p2 = a[7], k3 = a[8], k4 = a[9], k5 = a[10], k6 = a[11];
    const double qx = R[0] * X + R[1] * Y, qy = R[3] * X + R[4] * Y, qz = R[6] * X + R[7] * Y;
    const double px = qx + t[0], py = qy + t[1], pz = qz + t[2];
    const double ia = 1.0 / pz;
    const double x = px * ia, y = py * ia;
    const double r2 = x * x + y * y;
    const double num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
    const double den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2;
    const double iden = 1.0 / den;
    const double radial = num * iden;
    const double xy2 = 2.0 * x * y;
    const double xx2 = r2 + 2.0 * x * x, yy2 = r2 + 2.0 * y * y;
    const double xd = x * radial + (p1 * xy2 + p2 * xx2);
    const double yd = y * radial + (p1 * yy2 + p2 * xy2);
    au[18] = (fx * xd + cx) - ou;
    av[18] = (fy * yd + cy) - ov;
    // intrinsics
    const double r4 = r2 * r2, r6 = r4 * r2;
    const double dk1 = r2 * iden, dk2 = r4 * iden, dk3 = r6 * iden;
    const double m = radial * iden;
    const double dk4 = -(m * r2), dk5 = -(m * r4), dk6 = -(m * r6);
    const double gx = fx * x, gy = fy * y;
    au[0] = xd;  au[1] = 0.0; au[2] = 1.0; au[3] = 0.0;
    av[0] = 0.0; av[1] = yd;  av[2] = 0.0; av[3] = 1.0;
    au[4] = gx * dk1; au[5] = gx * dk2; au[8] = gx * dk3; au[9] = gx * dk4; au[10] = gx * dk5; au[11] = gx * dk6;
    av[4] = gy * dk1; av[5] = gy * dk2; av[8] = gy * dk3; av[9] = gy * dk4; av[10] = gy * dk5; av[11] = gy * dk6;
    au[6] = fx * xy2; au[7] = fx * xx2;
    av[6] = fy * yy2; av[7] = fy * xy2;
    // pose: d(xd, yd) / d(x, y), then d(x, y) / dP = ia (1, 0, -x), ia (0, 1, -y), dP / dw = -2 [q]x, dP / dt = I
    const double dnum = (3.0 * k3 * r2 + 2.0 * k2) * r2 + k1;
    const double dden = (3.0 * k6 * r2 + 2.0 * k5) * r2 + k4;
    const double dr = (dnum - radial * dden) * iden;
    const double xxd = ((radial + 2.0 * x * x * dr) + 2.0 * p1 * y) + 6.0 * p2 * x;
    const double xyd = ((2.0 * x * y * dr) + 2.0 * p1 * x) + 2.0 * p2 * y;
    const double yyd = ((radial + 2.0 * y * y * dr) + 6.0 * p1 * y) + 2.0 * p2 * x;
    const double cu = fx * ia, cv = fy * ia;
    const double u0 = cu * xxd, u1 = cu * xyd, u2 = -(cu * (xxd * x + xyd * y));
    const double v0 = cv * xyd, v1 = cv * yyd, v2 = -(cv * (xyd * x + yyd * y));
    const double q2x = 2.0 * qx, q2y = 2.0 * qy, q2z = 2.0 * qz;
    au[12] = u2 * q2y - u1 * q2z; au[13] = u0 * q2z - u2 * q2x; au[14] = u1 * q2x - u0 * q2y;
    av[12] = v2 * q2y - v1 * q2z; av[13] = v0 * q2z - v2 * q2x; av[14] = v1 * q2x - v0 * q2y;
    au[15] = u0; au[16] = u1; au[17] = u2;
    av[15] = v0; av[16] = v1; av[17] = v2;
}

// the two DLT rows of one Hartley-normalised correspondence (X, Y) -> (U, V): 9 values each (8 columns, the right-hand side)
__device__ __forceinline__ void hom_row(double X, double Y, double U, double V, double* au, double* av) {
    au[0] = X;   au[1] = Y;   au[2] = 1.0; au[3] = 0.0; au[4] = 0.0; au[5] = 0.0; au[6] = -(U * X); au[7] = -(U * Y); au[8] = U;
    av[0] = 0.0; av[1] = 0.0; av[2] = 0.0; av[3] = X;   av[4] = Y;   av[5] = 1.0; av[6] = -(V * X); av[7] = -(V * Y); av[8] = V;
}

// LDL^T of V + lambda diag(V), V the 6 x 6 pose block of a view's 190 entries: L below the diagonal, D; false on a pivot that is not
// positive and finite
__device__ __forceinline__ bool ldl6(const double* blk, double lambda, double L[6][6], double D[6]) {
    double A[6][6];
#pragma unroll
    for (int r = 0; r < 6; r++)
#pragma unroll
        for (int c = r; c < 6; c++) { const double v = blk[tri_index(12 + r, 12 + c, kCalAug)]; A[r][c] = v; A[c][r] = v; }
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

// R <- cay(w) R, the board pose's update in f64
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

}  // namespace a3
