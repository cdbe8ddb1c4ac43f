// a3_handeye.h -- the pieces of the hand-eye calibration of include/aruco3_hip.h (a3_calibrate_hand_eyes) that are its own: the
// quaternion conversion, a pair's terms of the start, the 3 x 3 solve with its pivot rule, the four charts and the augmented row of 13
// through G = (X . M_f) . Y, on top of the rig's poses and columns (a3_rig.h), all in f64.  k_handeye (k_handeye.hip) is the only user.
// Every expression is written in the contract's order and tests/handeye_oracle.c restates each one in the same order.
#pragma once
#include "a3_rig.h"

namespace a3 {

__device__ __forceinline__ void he_quat(const double* R, double q[4]) {
    const double tr = (R[0] + R[4]) + R[8];
    if (tr >= R[0] && tr >= R[4] && tr >= R[8]) {
        const double s = sqrt(tr + 1.0) * 2.0;
        q[0] = 0.25 * s; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s;
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        const double s = sqrt(((1.0 + R[0]) - R[4]) - R[8]) * 2.0;
        q[0] = (R[7] - R[5]) / s; q[1] = 0.25 * s; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s;
    } else if (R[4] >= R[8]) {
        const double s = sqrt(((1.0 + R[4]) - R[0]) - R[8]) * 2.0;
        q[0] = (R[2] - R[6]) / s; q[1] = (R[1] + R[3]) / s; q[2] = 0.25 * s; q[3] = (R[5] + R[7]) / s;
    } else {
        const double s = sqrt(((1.0 + R[8]) - R[0]) - R[4]) * 2.0;
        q[0] = (R[3] - R[1]) / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = 0.25 * s;
    }
    if (q[0] < 0.0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
}

__device__ __forceinline__ void he_quat_rot(const double q[4], double* R) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z); R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y); R[7] = 2.0 * (y * z + w * x); R[8] = 1.0 - 2.0 * (x * x + y * y);
}

// A = P_i . P_j^-1, B = M_i . M_j^-1 -> whether the pair counts
__device__ __forceinline__ bool he_pair(const double* Pi, const double* Pj, const double* Mi, const double* Mj, double* A, double* B, double qa[4],
                                        double qb[4]) {
    double I[12];
    pose_inv(Pj, I);
    pose_mul(Pi, I, A);
    pose_inv(Mj, I);
    pose_mul(Mi, I, B);
    he_quat(A, qa);
    he_quat(B, qb);
    return qb[0] >= A3_HANDEYE_COS_HALF_MAX_PAIR_ANGLE && qb[0] <= A3_HANDEYE_COS_HALF_MIN_PAIR_ANGLE;
}

// the pair's term of N (10 entries) added to s
__device__ __forceinline__ void he_pair_rot(const double qa[4], const double qb[4], double* s) {
    const double d = qa[0] - qb[0];
    const double dl[3] = {qa[1] - qb[1], qa[2] - qb[2], qa[3] - qb[3]};
    const double sg[3] = {qa[1] + qb[1], qa[2] + qb[2], qa[3] + qb[3]};
    const double K[4][4] = {{d, -dl[0], -dl[1], -dl[2]}, {dl[0], d, -sg[2], sg[1]}, {dl[1], sg[2], d, -sg[0]}, {dl[2], -sg[1], sg[0], d}};
    int e = 0;
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = a; b < 4; b++, e++) {
            double t = 0.0;
#pragma unroll
            for (int r = 0; r < 4; r++) t = t + K[r][a] * K[r][b];
            s[e] = s[e] + t;
        }
}

// the pair's terms of D^T D (6 entries) and D^T c (3) added to s
__device__ __forceinline__ void he_pair_tr(const double* A, const double* B, const double* RX, double* s) {
    double D[9], c[3];
#pragma unroll
    for (int q = 0; q < 9; q++) D[q] = A[q] - (q == 0 || q == 4 || q == 8 ? 1.0 : 0.0);
#pragma unroll
    for (int r = 0; r < 3; r++) c[r] = ((RX[3 * r] * B[9] + RX[3 * r + 1] * B[10]) + RX[3 * r + 2] * B[11]) - A[9 + r];
    int e = 0;
#pragma unroll
    for (int a = 0; a < 3; a++)
#pragma unroll
        for (int b = a; b < 3; b++, e++) {
            double t = 0.0;
#pragma unroll
            for (int r = 0; r < 3; r++) t = t + D[3 * r + a] * D[3 * r + b];
            s[e] = s[e] + t;
        }
#pragma unroll
    for (int a = 0; a < 3; a++) {
        double t = 0.0;
#pragma unroll
        for (int r = 0; r < 3; r++) t = t + D[3 * r + a] * c[r];
        s[6 + a] = s[6 + a] + t;
    }
}

// S: S00 S01 S02 S11 S12 S22.  -> false when degenerate
__device__ __forceinline__ bool he_solve3(const double S[6], const double b[3], double x[3]) {
    double mx = S[0];
    if (S[3] > mx) mx = S[3];
    if (S[5] > mx) mx = S[5];
    const double thr = A3_HANDEYE_MIN_PIVOT_RATIO * mx;
    const double d0 = S[0];
    if (!fin(d0) || !(d0 > thr)) return false;
    const double l10 = S[1] / d0, l20 = S[2] / d0;
    const double d1 = S[3] - l10 * l10 * d0;
    if (!fin(d1) || !(d1 > thr)) return false;
    const double l21 = (S[4] - l20 * l10 * d0) / d1;
    const double d2 = (S[5] - l20 * l20 * d0) - l21 * l21 * d1;
    if (!fin(d2) || !(d2 > thr)) return false;
    const double y0 = b[0], y1 = b[1] - l10 * y0, y2 = (b[2] - l20 * y0) - l21 * y1;
    x[2] = y2 / d2;
    x[1] = y1 / d1 - l21 * x[2];
    x[0] = (y0 / d0 - l10 * x[1]) - l20 * x[2];
    return true;
}

// the four charts over N (10 entries, upper triangle row by row) -> false when all are degenerate
__device__ inline bool he_charts(const double* N, double q[4]) {
    double Nf[4][4];
    int e = 0;
    for (int a = 0; a < 4; a++)
        for (int b = a; b < 4; b++, e++) { Nf[a][b] = N[e]; Nf[b][a] = N[e]; }
    int best = -1;
    double bn = 0.0;
    for (int k = 0; k < 4; k++) {
        int id[3], m = 0;
        for (int r = 0; r < 4; r++)
            if (r != k) id[m++] = r;
        const double S[6] = {Nf[id[0]][id[0]], Nf[id[0]][id[1]], Nf[id[0]][id[2]], Nf[id[1]][id[1]], Nf[id[1]][id[2]], Nf[id[2]][id[2]]};
        const double b[3] = {-Nf[id[0]][k], -Nf[id[1]][k], -Nf[id[2]][k]};
        double x[3], c[4];
        if (!he_solve3(S, b, x)) continue;
        c[k] = 1.0; c[id[0]] = x[0]; c[id[1]] = x[1]; c[id[2]] = x[2];
        const double n2 = ((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) + c[3] * c[3];
        if (best < 0 || n2 < bn) {
            best = k; bn = n2;
            const double n = sqrt(n2);
            for (int r = 0; r < 4; r++) q[r] = c[r] / n;
        }
    }
    return best >= 0;
}

// the two augmented rows of one point through G = (X . M) . Y; Ep = X . M
__device__ __forceinline__ void he_row(const double a[12], const double* X, const double* M, const double* Y, const double* Ep, const double* G,
                                       double Xc, double Yc, double ou, double ov, double* au, double* av) {
    double cu[kCalAug], cv[kCalAug];
    calib_row(a, G, G + 9, Xc, Yc, ou, ov, cu, cv);
    const double qf[3] = {Y[0] * Xc + Y[1] * Yc, Y[3] * Xc + Y[4] * Yc, Y[6] * Xc + Y[7] * Yc};
    const double y[3] = {qf[0] + Y[9], qf[1] + Y[10], qf[2] + Y[11]};
    double m[3], qc[3];
#pragma unroll
    for (int r = 0; r < 3; r++) m[r] = ((M[3 * r] * y[0] + M[3 * r + 1] * y[1]) + M[3 * r + 2] * y[2]) + M[9 + r];
#pragma unroll
    for (int r = 0; r < 3; r++) qc[r] = (X[3 * r] * m[0] + X[3 * r + 1] * m[1]) + X[3 * r + 2] * m[2];
    rig_cols(cu + 15, Ep, qc, qf, cu[18], au);
    rig_cols(cv + 15, Ep, qc, qf, cv[18], av);
}

}  // namespace a3
