// a3_rig.h -- the per-point pieces of the camera rig calibration of include/aruco3_hip.h (a3_calibrate_rigs): pose composition and the
// augmented row of 13 (6 extrinsic columns, 6 frame columns, the residual) on top of the calibration's model (a3_calib.h), all in
// f64.  k_rig (k_rig.hip) is the only user.  Every expression is written in the contract's order and tests/rig_oracle.c restates each
// one in the same order.
#pragma once
#include "a3_calib.h"

namespace a3 {

constexpr int kRigAug = 13;       // (w, t) of the extrinsics, (w, t) of the frame pose, the residual
constexpr int kRigEntries = 91;   // upper triangle of the 13 x 13 augmented sum
constexpr int kRigFrameTri = 63;  // its rows 6 .. 12 are the 7-triangle (V_f, g_f, cost) of the frame columns: entries 63 .. 90

// poses are 12 doubles: R (9, row-major), t (3); pose_update is in a3_solve.h.  O = A . B
__device__ __forceinline__ void pose_mul(const double* A, const double* B, double* O) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) O[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
        O[9 + r] = ((A[3 * r] * B[9] + A[3 * r + 1] * B[10]) + A[3 * r + 2] * B[11]) + A[9 + r];
    }
}

__device__ __forceinline__ void pose_inv(const double* A, double* O) {
#pragma unroll
    for (int r = 0; r < 3; r++) {
#pragma unroll
        for (int c = 0; c < 3; c++) O[3 * r + c] = A[3 * c + r];
        O[9 + r] = -((A[r] * A[9] + A[3 + r] * A[10]) + A[6 + r] * A[11]);
    }
}

__device__ __forceinline__ void rig_cols(const double u[3], const double* Rc, const double qc[3], const double qf[3], double res, double* o) {
    const double cx = 2.0 * qc[0], cy = 2.0 * qc[1], cz = 2.0 * qc[2];
    o[0] = u[2] * cy - u[1] * cz; o[1] = u[0] * cz - u[2] * cx; o[2] = u[1] * cx - u[0] * cy;
    o[3] = u[0]; o[4] = u[1]; o[5] = u[2];
    double ur[3];
#pragma unroll
    for (int j = 0; j < 3; j++) ur[j] = (u[0] * Rc[j] + u[1] * Rc[3 + j]) + u[2] * Rc[6 + j];
    const double fx = 2.0 * qf[0], fy = 2.0 * qf[1], fz = 2.0 * qf[2];
    o[6] = ur[2] * fy - ur[1] * fz; o[7] = ur[0] * fz - ur[2] * fx; o[8] = ur[1] * fx - ur[0] * fy;
    o[9] = ur[0]; o[10] = ur[1]; o[11] = ur[2];
    o[12] = res;
}

// the two augmented rows of one point: intrinsics a, E rig -> camera (its rotation is read), T board -> rig, G = E . T
__device__ __forceinline__ void rig_row(const double a[12], const double* E, const double* T, const double* G, double X, double Y, double ou,
                                        double ov, double* au, double* av) {
    double cu[kCalAug], cv[kCalAug];
    calib_row(a, G, G + 9, X, Y, ou, ov, cu, cv);
    const double qf[3] = {T[0] * X + T[1] * Y, T[3] * X + T[4] * Y, T[6] * X + T[7] * Y};
    const double y[3] = {qf[0] + T[9], qf[1] + T[10], qf[2] + T[11]};
    double qc[3];
#pragma unroll
    for (int r = 0; r < 3; r++) qc[r] = (E[3 * r] * y[0] + E[3 * r + 1] * y[1]) + E[3 * r + 2] * y[2];
    rig_cols(cu + 15, E, qc, qf, cu[18], au);
    rig_cols(cv + 15, E, qc, qf, cv[18], av);
}

}  // namespace a3
