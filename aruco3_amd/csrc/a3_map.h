// a3_map.h -- the per-point pieces of the marker map solve of include/aruco3_hip.h (a3_build_marker_maps) that the rig's headers do
// not have: the residual-only cost of one observation, the mirrored planar candidate and the index of the frame columns' 7-triangle
// in the row of 13, all in f64.  k_map (k_map.hip) is the only user.  Every expression is written in the contract's order and
// tests/map_oracle.c restates each one in the same order.
#pragma once
#include "a3_rig.h"

namespace a3 {

// cost(G, o): the model of calib_row, its residual only, over the four corners in order
__device__ __forceinline__ double map_cost(const double a[12], const double* G, const float* sq, const float* __restrict__ img) {
    const double fx = a[0], fy = a[1], cx = a[2], cy = a[3];
    const double k1 = a[4], k2 = a[5], p1 = a[6], p2 = a[7], k3 = a[8], k4 = a[9], k5 = a[10], k6 = a[11];
    double s = 0.0;
#pragma unroll 1
    for (int j = 0; j < 4; j++) {
        const double X = (double)sq[2 * j], Y = (double)sq[2 * j + 1], ou = (double)img[2 * j], ov = (double)img[2 * j + 1];
        const double qx = G[0] * X + G[1] * Y, qy = G[3] * X + G[4] * Y, qz = G[6] * X + G[7] * Y;
        const double px = qx + G[9], py = qy + G[10], pz = qz + G[11];
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
        const double ru = (fx * xd + cx) - ou;
        const double rv = (fy * yd + cy) - ov;
        s = s + ru * ru;
        s = s + rv * rv;
    }
    return fin(s) ? s : __builtin_inf();
}

// the second planar candidate's start: the rotation's columns mirrored through the plane across the line of sight, the normal negated
__device__ __forceinline__ void pose_flip(const double* P, double* Q) {
    const double n = sqrt((P[9] * P[9] + P[10] * P[10]) + P[11] * P[11]);
    const double v[3] = {P[9] / n, P[10] / n, P[11] / n};
#pragma unroll
    for (int c = 0; c < 3; c++) {
        const double d = (v[0] * P[c] + v[1] * P[3 + c]) + v[2] * P[6 + c];
        const double k = 2.0 * d;
#pragma unroll
        for (int r = 0; r < 3; r++) {
            const double x = P[3 * r + c] - k * v[r];
            Q[3 * r + c] = c < 2 ? x : -x;
        }
    }
#pragma unroll
    for (int q = 9; q < 12; q++) Q[q] = P[q];
}

// entry e of the 7-triangle over columns (0-5, 12) in the 13-triangle
__device__ __forceinline__ int map_frame_tri(int e) {
    int i, k;
    tri_ik(e, 7, &i, &k);
    return tri_index(i < 6 ? i : 12, k < 6 ? k : 12, kRigAug);
}

}  // namespace a3
