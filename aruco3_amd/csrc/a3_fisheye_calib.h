// a3_fisheye_calib.h -- the per-point pieces of the fisheye camera calibration of include/aruco3_hip.h (a3_calibrate_fisheye_cameras): the
// arctangent A64, the forward lens, the start's undistortion of an image point and the projection with its 14 Jacobian columns, all in
// f64.  k_calibrate_fisheye (k_calib_fisheye.hip) uses them with the homography, the LDL^T and the Cayley update of a3_calib.h.  Every
// expression is written in the contract's order and tests/fisheye_calib_oracle.c restates each one in the same order; the library is
// built with -ffp-contract=off, so nothing is fused.
#pragma once
#include "a3_calib.h"

namespace a3 {

constexpr int kFeAug = 15;        // 14 Jacobian columns (fx fy cx cy k1 k2 k3 k4, then w and t) + the residual
constexpr int kFeEntries = 120;   // upper triangle of the 15 x 15 augmented sum
constexpr int kFePose = 8;        // first pose column
constexpr int kFeRes = 14;        // the residual's column

// A64: Cephes' double atan, written out (never a library's atan: the host's and the device's need not agree)
__device__ __forceinline__ double fe_a64(double t) {
    constexpr double kMoreBits = 6.123233995736765886130e-17;
    double y0, z, m;
    if (t > 2.41421356237309504880) { y0 = 1.5707963267948966; z = -(1.0 / t); m = kMoreBits; }
    else if (t <= 0.66) { y0 = 0.0; z = t; m = 0.0; }
    else { y0 = 0.7853981633974483; z = (t - 1.0) / (t + 1.0); m = 0.5 * kMoreBits; }
    const double w = z * z;
    const double p = (((-8.750608600031904122785e-1 * w + -1.615753718733365076637e1) * w + -7.500855792314704667340e1) * w +
                      -1.228866684490136173410e2) * w + -6.485021904942025371773e1;
    const double q = ((((w + 2.485846490142306297962e1) * w + 1.650270098316988542046e2) * w + 4.328810604912902668951e2) * w +
                      4.853903996359136964868e2) * w + 1.945506571482613964425e2;
    return y0 + ((z * (w * p / q) + z) + m);
}

// step 2's undistortion of the image point (u, v) at the start parameters a: -> kept for the start, and the normalised point
__device__ __forceinline__ bool fe_start_point(const double a[8], double u, double v, double* xo, double* yo) {
    const double fx = a[0], fy = a[1], cx = a[2], cy = a[3], k1 = a[4], k2 = a[5], k3 = a[6], k4 = a[7];
    const double x0 = (u - cx) / fx, y0 = (v - cy) / fy;
    const double rd = sqrt(x0 * x0 + y0 * y0);
    double r = rd;
    for (int it = 0; it < 20; it++) {
        const double th = fe_a64(r), t2 = th * th;
        const double g = th * (1.0 + (((k4 * t2 + k3) * t2 + k2) * t2 + k1) * t2);
        const double dg = 1.0 + (((9.0 * k4 * t2 + 7.0 * k3) * t2 + 5.0 * k2) * t2 + 3.0 * k1) * t2;
        r = r - (g - rd) * (1.0 + r * r) / dg;
    }
    const double s = rd > 0.0 ? r / rd : 1.0;
    const double x = x0 * s, y = y0 * s;
    // the forward check
    const double rr = sqrt(x * x + y * y);
    const double th = fe_a64(rr), t2 = th * th;
    const double thd = th * (1.0 + (((k4 * t2 + k3) * t2 + k2) * t2 + k1) * t2);
    const double sf = rr > 0.0 ? thd / rr : 1.0;
    const double xd = x * sf, yd = y * sf;
    const double ex = (xd - x0) * fx, ey = (yd - y0) * fy;
    const double res = sqrt(ex * ex + ey * ey);
    *xo = x;
    *yo = y;
    return fin(r) && r <= A3_FISHEYE_START_MAX_R && res <= 0.1;
}

// the two augmented rows of one point: intrinsics a (fx fy cx cy k1 k2 k3 k4), pose (R, t), board point (X, Y, 0) seen at (ou, ov).
// au / av: 15 values each (columns 0-7 intrinsics, 8-10 w, 11-13 t, 14 the residual).
__device__ __forceinline__ void fisheye_row(const double a[8], const double R[9], const double t[3], double X, double Y, double ou, double ov,
                                            double* au, double* av) {
    const double fx = a[0], fy = a[1], cx = a[2], cy = a[3], k1 = a[4], k2 = a[5], k3 = a[6], k4 = a[7];
    const double qx = R[0] * X + R[1] * Y, qy = R[3] * X + R[4] * Y, qz = R[6] * X + R[7] * Y;
    const double px = qx + t[0], py = qy + t[1], pz = qz + t[2];
    const double ia = 1.0 / pz;
    const double x = px * ia, y = py * ia;
    const double r2 = x * x + y * y;
    const double r = sqrt(r2);
    const double th = fe_a64(r), t2 = th * th;
    const double poly = 1.0 + (((k4 * t2 + k3) * t2 + k2) * t2 + k1) * t2;
    const double thd = th * poly;
    const double s = r > 0.0 ? thd / r : 1.0;
    const double xd = x * s, yd = y * s;
    au[14] = (fx * xd + cx) - ou;
    av[14] = (fy * yd + cy) - ov;
    // intrinsics
    const double e = r > 0.0 ? th / r : 1.0;
    const double gx = fx * x * e, gy = fy * y * e;
    const double t4 = t2 * t2, t6 = t4 * t2, t8 = t6 * t2;
    au[0] = xd;  au[1] = 0.0; au[2] = 1.0; au[3] = 0.0;
    av[0] = 0.0; av[1] = yd;  av[2] = 0.0; av[3] = 1.0;
    au[4] = gx * t2; au[5] = gx * t4; au[6] = gx * t6; au[7] = gx * t8;
    av[4] = gy * t2; av[5] = gy * t4; av[6] = gy * t6; av[7] = gy * t8;
    // pose: d(xd, yd) / d(x, y) = s I + c (x, y)(x, y)^T, then the chain of calib_row
    const double dpoly = 1.0 + (((9.0 * k4 * t2 + 7.0 * k3) * t2 + 5.0 * k2) * t2 + 3.0 * k1) * t2;
    const double c = r > 0.0 ? (dpoly / (1.0 + r2) - s) / r2 : 0.0;
    const double xxd = s + x * x * c, xyd = x * y * c, yyd = s + y * y * c;
    const double cu = fx * ia, cv = fy * ia;
    const double u0 = cu * xxd, u1 = cu * xyd, u2 = -(cu * (xxd * x + xyd * y));
    const double v0 = cv * xyd, v1 = cv * yyd, v2 = -(cv * (xyd * x + yyd * y));
    const double q2x = 2.0 * qx, q2y = 2.0 * qy, q2z = 2.0 * qz;
    au[8] = u2 * q2y - u1 * q2z; au[9] = u0 * q2z - u2 * q2x; au[10] = u1 * q2x - u0 * q2y;
    av[8] = v2 * q2y - v1 * q2z; av[9] = v0 * q2z - v2 * q2x; av[10] = v1 * q2x - v0 * q2y;
    au[11] = u0; au[12] = u1; au[13] = u2;
    av[11] = v0; av[12] = v1; av[13] = v2;
}

}  // namespace a3
