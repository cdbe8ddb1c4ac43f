// a3_calib.h -- the per-point and per-view pieces of the camera calibration of include/aruco3_hip.h (a3_calibrate_cameras): the
// projection with its 18 Jacobian columns, the homography rows and the wave-level homography, all in f64, on top of
// the shared solver pieces of a3_solve.h.  k_calibrate (k_calib.hip) uses them, and through a3_rig.h k_rig, k_map and k_handeye.  Every
// expression is written in the contract's order and tests/calib_oracle.c restates each one in the same order; the library is built
// with -ffp-contract=off, so nothing is fused.
#pragma once
#include "a3_solve.h"

namespace a3 {

constexpr int kCalAug = 19;        // 18 Jacobian columns (12 intrinsics, then w and t) + the residual
constexpr int kCalEntries = 190;   // upper triangle of the 19 x 19 augmented sum
constexpr int kHomAug = 9;         // 8 homography columns + the right-hand side
constexpr int kHomEntries = 45;

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

// step 1 for one view with >= 4 points (wave-level): -> whether the homography (row-major, H22 = 1) was written to H
__device__ inline bool view_homography(const float* __restrict__ obj, const float* __restrict__ img, uint32_t p0, uint32_t np, double* rows, double* wv,
                                int lane, double* H) {
    if (lane == 0) {
        double sx = 0.0, sy = 0.0, su = 0.0, sv = 0.0;
        for (uint32_t j = 0; j < np; j++) {
            const size_t p = (size_t)p0 + j;
            sx = sx + (double)obj[2 * p];
            sy = sy + (double)obj[2 * p + 1];
            su = su + (double)img[2 * p];
            sv = sv + (double)img[2 * p + 1];
        }
        const double n = (double)np;
        const double mx = sx / n, my = sy / n, mu = su / n, mv = sv / n;
        double dob = 0.0, dim = 0.0;
        for (uint32_t j = 0; j < np; j++) {
            const size_t p = (size_t)p0 + j;
            const double ox = (double)obj[2 * p] - mx, oy = (double)obj[2 * p + 1] - my;
            const double ix = (double)img[2 * p] - mu, iy = (double)img[2 * p + 1] - mv;
            dob = dob + sqrt(ox * ox + oy * oy);
            dim = dim + sqrt(ix * ix + iy * iy);
        }
        wv[0] = mx; wv[1] = my; wv[2] = 1.4142135623730951 / (dob / n);
        wv[3] = mu; wv[4] = mv; wv[5] = 1.4142135623730951 / (dim / n);
    }
    wave_sync();
    const double mx = wv[0], my = wv[1], so = wv[2], mu = wv[3], mv = wv[4], si = wv[5];
    int ei = 0, ek = 0;
    if (lane < kHomEntries) tri_ik(lane, kHomAug, &ei, &ek);
    double acc = 0.0;
    for (uint32_t c0 = 0; c0 < np; c0 += 64) {
        const uint32_t cnt = min(64u, np - c0);
        if ((uint32_t)lane < cnt) {
            const size_t p = (size_t)p0 + c0 + (uint32_t)lane;
            hom_row(((double)obj[2 * p] - mx) * so, ((double)obj[2 * p + 1] - my) * so, ((double)img[2 * p] - mu) * si,
                    ((double)img[2 * p + 1] - mv) * si, rows + lane * 2 * kHomAug, rows + lane * 2 * kHomAug + kHomAug);
        }
        wave_sync();
        for (uint32_t j = 0; j < cnt; j++) {
            const double* u = rows + j * 2 * kHomAug;
            const double* v = u + kHomAug;
            acc = acc + u[ei] * u[ek];
            acc = acc + v[ei] * v[ek];
        }
        wave_sync();
    }
    if (lane < kHomEntries) rows[lane] = acc;
    wave_sync();
    if (lane == 0) {
        double* A = rows + 64;   // 8 x 8, then b (8), then h (8)
        double* b = A + 64;
        double* h = b + 8;
        for (int i = 0; i < 8; i++) {
            for (int k = 0; k < 8; k++) A[i * 8 + k] = rows[i <= k ? tri_index(i, k, kHomAug) : tri_index(k, i, kHomAug)];
            b[i] = rows[tri_index(i, 8, kHomAug)];
        }
        double amax = 0.0;
        for (int i = 0; i < 8; i++) {
            const double d = fabs(A[i * 9]);
            if (d > amax) amax = d;
        }
        const double thr = 1e-10 * amax;
        bool ok = true;
        for (int c = 0; c < 8 && ok; c++) {
            int piv = c;
            double best = fabs(A[c * 9]);
            for (int r = c + 1; r < 8; r++) {
                const double v = fabs(A[r * 8 + c]);
                if (v > best) { best = v; piv = r; }
            }
            if (!(best > thr) || !fin(best)) { ok = false; break; }
            if (piv != c) {
                for (int k = 0; k < 8; k++) { const double s = A[piv * 8 + k]; A[piv * 8 + k] = A[c * 8 + k]; A[c * 8 + k] = s; }
                const double s = b[piv]; b[piv] = b[c]; b[c] = s;
            }
            for (int r = c + 1; r < 8; r++) {
                const double f = A[r * 8 + c] / A[c * 9];
                for (int k = c + 1; k < 8; k++) A[r * 8 + k] = A[r * 8 + k] - f * A[c * 8 + k];
                b[r] = b[r] - f * b[c];
            }
        }
        if (ok) {
            for (int r = 7; r >= 0; r--) {
                double s = b[r];
                for (int k = r + 1; k < 8; k++) s = s - A[r * 8 + k] * h[k];
                h[r] = s / A[r * 9];
            }
            const double Hn[9] = {h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], 1.0};
            double M[9], G[9];
            for (int r = 0; r < 3; r++) {
                M[3 * r] = Hn[3 * r] * so;
                M[3 * r + 1] = Hn[3 * r + 1] * so;
                M[3 * r + 2] = Hn[3 * r + 2] - (M[3 * r] * mx + M[3 * r + 1] * my);
            }
            for (int c = 0; c < 3; c++) {
                G[c] = M[c] / si + mu * M[6 + c];
                G[3 + c] = M[3 + c] / si + mv * M[6 + c];
                G[6 + c] = M[6 + c];
            }
            const double h22 = G[8];
            for (int i = 0; i < 9; i++) {
                const double v = G[i] / h22;
                ok = ok && fin(v);
                H[i] = v;
            }
        }
        wv[6] = ok ? 1.0 : 0.0;
    }
    wave_sync();
    return wv[6] != 0.0;
}

}  // namespace a3
