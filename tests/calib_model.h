/* calib_model.h -- the rational lens model's row: what the camera calibration, the rig, the marker map and the hand-eye oracles all
 * project through.  TEST INFRASTRUCTURE ONLY. */
#ifndef A3_CALIB_MODEL_H
#define A3_CALIB_MODEL_H
#include "solve_oracle.h"

#define AUG 19    /* 12 intrinsics (fx fy cx cy k1 k2 p1 p2 k3 k4 k5 k6), w, t, the residual */

/* the model and its 18 Jacobian columns; column 18 the residual */
static inline void calib_row(const double a[12], const double R[9], const double t[3], double X, double Y, double ou, double ov, double *au, double *av) {
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

#endif
