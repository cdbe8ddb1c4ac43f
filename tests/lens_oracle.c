/* lens_oracle.c -- CPU restatement of the lens undistortion of include/aruco3_hip.h (a3_set_distortion / a3_undistort_points), the
 * contract the device kernel k_undistort_corners is held to bit for bit, and the forward (distorting) model it inverts.  TEST
 * INFRASTRUCTURE ONLY: built by tests/lens_oracle.py with -ffp-contract=off, so every expression below is evaluated as written, in
 * f32, with correctly rounded division and sqrtf. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

/* k: k1 k2 p1 p2 k3 k4 k5 k6; intr: fx fy cx cy */
void a3o_undistort(const float *xy, size_t n, const float *intr, const float *k, uint32_t iterations, float max_residual_px,
                   float *out_xy, float *residual_px) {
    const float fx = intr[0], fy = intr[1], cx = intr[2], cy = intr[3];
    const float k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4], k4 = k[5], k5 = k[6], k6 = k[7];
    for (size_t i = 0; i < n; i++) {
        const float u = xy[2 * i], v = xy[2 * i + 1];
        const float x0 = (u - cx) / fx, y0 = (v - cy) / fy;
        float x = x0, y = y0;
        for (uint32_t it = 0; it < iterations; it++) {
            const float r2 = x*x + y*y;
            const float icdist = (1 + ((k6*r2 + k5)*r2 + k4)*r2) / (1 + ((k3*r2 + k2)*r2 + k1)*r2);
            const float dx = 2*p1*x*y + p2*(r2 + 2*x*x);
            const float dy = p1*(r2 + 2*y*y) + 2*p2*x*y;
            x = (x0 - dx)*icdist;
            y = (y0 - dy)*icdist;
        }
        const float r2 = x*x + y*y;
        const float radial = (1 + ((k3*r2 + k2)*r2 + k1)*r2) / (1 + ((k6*r2 + k5)*r2 + k4)*r2);
        const float xd = x*radial + (2*p1*x*y + p2*(r2 + 2*x*x));
        const float yd = y*radial + (p1*(r2 + 2*y*y) + 2*p2*x*y);
        const float ex = (xd - x0)*fx, ey = (yd - y0)*fy;
        const float res = sqrtf(ex*ex + ey*ey);
        const int ok = isfinite(x) && isfinite(y) && isfinite(res) && res <= max_residual_px;
        out_xy[2 * i] = ok ? x*fx + cx : u;
        out_xy[2 * i + 1] = ok ? y*fy + cy : v;
        if (residual_px) residual_px[i] = ok ? res : INFINITY;
    }
}

/* the forward model: ideal pixels -> distorted pixels (the "check" step of the contract, taken to pixels) */
void a3o_distort(const float *xy, size_t n, const float *intr, const float *k, float *out_xy) {
    const float fx = intr[0], fy = intr[1], cx = intr[2], cy = intr[3];
    const float k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4], k4 = k[5], k5 = k[6], k6 = k[7];
    for (size_t i = 0; i < n; i++) {
        const float x = (xy[2 * i] - cx) / fx, y = (xy[2 * i + 1] - cy) / fy;
        const float r2 = x*x + y*y;
        const float radial = (1 + ((k3*r2 + k2)*r2 + k1)*r2) / (1 + ((k6*r2 + k5)*r2 + k4)*r2);
        const float xd = x*radial + (2*p1*x*y + p2*(r2 + 2*x*x));
        const float yd = y*radial + (p1*(r2 + 2*y*y) + 2*p2*x*y);
        out_xy[2 * i] = xd*fx + cx;
        out_xy[2 * i + 1] = yd*fy + cy;
    }
}
