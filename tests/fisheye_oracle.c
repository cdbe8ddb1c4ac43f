/* fisheye_oracle.c -- CPU restatement of the fisheye lens model of include/aruco3_hip.h (a3_distortion model A3_DIST_FISHEYE): the
 * fixed-arithmetic arctangent A, the forward model F, the corner undistortion (a3_set_distortion / a3_undistort_points) and the frame
 * rectification (a3_rectify_frames), the contracts the device kernels k_undistort_corners and k_rectify are held to bit for bit.  TEST
 * INFRASTRUCTURE ONLY: built by tests/fisheye_oracle.py with -ffp-contract=off, so every expression below is evaluated as written, in
 * f32, with correctly rounded division and sqrtf.  No other math function appears: atanf of libm is not the contract's A. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

/* the contract's A(t): Cephes' atanf polynomial on three ranges, evaluated as written for any input */
static float A(float t) {
    float y0, z;
    if (t > 2.414213562373095f) { y0 = 1.5707963267948966f; z = -(1.0f / t); }
    else if (t > 0.4142135623730950f) { y0 = 0.7853981633974483f; z = (t - 1.0f) / (t + 1.0f); }
    else { y0 = 0.0f; z = t; }
    const float w = z*z;
    return y0 + ((((8.05374449538e-2f*w - 1.38776856032e-1f)*w + 1.99777106478e-1f)*w - 3.33329491539e-1f)*w*z + z);
}

/* the contract's forward model F in the normalised plane */
static void F(float k1, float k2, float k3, float k4, float x, float y, float *xd, float *yd) {
    const float r = sqrtf(x*x + y*y);
    const float th = A(r), t2 = th*th;
    const float thd = th*(1 + (((k4*t2 + k3)*t2 + k2)*t2 + k1)*t2);
    const float s = r > 0 ? thd / r : 1;
    *xd = x*s;
    *yd = y*s;
}

void a3o_fisheye_atan(const float *t, size_t n, float *out) {
    for (size_t i = 0; i < n; i++) out[i] = A(t[i]);
}

/* the forward model: ideal pixels -> distorted pixels.  k: k1 k2 k3 k4; intr: fx fy cx cy */
void a3o_fisheye_distort(const float *xy, size_t n, const float *intr, const float *k, float *out_xy) {
    const float fx = intr[0], fy = intr[1], cx = intr[2], cy = intr[3];
    for (size_t i = 0; i < n; i++) {
        const float x = (xy[2 * i] - cx) / fx, y = (xy[2 * i + 1] - cy) / fy;
        float xd, yd;
        F(k[0], k[1], k[2], k[3], x, y, &xd, &yd);
        out_xy[2 * i] = xd*fx + cx;
        out_xy[2 * i + 1] = yd*fy + cy;
    }
}

/* k: k1 k2 k3 k4; intr: fx fy cx cy */
void a3o_fisheye_undistort(const float *xy, size_t n, const float *intr, const float *k, uint32_t iterations, float max_residual_px,
                           float *out_xy, float *residual_px) {
    const float fx = intr[0], fy = intr[1], cx = intr[2], cy = intr[3];
    const float k1 = k[0], k2 = k[1], k3 = k[2], k4 = k[3];
    for (size_t i = 0; i < n; i++) {
        const float u = xy[2 * i], v = xy[2 * i + 1];
        const float x0 = (u - cx) / fx, y0 = (v - cy) / fy;
        const float rd = sqrtf(x0*x0 + y0*y0);
        float r = rd;
        for (uint32_t it = 0; it < iterations; it++) {
            const float th = A(r), t2 = th*th;
            const float g = th*(1 + (((k4*t2 + k3)*t2 + k2)*t2 + k1)*t2);
            const float dg = 1 + (((9*k4*t2 + 7*k3)*t2 + 5*k2)*t2 + 3*k1)*t2;
            r = r - (g - rd)*(1 + r*r)/dg;
        }
        const float s = rd > 0 ? r / rd : 1;
        const float x = x0*s, y = y0*s;
        float xd, yd;
        F(k1, k2, k3, k4, x, y, &xd, &yd);
        const float ex = (xd - x0)*fx, ey = (yd - y0)*fy;
        const float res = sqrtf(ex*ex + ey*ey);
        const int ok = isfinite(x) && isfinite(y) && isfinite(res) && res <= max_residual_px;
        out_xy[2 * i] = ok ? x*fx + cx : u;
        out_xy[2 * i + 1] = ok ? y*fy + cy : v;
        if (residual_px) residual_px[i] = ok ? res : INFINITY;
    }
}

/* a3o_rectify's signature and blend (tests/rectify_oracle.c), restated, with (xd, yd) = F(x, y).  k: the 8 slots of a3_distortion,
 * k1 k2 p1 p2 k3 k4 k5 k6, of which the fisheye model reads k1 k2 k3 k4 (slots 0 1 4 5). */
void a3o_fisheye_rectify(const uint8_t *src, uint32_t sw, uint32_t sh, uint32_t bpp, size_t src_row, size_t src_frame, uint32_t n_frames,
                         const float *intr_src, const float *k, const float *intr_dst, const float *R, uint8_t fill, uint8_t *dst,
                         uint32_t dw, uint32_t dh, size_t dst_row, size_t dst_frame, uint8_t *inside_out) {
    const float sfx = intr_src[0], sfy = intr_src[1], scx = intr_src[2], scy = intr_src[3];
    const float dfx = intr_dst[0], dfy = intr_dst[1], dcx = intr_dst[2], dcy = intr_dst[3];
    const float k1 = k[0], k2 = k[1], k3 = k[4], k4 = k[5];
    for (uint32_t i = 0; i < dh; i++) {
        for (uint32_t j = 0; j < dw; j++) {
            const float a = ((float)j - dcx) / dfx, b = ((float)i - dcy) / dfy;
            const float X = (R[0]*a + R[3]*b) + R[6], Y = (R[1]*a + R[4]*b) + R[7], Wz = (R[2]*a + R[5]*b) + R[8];
            const float x = X / Wz, y = Y / Wz;
            float xd, yd;
            F(k1, k2, k3, k4, x, y, &xd, &yd);
            const float u = xd*sfx + scx, v = yd*sfy + scy;
            const int inside = Wz > 0 && isfinite(u) && isfinite(v) && 0 <= u && u <= (float)(sw - 1) && 0 <= v && v <= (float)(sh - 1);
            if (inside_out) inside_out[(size_t)i * dw + j] = (uint8_t)inside;
            if (!inside) {
                for (uint32_t f = 0; f < n_frames; f++)
                    for (uint32_t c = 0; c < bpp; c++) dst[f * dst_frame + i * dst_row + (size_t)j * bpp + c] = fill;
                continue;
            }
            const float fx0 = floorf(u), fy0 = floorf(v);
            const float ax = u - fx0, ay = v - fy0;
            const uint32_t x0 = (uint32_t)fx0, y0 = (uint32_t)fy0;
            const uint32_t x1 = x0 + 1 < sw - 1 ? x0 + 1 : sw - 1, y1 = y0 + 1 < sh - 1 ? y0 + 1 : sh - 1;
            for (uint32_t f = 0; f < n_frames; f++) {
                const uint8_t *r0 = src + f * src_frame + y0 * src_row, *r1 = src + f * src_frame + y1 * src_row;
                for (uint32_t c = 0; c < bpp; c++) {
                    const float i00 = r0[(size_t)x0 * bpp + c], i01 = r0[(size_t)x1 * bpp + c];
                    const float i10 = r1[(size_t)x0 * bpp + c], i11 = r1[(size_t)x1 * bpp + c];
                    const float val = (1-ay)*((1-ax)*i00 + ax*i01) + ay*((1-ax)*i10 + ax*i11);
                    const float q = floorf(val + 0.5f);
                    dst[f * dst_frame + i * dst_row + (size_t)j * bpp + c] = (uint8_t)(q < 255.0f ? q : 255.0f);
                }
            }
        }
    }
}
