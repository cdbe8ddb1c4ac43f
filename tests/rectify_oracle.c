/* rectify_oracle.c -- CPU restatement of the frame rectification of include/aruco3_hip.h (a3_rectify_frames), the contract the device
 * kernel k_rectify is held to byte for byte.  TEST INFRASTRUCTURE ONLY: built by tests/rectify_oracle.py with -ffp-contract=off, so
 * every expression below is evaluated as written, in f32, with correctly rounded division. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>

/* src: n_frames frames of sw x sh pixels, bpp bytes each, row y of frame f at f * src_frame + y * src_row; dst likewise, dw x dh.
 * intr_src / intr_dst: fx fy cx cy; k: k1 k2 p1 p2 k3 k4 k5 k6 (zeros for no lens); R: row-major, camera -> rectified view.
 * inside (nullable): dw x dh bytes, 1 where the pixel sees the source.  Bytes of dst outside the rows' pixels are not written. */
void a3o_rectify(const uint8_t *src, uint32_t sw, uint32_t sh, uint32_t bpp, size_t src_row, size_t src_frame, uint32_t n_frames,
                 const float *intr_src, const float *k, const float *intr_dst, const float *R, uint8_t fill, uint8_t *dst, uint32_t dw,
                 uint32_t dh, size_t dst_row, size_t dst_frame, uint8_t *inside_out) {
    const float sfx = intr_src[0], sfy = intr_src[1], scx = intr_src[2], scy = intr_src[3];
    const float dfx = intr_dst[0], dfy = intr_dst[1], dcx = intr_dst[2], dcy = intr_dst[3];
    const float k1 = k[0], k2 = k[1], p1 = k[2], p2 = k[3], k3 = k[4], k4 = k[5], k5 = k[6], k6 = k[7];
    for (uint32_t i = 0; i < dh; i++) {
        for (uint32_t j = 0; j < dw; j++) {
            const float a = ((float)j - dcx) / dfx, b = ((float)i - dcy) / dfy;
            const float X = (R[0]*a + R[3]*b) + R[6], Y = (R[1]*a + R[4]*b) + R[7], Wz = (R[2]*a + R[5]*b) + R[8];
            const float x = X / Wz, y = Y / Wz, r2 = x*x + y*y;
            const float radial = (1 + ((k3*r2 + k2)*r2 + k1)*r2) / (1 + ((k6*r2 + k5)*r2 + k4)*r2);
            const float xd = x*radial + (2*p1*x*y + p2*(r2 + 2*x*x)), yd = y*radial + (p1*(r2 + 2*y*y) + 2*p2*x*y);
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
