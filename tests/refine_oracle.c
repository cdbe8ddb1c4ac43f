/*
 * refine_oracle.c -- CPU restatement of sub-pixel corner refinement (include/aruco3_hip.h, a3_refine_config).
 *
 * TEST INFRASTRUCTURE ONLY (tests/refine_oracle.py compiles it into a temporary directory and loads it through ctypes).  The
 * reference has no corner refinement: this is the contract of an extension, restated here so that the device kernel
 * (aruco3_amd/csrc/k_refine.hip, k_refine_corners) can be held to it bit for bit.  Compiled with -ffp-contract=off: no fused
 * multiply-add, as in the kernel.
 *
 *   w      = win_half, or (relative_win > 0 and cell_px given) min(win_half, max(2, floorf(relative_win * cell_px))) (NaN -> 2)
 *   m(i,j) = g(i) * g(j), g(i) = (float)exp(-(double)(i*i) / (double)(w*w))
 *   one iteration at c: P = bilinear samples at (c.x + i, c.y + j), i, j in [-w-1, w+1] (border replicate);
 *     over the interior (2w+1)^2 pixels, k = row-major index: gx = P[j][i+1] - P[j][i-1], gy = P[j+1][i] - P[j-1][i],
 *     a += gx*gx*m, b += gx*gy*m, c2 += gy*gy*m, bb1 += gx*gx*m*i + gx*gy*m*j, bb2 += gx*gy*m*i + gy*gy*m*j,
 *     summed per lane l of 64 over k = l, l+64, ... then combined by an xor butterfly 32, 16, 8, 4, 2, 1;
 *     det = a*c2 - b*b: 0 or not finite -> stop; else s = 1/det, c' = c + (c2*s*bb1 - b*s*bb2, -b*s*bb1 + a*s*bb2);
 *     c' farther than w from the start q0 in x or y (or not finite) -> the corner is q0 and iteration stops;
 *     else c = c', and iteration stops once |c' - c|^2 <= min_shift^2 or after max_iterations.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

/* same layout as a3_refine_config */
typedef struct {
    uint32_t method;          /* 0 none, 1 subpix */
    uint32_t win_half;        /* 1..10 */
    float    relative_win;
    uint32_t max_iterations;
    float    min_shift;
} a3o_refine_config;

/* cell size of a quad (integer corners x0,y0..x3,y3): the shortest side (sqrtf of float squares) / cells */
float a3o_quad_cell_px(const uint32_t corners[8], uint32_t cells);
/* the window weight g(i) of half-width w for i = -w .. w (2w+1 values) */
void  a3o_refine_weights(uint32_t w, float *g);
/* refines n corners (x, y float pairs, in place) of one grey frame; cell_px (nullable) per corner; -> 0, or -1 on a bad config */
int   a3o_refine_corners(const uint8_t *grey, uint32_t w, uint32_t h, const a3o_refine_config *cfg, float *corners_xy,
                         const float *cell_px, size_t n);

float a3o_quad_cell_px(const uint32_t c[8], uint32_t cells) {
    float best = 0.0f;
    for (int k = 0; k < 4; k++) {
        const int k2 = (k + 1) & 3;
        const float dx = (float)c[2 * k2] - (float)c[2 * k], dy = (float)c[2 * k2 + 1] - (float)c[2 * k + 1];
        const float len = sqrtf(dx * dx + dy * dy);
        if (k == 0 || len < best) best = len;
    }
    return best / (float)cells;
}

void a3o_refine_weights(uint32_t w, float *g) {
    for (int i = -(int)w; i <= (int)w; i++) g[i + (int)w] = (float)exp(-(double)(i * i) / (double)(w * w));
}

static int refine_window(const a3o_refine_config *cfg, const float *cell_px, size_t k) {
    const int wh = (int)cfg->win_half;
    if (!(cfg->relative_win > 0.0f) || !cell_px) return wh;
    const float t = floorf(cfg->relative_win * cell_px[k]);
    const int v = t >= 2.0f ? (t >= (float)wh ? wh : (int)t) : 2;
    return v < wh ? v : wh;
}

/* bilinear grey level at (x, y), border replicate; the order of operations is the contract's */
static float refine_sample(const uint8_t *g, int W, int H, float x, float y) {
    const float x0f = floorf(x), y0f = floorf(y);
    const float fx = x - x0f, fy = y - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const int xa = x0 < 0 ? 0 : (x0 > W - 1 ? W - 1 : x0), xb = x0 + 1 < 0 ? 0 : (x0 + 1 > W - 1 ? W - 1 : x0 + 1);
    const int ya = y0 < 0 ? 0 : (y0 > H - 1 ? H - 1 : y0), yb = y0 + 1 < 0 ? 0 : (y0 + 1 > H - 1 ? H - 1 : y0 + 1);
    const float i00 = g[(size_t)ya * W + xa], i01 = g[(size_t)ya * W + xb], i10 = g[(size_t)yb * W + xa], i11 = g[(size_t)yb * W + xb];
    return (1.0f - fy) * ((1.0f - fx) * i00 + fx * i01) + fy * ((1.0f - fx) * i10 + fx * i11);
}

int a3o_refine_corners(const uint8_t *grey, uint32_t W, uint32_t H, const a3o_refine_config *cfg, float *xy, const float *cell_px, size_t n) {
    if (!cfg || cfg->win_half < 1 || cfg->win_half > 10 || !(cfg->relative_win >= 0.0f) || !(cfg->min_shift >= 0.0f)) return -1;
    if (cfg->method == 0 || W == 0 || H == 0) return 0;
    const float eps2 = cfg->min_shift * cfg->min_shift;
    for (size_t k = 0; k < n; k++) {
        const int w = refine_window(cfg, cell_px, k), side = 2 * w + 1;
        float g[21];
        a3o_refine_weights((uint32_t)w, g);
        const float q0x = xy[2 * k], q0y = xy[2 * k + 1];
        float cx = q0x, cy = q0y;
        for (uint32_t it = 0; it < cfg->max_iterations; it++) {
            float lane[5][64];
            for (int l = 0; l < 64; l++) {
                float a = 0.0f, b = 0.0f, c2 = 0.0f, bb1 = 0.0f, bb2 = 0.0f;
                for (int q = l; q < side * side; q += 64) {
                    const int i = q % side - w, j = q / side - w;
                    const float m = g[i + w] * g[j + w];
                    const float gx = refine_sample(grey, (int)W, (int)H, cx + (float)(i + 1), cy + (float)j) -
                                     refine_sample(grey, (int)W, (int)H, cx + (float)(i - 1), cy + (float)j);
                    const float gy = refine_sample(grey, (int)W, (int)H, cx + (float)i, cy + (float)(j + 1)) -
                                     refine_sample(grey, (int)W, (int)H, cx + (float)i, cy + (float)(j - 1));
                    const float fi = (float)i, fj = (float)j;
                    a += gx * gx * m;
                    b += gx * gy * m;
                    c2 += gy * gy * m;
                    bb1 += gx * gx * m * fi + gx * gy * m * fj;
                    bb2 += gx * gy * m * fi + gy * gy * m * fj;
                }
                lane[0][l] = a; lane[1][l] = b; lane[2][l] = c2; lane[3][l] = bb1; lane[4][l] = bb2;
            }
            for (int o = 32; o >= 1; o >>= 1)   /* xor butterfly: every lane ends with the same sums */
                for (int v = 0; v < 5; v++) {
                    float nxt[64];
                    for (int l = 0; l < 64; l++) nxt[l] = lane[v][l] + lane[v][l ^ o];
                    memcpy(lane[v], nxt, sizeof nxt);
                }
            const float a = lane[0][0], b = lane[1][0], c2 = lane[2][0], bb1 = lane[3][0], bb2 = lane[4][0];
            const float det = a * c2 - b * b;
            if (det == 0.0f || !isfinite(det)) break;
            const float s = 1.0f / det;
            const float nx = cx + (c2 * s * bb1 - b * s * bb2), ny = cy + (-b * s * bb1 + a * s * bb2);
            if (!(fabsf(nx - q0x) <= (float)w && fabsf(ny - q0y) <= (float)w)) { cx = q0x; cy = q0y; break; }
            const float dx = nx - cx, dy = ny - cy;
            cx = nx; cy = ny;
            if (dx * dx + dy * dy <= eps2) break;
        }
        xy[2 * k] = cx; xy[2 * k + 1] = cy;
    }
    return 0;
}
