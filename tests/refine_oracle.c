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

/* ---- the traced entry: the same iteration with a record of how it went, and deliberately wrong restatements of it ----
 *
 * a3o_refine_corners_trace(..., variant 0) is the contract above, written a second time so that each corner also reports the window it
 * used, the iterations it ran, how the iteration ended and how far the estimate went from its start (tests/refine_cases.py builds its
 * census from these; tests/test_refine_cases.py holds variant 0 bit-equal to a3o_refine_corners).  The other variants are mistakes
 * the kernel could make, stated here so that the designed cases can be shown to tell each of them from the contract:
 *   1  the tile one column and row short: integer sample coordinates clamped to F - 2w - 2 .. F + 2w + 2 (F = floor(q0))
 *   2  the tile origin from (int)q0 instead of floorf(q0): coordinates clamped to (int)q0 - 2w - 2 .. (int)q0 + 2w + 3
 *   3  the five sums in plain row-major order, one accumulator each, instead of per lane and butterfly
 *   4  no test of q < npx on a lane's first trip: q in npx .. 63 summed as pixels of the rows below the window (weights from the
 *      same expression, i and j from the same division)
 *   5  the weight row of w - 1 (of w + 1 at w == 1): g(i) = exp(-i*i / (w'*w'))
 *   6  zero outside the frame instead of border replicate
 *   7  the revert test measured from the current estimate instead of from q0
 *   8  the relative window rintf(relative_win * cell_px) with a floor of 1 instead of floorf with a floor of 2 (NaN -> 1)
 *   9  the tile short of a column the window needs: coordinates clamped to F - 2w .. F + 2w + 1
 * 1 and 2 only take the guard column from one side of the tile (a3_subpix.h, kRefineTile); 9 takes a column that is read.
 */
enum { A3O_EXIT_DET0 = 0, A3O_EXIT_NONFINITE = 1, A3O_EXIT_REVERT = 2, A3O_EXIT_CONVERGED = 3, A3O_EXIT_CAP = 4 };

typedef struct {
    const uint8_t *g;
    int W, H, variant;
    int lox, hix, loy, hiy;   /* the tile's columns and rows (variants 1, 2, 9) */
} trace_src;

static float trace_pixel(const trace_src *s, int x, int y) {
    if (s->variant == 1 || s->variant == 2 || s->variant == 9) {
        x = x < s->lox ? s->lox : (x > s->hix ? s->hix : x);
        y = y < s->loy ? s->loy : (y > s->hiy ? s->hiy : y);
    }
    if (s->variant == 6 && (x < 0 || x > s->W - 1 || y < 0 || y > s->H - 1)) return 0.0f;
    x = x < 0 ? 0 : (x > s->W - 1 ? s->W - 1 : x);
    y = y < 0 ? 0 : (y > s->H - 1 ? s->H - 1 : y);
    return (float)s->g[(size_t)y * s->W + x];
}

static float trace_sample(const trace_src *s, float x, float y) {
    const float x0f = floorf(x), y0f = floorf(y);
    const float fx = x - x0f, fy = y - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const float i00 = trace_pixel(s, x0, y0), i01 = trace_pixel(s, x0 + 1, y0), i10 = trace_pixel(s, x0, y0 + 1), i11 = trace_pixel(s, x0 + 1, y0 + 1);
    return (1.0f - fy) * ((1.0f - fx) * i00 + fx * i01) + fy * ((1.0f - fx) * i10 + fx * i11);
}

static int trace_window(const a3o_refine_config *cfg, const float *cell_px, size_t k, int variant) {
    if (variant != 8) return refine_window(cfg, cell_px, k);
    const int wh = (int)cfg->win_half;
    if (!(cfg->relative_win > 0.0f) || !cell_px) return wh;
    const float t = rintf(cfg->relative_win * cell_px[k]);
    const int v = t >= 1.0f ? (t >= (float)wh ? wh : (int)t) : 1;
    return v < wh ? v : wh;
}

/* as a3o_refine_corners; per corner (each nullable): win the window used, iters the iterations run, how one of A3O_EXIT_* (CAP also
 * when max_iterations == 0), excursion the largest max(|cx - q0x|, |cy - q0y|) over the estimates kept */
int a3o_refine_corners_trace(const uint8_t *grey, uint32_t W, uint32_t H, const a3o_refine_config *cfg, float *xy, const float *cell_px, size_t n,
                             int variant, int32_t *win, uint32_t *iters, int32_t *how, float *excursion);

int a3o_refine_corners_trace(const uint8_t *grey, uint32_t W, uint32_t H, const a3o_refine_config *cfg, float *xy, const float *cell_px, size_t n,
                             int variant, int32_t *win, uint32_t *iters, int32_t *how, float *excursion) {
    if (!cfg || cfg->win_half < 1 || cfg->win_half > 10 || !(cfg->relative_win >= 0.0f) || !(cfg->min_shift >= 0.0f)) return -1;
    if (variant < 0 || variant > 9) return -1;
    if (cfg->method == 0 || W == 0 || H == 0) return 0;
    const float eps2 = cfg->min_shift * cfg->min_shift;
    for (size_t k = 0; k < n; k++) {
        const int w = trace_window(cfg, cell_px, k, variant), side = 2 * w + 1, npx = side * side;
        const int wg = variant == 5 ? (w == 1 ? 2 : w - 1) : w;
        float g[64];   /* g[i + w]; past 2w for variant 4 alone */
        for (int t = 0; t < 64; t++) g[t] = (float)exp(-(double)((t - w) * (t - w)) / (double)(wg * wg));
        const float q0x = xy[2 * k], q0y = xy[2 * k + 1];
        const int fx0 = variant == 2 ? (int)q0x : (int)floorf(q0x), fy0 = variant == 2 ? (int)q0y : (int)floorf(q0y);
        trace_src s = {grey, (int)W, (int)H, variant, fx0 - 2 * w - 2, fx0 + 2 * w + 3, fy0 - 2 * w - 2, fy0 + 2 * w + 3};
        if (variant == 1) { s.hix--; s.hiy--; }
        if (variant == 9) { s.lox += 2; s.loy += 2; s.hix -= 2; s.hiy -= 2; }
        float cx = q0x, cy = q0y, far = 0.0f;
        uint32_t ran = 0;
        int end = A3O_EXIT_CAP;
        for (uint32_t it = 0; it < cfg->max_iterations; it++) {
            float lane[5][64];
            ran++;
            for (int l = 0; l < 64; l++) {
                float a = 0.0f, b = 0.0f, c2 = 0.0f, bb1 = 0.0f, bb2 = 0.0f;
                if (variant == 3 && l > 0) { lane[0][l] = lane[1][l] = lane[2][l] = lane[3][l] = lane[4][l] = 0.0f; continue; }
                for (int q = l, trip = 0; variant == 4 && trip == 0 ? q < 64 : q < npx; q += variant == 3 ? 1 : 64, trip++) {
                    const int i = q % side - w, j = q / side - w;
                    const float m = g[i + w] * g[j + w];
                    const float gx = trace_sample(&s, cx + (float)(i + 1), cy + (float)j) - trace_sample(&s, cx + (float)(i - 1), cy + (float)j);
                    const float gy = trace_sample(&s, cx + (float)i, cy + (float)(j + 1)) - trace_sample(&s, cx + (float)i, cy + (float)(j - 1));
                    const float fi = (float)i, fj = (float)j;
                    a += gx * gx * m;
                    b += gx * gy * m;
                    c2 += gy * gy * m;
                    bb1 += gx * gx * m * fi + gx * gy * m * fj;
                    bb2 += gx * gy * m * fi + gy * gy * m * fj;
                }
                lane[0][l] = a; lane[1][l] = b; lane[2][l] = c2; lane[3][l] = bb1; lane[4][l] = bb2;
            }
            for (int o = 32; o >= 1; o >>= 1)
                for (int v = 0; v < 5; v++) {
                    float nxt[64];
                    for (int l = 0; l < 64; l++) nxt[l] = lane[v][l] + lane[v][l ^ o];
                    memcpy(lane[v], nxt, sizeof nxt);
                }
            const float a = lane[0][0], b = lane[1][0], c2 = lane[2][0], bb1 = lane[3][0], bb2 = lane[4][0];
            const float det = a * c2 - b * b;
            if (det == 0.0f) { end = A3O_EXIT_DET0; break; }
            if (!isfinite(det)) { end = A3O_EXIT_NONFINITE; break; }
            const float sc = 1.0f / det;
            const float nx = cx + (c2 * sc * bb1 - b * sc * bb2), ny = cy + (-b * sc * bb1 + a * sc * bb2);
            const float rx = variant == 7 ? cx : q0x, ry = variant == 7 ? cy : q0y;
            if (!(fabsf(nx - rx) <= (float)w && fabsf(ny - ry) <= (float)w)) { cx = q0x; cy = q0y; end = A3O_EXIT_REVERT; break; }
            const float dx = nx - cx, dy = ny - cy;
            cx = nx; cy = ny;
            const float ex = fabsf(cx - q0x), ey = fabsf(cy - q0y), e = ex > ey ? ex : ey;
            if (e > far) far = e;
            if (dx * dx + dy * dy <= eps2) { end = A3O_EXIT_CONVERGED; break; }
        }
        xy[2 * k] = cx; xy[2 * k + 1] = cy;
        if (win) win[k] = w;
        if (iters) iters[k] = ran;
        if (how) how[k] = end;
        if (excursion) excursion[k] = far;
    }
    return 0;
}
