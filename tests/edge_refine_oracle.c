/*
 * edge_refine_oracle.c -- CPU restatement of edge-fit corner refinement (include/aruco3_hip.h, a3_refine_config.method
 * A3_REFINE_EDGES).
 *
 * TEST INFRASTRUCTURE ONLY (tests/edge_refine_oracle.py compiles it into a temporary directory and loads it through ctypes).  The
 * reference has no corner refinement: this is the contract of an extension, restated here so that the device kernel
 * (aruco3_amd/csrc/k_edge_refine.hip, k_refine_edges) can be held to it bit for bit.  Compiled with -ffp-contract=off: no fused
 * multiply-add, as in the kernel.  The summation order is the kernel's: a station's sums run over ascending offsets, a side's five
 * sums are an xor butterfly 8, 4, 2, 1 over its 16 stations.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define LIVE_LEVEL 20.0f   /* A3_REFINE_EDGES_LIVE_LEVEL */

/* same layout as a3_refine_config */
typedef struct {
    uint32_t method;          /* 2 edges (0: nothing is done) */
    uint32_t win_half;        /* 1..10: the search range r */
    float    relative_win;
    uint32_t max_iterations;
    float    min_shift;
} a3o_refine_config;

/* refines n_quads quads (8 floats each: x, y of four corners in a3_marker order, in place) of one grey frame; cell_px (nullable):
 * one value per quad; -> 0, or -1 on a bad config */
int a3o_refine_quads(const uint8_t *grey, uint32_t w, uint32_t h, const a3o_refine_config *cfg, float *quads_xy, const float *cell_px,
                     size_t n_quads);

static int search_range(const a3o_refine_config *cfg, const float *cell_px, size_t k) {
    const int wh = (int)cfg->win_half;
    if (!(cfg->relative_win > 0.0f) || !cell_px) return wh;
    const float t = floorf(cfg->relative_win * cell_px[k]);
    const int v = t >= 2.0f ? (t >= (float)wh ? wh : (int)t) : 2;
    return v < wh ? v : wh;
}

/* bilinear grey level at (x, y), border replicate; the order of operations is the contract's */
static float sample(const uint8_t *g, int W, int H, float x, float y) {
    const float x0f = floorf(x), y0f = floorf(y);
    const float fx = x - x0f, fy = y - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const int xa = x0 < 0 ? 0 : (x0 > W - 1 ? W - 1 : x0), xb = x0 + 1 < 0 ? 0 : (x0 + 1 > W - 1 ? W - 1 : x0 + 1);
    const int ya = y0 < 0 ? 0 : (y0 > H - 1 ? H - 1 : y0), yb = y0 + 1 < 0 ? 0 : (y0 + 1 > H - 1 ? H - 1 : y0 + 1);
    const float i00 = g[(size_t)ya * W + xa], i01 = g[(size_t)ya * W + xb], i10 = g[(size_t)yb * W + xa], i11 = g[(size_t)yb * W + xb];
    return (1.0f - fy) * ((1.0f - fx) * i00 + fx * i01) + fy * ((1.0f - fx) * i10 + fx * i11);
}

static float butterfly16(const float *v) {
    float cur[16], nxt[16];
    memcpy(cur, v, sizeof cur);
    for (int o = 8; o >= 1; o >>= 1) {
        for (int l = 0; l < 16; l++) nxt[l] = cur[l] + cur[l ^ o];
        memcpy(cur, nxt, sizeof cur);
    }
    return cur[0];
}

/* one pass from corners c (8 floats) -> new corners nc; 0, or 1 when the marker reverts (all but the 2r rule) */
static int pass(const uint8_t *grey, int W, int H, int r, const float *c, float *nc) {
    float Ox[4], Oy[4], Dx[4], Dy[4];
    for (int e = 0; e < 4; e++) {   /* (the kernel looks at every side's length before it samples any) */
        const int e2 = (e + 1) & 3;
        const float dx = c[2 * e2] - c[2 * e], dy = c[2 * e2 + 1] - c[2 * e + 1];
        if (!(sqrtf(dx * dx + dy * dy) >= 4.0f)) return 1;
    }
    for (int e = 0; e < 4; e++) {
        const int e2 = (e + 1) & 3;
        const float ax = c[2 * e], ay = c[2 * e + 1];
        const float dx = c[2 * e2] - ax, dy = c[2 * e2 + 1] - ay;
        const float L = sqrtf(dx * dx + dy * dy);
        const float Nx = dy / L, Ny = -(dx / L);
        float one[16], ss[16], sss[16], sm[16], ssm[16];
        for (int k = 0; k < 16; k++) {
            const float s = 0.125f + 0.75f * (((float)k + 0.5f) / 16.0f);
            const float px = ax + s * dx, py = ay + s * dy;
            float S[45], gmax = 0.0f, sw = 0.0f, swo = 0.0f;
            for (int i = -2 * r - 2; i <= 2 * r + 2; i++) {
                const float o = (float)i * 0.5f;
                S[i + 2 * r + 2] = sample(grey, W, H, px + o * Nx, py + o * Ny);
            }
            for (int j = -2 * r; j <= 2 * r; j++) {
                const float gj = S[j + 2 + 2 * r + 2] - S[j - 2 + 2 * r + 2], oj = (float)j * 0.5f;
                const float wj = gj > 0.0f ? gj * gj : 0.0f;
                gmax = gj > gmax ? gj : gmax;
                sw += wj;
                swo += wj * oj;
            }
            const int live = gmax >= LIVE_LEVEL;
            const float m = live ? swo / sw : 0.0f, sl = live ? s : 0.0f;
            one[k] = live ? 1.0f : 0.0f; ss[k] = sl; sss[k] = sl * sl; sm[k] = m; ssm[k] = sl * m;
        }
        const float fn = butterfly16(one), Ss = butterfly16(ss), Sss = butterfly16(sss), Sm = butterfly16(sm), Ssm = butterfly16(ssm);
        const float det = fn * Sss - Ss * Ss;
        if (!(fn >= 12.0f) || det == 0.0f || !isfinite(det)) return 1;
        const float alpha = (Sm * Sss - Ss * Ssm) / det, beta = (fn * Ssm - Ss * Sm) / det;
        Ox[e] = ax + alpha * Nx; Oy[e] = ay + alpha * Ny; Dx[e] = dx + beta * Nx; Dy[e] = dy + beta * Ny;
    }
    for (int e = 0; e < 4; e++) {
        const int p = (e + 3) & 3;
        const float wx = Ox[e] - Ox[p], wy = Oy[e] - Oy[p], dd = Dx[p] * Dy[e] - Dy[p] * Dx[e];
        const float v = (wx * Dy[p] - wy * Dx[p]) / dd;
        nc[2 * e] = Ox[e] + v * Dx[e]; nc[2 * e + 1] = Oy[e] + v * Dy[e];
        if (dd == 0.0f) return 1;
    }
    return 0;
}

int a3o_refine_quads(const uint8_t *grey, uint32_t W, uint32_t H, const a3o_refine_config *cfg, float *xy, const float *cell_px, size_t n) {
    if (!cfg || cfg->win_half < 1 || cfg->win_half > 10 || !(cfg->relative_win >= 0.0f) || !(cfg->min_shift >= 0.0f) || cfg->max_iterations > 100)
        return -1;
    if (cfg->method == 0 || W == 0 || H == 0) return 0;
    for (size_t u = 0; u < n; u++) {
        const int r = search_range(cfg, cell_px, u);
        const float reach = (float)(2 * r), ms = cfg->min_shift;
        float q[8], c[8], nc[8];
        int revert = 0;
        memcpy(q, xy + 8 * u, sizeof q);
        memcpy(c, q, sizeof c);
        for (uint32_t it = 0; it < cfg->max_iterations && !revert; it++) {
            int moved = 0;
            if (pass(grey, (int)W, (int)H, r, c, nc)) { revert = 1; break; }
            for (int k = 0; k < 8; k++) {
                if (!(fabsf(nc[k] - q[k]) <= reach)) revert = 1;
                if (fabsf(nc[k] - c[k]) > ms) moved = 1;
            }
            if (revert) break;
            memcpy(c, nc, sizeof c);
            if (!moved) break;
        }
        memcpy(xy + 8 * u, revert ? q : c, sizeof q);
    }
    return 0;
}
