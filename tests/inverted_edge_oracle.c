/*
 * inverted_edge_oracle.c -- CPU restatement of edge-fit corner refinement (include/aruco3_hip.h, method A3_REFINE_EDGES) with a
 * polarity per quad: the rule a batch in mode A3_POLARITY_BOTH applies to a marker flagged A3_MARKER_INVERTED.
 *
 * TEST INFRASTRUCTURE ONLY (tests/inverted_edge_oracle.py compiles it into a temporary directory and loads it through ctypes).  Every
 * line of the contract is restated here from the header; the one difference between the polarities is the sign of g_j:
 *   polarity 0 (dark inside):   g_j = S_(j+2) - S_(j-2)
 *   polarity 1 (bright inside): g_j = S_(j-2) - S_(j+2)
 * With polarity 0 throughout it must equal tests/edge_refine_oracle.c bit for bit (tests/test_inverted_edge_oracle.py holds it to
 * that).  Compiled with -ffp-contract=off, summation orders as the kernel's.
 */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#define LIVE_LEVEL 20.0f   /* A3_REFINE_EDGES_LIVE_LEVEL */
#define MIN_SIDE 4.0f
#define MIN_LIVE 12.0f

typedef struct {   /* a3_refine_config */
    uint32_t method, win_half;
    float    relative_win;
    uint32_t max_iterations;
    float    min_shift;
} a3i_refine_config;

/* n_quads quads (8 floats each, a3_marker order, refined in place) of one grey frame; cell_px (nullable): one per quad; polarity
 * (nullable: all 0): one word per quad, bit 0 = bright inside; -> 0, or -1 on a bad config */
int a3i_refine_quads(const uint8_t *grey, uint32_t w, uint32_t h, const a3i_refine_config *cfg, float *quads_xy, const float *cell_px,
                     const uint32_t *polarity, size_t n_quads);

static int clampi(int v, int hi) { return v < 0 ? 0 : (v > hi ? hi : v); }

static float bilinear(const uint8_t *g, int W, int H, float x, float y) {
    const float xf = floorf(x), yf = floorf(y);
    const float fx = x - xf, fy = y - yf;
    const int x0 = (int)xf, y0 = (int)yf;
    const int xa = clampi(x0, W - 1), xb = clampi(x0 + 1, W - 1), ya = clampi(y0, H - 1), yb = clampi(y0 + 1, H - 1);
    const float i00 = g[(size_t)ya * W + xa], i01 = g[(size_t)ya * W + xb], i10 = g[(size_t)yb * W + xa], i11 = g[(size_t)yb * W + xb];
    return (1.0f - fy) * ((1.0f - fx) * i00 + fx * i01) + fy * ((1.0f - fx) * i10 + fx * i11);
}

static float xor_sum16(const float *v) {
    float a[16], b[16];
    memcpy(a, v, sizeof a);
    for (int o = 8; o >= 1; o >>= 1) {
        for (int l = 0; l < 16; l++) b[l] = a[l] + a[l ^ o];
        memcpy(a, b, sizeof a);
    }
    return a[0];
}

typedef struct { float ox, oy, dx, dy; } line_t;

/* the line of side a -> b; 1: the marker reverts */
static int fit_side(const uint8_t *g, int W, int H, int r, int bright, float ax, float ay, float bx, float by, line_t *out) {
    const float dx = bx - ax, dy = by - ay;
    const float L = sqrtf(dx * dx + dy * dy);
    const float Nx = dy / L, Ny = -(dx / L);
    float one[16], vs[16], vss[16], vm[16], vsm[16];
    for (int k = 0; k < 16; k++) {
        const float s = 0.125f + 0.75f * (((float)k + 0.5f) / 16.0f);
        const float px = ax + s * dx, py = ay + s * dy;
        float S[45];
        for (int i = -2 * r - 2; i <= 2 * r + 2; i++) {
            const float o = (float)i * 0.5f;
            S[i + 2 * r + 2] = bilinear(g, W, H, px + o * Nx, py + o * Ny);
        }
        float gmax = 0.0f, sw = 0.0f, swo = 0.0f;
        for (int j = -2 * r; j <= 2 * r; j++) {
            const float outer = S[j + 2 + 2 * r + 2], inner = S[j - 2 + 2 * r + 2];
            const float gj = bright ? inner - outer : outer - inner;
            const float oj = (float)j * 0.5f;
            const float wj = gj > 0.0f ? gj * gj : 0.0f;
            if (gj > gmax) gmax = gj;
            sw += wj;
            swo += wj * oj;
        }
        const int live = gmax >= LIVE_LEVEL;
        const float m = live ? swo / sw : 0.0f, sl = live ? s : 0.0f;
        one[k] = live ? 1.0f : 0.0f; vs[k] = sl; vss[k] = sl * sl; vm[k] = m; vsm[k] = sl * m;
    }
    const float n = xor_sum16(one), Ss = xor_sum16(vs), Sss = xor_sum16(vss), Sm = xor_sum16(vm), Ssm = xor_sum16(vsm);
    const float det = n * Sss - Ss * Ss;
    if (!(n >= MIN_LIVE) || det == 0.0f || !isfinite(det)) return 1;
    const float alpha = (Sm * Sss - Ss * Ssm) / det, beta = (n * Ssm - Ss * Sm) / det;
    out->ox = ax + alpha * Nx; out->oy = ay + alpha * Ny; out->dx = dx + beta * Nx; out->dy = dy + beta * Ny;
    return 0;
}

/* one pass c -> nc; 1: the marker reverts (every case but the 2r rule) */
static int one_pass(const uint8_t *g, int W, int H, int r, int bright, const float *c, float *nc) {
    line_t ln[4];
    for (int e = 0; e < 4; e++) {   /* every side's length is looked at before any side is sampled */
        const int f = (e + 1) & 3;
        const float dx = c[2 * f] - c[2 * e], dy = c[2 * f + 1] - c[2 * e + 1];
        if (!(sqrtf(dx * dx + dy * dy) >= MIN_SIDE)) return 1;
    }
    for (int e = 0; e < 4; e++) {
        const int f = (e + 1) & 3;
        if (fit_side(g, W, H, r, bright, c[2 * e], c[2 * e + 1], c[2 * f], c[2 * f + 1], &ln[e])) return 1;
    }
    for (int e = 0; e < 4; e++) {
        const line_t *p = &ln[(e + 3) & 3], *q = &ln[e];
        const float wx = q->ox - p->ox, wy = q->oy - p->oy, dd = p->dx * q->dy - p->dy * q->dx;
        const float v = (wx * p->dy - wy * p->dx) / dd;
        nc[2 * e] = q->ox + v * q->dx; nc[2 * e + 1] = q->oy + v * q->dy;
        if (dd == 0.0f) return 1;
    }
    return 0;
}

static int range_of(const a3i_refine_config *cfg, const float *cell_px, size_t u) {
    const int wh = (int)cfg->win_half;
    if (!(cfg->relative_win > 0.0f) || !cell_px) return wh;
    const float t = floorf(cfg->relative_win * cell_px[u]);
    const int v = t >= 2.0f ? (t >= (float)wh ? wh : (int)t) : 2;
    return v < wh ? v : wh;
}

int a3i_refine_quads(const uint8_t *grey, uint32_t W, uint32_t H, const a3i_refine_config *cfg, float *xy, const float *cell_px,
                     const uint32_t *polarity, size_t n) {
    if (!cfg || cfg->win_half < 1 || cfg->win_half > 10 || !(cfg->relative_win >= 0.0f) || !(cfg->min_shift >= 0.0f) || cfg->max_iterations > 100)
        return -1;
    if (cfg->method == 0 || W == 0 || H == 0) return 0;
    for (size_t u = 0; u < n; u++) {
        const int r = range_of(cfg, cell_px, u), bright = polarity ? (int)(polarity[u] & 1u) : 0;
        const float reach = (float)(2 * r);
        float start[8], c[8], nc[8];
        int revert = 0;
        memcpy(start, xy + 8 * u, sizeof start);
        memcpy(c, start, sizeof c);
        for (uint32_t it = 0; it < cfg->max_iterations; it++) {
            if (one_pass(grey, (int)W, (int)H, r, bright, c, nc)) { revert = 1; break; }
            int moved = 0;
            for (int k = 0; k < 8; k++) {
                if (!(fabsf(nc[k] - start[k]) <= reach)) revert = 1;
                if (fabsf(nc[k] - c[k]) > cfg->min_shift) moved = 1;
            }
            if (revert) break;
            memcpy(c, nc, sizeof c);
            if (!moved) break;
        }
        memcpy(xy + 8 * u, revert ? start : c, sizeof start);
    }
    return 0;
}
