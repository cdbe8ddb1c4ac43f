/* tests/charuco_oracle.c -- CPU restatement of the ChArUco corners and their pose (include/aruco3_hip.h, a3_set_charuco; device:
 * aruco3_amd/csrc/k_charuco.hip), in the contract's order of operations.  Built with -ffp-contract=off like the kernels, together
 * with refine_oracle.c (the cornerSubPix iteration), lens_oracle.c (undistortion) and oracle/a3_oracle.c (from_control_points).
 * TEST INFRASTRUCTURE ONLY.
 *
 * The board pose's IPPE start, residual sums, 64-lane reduction and LM loop are board_oracle.c's, compiled beside this file and
 * reached through board_oracle.h. */
#include <math.h>
#include <stddef.h>
#include <stdlib.h>
#include <string.h>

#include "board_oracle.h"

int a3o_from_control_points(const float from[8], const float to[8], float transform[9], float inverse[9]);
void a3o_undistort(const float *xy, size_t n, const float *intr, const float *k, uint32_t iterations, float max_residual_px, float *out_xy,
                   float *residual_px);

typedef struct {   /* same layout as a3_refine_config */
    uint32_t method, win_half;
    float relative_win;
    uint32_t max_iterations;
    float min_shift;
} a3o_refine_cfg;
int a3o_refine_corners(const uint8_t *grey, uint32_t w, uint32_t h, const a3o_refine_cfg *cfg, float *corners_xy, const float *cell_px, size_t n);

typedef struct {   /* same layout as a3_charuco_config */
    uint32_t min_markers, refine, win_half;
    float relative_win;
    uint32_t max_iterations;
    float min_shift;
} a3o_charuco_cfg;
typedef struct {   /* same layout as a3_charuco_corner */
    uint32_t frame, id;
    float x, y, interp_x, interp_y;
    uint32_t markers_used, window;
} a3o_charuco_corner;
typedef struct {   /* same layout as a3_charuco_pose */
    uint32_t status, corners_used, iterations, reserved;
    float rms_px, alt_rms_px, rotation[9], translation[3];
} a3o_charuco_pose_rec;

#define A3O_NO_ADJ 0xFFFFFFFFu

static uint32_t board_slot_of(const uint32_t *board_ids, uint32_t n_board, uint32_t id) {
    for (uint32_t s = 0; s < n_board; s++)
        if (board_ids[s] == id) return s;
    return 0xFFFFu;
}

/* the window rule (refine_oracle.c's with cell_px = d) */
static uint32_t charuco_window(const a3o_charuco_cfg *cfg, float d) {
    const int wh = (int)cfg->win_half;
    if (!(cfg->relative_win > 0.0f)) return (uint32_t)wh;
    const float t = floorf(cfg->relative_win * d);
    const int v = t >= 2.0f ? (t >= (float)wh ? wh : (int)t) : 2;
    return (uint32_t)(v < wh ? v : wh);
}

/* The corners of one frame.  Board: n_board markers (ids, 8 corners each); chessboard: nc corners (xy, 4 adjacent ids each).  Frame:
 * cnt markers (ids, 8 float image corners each, batch order).  grey (W x H into_luma8) is sampled with cfg->refine.  -> the number of
 * records written to out (nc at most, id order, frame index `frame`). */
uint32_t a3o_charuco_corners(const uint32_t *board_ids, const float *board_xy, uint32_t n_board, const float *cxy, const uint32_t *adj, uint32_t nc,
                             const a3o_charuco_cfg *cfg, const uint32_t *ids, const float *px, uint32_t cnt, const uint8_t *grey, uint32_t W,
                             uint32_t H, uint32_t frame, a3o_charuco_corner *out) {
    static uint8_t seen[A3O_MAX_MARKERS], dup[A3O_MAX_MARKERS], ok[A3O_MAX_MARKERS];
    static uint32_t mi[A3O_MAX_MARKERS];
    static float hom[A3O_MAX_MARKERS][9];
    for (uint32_t s = 0; s < n_board; s++) { seen[s] = dup[s] = ok[s] = 0; }
    for (uint32_t i = 0; i < cnt; i++) {   /* 1. the duplicate rule */
        const uint32_t s = board_slot_of(board_ids, n_board, ids[i]);
        if (s == 0xFFFFu) continue;
        if (seen[s]) dup[s] = 1;
        seen[s] = 1;
    }
    for (uint32_t i = 0; i < cnt; i++) {   /* 2. one homography per used marker */
        const uint32_t s = board_slot_of(board_ids, n_board, ids[i]);
        if (s == 0xFFFFu || dup[s]) continue;
        float inv[9];
        if (a3o_from_control_points(board_xy + 8 * s, px + 8 * i, hom[s], inv)) { ok[s] = 1; mi[s] = i; }
    }
    uint32_t n = 0;
    for (uint32_t k = 0; k < nc; k++) {   /* 3. interpolation */
        const float X = cxy[2 * k], Y = cxy[2 * k + 1];
        float sx = 0.0f, sy = 0.0f;
        uint32_t used = 0, slots[4];
        for (int j = 0; j < 4; j++) {
            const uint32_t id = adj[4 * k + j];
            if (id == A3O_NO_ADJ) continue;
            const uint32_t s = board_slot_of(board_ids, n_board, id);
            if (s == 0xFFFFu || !ok[s]) continue;
            const float *h = hom[s];
            const float den = (h[6] * X + h[7] * Y) + 1.0f;
            sx = sx + ((h[0] * X + h[1] * Y) + h[2]) / den;
            sy = sy + ((h[3] * X + h[4] * Y) + h[5]) / den;
            slots[used++] = s;
        }
        if (used < cfg->min_markers) continue;
        const float ix = sx / (float)used, iy = sy / (float)used;
        if (!(ix >= 0.0f && ix <= (float)(W - 1) && iy >= 0.0f && iy <= (float)(H - 1))) continue;
        a3o_charuco_corner r = {frame, k, ix, iy, ix, iy, used, 0};
        if (cfg->refine) {   /* 4. refinement */
            float d = INFINITY;
            for (uint32_t j = 0; j < used; j++)
                for (int q = 0; q < 4; q++) {
                    const float *c = px + 8 * mi[slots[j]] + 2 * q;
                    const float dx = c[0] - ix, dy = c[1] - iy;
                    const float dist = sqrtf(dx * dx + dy * dy);
                    if (dist < d) d = dist;
                }
            r.window = charuco_window(cfg, d);
            const a3o_refine_cfg rc = {1, cfg->win_half, cfg->relative_win, cfg->max_iterations, cfg->min_shift};
            float xy[2] = {ix, iy};
            a3o_refine_corners(grey, W, H, &rc, xy, &d, 1);
            r.x = xy[0]; r.y = xy[1];
        }
        out[n++] = r;
    }
    return n;
}

/* the frame's records as correspondences: lanes l of 64 sum the records l, l + 64, ..., then the xor butterfly */
typedef struct {
    const frame_t *F;
    const float *bxy, *mxy;
    uint32_t n;
} records_t;

static void charuco_evaluate(const void *ctx, const float R[9], const float t[3], acc_t *out) {
    const records_t *g = (const records_t *)ctx;
    acc_t lane[64];
    memset(lane, 0, sizeof lane);
    for (uint32_t c = 0; c < g->n; c++)
        a3o_accum(&lane[c & 63], R, t, g->bxy[2 * c], g->bxy[2 * c + 1], g->mxy[2 * c], g->mxy[2 * c + 1], g->F->sx, g->F->sy);
    a3o_reduce64(lane, out);
}

/* The ChArUco pose of one frame: cnt markers (ids; px: the corners the board pose reads -- undistorted with a distortion set), the
 * frame's n records (rec), intr (fx fy cx cy, or NULL: normalise by w, h), dist (k1..k6 + iterations as float + max residual, or NULL) */
int a3o_charuco_pose(const uint32_t *board_ids, const float *board_xy, uint32_t n_board, const float *cxy, const uint32_t *ids, const float *px,
                     uint32_t cnt, const a3o_charuco_corner *rec, uint32_t n, const float *intr, const float *dist, uint32_t w, uint32_t h,
                     a3o_charuco_pose_rec *out) {
    a3o_board_rec br;
    float starts[24];
    memset(out, 0, sizeof *out);
    out->corners_used = n;
    if (a3o_board_pose(board_ids, board_xy, n_board, ids, px, cnt, intr, w, h, &br, starts) != 0) return -1;
    if (br.status == 0 || n < 4) return 0;
    static a3o_slot slots[A3O_MAX_MARKERS];
    static uint8_t nodup[A3O_MAX_MARKERS];
    for (uint32_t s = 0; s < n_board; s++) { a3o_slot_from(board_xy + 8 * s, &slots[s]); nodup[s] = 0; }
    frame_t F = {ids, px, cnt, board_ids, slots, n_board, nodup, intr != NULL, (float)w, (float)h, 0, 0, 0, 0, 0, 0};
    if (intr) { F.fx = intr[0]; F.fy = intr[1]; F.cx = intr[2]; F.cy = intr[3]; }
    F.sx = intr ? F.fx : F.iw; F.sy = intr ? F.fy : F.ih;
    float *bxy = malloc(sizeof(float) * 2 * n), *mxy = malloc(sizeof(float) * 2 * n);
    for (uint32_t c = 0; c < n; c++) {
        float xy[2] = {rec[c].x, rec[c].y};
        if (dist) {
            float u[2], res;
            a3o_undistort(xy, 1, intr, dist, (uint32_t)dist[8], dist[9], u, &res);
            xy[0] = u[0]; xy[1] = u[1];
        }
        bxy[2 * c] = cxy[2 * rec[c].id]; bxy[2 * c + 1] = cxy[2 * rec[c].id + 1];
        a3o_normalise(&F, xy[0], xy[1], &mxy[2 * c], &mxy[2 * c + 1]);
    }
    const records_t g = {&F, bxy, mxy, n};
    float R[2][9], t[2][3], cost[2], pix[2];
    uint32_t ev[2];
    for (int st = 0; st < 2; st++) {
        memcpy(R[st], starts + 12 * st, 36); memcpy(t[st], starts + 12 * st + 9, 12);
        ev[st] = a3o_lm(charuco_evaluate, &g, R[st], t[st], &cost[st], &pix[st]);
    }
    free(bxy); free(mxy);
    const int keep = cost[1] < cost[0] ? 1 : 0;
    const float nf = (float)n;
    out->status = 1u;
    out->iterations = ev[keep];
    out->rms_px = sqrtf(pix[keep] / nf);
    out->alt_rms_px = sqrtf(pix[1 - keep] / nf);
    memcpy(out->rotation, R[keep], 36);
    memcpy(out->translation, t[keep], 12);
    return 0;
}
