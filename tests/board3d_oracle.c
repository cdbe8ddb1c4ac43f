/* tests/board3d_oracle.c -- CPU restatement of the 3-D board pose (include/aruco3_hip.h, a3_set_board3d; device: k_board3d_pose in
 * aruco3_amd/csrc/k_board3d.hip), in the contract's order of operations.  Linked with tests/board_oracle.c, whose IPPE (a3o_ippe), LM
 * loop with its LDL^T and Cayley update (a3o_lm), normalisation (a3o_normalise) and 64-lane butterfly (a3o_reduce64) are the planar
 * contract's and are used as they stand; what the 3-D contract states anew is restated here: the slot record, the start carried
 * through the marker's frame, and the sums with q = R (X, Y, Z).  Built with -ffp-contract=off like the kernels.
 * TEST INFRASTRUCTURE ONLY. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "board_oracle.h"

void a3o_ippe(const float pts[8], float marker_size, a3o_pose out[2]);

typedef struct a3o_slot3 { float x[4], y[4], z[4], side, ex[3], ey[3], ez[3], c[3]; } a3o_slot3;   /* 25 floats */

typedef struct {
    const uint32_t* ids; const float* px; uint32_t cnt;   /* the frame's markers, batch order; pixel corners */
    const uint32_t* board_ids; const a3o_slot3* slots; uint32_t n_slots;
    const uint8_t* dup;
    frame_t norm;   /* the normalisation (has_intr, iw, ih, fx, fy, cx, cy, sx, sy) as a3o_normalise reads it */
} frame3_t;

/* the contract's slot data, float */
void a3o_board3d_slot(const float xyz[12], a3o_slot3* s) {
    for (int k = 0; k < 4; k++) { s->x[k] = xyz[3 * k]; s->y[k] = xyz[3 * k + 1]; s->z[k] = xyz[3 * k + 2]; }
    const float d[3] = {s->x[1] - s->x[0], s->y[1] - s->y[0], s->z[1] - s->z[0]};
    s->side = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    for (int j = 0; j < 3; j++) s->ex[j] = d[j] / s->side;
    const float v[3] = {s->x[0] - s->x[3], s->y[0] - s->y[3], s->z[0] - s->z[3]};
    const float k = (v[0] * s->ex[0] + v[1] * s->ex[1]) + v[2] * s->ex[2];
    float w[3];
    for (int j = 0; j < 3; j++) w[j] = v[j] - k * s->ex[j];
    const float wn = sqrtf((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    for (int j = 0; j < 3; j++) s->ey[j] = w[j] / wn;
    s->ez[0] = s->ex[1] * s->ey[2] - s->ex[2] * s->ey[1];
    s->ez[1] = s->ex[2] * s->ey[0] - s->ex[0] * s->ey[2];
    s->ez[2] = s->ex[0] * s->ey[1] - s->ex[1] * s->ey[0];
    s->c[0] = 0.25f * ((s->x[0] + s->x[1]) + (s->x[2] + s->x[3]));
    s->c[1] = 0.25f * ((s->y[0] + s->y[1]) + (s->y[2] + s->y[3]));
    s->c[2] = 0.25f * ((s->z[0] + s->z[1]) + (s->z[2] + s->z[3]));
}

static uint32_t slot_of(const frame3_t* F, uint32_t id) {
    for (uint32_t s = 0; s < F->n_slots; s++)
        if (F->board_ids[s] == id) return s;
    return 0xFFFFu;
}

static int corner(const frame3_t* F, uint32_t c, float b[3], float* mx, float* my) {
    const uint32_t m = c >> 2; const int k = (int)(c & 3u);
    const uint32_t slot = slot_of(F, F->ids[m]);
    if (slot == 0xFFFFu || F->dup[slot]) return 0;
    b[0] = F->slots[slot].x[k]; b[1] = F->slots[slot].y[k]; b[2] = F->slots[slot].z[k];
    a3o_normalise(&F->norm, F->px[8 * m + 2 * k], F->px[8 * m + 2 * k + 1], mx, my);
    return 1;
}

static void accum3(acc_t* s, const float R[9], const float t[3], const float b[3], float mx, float my, float sx, float sy) {
    const float qx = (R[0] * b[0] + R[1] * b[1]) + R[2] * b[2], qy = (R[3] * b[0] + R[4] * b[1]) + R[5] * b[2], qz = (R[6] * b[0] + R[7] * b[1]) + R[8] * b[2];
    const float px = qx + t[0], py = qy + t[1], pz = qz + t[2];
    const float zz = pz > 1e-5f ? pz : 1e-5f;
    const float u = px / zz, v = py / zz;
    const float a = 1.0f / zz, a2 = 2.0f * a;
    const float ru = u - mx, rv = v - my;
    const float ju[6] = {-(a2 * u) * qy, a2 * (qz + u * qx), -a2 * qy, a, 0.0f, -(a * u)};
    const float jv[6] = {-a2 * (qz + v * qy), (a2 * v) * qx, a2 * qx, 0.0f, a, -(a * v)};
    int idx = 0;
    for (int r = 0; r < 6; r++) {
        for (int c = r; c < 6; c++) { s->h[idx] += ju[r] * ju[c] + jv[r] * jv[c]; idx++; }
        s->g[r] += ju[r] * ru + jv[r] * rv;
    }
    s->cost += ru * ru + rv * rv;
    const float eu = ru * sx, ev = rv * sy;
    s->pix += eu * eu + ev * ev;
}

/* 64 lanes, corners l, l + 64, ... in order, then the butterfly */
static void evaluate(const void* ctx, const float R[9], const float t[3], acc_t* out) {
    const frame3_t* F = (const frame3_t*)ctx;
    acc_t lanes[64];
    memset(lanes, 0, sizeof lanes);
    for (int l = 0; l < 64; l++)
        for (uint32_t c = (uint32_t)l; c < 4 * F->cnt; c += 64) {
            float b[3], mx, my;
            if (corner(F, c, b, &mx, &my)) accum3(&lanes[l], R, t, b, mx, my, F->norm.sx, F->norm.sy);
        }
    a3o_reduce64(lanes, out);
}

static int pose_finite(const a3o_pose* p) {
    for (int q = 0; q < 9; q++)
        if (!isfinite(p->rotation[q])) return 0;
    for (int q = 0; q < 3; q++)
        if (!isfinite(p->translation[q])) return 0;
    return 1;
}

static a3o_slot3 g_slots[A3O_MAX_MARKERS];
static uint8_t g_seen[A3O_MAX_MARKERS], g_dup[A3O_MAX_MARKERS];

static void frame_init(frame3_t* F, const uint32_t* board_ids, const float* board_xyz, uint32_t n_board, const uint32_t* ids, const float* px,
                       uint32_t cnt, const float* intr, uint32_t w, uint32_t h) {
    for (uint32_t s = 0; s < n_board; s++) { a3o_board3d_slot(board_xyz + 12 * s, &g_slots[s]); g_seen[s] = g_dup[s] = 0; }
    memset(F, 0, sizeof *F);
    F->ids = ids; F->px = px; F->cnt = cnt; F->board_ids = board_ids; F->slots = g_slots; F->n_slots = n_board; F->dup = g_dup;
    F->norm.has_intr = intr != NULL; F->norm.iw = (float)w; F->norm.ih = (float)h;
    if (intr) { F->norm.fx = intr[0]; F->norm.fy = intr[1]; F->norm.cx = intr[2]; F->norm.cy = intr[3]; }
    F->norm.sx = intr ? F->norm.fx : F->norm.iw; F->norm.sy = intr ? F->norm.fy : F->norm.ih;
}

/* LM from a caller-given start (board frame) -> evaluations; cost_pix2: the final normalised and pixel costs */
uint32_t a3o_board3d_refine_from(const uint32_t* board_ids, const float* board_xyz, uint32_t n_board, const uint32_t* ids, const float* px,
                                 uint32_t cnt, const float* intr /* fx, fy, cx, cy or NULL */, uint32_t w, uint32_t h, float R[9], float t[3],
                                 float* cost_pix2) {
    frame3_t F;
    if (n_board > A3O_MAX_MARKERS) return 0;
    frame_init(&F, board_ids, board_xyz, n_board, ids, px, cnt, intr, w, h);
    return a3o_lm(evaluate, &F, R, t, &cost_pix2[0], &cost_pix2[1]);
}

/* the sums of one state (cost, pixel cost) with no LM step: what the first evaluation of a start sees */
void a3o_board3d_cost_at(const uint32_t* board_ids, const float* board_xyz, uint32_t n_board, const uint32_t* ids, const float* px, uint32_t cnt,
                         const float* intr, uint32_t w, uint32_t h, const float R[9], const float t[3], float* cost_pix2) {
    frame3_t F;
    acc_t s;
    frame_init(&F, board_ids, board_xyz, n_board, ids, px, cnt, intr, w, h);
    evaluate(&F, R, t, &s);
    cost_pix2[0] = s.cost; cost_pix2[1] = s.pix;
}

/* the board pose of one frame: cnt markers (ids, 8 pixel corners each, batch order); start_out (nullable, 2 x 12 floats): both
 * starts (R row-major, t) in the board frame, before refinement */
int a3o_board3d_pose(const uint32_t* board_ids, const float* board_xyz, uint32_t n_board, const uint32_t* ids, const float* px, uint32_t cnt,
                     const float* intr /* fx, fy, cx, cy or NULL */, uint32_t w, uint32_t h, a3o_board_rec* out, float* start_out) {
    frame3_t F;
    if (n_board > A3O_MAX_MARKERS) return -1;
    frame_init(&F, board_ids, board_xyz, n_board, ids, px, cnt, intr, w, h);
    for (uint32_t i = 0; i < cnt; i++) {
        const uint32_t s = slot_of(&F, ids[i]);
        if (s == 0xFFFFu) continue;
        if (g_seen[s]) g_dup[s] = 1;
        g_seen[s] = 1;
    }
    memset(out, 0, sizeof *out);
    uint32_t used = 0, rejected = 0, best_i = 0, best_slot = 0;
    float best_area = -1.0f;
    for (uint32_t i = 0; i < cnt; i++) {
        const uint32_t slot = slot_of(&F, ids[i]);
        if (slot == 0xFFFFu) continue;
        if (g_dup[slot]) { rejected++; continue; }
        used++;
        const float* x = px + 8 * i;
        float s = 0.0f;
        for (int k = 0; k < 4; k++) { const int k1 = (k + 1) & 3; s = s + (x[2 * k] * x[2 * k1 + 1] - x[2 * k1] * x[2 * k + 1]); }
        const float area = 0.5f * fabsf(s);
        if (area > best_area || (area == best_area && slot < best_slot)) {
            float q[8];
            a3o_pose p2[2];
            for (int k = 0; k < 4; k++) a3o_normalise(&F.norm, x[2 * k], x[2 * k + 1], &q[2 * k], &q[2 * k + 1]);
            a3o_ippe(q, g_slots[slot].side, p2);
            if (pose_finite(&p2[0]) && pose_finite(&p2[1])) { best_area = area; best_i = i; best_slot = slot; }
        }
    }
    out->markers_used = used;
    out->markers_rejected = rejected;
    if (!used || best_area < 0.0f) return 0;   /* no used marker, or none with finite IPPE poses: A3_BOARD_NONE */
    out->status = 1u;
    const a3o_slot3* bs = &g_slots[best_slot];
    float pts[8];
    for (int k = 0; k < 4; k++) a3o_normalise(&F.norm, px[8 * best_i + 2 * k], px[8 * best_i + 2 * k + 1], &pts[2 * k], &pts[2 * k + 1]);
    a3o_pose p[2];
    a3o_ippe(pts, bs->side, p);
    float R[2][9], t[2][3], cost[2], pix[2];
    uint32_t ev[2];
    for (int st = 0; st < 2; st++) {
        const float* Rm = p[st].rotation;
        for (int r = 0; r < 3; r++)
            for (int j = 0; j < 3; j++) R[st][3 * r + j] = (Rm[3 * r] * bs->ex[j] + Rm[3 * r + 1] * bs->ey[j]) + Rm[3 * r + 2] * bs->ez[j];
        for (int r = 0; r < 3; r++)
            t[st][r] = p[st].translation[r] - ((R[st][3 * r] * bs->c[0] + R[st][3 * r + 1] * bs->c[1]) + R[st][3 * r + 2] * bs->c[2]);
        if (start_out) { memcpy(start_out + 12 * st, R[st], 36); memcpy(start_out + 12 * st + 9, t[st], 12); }
        ev[st] = a3o_lm(evaluate, &F, R[st], t[st], &cost[st], &pix[st]);
    }
    const int keep = cost[1] < cost[0] ? 1 : 0;
    const float nc = (float)(4u * used);
    out->iterations = ev[keep];
    out->rms_px = sqrtf(pix[keep] / nc);
    out->alt_rms_px = sqrtf(pix[1 - keep] / nc);
    memcpy(out->rotation, R[keep], 36);
    memcpy(out->translation, t[keep], 12);
    return 0;
}
