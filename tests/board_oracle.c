/* tests/board_oracle.c -- CPU restatement of the board pose (include/aruco3_hip.h, a3_set_board; device: k_board_pose in
 * aruco3_amd/csrc/k_board.hip), in the contract's order of operations: 64 "lanes" each summing the corners l, l + 64, ..., then the
 * xor butterfly.  Built with -ffp-contract=off like the kernels.  TEST INFRASTRUCTURE ONLY.
 *
 * The IPPE start below is a host copy of aruco3_amd/csrc/a3_ippe.h (solve_normalized and its helpers), operation for operation. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <string.h>

#include "board_oracle.h"

/* ---------------- IPPE (host copy of a3_ippe.h) ---------------- */
static void find_rotation_to_z(const float v[3], float rot[9]) {  // src/pose.rs:238-267
    for (int i = 0; i < 9; i++) rot[i] = 0.0f;
    const float a = v[0] * v[0], b = v[1] * v[1], c = v[2] * v[2];
    const float nrm = sqrtf(a + b + c);
    const float ax = v[0] / nrm, ay = v[1] / nrm, az = v[2] / nrm;
    if (fabsf(1.0f + az) < 1e-6f) {
        rot[0] = 1.0f; rot[4] = 1.0f; rot[8] = -1.0f;
    } else {
        const float d = 1.0f / (1.0f + az);
        const float ax2 = ax * ax, ay2 = ay * ay, axay = ax * ay;
        rot[0] = -ax2 * d + 1.0f; rot[1] = -axay * d;       rot[2] = -ax;
        rot[3] = -axay * d;       rot[4] = -ay2 * d + 1.0f; rot[5] = -ay;
        rot[6] = ax;              rot[7] = ay;              rot[8] = 1.0f - (ax2 + ay2) * d;
    }
}

static void compute_rotations(const float j[4], float tx, float ty, float r1[9], float r2[9]) {  // src/pose.rs:158-235
    const float t[3] = {tx, ty, 1.0f};
    float rz[9], rv[9];
    find_rotation_to_z(t, rz);
    for (int r = 0; r < 3; r++) for (int c = 0; c < 3; c++) rv[r * 3 + c] = rz[c * 3 + r];
#define RV(r, c) rv[((r) - 1) * 3 + ((c) - 1)]
    const float b00 = RV(1, 1) - tx * RV(3, 1);
    const float b01 = RV(1, 2) - tx * RV(3, 2);
    const float b10 = RV(2, 1) - ty * RV(3, 1);
    const float b11 = RV(2, 2) - ty * RV(3, 2);
    const float inv_det = 1.0f / (b00 * b11 - b01 * b10);
    const float binv00 = inv_det * b11, binv01 = -inv_det * b01, binv10 = -inv_det * b10, binv11 = inv_det * b00;
    const float a00 = binv00 * j[0] + binv01 * j[2];
    const float a01 = binv00 * j[1] + binv01 * j[3];
    const float a10 = binv10 * j[0] + binv11 * j[2];
    const float a11 = binv10 * j[1] + binv11 * j[3];
    const float ata00 = a00 * a00 + a01 * a01;
    const float ata01 = a00 * a10 + a01 * a11;
    const float ata11 = a10 * a10 + a11 * a11;
    const float gamma = sqrtf(0.5f * (ata00 + ata11 + sqrtf((ata00 - ata11) * (ata00 - ata11) + 4.0f * ata01 * ata01)));
    const float rt00 = a00 / gamma, rt01 = a01 / gamma, rt10 = a10 / gamma, rt11 = a11 / gamma;
    const float rt00_2 = rt00 * rt00, rt01_2 = rt01 * rt01, rt10_2 = rt10 * rt10, rt11_2 = rt11 * rt11;
    const float b0 = sqrtf(-rt00_2 - rt10_2 + 1.0f);
    float b1 = sqrtf(-rt01_2 - rt11_2 + 1.0f);
    const float sp = -rt00 * rt01 - rt10 * rt11;
    if (sp < 0.0f) b1 = -b1;
    for (int r = 1; r <= 3; r++) {
        r1[(r - 1) * 3 + 0] = (rt00) * RV(r, 1) + (rt10) * RV(r, 2) + (b0) * RV(r, 3);
        r1[(r - 1) * 3 + 1] = (rt01) * RV(r, 1) + (rt11) * RV(r, 2) + (b1) * RV(r, 3);
        r1[(r - 1) * 3 + 2] = (b1 * rt10 - b0 * rt11) * RV(r, 1) + (b0 * rt01 - b1 * rt00) * RV(r, 2) + (rt00 * rt11 - rt01 * rt10) * RV(r, 3);
        r2[(r - 1) * 3 + 0] = (rt00) * RV(r, 1) + (rt10) * RV(r, 2) + (-b0) * RV(r, 3);
        r2[(r - 1) * 3 + 1] = (rt01) * RV(r, 1) + (rt11) * RV(r, 2) + (-b1) * RV(r, 3);
        r2[(r - 1) * 3 + 2] = (b0 * rt11 - b1 * rt10) * RV(r, 1) + (b1 * rt00 - b0 * rt01) * RV(r, 2) + (rt00 * rt11 - rt01 * rt10) * RV(r, 3);
    }
#undef RV
}

static void compute_translation(const float obj[12], const float pts[8], const float rot[9], float t[3]) {  // src/pose.rs:269-335
    float m11 = 4.0f, m13 = 0.0f, m22 = 4.0f, m23 = 0.0f, m31 = 0.0f, m32 = 0.0f, m33 = 0.0f;
    float atb0 = 0.0f, atb1 = 0.0f, atb2 = 0.0f;
    for (int i = 0; i < 4; i++) {
        const float ox = obj[3 * i], oy = obj[3 * i + 1];
        const float rx = rot[0] * ox + rot[1] * oy;
        const float ry = rot[3] * ox + rot[4] * oy;
        const float rz = rot[6] * ox + rot[7] * oy;
        const float a2 = -pts[2 * i], b2 = -pts[2 * i + 1];
        m13 += a2; m23 += b2; m31 += a2; m32 += b2;
        m33 += a2 * a2 + b2 * b2;
        const float bx = -a2 * rz - rx;
        const float by = -b2 * rz - ry;
        atb0 += bx; atb1 += by;
        atb2 += a2 * bx + b2 * by;
    }
    const float det_a_inv = 1.0f / (m11 * m22 * m33 - m11 * m23 * m32 - m13 * m22 * m31);
    const float s11 = m22 * m33 - m23 * m32, s12 = m13 * m32, s13 = -m13 * m22;
    const float s21 = m23 * m31, s22 = m11 * m33 - m13 * m31, s23 = -m11 * m23;
    const float s31 = -m22 * m31, s32 = -m11 * m32, s33 = m11 * m22;
    t[0] = det_a_inv * (s11 * atb0 + s12 * atb1 + s13 * atb2);
    t[1] = det_a_inv * (s21 * atb0 + s22 * atb1 + s23 * atb2);
    t[2] = det_a_inv * (s31 * atb0 + s32 * atb1 + s33 * atb2);
}

static float reprojection_error(const a3o_pose* p, const float obj[12], const float pts[8]) {  // src/pose.rs:337-348
    float error = 0.0f;
    const float* r = p->rotation;
    for (int i = 0; i < 4; i++) {
        const float x = obj[3 * i], y = obj[3 * i + 1], z = obj[3 * i + 2];
        const float px = (r[0] * x + r[1] * y + r[2] * z) + p->translation[0];
        const float py = (r[3] * x + r[4] * y + r[5] * z) + p->translation[1];
        const float pz = (r[6] * x + r[7] * y + r[8] * z) + p->translation[2];
        const float zz = pz > 1e-5f ? pz : 1e-5f;
        const float dx = (px / zz) - pts[2 * i];
        const float dy = (py / zz) - pts[2 * i + 1];
        error += sqrtf(dx * dx + dy * dy);
    }
    return error;
}

static void solve_normalized(const float pts[8], float marker_size_mm, a3o_pose* o1, a3o_pose* o2) {  // src/pose.rs:64-156
    const float hw = 0.5f * marker_size_mm;
    const float obj[12] = {-hw, hw, 0.0f, hw, hw, 0.0f, hw, -hw, 0.0f, -hw, -hw, 0.0f};
    const float p1x = -pts[0], p1y = -pts[1], p2x = -pts[2], p2y = -pts[3], p3x = -pts[4], p3y = -pts[5], p4x = -pts[6], p4y = -pts[7];
    const float half_width = marker_size_mm / 2.0f;
    const float det_inv = -1.0f / (half_width * (p1x * p2y - p2x * p1y - p1x * p4y + p2x * p3y - p3x * p2y + p4x * p1y + p3x * p4y - p4x * p3y));
    float h[9];
    h[0] = det_inv * (p1x * p3x * p2y - p2x * p3x * p1y - p1x * p4x * p2y + p2x * p4x * p1y - p1x * p3x * p4y + p1x * p4x * p3y + p2x * p3x * p4y - p2x * p4x * p3y);
    h[1] = det_inv * (p1x * p2x * p3y - p1x * p3x * p2y - p1x * p2x * p4y + p2x * p4x * p1y + p1x * p3x * p4y - p3x * p4x * p1y - p2x * p4x * p3y + p3x * p4x * p2y);
    h[2] = det_inv * half_width * (p1x * p2x * p3y - p2x * p3x * p1y - p1x * p2x * p4y + p1x * p4x * p2y - p1x * p4x * p3y + p3x * p4x * p1y + p2x * p3x * p4y - p3x * p4x * p2y);
    h[3] = det_inv * (p1x * p2y * p3y - p2x * p1y * p3y - p1x * p2y * p4y + p2x * p1y * p4y - p3x * p1y * p4y + p4x * p1y * p3y + p3x * p2y * p4y - p4x * p2y * p3y);
    h[4] = det_inv * (p2x * p1y * p3y - p3x * p1y * p2y - p1x * p2y * p4y + p4x * p1y * p2y + p1x * p3y * p4y - p4x * p1y * p3y - p2x * p3y * p4y + p3x * p2y * p4y);
    h[5] = det_inv * half_width * (p1x * p2y * p3y - p3x * p1y * p2y - p2x * p1y * p4y + p4x * p1y * p2y - p1x * p3y * p4y + p3x * p1y * p4y + p2x * p3y * p4y - p4x * p2y * p3y);
    h[6] = -det_inv * (p1x * p3y - p3x * p1y - p1x * p4y - p2x * p3y + p3x * p2y + p4x * p1y + p2x * p4y - p4x * p2y);
    h[7] = det_inv * (p1x * p2y - p2x * p1y - p1x * p3y + p3x * p1y + p2x * p4y - p4x * p2y - p3x * p4y + p4x * p3y);
    h[8] = 1.0f;
    const float j[4] = {h[0] - h[6] * h[2], h[1] - h[7] * h[2], h[3] - h[6] * h[5], h[4] - h[7] * h[5]};
    a3o_pose a, b;
    compute_rotations(j, h[2], h[5], a.rotation, b.rotation);
    compute_translation(obj, pts, a.rotation, a.translation);
    compute_translation(obj, pts, b.rotation, b.translation);
    a.error = reprojection_error(&a, obj, pts);
    b.error = reprojection_error(&b, obj, pts);
    if (a.error < b.error) { *o1 = a; *o2 = b; } else { *o1 = b; *o2 = a; }
}

static int pose_finite(const a3o_pose* p) {
    for (int q = 0; q < 9; q++)
        if (!isfinite(p->rotation[q])) return 0;
    for (int q = 0; q < 3; q++)
        if (!isfinite(p->translation[q])) return 0;
    return 1;
}

/* the start solver on its own (a3_estimate_pose_normalized) */
void a3o_ippe(const float pts[8], float marker_size, a3o_pose out[2]) { solve_normalized(pts, marker_size, &out[0], &out[1]); }

/* ---------------- board slots and their check (a3_set_board) ---------------- */
/* 0: a square wound top-left, top-right, bottom-right, bottom-left with y up; 1: no size; 2: sides differ; 3: not right angles;
 * 4: wound the wrong way; 5: not finite */
int a3o_check_marker(const float c[8]) {
    double ex[4], ey[4];
    for (int k = 0; k < 8; k++)
        if (!isfinite(c[k])) return 5;
    for (int k = 0; k < 4; k++) { ex[k] = (double)c[2 * ((k + 1) & 3)] - c[2 * k]; ey[k] = (double)c[2 * ((k + 1) & 3) + 1] - c[2 * k + 1]; }
    const double s = sqrt(ex[0] * ex[0] + ey[0] * ey[0]);
    if (!(s > 0.0)) return 1;
    for (int k = 0; k < 4; k++) {
        const int k1 = (k + 1) & 3;
        if (fabs(sqrt(ex[k] * ex[k] + ey[k] * ey[k]) - s) > 1e-3 * s) return 2;
        if (fabs(ex[k] * ex[k1] + ey[k] * ey[k1]) > 1e-3 * s * s) return 3;
    }
    if (!(ex[0] * ey[1] - ey[0] * ex[1] < 0.0)) return 4;
    return 0;
}

void a3o_slot_from(const float xy[8], a3o_slot* s) {
    for (int k = 0; k < 4; k++) { s->x[k] = xy[2 * k]; s->y[k] = xy[2 * k + 1]; }
    const float ex = s->x[1] - s->x[0], ey = s->y[1] - s->y[0];
    s->side = sqrtf(ex * ex + ey * ey);
    s->cs = ex / s->side; s->sn = ey / s->side;
    s->cx = 0.25f * ((s->x[0] + s->x[1]) + (s->x[2] + s->x[3]));
    s->cy = 0.25f * ((s->y[0] + s->y[1]) + (s->y[2] + s->y[3]));
}

/* ---------------- one frame ---------------- */
static uint32_t slot_of(const frame_t* F, uint32_t id) {
    for (uint32_t s = 0; s < F->n_slots; s++)
        if (F->board_ids[s] == id) return s;
    return 0xFFFFu;
}

void a3o_normalise(const frame_t* F, float x, float y, float* u, float* v) {
    if (F->has_intr) { *u = (x - F->cx) / F->fx; *v = (y - F->cy) / F->fy; }
    else { *u = x / F->iw; *v = y / F->ih; }
}

static int corner(const frame_t* F, uint32_t c, float* bx, float* by, float* mx, float* my) {
    const uint32_t m = c >> 2; const int k = (int)(c & 3u);
    const uint32_t slot = slot_of(F, F->ids[m]);
    if (slot == 0xFFFFu || F->dup[slot]) return 0;
    *bx = F->slots[slot].x[k]; *by = F->slots[slot].y[k];
    a3o_normalise(F, F->px[8 * m + 2 * k], F->px[8 * m + 2 * k + 1], mx, my);
    return 1;
}

void a3o_accum(acc_t* s, const float R[9], const float t[3], float bx, float by, float mx, float my, float sx, float sy) {
    const float qx = R[0] * bx + R[1] * by, qy = R[3] * bx + R[4] * by, qz = R[6] * bx + R[7] * by;
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

/* lane 0 after the xor butterfly 32 .. 1 over 64 lanes (lane 0's bits = every lane's); lanes is overwritten */
void a3o_reduce64(acc_t lanes[64], acc_t* out) {
    acc_t nxt[64];
    for (int o = 32; o >= 1; o >>= 1) {
        for (int l = 0; l < 64; l++) {
            const acc_t* a = &lanes[l]; const acc_t* b = &lanes[l ^ o];
            for (int q = 0; q < 21; q++) nxt[l].h[q] = a->h[q] + b->h[q];
            for (int q = 0; q < 6; q++) nxt[l].g[q] = a->g[q] + b->g[q];
            nxt[l].cost = a->cost + b->cost;
            nxt[l].pix = a->pix + b->pix;
        }
        memcpy(lanes, nxt, sizeof nxt);
    }
    *out = lanes[0];
}

/* 64 lanes, corners l, l + 64, ... in order, then the butterfly */
static void evaluate(const void* ctx, const float R[9], const float t[3], acc_t* out) {
    const frame_t* F = (const frame_t*)ctx;
    acc_t lanes[64];
    memset(lanes, 0, sizeof lanes);
    for (int l = 0; l < 64; l++)
        for (uint32_t c = (uint32_t)l; c < 4 * F->cnt; c += 64) {
            float bx, by, mx, my;
            if (corner(F, c, &bx, &by, &mx, &my)) a3o_accum(&lanes[l], R, t, bx, by, mx, my, F->sx, F->sy);
        }
    a3o_reduce64(lanes, out);
}

static int solve6(const float h[21], const float g[6], float lambda, float d[6]) {
    float A[6][6];
    int idx = 0;
    for (int r = 0; r < 6; r++)
        for (int c = r; c < 6; c++) { A[r][c] = h[idx]; A[c][r] = h[idx]; idx++; }
    for (int r = 0; r < 6; r++) A[r][r] = A[r][r] + lambda * A[r][r];
    float L[6][6], D[6];
    for (int j = 0; j < 6; j++) {
        for (int i = j; i < 6; i++) {
            float s = A[i][j];
            for (int k = 0; k < j; k++) s = s - L[i][k] * L[j][k] * D[k];
            if (i == j) {
                if (!(s > 0.0f) || !isfinite(s)) return 0;
                D[j] = s;
                L[j][j] = 1.0f;
            } else L[i][j] = s / D[j];
        }
    }
    float y[6];
    for (int i = 0; i < 6; i++) {
        float s = -g[i];
        for (int k = 0; k < i; k++) s = s - L[i][k] * y[k];
        y[i] = s;
    }
    for (int i = 5; i >= 0; i--) {
        float s = y[i] / D[i];
        for (int k = i + 1; k < 6; k++) s = s - L[k][i] * d[k];
        d[i] = s;
    }
    return 1;
}

/* R <- cay(w) R */
void a3o_cayley(const float w[3], const float R[9], float Rn[9]) {
    const float n2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const float k = 2.0f / (1.0f + n2);
    const float W[9] = {0.0f, -w[2], w[1], w[2], 0.0f, -w[0], -w[1], w[0], 0.0f};
    float C[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const float w2 = w[r] * w[c] - (r == c ? n2 : 0.0f);
            C[3 * r + c] = (r == c ? 1.0f : 0.0f) + k * (W[3 * r + c] + w2);
        }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Rn[3 * r + c] = (C[3 * r] * R[c] + C[3 * r + 1] * R[3 + c]) + C[3 * r + 2] * R[6 + c];
}

/* LM from one start (R, t in the board frame, updated in place) -> evaluations; *cost / *pix of the final state */
uint32_t a3o_lm(a3o_eval_fn eval, const void* ctx, float R[9], float t[3], float* cost, float* pix) {
    acc_t s;
    eval(ctx, R, t, &s);
    uint32_t evals = 1;
    float lambda = 1e-3f;
    while (evals < A3O_MAX_EVALS && s.cost > 0.0f) {
        float d[6];
        if (!solve6(s.h, s.g, lambda, d)) { lambda = lambda * 10.0f; evals++; continue; }
        float Rn[9], tn[3];
        a3o_cayley(d, R, Rn);
        for (int r = 0; r < 3; r++) tn[r] = t[r] + d[3 + r];
        acc_t s2;
        eval(ctx, Rn, tn, &s2);
        evals++;
        if (s2.cost < s.cost) {
            const float rel = (s.cost - s2.cost) / s.cost;
            memcpy(R, Rn, sizeof Rn); memcpy(t, tn, sizeof tn);
            s = s2;
            lambda = lambda / 10.0f;
            if (rel < A3O_REL_TOL) break;
        } else lambda = lambda * 10.0f;
    }
    *cost = s.cost; *pix = s.pix;
    return evals;
}

/* LM from a caller-given start (board frame) -> evaluations; for the tests of the update on its own */
uint32_t a3o_refine_from(const uint32_t* board_ids, const float* board_xy, uint32_t n_board, const uint32_t* ids, const float* px, uint32_t cnt,
                         const float* intr /* fx, fy, cx, cy or NULL */, uint32_t w, uint32_t h, float R[9], float t[3], float* cost_pix2) {
    static a3o_slot slots[A3O_MAX_MARKERS];
    static uint8_t dup[A3O_MAX_MARKERS];
    for (uint32_t s = 0; s < n_board; s++) { a3o_slot_from(board_xy + 8 * s, &slots[s]); dup[s] = 0; }
    frame_t F = {ids, px, cnt, board_ids, slots, n_board, dup, intr != NULL, (float)w, (float)h, 0, 0, 0, 0, 0, 0};
    if (intr) { F.fx = intr[0]; F.fy = intr[1]; F.cx = intr[2]; F.cy = intr[3]; }
    F.sx = intr ? F.fx : F.iw; F.sy = intr ? F.fy : F.ih;
    return a3o_lm(evaluate, &F, R, t, &cost_pix2[0], &cost_pix2[1]);
}

/* the board pose of one frame: cnt markers (ids, 8 pixel corners each, batch order); start_out (nullable, 2 x 12 floats): both
 * starts (R row-major, t) in the board frame, before refinement */
int a3o_board_pose(const uint32_t* board_ids, const float* board_xy, uint32_t n_board, const uint32_t* ids, const float* px, uint32_t cnt,
                   const float* intr /* fx, fy, cx, cy or NULL */, uint32_t w, uint32_t h, a3o_board_rec* out, float* start_out) {
    static a3o_slot slots[A3O_MAX_MARKERS];
    static uint8_t seen[A3O_MAX_MARKERS], dup[A3O_MAX_MARKERS];
    if (n_board > A3O_MAX_MARKERS) return -1;
    for (uint32_t s = 0; s < n_board; s++) { a3o_slot_from(board_xy + 8 * s, &slots[s]); seen[s] = dup[s] = 0; }
    frame_t F = {ids, px, cnt, board_ids, slots, n_board, dup, intr != NULL, (float)w, (float)h, 0, 0, 0, 0, 0, 0};
    if (intr) { F.fx = intr[0]; F.fy = intr[1]; F.cx = intr[2]; F.cy = intr[3]; }
    F.sx = intr ? F.fx : F.iw; F.sy = intr ? F.fy : F.ih;
    for (uint32_t i = 0; i < cnt; i++) {
        const uint32_t s = slot_of(&F, ids[i]);
        if (s == 0xFFFFu) continue;
        if (seen[s]) dup[s] = 1;
        seen[s] = 1;
    }
    memset(out, 0, sizeof *out);
    uint32_t used = 0, rejected = 0, best_i = 0, best_slot = 0;
    float best_area = -1.0f;
    for (uint32_t i = 0; i < cnt; i++) {
        const uint32_t slot = slot_of(&F, ids[i]);
        if (slot == 0xFFFFu) continue;
        if (dup[slot]) { rejected++; continue; }
        used++;
        const float* x = px + 8 * i;
        float s = 0.0f;
        for (int k = 0; k < 4; k++) { const int k1 = (k + 1) & 3; s = s + (x[2 * k] * x[2 * k1 + 1] - x[2 * k1] * x[2 * k + 1]); }
        const float area = 0.5f * fabsf(s);
        if (area > best_area || (area == best_area && slot < best_slot)) {
            float q[8];
            a3o_pose p2[2];
            for (int k = 0; k < 4; k++) a3o_normalise(&F, x[2 * k], x[2 * k + 1], &q[2 * k], &q[2 * k + 1]);
            solve_normalized(q, slots[slot].side, &p2[0], &p2[1]);
            if (pose_finite(&p2[0]) && pose_finite(&p2[1])) { best_area = area; best_i = i; best_slot = slot; }
        }
    }
    out->markers_used = used;
    out->markers_rejected = rejected;
    if (!used || best_area < 0.0f) return 0;   /* no used marker, or none with finite IPPE poses: A3_BOARD_NONE */
    out->status = 1u;
    const a3o_slot* bs = &slots[best_slot];
    float pts[8];
    for (int k = 0; k < 4; k++) a3o_normalise(&F, px[8 * best_i + 2 * k], px[8 * best_i + 2 * k + 1], &pts[2 * k], &pts[2 * k + 1]);
    a3o_pose p[2];
    solve_normalized(pts, bs->side, &p[0], &p[1]);
    float R[2][9], t[2][3], cost[2], pix[2];
    uint32_t ev[2];
    for (int st = 0; st < 2; st++) {
        const float* Rm = p[st].rotation;
        for (int r = 0; r < 3; r++) {
            R[st][3 * r] = Rm[3 * r] * bs->cs - Rm[3 * r + 1] * bs->sn;
            R[st][3 * r + 1] = Rm[3 * r] * bs->sn + Rm[3 * r + 1] * bs->cs;
            R[st][3 * r + 2] = Rm[3 * r + 2];
        }
        for (int r = 0; r < 3; r++) t[st][r] = p[st].translation[r] - (R[st][3 * r] * bs->cx + R[st][3 * r + 1] * bs->cy);
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
