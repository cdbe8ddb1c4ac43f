/* handeye_oracle.c -- the CPU restatement of the hand-eye calibration of include/aruco3_hip.h (a3_calibrate_hand_eyes) that the device
 * kernel k_handeye is held to bit for bit.  One problem at a time, in the contract's order of operations.  The homography, the LDL^T
 * pieces, the Cayley update and the pose LM are solve_oracle.h's, the lens model calib_model.h's, pose composition, the rig's columns
 * and a frame's pose rig_model.h's; what is written out here is the hand-eye solve's own: the quaternion conversion, the pairs' K
 * rows, the four charts, the row of 13 through X . M_f . Y and the 12 x 12 system.  Compiled with -ffp-contract=off
 * (tests/oracle_build.py).  TEST INFRASTRUCTURE ONLY. */
#include "rig_model.h"

static void he_quat(const double *R, double q[4]) {
    const double tr = (R[0] + R[4]) + R[8];
    if (tr >= R[0] && tr >= R[4] && tr >= R[8]) {
        const double s = sqrt(tr + 1.0) * 2.0;
        q[0] = 0.25 * s; q[1] = (R[7] - R[5]) / s; q[2] = (R[2] - R[6]) / s; q[3] = (R[3] - R[1]) / s;
    } else if (R[0] >= R[4] && R[0] >= R[8]) {
        const double s = sqrt(((1.0 + R[0]) - R[4]) - R[8]) * 2.0;
        q[0] = (R[7] - R[5]) / s; q[1] = 0.25 * s; q[2] = (R[1] + R[3]) / s; q[3] = (R[2] + R[6]) / s;
    } else if (R[4] >= R[8]) {
        const double s = sqrt(((1.0 + R[4]) - R[0]) - R[8]) * 2.0;
        q[0] = (R[2] - R[6]) / s; q[1] = (R[1] + R[3]) / s; q[2] = 0.25 * s; q[3] = (R[5] + R[7]) / s;
    } else {
        const double s = sqrt(((1.0 + R[8]) - R[0]) - R[4]) * 2.0;
        q[0] = (R[3] - R[1]) / s; q[1] = (R[2] + R[6]) / s; q[2] = (R[5] + R[7]) / s; q[3] = 0.25 * s;
    }
    if (q[0] < 0.0) { q[0] = -q[0]; q[1] = -q[1]; q[2] = -q[2]; q[3] = -q[3]; }
}

static void he_quat_rot(const double q[4], double *R) {
    const double w = q[0], x = q[1], y = q[2], z = q[3];
    R[0] = 1.0 - 2.0 * (y * y + z * z); R[1] = 2.0 * (x * y - w * z); R[2] = 2.0 * (x * z + w * y);
    R[3] = 2.0 * (x * y + w * z); R[4] = 1.0 - 2.0 * (x * x + z * z); R[5] = 2.0 * (y * z - w * x);
    R[6] = 2.0 * (x * z - w * y); R[7] = 2.0 * (y * z + w * x); R[8] = 1.0 - 2.0 * (x * x + y * y);
}

/* A = P_i . P_j^-1, B = M_i . M_j^-1 -> whether the pair counts */
static int he_pair(const double *Pi, const double *Pj, const double *Mi, const double *Mj, double *A, double *B, double qa[4], double qb[4]) {
    double I[12];
    pose_inv(Pj, I);
    pose_mul(Pi, I, A);
    pose_inv(Mj, I);
    pose_mul(Mi, I, B);
    he_quat(A, qa);
    he_quat(B, qb);
    return qb[0] >= A3_HANDEYE_COS_HALF_MAX_PAIR_ANGLE && qb[0] <= A3_HANDEYE_COS_HALF_MIN_PAIR_ANGLE;
}

/* the pair's term of N (10 entries) added to s */
static void he_pair_rot(const double qa[4], const double qb[4], double *s) {
    const double d = qa[0] - qb[0];
    const double dl[3] = {qa[1] - qb[1], qa[2] - qb[2], qa[3] - qb[3]};
    const double sg[3] = {qa[1] + qb[1], qa[2] + qb[2], qa[3] + qb[3]};
    const double K[4][4] = {{d, -dl[0], -dl[1], -dl[2]}, {dl[0], d, -sg[2], sg[1]}, {dl[1], sg[2], d, -sg[0]}, {dl[2], -sg[1], sg[0], d}};
    int e = 0;
    for (int a = 0; a < 4; a++)
        for (int b = a; b < 4; b++, e++) {
            double t = 0.0;
            for (int r = 0; r < 4; r++) t = t + K[r][a] * K[r][b];
            s[e] = s[e] + t;
        }
}

/* the pair's terms of D^T D (6 entries) and D^T c (3) added to s */
static void he_pair_tr(const double *A, const double *B, const double *RX, double *s) {
    double D[9], c[3];
    for (int q = 0; q < 9; q++) D[q] = A[q] - (q == 0 || q == 4 || q == 8 ? 1.0 : 0.0);
    for (int r = 0; r < 3; r++) c[r] = ((RX[3 * r] * B[9] + RX[3 * r + 1] * B[10]) + RX[3 * r + 2] * B[11]) - A[9 + r];
    int e = 0;
    for (int a = 0; a < 3; a++)
        for (int b = a; b < 3; b++, e++) {
            double t = 0.0;
            for (int r = 0; r < 3; r++) t = t + D[3 * r + a] * D[3 * r + b];
            s[e] = s[e] + t;
        }
    for (int a = 0; a < 3; a++) {
        double t = 0.0;
        for (int r = 0; r < 3; r++) t = t + D[3 * r + a] * c[r];
        s[6 + a] = s[6 + a] + t;
    }
}

/* S: S00 S01 S02 S11 S12 S22.  -> 0 when degenerate; *ratio: the smallest pivot over the largest diagonal entry (a diagnostic) */
static int he_solve3(const double S[6], const double b[3], double x[3], double *ratio) {
    double mx = S[0];
    if (S[3] > mx) mx = S[3];
    if (S[5] > mx) mx = S[5];
    const double thr = A3_HANDEYE_MIN_PIVOT_RATIO * mx;
    *ratio = 0.0;
    const double d0 = S[0];
    if (!fin(d0) || !(d0 > thr)) return 0;
    const double l10 = S[1] / d0, l20 = S[2] / d0;
    const double d1 = S[3] - l10 * l10 * d0;
    if (!fin(d1) || !(d1 > thr)) return 0;
    const double l21 = (S[4] - l20 * l10 * d0) / d1;
    const double d2 = (S[5] - l20 * l20 * d0) - l21 * l21 * d1;
    if (!fin(d2) || !(d2 > thr)) return 0;
    const double y0 = b[0], y1 = b[1] - l10 * y0, y2 = (b[2] - l20 * y0) - l21 * y1;
    x[2] = y2 / d2;
    x[1] = y1 / d1 - l21 * x[2];
    x[0] = (y0 / d0 - l10 * x[1]) - l20 * x[2];
    double mn = d0 < d1 ? d0 : d1;
    if (d2 < mn) mn = d2;
    *ratio = mn / mx;
    return 1;
}

/* the four charts over N (10 entries, upper triangle row by row) -> 0 when all are degenerate */
static int he_charts(const double *N, double q[4], double *ratio) {
    double Nf[4][4];
    int e = 0;
    for (int a = 0; a < 4; a++)
        for (int b = a; b < 4; b++, e++) { Nf[a][b] = N[e]; Nf[b][a] = N[e]; }
    int best = -1;
    double bn = 0.0;
    for (int k = 0; k < 4; k++) {
        int id[3], m = 0;
        for (int r = 0; r < 4; r++)
            if (r != k) id[m++] = r;
        const double S[6] = {Nf[id[0]][id[0]], Nf[id[0]][id[1]], Nf[id[0]][id[2]], Nf[id[1]][id[1]], Nf[id[1]][id[2]], Nf[id[2]][id[2]]};
        const double b[3] = {-Nf[id[0]][k], -Nf[id[1]][k], -Nf[id[2]][k]};
        double x[3], c[4], rt;
        if (!he_solve3(S, b, x, &rt)) continue;
        c[k] = 1.0; c[id[0]] = x[0]; c[id[1]] = x[1]; c[id[2]] = x[2];
        const double n2 = ((c[0] * c[0] + c[1] * c[1]) + c[2] * c[2]) + c[3] * c[3];
        if (best < 0 || n2 < bn) {
            best = k; bn = n2; *ratio = rt;
            const double n = sqrt(n2);
            for (int r = 0; r < 4; r++) q[r] = c[r] / n;
        }
    }
    return best >= 0;
}

/* the two augmented rows of one point through G = (X . M) . Y; Ep = X . M */
typedef struct HeAt {
    const double *a, *X, *M, *Y, *Ep, *G;
} HeAt;

static void he_row(const void *ctx, double Xc, double Yc, double ou, double ov, double *au, double *av) {
    const HeAt *g = (const HeAt *)ctx;
    const double *X = g->X, *M = g->M, *Y = g->Y;
    double cu[AUG], cv[AUG];
    calib_row(g->a, g->G, g->G + 9, Xc, Yc, ou, ov, cu, cv);
    const double qf[3] = {Y[0] * Xc + Y[1] * Yc, Y[3] * Xc + Y[4] * Yc, Y[6] * Xc + Y[7] * Yc};
    const double y[3] = {qf[0] + Y[9], qf[1] + Y[10], qf[2] + Y[11]};
    double m[3], qc[3];
    for (int r = 0; r < 3; r++) m[r] = ((M[3 * r] * y[0] + M[3 * r + 1] * y[1]) + M[3 * r + 2] * y[2]) + M[9 + r];
    for (int r = 0; r < 3; r++) qc[r] = (X[3 * r] * m[0] + X[3 * r + 1] * m[1]) + X[3 * r + 2] * m[2];
    rig_cols(cu + 15, g->Ep, qc, qf, cu[18], au);
    rig_cols(cv + 15, g->Ep, qc, qf, cv[18], av);
}

static void he_block(const double a[12], const double *X, const double *M, const double *Y, const float *obj, const float *img, uint32_t p0,
                     uint32_t np, double out[RENT]) {
    double Ep[12], G[12];
    pose_mul(X, M, Ep);
    pose_mul(Ep, Y, G);
    const HeAt g = {a, X, M, Y, Ep, G};
    const Points P = {obj, img, p0, np};
    aug_block(he_row, &g, RAUG, &P, out);
}

typedef struct HeFrame {
    double blk[2][RENT];
    double P[12];
    double cost;
} HeFrame;

static double he_pivots[2];   /* diagnostics of the last problem that ran step 2: the winning chart's and the translation's ratio */

static void frame_M(const a3_handeye_frame *fr, double *M) {
    memcpy(M, fr->rotation, 9 * sizeof(double));
    memcpy(M + 9, fr->translation, 3 * sizeof(double));
}

static void he_sums(const a3_handeye_frame_result *fres, const HeFrame *fs, uint32_t f0, uint32_t F, int slot, double *S) {
    for (int e = 0; e < RENT; e++) {
        double s = 0.0;
        for (uint32_t j = 0; j < F; j++)
            if (fres[f0 + j].status == A3_HANDEYE_FRAME_USED) s = s + fs[f0 + j].blk[slot][e];
        S[e] = s;
    }
}

/* the free part of S damped by lambda -> LDL^T in A, D; 0 on a bad pivot */
static int he_system(const double *S, int n, int off, double lambda, double A[12][12], double D[12]) {
    for (int i = 0; i < n; i++)
        for (int k = i; k < n; k++) { const double v = S[tri_index(off + i, off + k, RAUG)]; A[i][k] = v; A[k][i] = v; }
    for (int i = 0; i < n; i++) A[i][i] = A[i][i] + lambda * A[i][i];
    return ldl_n(&A[0][0], 12, n, D);
}

static void handeye_one(const a3_handeye_problem *R, const a3_handeye_frame *frames, const float *obj, const float *img, HeFrame *fs,
                        a3_handeye_result *res, a3_handeye_frame_result *fres) {
    const uint32_t f0 = R->first_frame, F = R->n_frames;
    const int fixx = (R->flags & A3_HANDEYE_FIX_X) != 0, guess = (R->flags & A3_HANDEYE_USE_GUESS) != 0;
    const double *a = R->a;
    uint32_t fu = 0, N = 0, pairs = 0;
    /* 1 */
    for (uint32_t j = 0; j < F; j++) {
        const uint32_t f = f0 + j, p0 = frames[f].first_point, np = frames[f].n_points;
        a3_handeye_frame_result *rec = &fres[f];
        memset(rec, 0, sizeof *rec);
        rec->points = np;
        double H[9];
        rec->status = np < 4 ? A3_HANDEYE_FRAME_TOO_FEW_POINTS : view_homography(obj, img, p0, np, H) ? A3_HANDEYE_FRAME_USED : A3_HANDEYE_FRAME_DEGENERATE;
        if (rec->status != A3_HANDEYE_FRAME_USED) continue;
        fu++;
        N += np;
        double *T = fs[f].P;
        obs_pose_start(a, H, T);
        fs[f].cost = obs_pose_lm(a, obj, img, p0, np, T);
        for (int q = 0; q < 9; q++) { rec->rotation[q] = T[q]; rec->rotation_f[q] = (float)T[q]; }
        for (int q = 0; q < 3; q++) { rec->translation[q] = T[9 + q]; rec->translation_f[q] = (float)T[9 + q]; }
    }
    int status = fu < 3 ? A3_HANDEYE_TOO_FEW_FRAMES : A3_HANDEYE_OK;
    /* 2 */
    double X[2][12], Y[2][12];
    memcpy(X[0], POSE_ID, sizeof POSE_ID);
    memcpy(Y[0], POSE_ID, sizeof POSE_ID);
    if (status == A3_HANDEYE_OK && (fixx || guess)) {
        memcpy(X[0], R->guess_x_rotation, 9 * sizeof(double));
        memcpy(X[0] + 9, R->guess_x_translation, 3 * sizeof(double));
    }
    if (status == A3_HANDEYE_OK && !(fixx || guess)) {
        double Nq[10], A[12], B[12], Mi[12], Mj[12], qa[4], qb[4];
        for (int e = 0; e < 10; e++) Nq[e] = 0.0;
        for (uint32_t i = 0; i < F; i++) {
            double part[10];
            for (int e = 0; e < 10; e++) part[e] = 0.0;
            if (fres[f0 + i].status == A3_HANDEYE_FRAME_USED) {
                frame_M(&frames[f0 + i], Mi);
                for (uint32_t j = i + 1; j < F; j++) {
                    if (fres[f0 + j].status != A3_HANDEYE_FRAME_USED) continue;
                    frame_M(&frames[f0 + j], Mj);
                    if (!he_pair(fs[f0 + i].P, fs[f0 + j].P, Mi, Mj, A, B, qa, qb)) continue;
                    pairs++;
                    he_pair_rot(qa, qb, part);
                }
            }
            for (int e = 0; e < 10; e++) Nq[e] = Nq[e] + part[e];
        }
        double q[4];
        he_pivots[0] = he_pivots[1] = 0.0;
        if (pairs == 0 || !he_charts(Nq, q, &he_pivots[0])) status = A3_HANDEYE_NO_MOTION;
        else {
            he_quat_rot(q, X[0]);
            double St[9];
            for (int e = 0; e < 9; e++) St[e] = 0.0;
            for (uint32_t i = 0; i < F; i++) {
                double part[9];
                for (int e = 0; e < 9; e++) part[e] = 0.0;
                if (fres[f0 + i].status == A3_HANDEYE_FRAME_USED) {
                    frame_M(&frames[f0 + i], Mi);
                    for (uint32_t j = i + 1; j < F; j++) {
                        if (fres[f0 + j].status != A3_HANDEYE_FRAME_USED) continue;
                        frame_M(&frames[f0 + j], Mj);
                        if (!he_pair(fs[f0 + i].P, fs[f0 + j].P, Mi, Mj, A, B, qa, qb)) continue;
                        he_pair_tr(A, B, X[0], part);
                    }
                }
                for (int e = 0; e < 9; e++) St[e] = St[e] + part[e];
            }
            if (!he_solve3(St, St + 6, X[0] + 9, &he_pivots[1])) status = A3_HANDEYE_NO_MOTION;
        }
    }
    if (status == A3_HANDEYE_OK) {
        if (guess) {
            memcpy(Y[0], R->guess_y_rotation, 9 * sizeof(double));
            memcpy(Y[0] + 9, R->guess_y_translation, 3 * sizeof(double));
        } else {
            int bf = -1;
            double bs = 0.0;
            for (uint32_t j = 0; j < F; j++) {
                if (fres[f0 + j].status != A3_HANDEYE_FRAME_USED) continue;
                const double s = fs[f0 + j].cost / (double)frames[f0 + j].n_points;
                if (bf < 0 || s < bs) { bf = (int)j; bs = s; }
            }
            double M[12], Mi[12], Xi[12], Z[12];
            frame_M(&frames[f0 + (uint32_t)bf], M);
            pose_inv(M, Mi);
            pose_inv(X[0], Xi);
            pose_mul(Xi, fs[f0 + (uint32_t)bf].P, Z);
            pose_mul(Mi, Z, Y[0]);
        }
    }
    /* 3 */
    const int n = fixx ? 6 : 12, off = fixx ? 6 : 0;
    const int maxit = R->max_iterations ? (int)R->max_iterations : A3_CALIB_DEFAULT_ITERATIONS;
    double S[2][RENT], cost = 0.0, std[12];
    int cur = 0, iter = 0, conv = 0;
    for (int i = 0; i < 12; i++) std[i] = 0.0;
    if (status == A3_HANDEYE_OK) {
        for (uint32_t j = 0; j < F; j++) {
            const uint32_t f = f0 + j;
            if (fres[f].status != A3_HANDEYE_FRAME_USED) continue;
            double M[12];
            frame_M(&frames[f], M);
            he_block(a, X[0], M, Y[0], obj, img, frames[f].first_point, frames[f].n_points, fs[f].blk[0]);
        }
        he_sums(fres, fs, f0, F, 0, S[0]);
        cost = S[0][RENT - 1];
        if (!fin(cost)) status = A3_HANDEYE_NOT_FINITE;
    }
    if (status == A3_HANDEYE_OK) {
        double A[12][12], D[12], b[12], d[12];
        double lambda = 1e-3;
        int stop = 0;
        if (cost == 0.0) { stop = 1; conv = 1; }
        while (!stop) {
            if (!he_system(S[cur], n, off, lambda, A, D)) {
                lambda = lambda * 10.0;
                iter = iter + 1;
                if (iter >= maxit) stop = 1;
                continue;
            }
            for (int i = 0; i < n; i++) b[i] = -S[cur][tri_index(off + i, 12, RAUG)];
            ldl_n_solve(&A[0][0], 12, n, D, b, d, 0);
            if (fixx) memcpy(X[1 - cur], X[cur], sizeof X[0]);
            else pose_update(X[cur], d, X[1 - cur]);
            pose_update(Y[cur], d + (n - 6), Y[1 - cur]);
            for (uint32_t j = 0; j < F; j++) {
                const uint32_t f = f0 + j;
                if (fres[f].status != A3_HANDEYE_FRAME_USED) continue;
                double M[12];
                frame_M(&frames[f], M);
                he_block(a, X[1 - cur], M, Y[1 - cur], obj, img, frames[f].first_point, frames[f].n_points, fs[f].blk[1 - cur]);
            }
            he_sums(fres, fs, f0, F, 1 - cur, S[1 - cur]);
            const double c2 = S[1 - cur][RENT - 1];
            iter = iter + 1;
            if (c2 < cost) {
                const double rel = (cost - c2) / cost;
                cur = 1 - cur;
                cost = c2;
                lambda = lambda / 10.0;
                if (rel < A3_CALIB_REL_TOL || c2 == 0.0) { conv = 1; stop = 1; }
            } else lambda = lambda * 10.0;
            if (iter >= maxit) stop = 1;
        }
        /* 4 */
        const int bad = !he_system(S[cur], n, off, 0.0, A, D);
        const double sigma2 = cost / (double)(2ll * N - n);
        for (int i = 0; i < n; i++) {
            double dv = INFINITY;
            if (!bad) {
                double e[12], x[12];
                for (int k = 0; k < n; k++) e[k] = k == i ? 1.0 : 0.0;
                ldl_n_solve(&A[0][0], 12, n, D, e, x, 0);
                dv = sqrt(sigma2 * x[i]);
            }
            std[off + i] = dv;
        }
    }
    memset(res, 0, sizeof *res);
    res->status = (uint32_t)status;
    res->frames_used = fu;
    res->points_used = N;
    res->pairs_used = pairs;
    if (status != A3_HANDEYE_OK) return;
    res->iterations = (uint32_t)iter;
    res->converged = (uint32_t)conv;
    res->rms_px = sqrt(cost / (double)N);
    for (int q = 0; q < 9; q++) {
        res->x_rotation[q] = X[cur][q]; res->x_rotation_f[q] = (float)X[cur][q];
        res->y_rotation[q] = Y[cur][q]; res->y_rotation_f[q] = (float)Y[cur][q];
    }
    for (int q = 0; q < 3; q++) {
        res->x_translation[q] = X[cur][9 + q]; res->x_translation_f[q] = (float)X[cur][9 + q];
        res->y_translation[q] = Y[cur][9 + q]; res->y_translation_f[q] = (float)Y[cur][9 + q];
    }
    for (int q = 0; q < 12; q++) res->std_dev[q] = std[q];
    for (uint32_t j = 0; j < F; j++) {
        a3_handeye_frame_result *rec = &fres[f0 + j];
        if (rec->status == A3_HANDEYE_FRAME_USED) rec->rms_px = (float)sqrt(fs[f0 + j].blk[cur][RENT - 1] / (double)rec->points);
    }
}

/* a3_calibrate_hand_eyes on valid input (the argument checks are the library's) */
int a3o_calibrate_hand_eyes(const a3_handeye_problem *problems, size_t n_problems, const a3_handeye_frame *frames, size_t n_frames,
                            const float *object_xy, const float *image_xy, a3_handeye_result *results, a3_handeye_frame_result *frame_results) {
    HeFrame *fs = (HeFrame *)calloc(n_frames ? n_frames : 1, sizeof(HeFrame));
    if (!fs) return -1;
    memset(frame_results, 0, n_frames * sizeof *frame_results);
    for (size_t r = 0; r < n_problems; r++) handeye_one(&problems[r], frames, object_xy, image_xy, fs, &results[r], frame_results);
    free(fs);
    return 0;
}

/* the pivot ratios of the last problem that ran the start: the winning chart's, the translation system's */
void a3o_handeye_pivots(double *out) { out[0] = he_pivots[0]; out[1] = he_pivots[1]; }

/* layout of the ABI structs as this compiler sees the header */
void a3o_handeye_layout(size_t *out) {
    out[0] = sizeof(a3_handeye_problem); out[1] = offsetof(a3_handeye_problem, flags); out[2] = offsetof(a3_handeye_problem, a);
    out[3] = offsetof(a3_handeye_problem, guess_x_rotation); out[4] = offsetof(a3_handeye_problem, guess_y_translation);
    out[5] = sizeof(a3_handeye_frame); out[6] = offsetof(a3_handeye_frame, translation); out[7] = offsetof(a3_handeye_frame, first_point);
    out[8] = sizeof(a3_handeye_result); out[9] = offsetof(a3_handeye_result, pairs_used); out[10] = offsetof(a3_handeye_result, rms_px);
    out[11] = offsetof(a3_handeye_result, x_rotation); out[12] = offsetof(a3_handeye_result, y_translation);
    out[13] = offsetof(a3_handeye_result, std_dev); out[14] = offsetof(a3_handeye_result, x_rotation_f);
    out[15] = offsetof(a3_handeye_result, y_translation_f);
    out[16] = sizeof(a3_handeye_frame_result); out[17] = offsetof(a3_handeye_frame_result, rms_px);
    out[18] = offsetof(a3_handeye_frame_result, rotation); out[19] = offsetof(a3_handeye_frame_result, rotation_f);
}
