/* rig_oracle.c -- the CPU restatement of the camera rig calibration of include/aruco3_hip.h (a3_calibrate_rigs) that the device kernel
 * k_rig is held to bit for bit.  One rig at a time, in the contract's order of operations.  The model, the homography, the 6 x 6 LDL^T
 * and the Cayley update are the calibration contract's, so this file includes calib_oracle.c and uses its static functions; what is
 * the rig's own (pose composition, the row of 13, the start over the co-visibility graph, the Schur system over the extrinsics) is
 * written out here.  Compiled with -ffp-contract=off (tests/rig_oracle.py).  TEST INFRASTRUCTURE ONLY. */
#include "calib_oracle.c"

#define RAUG 13
#define RENT 91
#define NONE 0xffffffffu
#define MAXC A3_RIG_MAX_CAMERAS
#define MAXN (6 * (A3_RIG_MAX_CAMERAS - 1))

static void pose_mul(const double *A, const double *B, double *O) {   /* poses as R (9), t (3) */
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) O[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
        O[9 + r] = ((A[3 * r] * B[9] + A[3 * r + 1] * B[10]) + A[3 * r + 2] * B[11]) + A[9 + r];
    }
}

static void pose_inv(const double *A, double *O) {
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) O[3 * r + c] = A[3 * c + r];
        O[9 + r] = -((A[r] * A[9] + A[3 + r] * A[10]) + A[6 + r] * A[11]);
    }
}

static void rig_cols(const double u[3], const double Rc[9], const double qc[3], const double qf[3], double res, double *o) {
    const double cx = 2.0 * qc[0], cy = 2.0 * qc[1], cz = 2.0 * qc[2];
    o[0] = u[2] * cy - u[1] * cz; o[1] = u[0] * cz - u[2] * cx; o[2] = u[1] * cx - u[0] * cy;
    o[3] = u[0]; o[4] = u[1]; o[5] = u[2];
    double ur[3];
    for (int j = 0; j < 3; j++) ur[j] = (u[0] * Rc[j] + u[1] * Rc[3 + j]) + u[2] * Rc[6 + j];
    const double fx = 2.0 * qf[0], fy = 2.0 * qf[1], fz = 2.0 * qf[2];
    o[6] = ur[2] * fy - ur[1] * fz; o[7] = ur[0] * fz - ur[2] * fx; o[8] = ur[1] * fx - ur[0] * fy;
    o[9] = ur[0]; o[10] = ur[1]; o[11] = ur[2];
    o[12] = res;
}

/* E = (Rc, .) rig -> camera, T board -> rig, G = E . T */
static void rig_row(const double a[12], const double *E, const double *T, const double *G, double X, double Y, double ou, double ov, double *au,
                    double *av) {
    double cu[AUG], cv[AUG];
    calib_row(a, G, G + 9, X, Y, ou, ov, cu, cv);
    const double qf[3] = {T[0] * X + T[1] * Y, T[3] * X + T[4] * Y, T[6] * X + T[7] * Y};
    const double y[3] = {qf[0] + T[9], qf[1] + T[10], qf[2] + T[11]};
    double qc[3];
    for (int r = 0; r < 3; r++) qc[r] = (E[3 * r] * y[0] + E[3 * r + 1] * y[1]) + E[3 * r + 2] * y[2];
    rig_cols(cu + 15, E, qc, qf, cu[18], au);
    rig_cols(cv + 15, E, qc, qf, cv[18], av);
}

static void obs_block(const double a[12], const double *E, const double *T, const double *G, const float *obj, const float *img, uint32_t p0,
                      uint32_t np, double out[RENT]) {
    double au[RAUG], av[RAUG];
    for (int e = 0; e < RENT; e++) out[e] = 0.0;
    for (uint32_t j = 0; j < np; j++) {
        const size_t p = (size_t)p0 + j;
        rig_row(a, E, T, G, (double)obj[2 * p], (double)obj[2 * p + 1], (double)img[2 * p], (double)img[2 * p + 1], au, av);
        for (int e = 0; e < RENT; e++) {
            int i, k;
            tri_ik(e, RAUG, &i, &k);
            out[e] = out[e] + au[i] * au[k];
            out[e] = out[e] + av[i] * av[k];
        }
    }
}

/* LDL^T of V + lambda diag(V), V the 6 x 6 block at columns off .. off + 5 of an aug-triangle */
static int ldl6_at(const double *blk, int off, int aug, double lambda, double L[6][6], double D[6]) {
    double A[6][6];
    for (int r = 0; r < 6; r++)
        for (int c = r; c < 6; c++) { const double v = blk[tri_index(off + r, off + c, aug)]; A[r][c] = v; A[c][r] = v; }
    for (int r = 0; r < 6; r++) A[r][r] = A[r][r] + lambda * A[r][r];
    int ok = 1;
    for (int j = 0; j < 6; j++)
        for (int i = j; i < 6; i++) {
            double s = A[i][j];
            for (int k = 0; k < j; k++) s = s - L[i][k] * L[j][k] * D[k];
            if (i == j) {
                ok = ok && s > 0.0 && fin(s);
                D[j] = s;
                L[j][j] = 1.0;
            } else L[i][j] = s / D[j];
        }
    return ok;
}

static int ldl_m(double A[MAXN][MAXN], int n, double D[MAXN]) {
    for (int j = 0; j < n; j++)
        for (int i = j; i < n; i++) {
            double s = A[i][j];
            for (int k = 0; k < j; k++) s = s - A[i][k] * A[j][k] * D[k];
            if (i == j) {
                if (!(s > 0.0) || !fin(s)) return 0;
                D[j] = s;
            } else A[i][j] = s / D[j];
        }
    return 1;
}

static void ldl_m_solve(double A[MAXN][MAXN], int n, const double D[MAXN], const double *b, double *x) {
    for (int i = 0; i < n; i++) {
        double s = b[i];
        for (int k = 0; k < i; k++) s = s - A[i][k] * x[k];
        x[i] = s;
    }
    for (int i = n - 1; i >= 0; i--) {
        double s = x[i] / D[i];
        for (int k = i + 1; k < n; k++) s = s - A[k][i] * x[k];
        x[i] = s;
    }
}

typedef struct Obs {
    double blk[2][RENT];
    double P[12];          /* board -> camera from step 1 */
    double cost;
} Obs;

typedef struct Frame {
    double pose[2][12];
    double vg[2][28];      /* the 7-triangle of columns 6-12: V_f, g_f, cost_f */
    double Y[MAXN + 1][6];
    int cur;
} Frame;

static void pose_update(const double *T, const double d[6], double *Tn) {
    cayley_d(d, T, Tn);
    for (int q = 0; q < 3; q++) Tn[9 + q] = T[9 + q] + d[3 + q];
}

typedef struct Rig {
    const a3_rig *R;
    const a3_rig_camera *cams;
    const a3_rig_observation *obs;
    const float *obj, *img;
    Obs *os;
    Frame *fs;
    uint32_t *tab;    /* [frame][MAXC] -> observation with status USED, or NONE */
} Rig;

/* the blocks of frame f (call index) at (E, T) into slot, then the frame's sums */
static void frame_eval(const Rig *g, uint32_t f, const double E[MAXC][12], const double *T, int slot) {
    const uint32_t C = g->R->n_cameras;
    double *vg = g->fs[f].vg[slot];
    for (int e = 0; e < 28; e++) vg[e] = 0.0;
    for (uint32_t c = 0; c < C; c++) {
        const uint32_t o = g->tab[(size_t)f * MAXC + c];
        if (o == NONE) continue;
        double G[12];
        pose_mul(E[c], T, G);
        obs_block(g->cams[g->R->first_camera + c].a, E[c], T, G, g->obj, g->img, g->obs[o].first_point, g->obs[o].n_points, g->os[o].blk[slot]);
        for (int e = 0; e < 28; e++) vg[e] = vg[e] + g->os[o].blk[slot][63 + e];
    }
}

static void rig_one(const a3_rig *R, const a3_rig_camera *cams, const a3_rig_observation *obs, const float *obj, const float *img, Obs *os,
                    Frame *fs, uint32_t *tab, a3_rig_result *res, a3_rig_camera_result *cres, a3_rig_frame *frames,
                    a3_rig_observation_result *ores) {
    const uint32_t C = R->n_cameras, c0 = R->first_camera, f0 = R->first_frame, F = R->n_frames, o0 = R->first_obs, NO = R->n_obs;
    const Rig g = {R, cams, obs, obj, img, os, fs, tab};
    const int fix = (R->flags & A3_RIG_FIX_EXTRINSICS) != 0, guess = fix || (R->flags & A3_RIG_USE_EXTRINSIC_GUESS);
    static const double ID[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};
    for (uint32_t j = 0; j < F; j++)
        for (uint32_t c = 0; c < MAXC; c++) tab[(size_t)(f0 + j) * MAXC + c] = NONE;
    /* 1 */
    for (uint32_t j = 0; j < NO; j++) {
        const uint32_t o = o0 + j, p0 = obs[o].first_point, np = obs[o].n_points;
        const double *a = cams[obs[o].camera].a;
        a3_rig_observation_result *rec = &ores[o];
        memset(rec, 0, sizeof *rec);
        rec->points = np;
        double H[9];
        rec->status = np < 4 ? A3_RIG_OBS_TOO_FEW_POINTS : view_homography(obj, img, p0, np, H) ? A3_RIG_OBS_USED : A3_RIG_OBS_DEGENERATE;
        if (rec->status != A3_RIG_OBS_USED) continue;
        tab[(size_t)obs[o].frame * MAXC + (obs[o].camera - c0)] = o;
        double m[3][3];
        for (int c = 0; c < 3; c++) {
            m[c][0] = (H[c] - a[2] * H[6 + c]) / a[0];
            m[c][1] = (H[3 + c] - a[3] * H[6 + c]) / a[1];
            m[c][2] = H[6 + c];
        }
        const double n0 = sqrt((m[0][0] * m[0][0] + m[0][1] * m[0][1]) + m[0][2] * m[0][2]);
        const double r00 = m[0][0] / n0, r01 = m[0][1] / n0, r02 = m[0][2] / n0;
        const double dd = (r00 * m[1][0] + r01 * m[1][1]) + r02 * m[1][2];
        const double e0 = m[1][0] - dd * r00, e1 = m[1][1] - dd * r01, e2 = m[1][2] - dd * r02;
        const double ne = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
        const double r10 = e0 / ne, r11 = e1 / ne, r12 = e2 / ne;
        const double n1 = sqrt((m[1][0] * m[1][0] + m[1][1] * m[1][1]) + m[1][2] * m[1][2]);
        const double den = n0 + n1;
        double T[12] = {r00, r10, r01 * r12 - r02 * r11, r01, r11, r02 * r10 - r00 * r12, r02, r12, r00 * r11 - r01 * r10,
                        (2.0 * m[2][0]) / den, (2.0 * m[2][1]) / den, (2.0 * m[2][2]) / den};
        double *pc = os[o].blk[0], *po = os[o].blk[1];
        obs_block(a, ID, T, T, obj, img, p0, np, pc);
        double c1 = pc[RENT - 1], lam = 1e-3;
        int evals = 1;
        while (evals < A3_CALIB_POSE_EVALS && c1 > 0.0) {
            double L[6][6], D[6];
            if (!ldl6_at(pc, 6, RAUG, lam, L, D)) { lam = lam * 10.0; evals++; continue; }
            double b[6], d[6], Tn[12];
            for (int q = 0; q < 6; q++) b[q] = -pc[tri_index(6 + q, 12, RAUG)];
            ldl6_solve(L, D, b, d);
            pose_update(T, d, Tn);
            obs_block(a, ID, Tn, Tn, obj, img, p0, np, po);
            evals++;
            const double c2 = po[RENT - 1];
            if (c2 < c1) {
                const double rel = (c1 - c2) / c1;
                memcpy(T, Tn, sizeof T);
                double *s = pc; pc = po; po = s;
                c1 = c2;
                lam = lam / 10.0;
                if (rel < A3_CALIB_REL_TOL) break;
            } else lam = lam * 10.0;
        }
        memcpy(os[o].P, T, sizeof T);
        os[o].cost = c1;
    }
    /* counts */
    uint32_t fu = 0, ou = 0, N = 0;
    for (uint32_t c = 0; c < C; c++) memset(&cres[c0 + c], 0, sizeof cres[0]);
    for (uint32_t j = 0; j < F; j++) {
        a3_rig_frame *fr = &frames[f0 + j];
        memset(fr, 0, sizeof *fr);
        for (uint32_t c = 0; c < C; c++) {
            const uint32_t o = tab[(size_t)(f0 + j) * MAXC + c];
            if (o == NONE) continue;
            fr->obs_used++;
            fr->points_used += obs[o].n_points;
            cres[c0 + c].obs_used++;
            cres[c0 + c].points_used += obs[o].n_points;
        }
        fr->status = fr->obs_used ? A3_RIG_FRAME_USED : A3_RIG_FRAME_UNUSED;
        if (fr->obs_used) fu++;
        ou += fr->obs_used;
        N += fr->points_used;
    }
    /* 2 */
    double E[2][MAXC][12];
    int reached[MAXC] = {1, 0, 0, 0, 0, 0, 0, 0};
    int32_t best[MAXC][MAXC];
    for (uint32_t c = 0; c < C; c++)
        for (uint32_t b = 0; b < C; b++) {
            best[c][b] = -1;
            double bs = 0.0;
            if (c == b) continue;
            for (uint32_t j = 0; j < F; j++) {
                const uint32_t oc = tab[(size_t)(f0 + j) * MAXC + c], ob = tab[(size_t)(f0 + j) * MAXC + b];
                if (oc == NONE || ob == NONE) continue;
                const double s = os[oc].cost / (double)obs[oc].n_points + os[ob].cost / (double)obs[ob].n_points;
                if (best[c][b] < 0 || s < bs) { best[c][b] = (int32_t)j; bs = s; }
            }
        }
    memcpy(E[0][0], ID, sizeof ID);
    for (uint32_t c = 1; c < C; c++) {
        memcpy(E[0][c], ID, sizeof ID);
        if (guess) {
            memcpy(E[0][c], cams[c0 + c].guess_rotation, 9 * sizeof(double));
            memcpy(E[0][c] + 9, cams[c0 + c].guess_translation, 3 * sizeof(double));
        }
    }
    for (int found = 1; found;) {
        found = 0;
        for (uint32_t c = 1; c < C && !found; c++) {
            if (reached[c]) continue;
            for (uint32_t b = 0; b < C && !found; b++) {
                if (!reached[b] || best[c][b] < 0) continue;
                const uint32_t f = f0 + (uint32_t)best[c][b];
                const uint32_t oc = tab[(size_t)f * MAXC + c], ob = tab[(size_t)f * MAXC + b];
                if (!guess) {
                    double X[12], Y[12];
                    pose_inv(os[ob].P, X);
                    pose_mul(X, E[0][b], Y);
                    pose_mul(os[oc].P, Y, E[0][c]);
                }
                reached[c] = 1;
                found = 1;
            }
        }
    }
    int status = A3_RIG_OK;
    if (!fix)
        for (uint32_t c = 1; c < C; c++)
            if (!reached[c]) status = A3_RIG_NOT_CONNECTED;
    double cost = 0.0;
    int iter = 0, conv = 0, cur = 0;
    const int maxit = R->max_iterations ? (int)R->max_iterations : A3_CALIB_DEFAULT_ITERATIONS;
    const int n = fix ? 0 : 6 * ((int)C - 1);
    double std[MAXN];
    for (int i = 0; i < MAXN; i++) std[i] = 0.0;
    if (status == A3_RIG_OK) {
        for (uint32_t j = 0; j < F; j++) {
            const uint32_t f = f0 + j;
            if (frames[f].status != A3_RIG_FRAME_USED) continue;
            int bc = -1;
            double bs = 0.0;
            for (uint32_t c = 0; c < C; c++) {
                const uint32_t o = tab[(size_t)f * MAXC + c];
                if (o == NONE) continue;
                const double s = os[o].cost / (double)obs[o].n_points;
                if (bc < 0 || s < bs) { bc = (int)c; bs = s; }
            }
            double X[12];
            pose_inv(E[0][bc], X);
            pose_mul(X, os[tab[(size_t)f * MAXC + bc]].P, fs[f].pose[0]);
            fs[f].cur = 0;
            frame_eval(&g, f, E[0], fs[f].pose[0], 0);
        }
        for (uint32_t j = 0; j < F; j++)
            if (frames[f0 + j].status == A3_RIG_FRAME_USED) cost = cost + fs[f0 + j].vg[0][27];
        if (!fin(cost)) status = A3_RIG_NOT_FINITE;
    }
    if (status == A3_RIG_OK && fix) {
        /* 3, every frame alone */
        conv = 1;
        for (uint32_t j = 0; j < F; j++) {
            const uint32_t f = f0 + j;
            if (frames[f].status != A3_RIG_FRAME_USED) continue;
            Frame *fr = &fs[f];
            double c1 = fr->vg[0][27], lam = 1e-3;
            int it = 0, cv = 0, stop = 0, fc = 0;
            if (c1 == 0.0) { stop = 1; cv = 1; }
            while (!stop) {
                double L[6][6], D[6], b[6], d[6];
                if (!ldl6_at(fr->vg[fc], 0, 7, lam, L, D)) {
                    lam = lam * 10.0;
                    it = it + 1;
                    if (it >= maxit) stop = 1;
                    continue;
                }
                for (int q = 0; q < 6; q++) b[q] = -fr->vg[fc][tri_index(q, 6, 7)];
                ldl6_solve(L, D, b, d);
                pose_update(fr->pose[fc], d, fr->pose[1 - fc]);
                frame_eval(&g, f, E[0], fr->pose[1 - fc], 1 - fc);
                const double c2 = fr->vg[1 - fc][27];
                it = it + 1;
                if (c2 < c1) {
                    const double rel = (c1 - c2) / c1;
                    fc = 1 - fc;
                    c1 = c2;
                    lam = lam / 10.0;
                    if (rel < A3_CALIB_REL_TOL || c2 == 0.0) { cv = 1; stop = 1; }
                } else lam = lam * 10.0;
                if (it >= maxit) stop = 1;
            }
            fr->cur = fc;
            if (it > iter) iter = it;
            if (!cv) conv = 0;
        }
        cost = 0.0;
        for (uint32_t j = 0; j < F; j++)
            if (frames[f0 + j].status == A3_RIG_FRAME_USED) cost = cost + fs[f0 + j].vg[fs[f0 + j].cur][27];
    }
    if (status == A3_RIG_OK && !fix) {
        /* 3, joint */
        static double S[MAXN][MAXN];
        double U[MAXC][27], rhs[MAXN], Dg[MAXN], de[MAXN];
        int stop = 0, sums = 1, covariance = 0;
        double lambda = 1e-3;
        if (cost == 0.0) { stop = 1; conv = 1; }
        while (1) {
            if (stop) {   /* 4: one more pass at lambda 0 for the deviations */
                covariance = 1;
                lambda = 0.0;
            }
            if (sums)
                for (uint32_t c = 1; c < C; c++)
                    for (int e = 0; e < 27; e++) {
                        int i = 0, k = 0;
                        if (e < 21) tri_ik(e, 6, &i, &k);
                        const int idx = e < 21 ? tri_index(i, k, RAUG) : tri_index(e - 21, 12, RAUG);
                        double s = 0.0;
                        for (uint32_t j = 0; j < F; j++) {
                            const uint32_t o = tab[(size_t)(f0 + j) * MAXC + c];
                            if (o != NONE) s = s + os[o].blk[cur][idx];
                        }
                        U[c][e] = s;
                    }
            sums = 0;
            int bad = 0;
            for (uint32_t j = 0; j < F; j++) {
                const uint32_t f = f0 + j;
                if (frames[f].status != A3_RIG_FRAME_USED) continue;
                double L[6][6], D[6], b[6];
                if (!ldl6_at(fs[f].vg[cur], 0, 7, lambda, L, D)) { bad = 1; continue; }
                for (int i = 0; i <= n; i++) {
                    if (i < n) {
                        const uint32_t o = tab[(size_t)f * MAXC + (uint32_t)(i / 6 + 1)];
                        if (o == NONE) continue;
                        for (int m = 0; m < 6; m++) b[m] = os[o].blk[cur][tri_index(i % 6, 6 + m, RAUG)];
                    } else
                        for (int m = 0; m < 6; m++) b[m] = fs[f].vg[cur][tri_index(m, 6, 7)];
                    ldl6_solve(L, D, b, fs[f].Y[i]);
                }
            }
            if (!bad) {
                for (int i = 0; i < n; i++)
                    for (int k = i; k <= n; k++) {   /* k = n: the right-hand side of row i */
                        const uint32_t ci = (uint32_t)(i / 6 + 1), ck = k < n ? (uint32_t)(k / 6 + 1) : ci;
                        double s;
                        if (k < n) {
                            s = ci == ck ? U[ci][tri_index(i % 6, k % 6, 6)] : 0.0;
                            if (i == k) s = s + lambda * s;
                        } else s = -U[ci][21 + i % 6];
                        for (uint32_t j = 0; j < F; j++) {
                            const uint32_t f = f0 + j;
                            if (frames[f].status != A3_RIG_FRAME_USED) continue;
                            const uint32_t oi = tab[(size_t)f * MAXC + ci], ok = tab[(size_t)f * MAXC + ck];
                            if (oi == NONE || ok == NONE) continue;
                            double t = 0.0;
                            for (int m = 0; m < 6; m++) t = t + os[oi].blk[cur][tri_index(i % 6, 6 + m, RAUG)] * fs[f].Y[k][m];
                            s = k < n ? s - t : s + t;
                        }
                        if (k < n) { S[i][k] = s; S[k][i] = s; }
                        else rhs[i] = s;
                    }
                bad = !ldl_m(S, n, Dg);
            }
            if (covariance) {
                const double sigma2 = cost / (double)(2ll * N - n - 6ll * fu);
                for (int i = 0; i < n; i++) {
                    double dv = INFINITY;
                    if (!bad) {
                        double e[MAXN], x[MAXN];
                        for (int k = 0; k < n; k++) e[k] = k == i ? 1.0 : 0.0;
                        ldl_m_solve(S, n, Dg, e, x);
                        dv = sqrt(sigma2 * x[i]);
                    }
                    std[i] = dv;
                }
                break;
            }
            if (bad) {
                lambda = lambda * 10.0;
                iter = iter + 1;
                if (iter >= maxit) stop = 1;
                continue;
            }
            ldl_m_solve(S, n, Dg, rhs, de);
            memcpy(E[1 - cur][0], ID, sizeof ID);
            for (uint32_t c = 1; c < C; c++) pose_update(E[cur][c], de + 6 * (c - 1), E[1 - cur][c]);
            for (uint32_t j = 0; j < F; j++) {
                const uint32_t f = f0 + j;
                if (frames[f].status != A3_RIG_FRAME_USED) continue;
                double L[6][6], D[6], b[6], d[6];
                ldl6_at(fs[f].vg[cur], 0, 7, lambda, L, D);
                for (int q = 0; q < 6; q++) {
                    double s = 0.0;
                    for (int k = 0; k < n; k++) {
                        const uint32_t o = tab[(size_t)f * MAXC + (uint32_t)(k / 6 + 1)];
                        if (o != NONE) s = s + os[o].blk[cur][tri_index(k % 6, 6 + q, RAUG)] * de[k];
                    }
                    b[q] = -fs[f].vg[cur][tri_index(q, 6, 7)] - s;
                }
                ldl6_solve(L, D, b, d);
                pose_update(fs[f].pose[cur], d, fs[f].pose[1 - cur]);
                frame_eval(&g, f, E[1 - cur], fs[f].pose[1 - cur], 1 - cur);
            }
            double c2 = 0.0;
            for (uint32_t j = 0; j < F; j++)
                if (frames[f0 + j].status == A3_RIG_FRAME_USED) c2 = c2 + fs[f0 + j].vg[1 - cur][27];
            iter = iter + 1;
            if (c2 < cost) {
                const double rel = (cost - c2) / cost;
                cur = 1 - cur;
                cost = c2;
                lambda = lambda / 10.0;
                sums = 1;
                if (rel < A3_CALIB_REL_TOL || c2 == 0.0) { conv = 1; stop = 1; }
            } else lambda = lambda * 10.0;
            if (iter >= maxit) stop = 1;
        }
        for (uint32_t j = 0; j < F; j++) fs[f0 + j].cur = cur;
    }
    /* results */
    const int ok = status == A3_RIG_OK;
    memset(res, 0, sizeof *res);
    res->status = (uint32_t)status;
    res->frames_used = fu;
    res->obs_used = ou;
    res->points_used = N;
    if (!ok) return;
    res->iterations = (uint32_t)iter;
    res->converged = (uint32_t)conv;
    res->rms_px = N ? sqrt(cost / (double)N) : 0.0;
    for (uint32_t c = 0; c < C; c++) {
        a3_rig_camera_result *cr = &cres[c0 + c];
        const double *Ec = E[fix ? 0 : cur][c];
        double cc = 0.0;
        for (uint32_t j = 0; j < F; j++) {
            const uint32_t o = tab[(size_t)(f0 + j) * MAXC + c];
            if (o != NONE) cc = cc + os[o].blk[fs[f0 + j].cur][RENT - 1];
        }
        for (int q = 0; q < 9; q++) { cr->rotation[q] = Ec[q]; cr->rotation_f[q] = (float)Ec[q]; }
        for (int q = 0; q < 3; q++) { cr->translation[q] = Ec[9 + q]; cr->translation_f[q] = (float)Ec[9 + q]; }
        for (int q = 0; q < 6; q++) cr->std_dev[q] = c >= 1 && !fix ? std[6 * (c - 1) + q] : 0.0;
        cr->rms_px = cr->points_used ? sqrt(cc / (double)cr->points_used) : 0.0;
    }
    for (uint32_t j = 0; j < F; j++) {
        const uint32_t f = f0 + j;
        a3_rig_frame *fr = &frames[f];
        if (fr->status != A3_RIG_FRAME_USED) continue;
        const int fc = fs[f].cur;
        fr->rms_px = (float)sqrt(fs[f].vg[fc][27] / (double)fr->points_used);
        for (int q = 0; q < 9; q++) { fr->rotation[q] = fs[f].pose[fc][q]; fr->rotation_f[q] = (float)fs[f].pose[fc][q]; }
        for (int q = 0; q < 3; q++) { fr->translation[q] = fs[f].pose[fc][9 + q]; fr->translation_f[q] = (float)fs[f].pose[fc][9 + q]; }
        for (uint32_t c = 0; c < C; c++) {
            const uint32_t o = tab[(size_t)f * MAXC + c];
            if (o != NONE) ores[o].rms_px = (float)sqrt(os[o].blk[fc][RENT - 1] / (double)ores[o].points);
        }
    }
}

/* a3_calibrate_rigs on valid input (the argument checks are the library's); frames must hold n_frames records */
int a3o_calibrate_rigs(const a3_rig *rigs, size_t n_rigs, const a3_rig_camera *cameras, size_t n_cameras, const a3_rig_observation *obs,
                       size_t n_obs, const float *object_xy, const float *image_xy, a3_rig_result *results,
                       a3_rig_camera_result *camera_results, a3_rig_frame *frames, size_t n_frames, a3_rig_observation_result *obs_results) {
    Obs *os = (Obs *)calloc(n_obs ? n_obs : 1, sizeof(Obs));
    Frame *fs = (Frame *)calloc(n_frames ? n_frames : 1, sizeof(Frame));
    uint32_t *tab = (uint32_t *)calloc((n_frames ? n_frames : 1) * MAXC, sizeof(uint32_t));
    if (!os || !fs || !tab) { free(os); free(fs); free(tab); return -1; }
    memset(camera_results, 0, n_cameras * sizeof *camera_results);
    memset(frames, 0, n_frames * sizeof *frames);
    memset(obs_results, 0, n_obs * sizeof *obs_results);
    for (size_t r = 0; r < n_rigs; r++)
        rig_one(&rigs[r], cameras, obs, object_xy, image_xy, os, fs, tab, &results[r], camera_results, frames, obs_results);
    free(os); free(fs); free(tab);
    return 0;
}

/* layout of the ABI structs as this compiler sees the header */
void a3o_rig_layout(size_t *out) {
    out[0] = sizeof(a3_rig); out[1] = offsetof(a3_rig, flags);
    out[2] = sizeof(a3_rig_camera); out[3] = offsetof(a3_rig_camera, guess_rotation); out[4] = offsetof(a3_rig_camera, guess_translation);
    out[5] = sizeof(a3_rig_observation); out[6] = offsetof(a3_rig_observation, first_point);
    out[7] = sizeof(a3_rig_result); out[8] = offsetof(a3_rig_result, rms_px);
    out[9] = sizeof(a3_rig_camera_result); out[10] = offsetof(a3_rig_camera_result, std_dev); out[11] = offsetof(a3_rig_camera_result, rms_px);
    out[12] = offsetof(a3_rig_camera_result, rotation_f); out[13] = offsetof(a3_rig_camera_result, obs_used);
    out[14] = sizeof(a3_rig_frame); out[15] = offsetof(a3_rig_frame, rms_px); out[16] = offsetof(a3_rig_frame, rotation);
    out[17] = offsetof(a3_rig_frame, rotation_f); out[18] = sizeof(a3_rig_observation_result); out[19] = offsetof(a3_rig_observation_result, rms_px);
}
