/* rig_oracle.c -- the CPU restatement of the camera rig calibration of include/aruco3_hip.h (a3_calibrate_rigs) that the device kernel
 * k_rig is held to bit for bit.  One rig at a time, in the contract's order of operations.  The homography, the LDL^T pieces, the
 * Cayley update and the pose LM are solve_oracle.h's, the lens model calib_model.h's, pose composition and the row of 13 rig_model.h's;
 * what is written out here is the rig's own: the start over the co-visibility graph and the Schur system over the extrinsics.
 * Compiled with -ffp-contract=off (tests/oracle_build.py).  TEST INFRASTRUCTURE ONLY. */
#include "rig_model.h"

#define NONE 0xffffffffu
#define MAXC A3_RIG_MAX_CAMERAS
#define MAXN (6 * (A3_RIG_MAX_CAMERAS - 1))

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
        obs_pose_start(a, H, os[o].P);
        os[o].cost = obs_pose_lm(a, obj, img, p0, np, os[o].P);
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
    memcpy(E[0][0], POSE_ID, sizeof POSE_ID);
    for (uint32_t c = 1; c < C; c++) {
        memcpy(E[0][c], POSE_ID, sizeof POSE_ID);
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
                bad = !ldl_n(&S[0][0], MAXN, n, Dg);
            }
            if (covariance) {
                const double sigma2 = cost / (double)(2ll * N - n - 6ll * fu);
                for (int i = 0; i < n; i++) {
                    double dv = INFINITY;
                    if (!bad) {
                        double e[MAXN], x[MAXN];
                        for (int k = 0; k < n; k++) e[k] = k == i ? 1.0 : 0.0;
                        ldl_n_solve(&S[0][0], MAXN, n, Dg, e, x, 0);
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
            ldl_n_solve(&S[0][0], MAXN, n, Dg, rhs, de, 0);
            memcpy(E[1 - cur][0], POSE_ID, sizeof POSE_ID);
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
