/* map_oracle.c -- the CPU restatement of the marker map solve of include/aruco3_hip.h (a3_build_marker_maps) that the device kernel
 * k_map is held to bit for bit.  One map at a time, in the contract's order of operations.  The homography, the LDL^T pieces, the
 * Cayley update and the pose LM are solve_oracle.h's, the lens model calib_model.h's, pose composition, the row of 13 and an
 * observation's pose rig_model.h's; what is written out here is the map's own: the two planar candidates, the start in rounds and
 * the reduced system over the markers.  Compiled with -ffp-contract=off (tests/oracle_build.py).  TEST INFRASTRUCTURE ONLY. */
#include "rig_model.h"

#define MM A3_MAP_MAX_MARKERS

typedef struct MObs {
    double blk[2][RENT];
    double P[2][12], c[2];   /* step 1's candidates marker -> camera and their costs */
    double Y[6][6];          /* y_o,k */
    int act;
} MObs;

typedef struct MFrame {
    double pose[2][12];
    double vg[2][28];        /* the 7-triangle of columns 0-5 and 12: V_f, g_f, cost_f */
    double yg[6];
    double K[2];             /* step 2: the cost of each of the frame's two candidate poses */
    int cur, located;
} MFrame;

static int FT[28];           /* entry e of that 7-triangle in the 13-triangle */

static double map_cost(const double a[12], const double *G, const float *sq, const float *img) {
    double s = 0.0, au[AUG], av[AUG];
    for (int j = 0; j < 4; j++) {
        calib_row(a, G, G + 9, (double)sq[2 * j], (double)sq[2 * j + 1], (double)img[2 * j], (double)img[2 * j + 1], au, av);
        s = s + au[18] * au[18];
        s = s + av[18] * av[18];
    }
    return fin(s) ? s : INFINITY;
}

static void pose_flip(const double *P, double *Q) {
    const double n = sqrt((P[9] * P[9] + P[10] * P[10]) + P[11] * P[11]);
    const double v[3] = {P[9] / n, P[10] / n, P[11] / n};
    for (int c = 0; c < 3; c++) {
        const double d = (v[0] * P[c] + v[1] * P[3 + c]) + v[2] * P[6 + c];
        const double k = 2.0 * d;
        for (int r = 0; r < 3; r++) {
            const double x = P[3 * r + c] - k * v[r];
            Q[3 * r + c] = c < 2 ? x : -x;
        }
    }
    for (int q = 9; q < 12; q++) Q[q] = P[q];
}

typedef struct Map {
    const a3_map *R;
    const a3_map_observation *obs;
    const float *img;
    float sq[8];
    MObs *os;
    MFrame *fs;
    const uint32_t *fo;   /* per frame of the call: its first observation; fo[f + 1] ends it */
} Map;

static void mframe_eval(const Map *g, uint32_t f, double (*M)[12], const double *T, int slot) {
    double *vg = g->fs[f].vg[slot];
    for (int e = 0; e < 28; e++) vg[e] = 0.0;
    for (uint32_t o = g->fo[f]; o < g->fo[f + 1]; o++) {
        if (!g->os[o].act) continue;
        const double *Mm = M[g->obs[o].marker - g->R->first_marker];
        double G[12];
        pose_mul(T, Mm, G);
        obs_block(g->R->a, T, Mm, G, g->sq, g->img + 8 * (size_t)o, 0, 4, g->os[o].blk[slot]);
        for (int e = 0; e < 28; e++) vg[e] = vg[e] + g->os[o].blk[slot][FT[e]];
    }
}

static void map_one(const a3_map *R, const a3_map_marker *markers, const a3_map_observation *obs, const float *img, MObs *os, MFrame *fs,
                    uint32_t *fo, a3_map_result *res, a3_map_marker_result *mres, a3_map_frame *frames, a3_map_observation_result *ores) {
    const uint32_t M = R->n_markers, m0 = R->first_marker, f0 = R->first_frame, F = R->n_frames, o0 = R->first_obs, NO = R->n_obs;
    const int fix = (R->flags & A3_MAP_FIX_MAP) != 0, guess = fix || (R->flags & A3_MAP_USE_GUESS);
    const double *a = R->a;
    Map g = {R, obs, img, {0}, os, fs, fo};
    const float h = R->marker_length * 0.5f;
    const float sq[8] = {-h, h, h, h, h, -h, -h, -h};
    memcpy(g.sq, sq, sizeof sq);
    for (int e = 0; e < 28; e++) {
        int i, k;
        tri_ik(e, 7, &i, &k);
        FT[e] = tri_index(i < 6 ? i : 12, k < 6 ? k : 12, RAUG);
    }
    {   /* the frames' observation ranges */
        uint32_t o = o0;
        for (uint32_t j = 0; j <= F; j++) {
            while (o < o0 + NO && obs[o].frame < f0 + j) o++;
            fo[f0 + j] = o;
        }
    }
    uint32_t mo[MM + 1], *ml = (uint32_t *)malloc((NO ? NO : 1) * sizeof(uint32_t));   /* a marker's observations, in order */
    {
        uint32_t q = 0;
        for (uint32_t m = 0; m < M; m++) {
            mo[m] = q;
            for (uint32_t o = o0; o < o0 + NO; o++)
                if (obs[o].marker == m0 + m) ml[q++] = o;
        }
        mo[M] = q;
    }
    /* 1 */
    for (uint32_t j = 0; j < NO; j++) {
        const uint32_t o = o0 + j;
        const float *im = img + 8 * (size_t)o;
        a3_map_observation_result *rec = &ores[o];
        memset(rec, 0, sizeof *rec);
        os[o].act = 0;
        double H[9];
        rec->status = view_homography(sq, im, 0, 4, H) ? A3_MAP_OBS_USED : A3_MAP_OBS_DEGENERATE;
        if (rec->status != A3_MAP_OBS_USED) continue;
        obs_pose_start(a, H, os[o].P[0]);
        os[o].c[0] = obs_pose_lm(a, sq, im, 0, 4, os[o].P[0]);
        pose_flip(os[o].P[0], os[o].P[1]);
        os[o].c[1] = obs_pose_lm(a, sq, im, 0, 4, os[o].P[1]);
        rec->start_rms_px[0] = (float)sqrt(os[o].c[0] / 4.0);
        rec->start_rms_px[1] = (float)sqrt(os[o].c[1] / 4.0);
    }
    /* 2 */
    double Mp[2][MM][12];
    int reached[MM];
    for (uint32_t m = 0; m < M; m++) {
        memcpy(Mp[0][m], POSE_ID, sizeof POSE_ID);
        memcpy(Mp[1][m], POSE_ID, sizeof POSE_ID);
        if (guess && m >= 1) {
            memcpy(Mp[0][m], markers[m0 + m].guess_rotation, 9 * sizeof(double));
            memcpy(Mp[0][m] + 9, markers[m0 + m].guess_translation, 3 * sizeof(double));
        }
        reached[m] = fix || m == 0;
    }
    for (uint32_t j = 0; j < F; j++) fs[f0 + j].located = 0;
    for (int changed = 1; changed;) {
        changed = 0;
        for (uint32_t j = 0; j < F; j++) {   /* a */
            const uint32_t f = f0 + j;
            int cnt = 0, have = 0, bk = 0;
            uint32_t bo = 0;
            double bc = 0.0, alt = 0.0;
            for (uint32_t o = fo[f]; o < fo[f + 1]; o++)
                if (ores[o].status == A3_MAP_OBS_USED && reached[obs[o].marker - m0]) cnt++;
            if (cnt == 0 || cnt == fs[f].located) continue;
            for (uint32_t o = fo[f]; o < fo[f + 1]; o++) {
                if (ores[o].status != A3_MAP_OBS_USED || !reached[obs[o].marker - m0]) continue;
                double k[2];
                for (int c = 0; c < 2; c++) {
                    double X[12], T[12], cs = 0.0;
                    pose_inv(Mp[0][obs[o].marker - m0], X);
                    pose_mul(os[o].P[c], X, T);
                    for (uint32_t p = fo[f]; p < fo[f + 1]; p++) {
                        if (ores[p].status != A3_MAP_OBS_USED || !reached[obs[p].marker - m0]) continue;
                        double G[12];
                        pose_mul(T, Mp[0][obs[p].marker - m0], G);
                        cs = cs + map_cost(a, G, sq, img + 8 * (size_t)p);
                    }
                    k[c] = cs;
                }
                if (!have || k[0] < bc) { have = 1; bc = k[0]; alt = k[1]; bo = o; bk = 0; }
                if (k[1] < bc) { bc = k[1]; alt = k[0]; bo = o; bk = 1; }
            }
            fs[f].K[0] = bc;
            fs[f].K[1] = alt;
            double X[12];
            pose_inv(Mp[0][obs[bo].marker - m0], X);
            pose_mul(os[bo].P[bk], X, fs[f].pose[0]);
            pose_mul(os[bo].P[1 - bk], X, fs[f].pose[1]);
            fs[f].located = cnt;
            changed = 1;
        }
        for (uint32_t m = 1; m < M; m++) {   /* b */
            if (reached[m]) continue;
            int have = 0, nh = 0;
            double bc = 0.0, best[12];
            for (uint32_t qo = mo[m]; qo < mo[m + 1] && nh < A3_MAP_START_OBSERVATIONS; qo++) {
                const uint32_t o = ml[qo];
                if (ores[o].status != A3_MAP_OBS_USED || !fs[obs[o].frame].located) continue;
                nh++;
                for (int h = 0; h < 4; h++) {   /* the frame's candidate h / 2, the observation's h % 2 */
                    double X[12], Mh[12], cs = 0.0;
                    pose_inv(fs[obs[o].frame].pose[h / 2], X);
                    pose_mul(X, os[o].P[h % 2], Mh);
                    for (uint32_t qp = mo[m]; qp < mo[m + 1]; qp++) {
                        const uint32_t p = ml[qp];
                        if (ores[p].status != A3_MAP_OBS_USED || !fs[obs[p].frame].located) continue;
                        double G[12];
                        pose_mul(fs[obs[p].frame].pose[0], Mh, G);
                        const double k0 = fs[obs[p].frame].K[0] + map_cost(a, G, sq, img + 8 * (size_t)p);
                        pose_mul(fs[obs[p].frame].pose[1], Mh, G);
                        const double k1 = fs[obs[p].frame].K[1] + map_cost(a, G, sq, img + 8 * (size_t)p);
                        cs = cs + (k1 < k0 ? k1 : k0);
                    }
                    if (!have || cs < bc) { have = 1; bc = cs; memcpy(best, Mh, sizeof best); }
                }
            }
            if (have) {
                if (!guess) memcpy(Mp[0][m], best, sizeof best);
                reached[m] = 1;
                changed = 1;
            }
        }
    }
    /* counts */
    uint32_t fu = 0, ou = 0, mu = 0;
    int ua[MM], pos[MM], nu = 0;
    for (uint32_t m = 0; m < M; m++) {
        memset(&mres[m0 + m], 0, sizeof mres[0]);
        pos[m] = -1;
    }
    for (uint32_t j = 0; j < F; j++) {
        a3_map_frame *fr = &frames[f0 + j];
        memset(fr, 0, sizeof *fr);
        fr->status = fs[f0 + j].located ? A3_MAP_FRAME_USED : A3_MAP_FRAME_UNUSED;
        if (fs[f0 + j].located) fu++;
    }
    for (uint32_t j = 0; j < NO; j++) {
        const uint32_t o = o0 + j, m = obs[o].marker - m0;
        if (ores[o].status != A3_MAP_OBS_USED) continue;
        if (mres[m0 + m].status == 0) mres[m0 + m].status = A3_MAP_MARKER_USED;   /* seen */
        if (!reached[m]) { ores[o].status = A3_MAP_OBS_UNREACHED; continue; }
        os[o].act = 1;
        ou++;
        mres[m0 + m].obs_used++;
        frames[obs[o].frame].obs_used++;
    }
    for (uint32_t m = 0; m < M; m++) {
        a3_map_marker_result *mr = &mres[m0 + m];
        if (mr->status == 0) mr->status = A3_MAP_MARKER_UNSEEN;
        else if (!reached[m]) mr->status = A3_MAP_MARKER_UNREACHED;
        else {
            mu++;
            if (m >= 1 && !fix) { pos[m] = nu; ua[nu++] = (int)m; }
        }
    }
    const uint32_t N = 4 * ou;
    int status = A3_MAP_OK;
    if (!fix && (nu == 0 || mres[m0].status != A3_MAP_MARKER_USED)) status = A3_MAP_NOT_CONNECTED;
    double cost = 0.0;
    int iter = 0, conv = 0, cur = 0;
    const int maxit = R->max_iterations ? (int)R->max_iterations : A3_CALIB_DEFAULT_ITERATIONS;
    const int n = 6 * nu;
    double *S = NULL, *std = NULL, *rhs = NULL, *Dg = NULL, *de = NULL, *ev = NULL;
    if (status == A3_MAP_OK) {
        for (uint32_t j = 0; j < F; j++) {
            const uint32_t f = f0 + j;
            if (!fs[f].located) continue;
            fs[f].cur = 0;
            mframe_eval(&g, f, Mp[0], fs[f].pose[0], 0);
        }
        for (uint32_t j = 0; j < F; j++)
            if (fs[f0 + j].located) cost = cost + fs[f0 + j].vg[0][27];
        if (!fin(cost)) status = A3_MAP_NOT_FINITE;
    }
    if (status == A3_MAP_OK && fix) {
        conv = 1;
        for (uint32_t j = 0; j < F; j++) {
            const uint32_t f = f0 + j;
            if (!fs[f].located) continue;
            MFrame *fr = &fs[f];
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
                mframe_eval(&g, f, Mp[0], fr->pose[1 - fc], 1 - fc);
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
            if (fs[f0 + j].located) cost = cost + fs[f0 + j].vg[fs[f0 + j].cur][27];
    }
    if (status == A3_MAP_OK && !fix) {
        S = (double *)calloc((size_t)n * n, sizeof(double));
        std = (double *)calloc(5 * (size_t)n, sizeof(double));
        rhs = std + n; Dg = rhs + n; de = Dg + n; ev = de + n;
        double (*U)[27] = (double (*)[27])calloc(nu, sizeof(double[27]));
        int stop = 0, sums = 1, covariance = 0;
        double lambda = 1e-3;
        if (cost == 0.0) { stop = 1; conv = 1; }
        while (1) {
            if (stop) { covariance = 1; lambda = 0.0; }
            if (sums)
                for (int u = 0; u < nu; u++)
                    for (int e = 0; e < 27; e++) {
                        int i = 0, k = 0;
                        if (e < 21) tri_ik(e, 6, &i, &k);
                        const int idx = e < 21 ? tri_index(6 + i, 6 + k, RAUG) : tri_index(6 + (e - 21), 12, RAUG);
                        double s = 0.0;
                        for (uint32_t q = mo[ua[u]]; q < mo[ua[u] + 1]; q++)
                            if (os[ml[q]].act) s = s + os[ml[q]].blk[cur][idx];
                        U[u][e] = s;
                    }
            sums = 0;
            int bad = 0;
            for (uint32_t j = 0; j < F; j++) {
                const uint32_t f = f0 + j;
                if (!fs[f].located) continue;
                double L[6][6], D[6], b[6];
                if (!ldl6_at(fs[f].vg[cur], 0, 7, lambda, L, D)) { bad = 1; continue; }
                for (uint32_t o = fo[f]; o < fo[f + 1]; o++) {
                    if (!os[o].act || obs[o].marker == m0) continue;
                    for (int k = 0; k < 6; k++) {
                        for (int q = 0; q < 6; q++) b[q] = os[o].blk[cur][tri_index(q, 6 + k, RAUG)];
                        ldl6_solve(L, D, b, os[o].Y[k]);
                    }
                }
                for (int q = 0; q < 6; q++) b[q] = fs[f].vg[cur][tri_index(q, 6, 7)];
                ldl6_solve(L, D, b, fs[f].yg);
            }
            if (!bad) {
                for (int i = 0; i < n; i++)
                    for (int k = i; k <= n; k++) {   /* k = n: the right-hand side of row i */
                        const uint32_t mi = m0 + (uint32_t)ua[i / 6], mk = k < n ? m0 + (uint32_t)ua[k / 6] : mi;
                        double s;
                        if (k < n) {
                            s = mi == mk ? U[i / 6][tri_index(i % 6, k % 6, 6)] : 0.0;
                            if (i == k) s = s + lambda * s;
                        } else s = -U[i / 6][21 + i % 6];
                        for (uint32_t qi = mo[ua[i / 6]]; qi < mo[ua[i / 6] + 1]; qi++) {
                            const uint32_t oi = ml[qi];
                            if (!os[oi].act) continue;
                            const uint32_t f = obs[oi].frame;
                            const double *y = NULL;
                            if (k == n) y = fs[f].yg;
                            else
                                for (uint32_t p = fo[f]; p < fo[f + 1]; p++)
                                    if (os[p].act && obs[p].marker == mk) y = os[p].Y[k % 6];
                            if (!y) continue;
                            double t = 0.0;
                            for (int q = 0; q < 6; q++) t = t + os[oi].blk[cur][tri_index(q, 6 + i % 6, RAUG)] * y[q];
                            s = k < n ? s - t : s + t;
                        }
                        if (k < n) { S[(size_t)i * n + k] = s; S[(size_t)k * n + i] = s; }
                        else rhs[i] = s;
                    }
                bad = !ldl_n(S, n, n, Dg);
            }
            if (covariance) {
                const long long dof = 2ll * N - n - 6ll * fu;
                const double sigma2 = cost / (double)dof;
                for (int i = 0; i < n; i++) {
                    double dv = INFINITY;
                    if (!bad && dof > 0) {
                        for (int k = 0; k < n; k++) ev[k] = k == i ? 1.0 : 0.0;
                        ldl_n_solve(S, n, n, Dg, ev, ev, 1);
                        dv = sqrt(sigma2 * ev[i]);
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
            ldl_n_solve(S, n, n, Dg, rhs, de, 1);
            for (uint32_t m = 0; m < M; m++) memcpy(Mp[1 - cur][m], Mp[cur][m], sizeof POSE_ID);
            for (int u = 0; u < nu; u++) pose_update(Mp[cur][ua[u]], de + 6 * u, Mp[1 - cur][ua[u]]);
            for (uint32_t j = 0; j < F; j++) {
                const uint32_t f = f0 + j;
                if (!fs[f].located) continue;
                double L[6][6], D[6], b[6], d[6], sm[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
                ldl6_at(fs[f].vg[cur], 0, 7, lambda, L, D);
                for (uint32_t o = fo[f]; o < fo[f + 1]; o++) {
                    if (!os[o].act || obs[o].marker == m0) continue;
                    const int u = pos[obs[o].marker - m0];
                    for (int k = 0; k < 6; k++)
                        for (int q = 0; q < 6; q++) sm[q] = sm[q] + os[o].blk[cur][tri_index(q, 6 + k, RAUG)] * de[6 * u + k];
                }
                for (int q = 0; q < 6; q++) b[q] = -fs[f].vg[cur][tri_index(q, 6, 7)] - sm[q];
                ldl6_solve(L, D, b, d);
                pose_update(fs[f].pose[cur], d, fs[f].pose[1 - cur]);
                mframe_eval(&g, f, Mp[1 - cur], fs[f].pose[1 - cur], 1 - cur);
            }
            double c2 = 0.0;
            for (uint32_t j = 0; j < F; j++)
                if (fs[f0 + j].located) c2 = c2 + fs[f0 + j].vg[1 - cur][27];
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
        free(U);
    }
    /* results */
    const int ok = status == A3_MAP_OK;
    memset(res, 0, sizeof *res);
    res->status = (uint32_t)status;
    res->markers_used = mu;
    res->frames_used = fu;
    res->obs_used = ou;
    if (ok) {
        res->iterations = (uint32_t)iter;
        res->converged = (uint32_t)conv;
        res->rms_px = N ? sqrt(cost / (double)N) : 0.0;
        for (uint32_t m = 0; m < M; m++) {
            a3_map_marker_result *mr = &mres[m0 + m];
            if (mr->status != A3_MAP_MARKER_USED) continue;
            const double *Mm = Mp[fix ? 0 : cur][m];
            double cc = 0.0;
            for (uint32_t q = mo[m]; q < mo[m + 1]; q++)
                if (os[ml[q]].act) cc = cc + os[ml[q]].blk[fs[obs[ml[q]].frame].cur][RENT - 1];
            for (int q = 0; q < 9; q++) { mr->rotation[q] = Mm[q]; mr->rotation_f[q] = (float)Mm[q]; }
            for (int q = 0; q < 3; q++) { mr->translation[q] = Mm[9 + q]; mr->translation_f[q] = (float)Mm[9 + q]; }
            for (int q = 0; q < 6; q++) mr->std_dev[q] = pos[m] >= 0 ? std[6 * pos[m] + q] : 0.0;
            mr->rms_px = mr->obs_used ? sqrt(cc / (double)(4 * mr->obs_used)) : 0.0;
            for (int j = 0; j < 4; j++)
                for (int r = 0; r < 3; r++)
                    mr->corners[3 * j + r] = (Mm[3 * r] * (double)sq[2 * j] + Mm[3 * r + 1] * (double)sq[2 * j + 1]) + Mm[9 + r];
        }
        for (uint32_t j = 0; j < F; j++) {
            const uint32_t f = f0 + j;
            a3_map_frame *fr = &frames[f];
            if (fr->status != A3_MAP_FRAME_USED) continue;
            const int fc = fs[f].cur;
            fr->rms_px = (float)sqrt(fs[f].vg[fc][27] / (double)(4 * fr->obs_used));
            for (int q = 0; q < 9; q++) { fr->rotation[q] = fs[f].pose[fc][q]; fr->rotation_f[q] = (float)fs[f].pose[fc][q]; }
            for (int q = 0; q < 3; q++) { fr->translation[q] = fs[f].pose[fc][9 + q]; fr->translation_f[q] = (float)fs[f].pose[fc][9 + q]; }
            for (uint32_t o = fo[f]; o < fo[f + 1]; o++)
                if (os[o].act) ores[o].rms_px = (float)sqrt(os[o].blk[fc][RENT - 1] / 4.0);
        }
    }
    free(S); free(std); free(ml);
}

/* step 1 for one observation: both candidates marker -> camera (P: 24 doubles) and their costs -> whether it is USED */
int a3o_map_candidates(const double *a, float marker_length, const float *img, double *P, double *c) {
    const float h = marker_length * 0.5f;
    const float sq[8] = {-h, h, h, h, h, -h, -h, -h};
    double H[9];
    if (!view_homography(sq, img, 0, 4, H)) return 0;
    obs_pose_start(a, H, P);
    c[0] = obs_pose_lm(a, sq, img, 0, 4, P);
    pose_flip(P, P + 12);
    c[1] = obs_pose_lm(a, sq, img, 0, 4, P + 12);
    return 1;
}

/* a3_build_marker_maps on valid input (the argument checks are the library's); frames must hold n_frames records */
int a3o_build_marker_maps(const a3_map *maps, size_t n_maps, const a3_map_marker *markers, size_t n_markers, const a3_map_observation *obs,
                          size_t n_obs, const float *image_xy, a3_map_result *results, a3_map_marker_result *marker_results,
                          a3_map_frame *frames, size_t n_frames, a3_map_observation_result *obs_results) {
    MObs *os = (MObs *)calloc(n_obs ? n_obs : 1, sizeof(MObs));
    MFrame *fs = (MFrame *)calloc(n_frames + 1, sizeof(MFrame));
    uint32_t *fo = (uint32_t *)calloc(n_frames + 2, sizeof(uint32_t));
    if (!os || !fs || !fo) { free(os); free(fs); free(fo); return -1; }
    memset(marker_results, 0, n_markers * sizeof *marker_results);
    memset(frames, 0, n_frames * sizeof *frames);
    memset(obs_results, 0, n_obs * sizeof *obs_results);
    for (size_t r = 0; r < n_maps; r++)
        map_one(&maps[r], markers, obs, image_xy, os, fs, fo, &results[r], marker_results, frames, obs_results);
    free(os); free(fs); free(fo);
    return 0;
}

/* layout of the ABI structs as this compiler sees the header */
void a3o_map_layout(size_t *out) {
    out[0] = sizeof(a3_map); out[1] = offsetof(a3_map, a); out[2] = offsetof(a3_map, marker_length);
    out[3] = sizeof(a3_map_marker); out[4] = offsetof(a3_map_marker, guess_translation);
    out[5] = sizeof(a3_map_observation);
    out[6] = sizeof(a3_map_result); out[7] = offsetof(a3_map_result, rms_px);
    out[8] = sizeof(a3_map_marker_result); out[9] = offsetof(a3_map_marker_result, std_dev); out[10] = offsetof(a3_map_marker_result, corners);
    out[11] = offsetof(a3_map_marker_result, rotation_f); out[12] = offsetof(a3_map_marker_result, status);
    out[13] = sizeof(a3_map_frame); out[14] = offsetof(a3_map_frame, rotation); out[15] = offsetof(a3_map_frame, rotation_f);
    out[16] = sizeof(a3_map_observation_result); out[17] = offsetof(a3_map_observation_result, start_rms_px);
}
