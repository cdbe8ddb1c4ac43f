/* calib_driver.h -- the part of a camera calibration that does not depend on the lens model, once for calib_oracle.c (rational) and
 * fisheye_calib_oracle.c: the per-view pose LM, the joint LM over the Schur system, the standard deviations, and the result fields
 * both fill alike.  The start, the guess handling and the model's own result fields stay with each oracle.
 * TEST INFRASTRUCTURE ONLY. */
#ifndef A3_CALIB_DRIVER_H
#define A3_CALIB_DRIVER_H
#include "solve_oracle.h"

#define MAX_NP 12    /* the rational model's intrinsics; View and the systems below are sized for it */

typedef struct CalModel {
    int np, aug, po, rc;    /* intrinsics, row length, first pose column, the residual's column */
    void (*row)(const double *a, const double *R, const double *t, double X, double Y, double ou, double ov, double *au, double *av);
    int (*is_free)(uint32_t flags, int i);
} CalModel;

typedef struct View {
    double blk[2][MAX_NENT];
    double pose[2][12];
    double con[MAX_NP * (MAX_NP + 1) / 2 + MAX_NP];
    double H[9];
} View;

typedef struct CalState {
    int fr[MAX_NP], nf;    /* the free intrinsics */
    uint32_t vu, n;        /* used views and their points */
    int status, iter, conv, cur;
    double cost, std[MAX_NP];
} CalState;

typedef struct CalView {
    const CalModel *m;
    const double *a, *pose;
    Points pts;
} CalView;

static inline void cal_row(const void *ctx, double X, double Y, double ou, double ov, double *au, double *av) {
    const CalView *c = (const CalView *)ctx;
    c->m->row(c->a, c->pose, c->pose + 9, X, Y, ou, ov, au, av);
}

static inline void cal_block(const void *ctx, const double *pose, double *out) {
    CalView c = *(const CalView *)ctx;
    c.pose = pose;
    aug_block(cal_row, &c, c.m->aug, &c.pts, out);
}

static inline void view_block(const CalModel *m, const double *a, const double *pose, const uint32_t *off, const float *obj, const float *img,
                              uint32_t v, double *out) {
    const CalView c = {m, a, pose, {obj, img, off[v], off[v + 1] - off[v]}};
    cal_block(&c, pose, out);
}

/* the per-view Schur terms at lambda from slot `slot`; -> 0 when a V_j has a bad pivot */
static inline int schur_terms(const CalModel *m, View *vs, const a3_calib_view *views, uint32_t v0, uint32_t nv, int slot, int nf,
                              const int *fr, double lambda) {
    const int nt = nf * (nf + 1) / 2;
    int ok = 1;
    for (uint32_t j = 0; j < nv; j++) {
        if (views[v0 + j].status != A3_CALIB_VIEW_USED) continue;
        View *V = &vs[v0 + j];
        const double *blk = V->blk[slot];
        double L[6][6], D[6];
        if (!ldl6_at(blk, m->po, m->aug, lambda, L, D)) { ok = 0; continue; }
        for (int c = 0; c <= nf; c++) {
            double b[6], y[6];
            for (int q = 0; q < 6; q++) b[q] = c < nf ? blk[tri_index(fr[c], m->po + q, m->aug)] : blk[tri_index(m->po + q, m->rc, m->aug)];
            ldl6_solve(L, D, b, y);
            for (int k = c < nf ? c : 0; k < nf; k++) {
                double s = 0.0;
                for (int q = 0; q < 6; q++) s = s + blk[tri_index(fr[k], m->po + q, m->aug)] * y[q];
                V->con[c < nf ? tri_index(c, k, nf) : nt + k] = s;
            }
        }
    }
    return ok;
}

static inline void schur_matrix(const View *vs, const a3_calib_view *views, uint32_t v0, uint32_t nv, int nf, const double *U, double lambda,
                                double S[MAX_NP][MAX_NP], double rhs[MAX_NP]) {
    const int nt = nf * (nf + 1) / 2, ne = nt + nf;
    for (int e = 0; e < ne; e++) {
        int c = 0, k = 0;
        if (e < nt) tri_ik(e, nf, &c, &k);
        double s = e < nt ? U[e] : -U[e];
        if (e < nt && c == k) s = s + lambda * s;
        for (uint32_t j = 0; j < nv; j++) {
            if (views[v0 + j].status != A3_CALIB_VIEW_USED) continue;
            const double t = vs[v0 + j].con[e];
            s = e < nt ? s - t : s + t;
        }
        if (e < nt) { S[c][k] = s; S[k][c] = s; }
        else rhs[e - nt] = s;
    }
}

static inline void camera_sums(const CalModel *m, const View *vs, const a3_calib_view *views, uint32_t v0, uint32_t nv, int slot, int nf,
                               const int *fr, double *U) {
    const int nt = nf * (nf + 1) / 2, ne = nt + nf;
    for (int e = 0; e < ne; e++) {
        int idx;
        if (e < nt) {
            int c, k;
            tri_ik(e, nf, &c, &k);
            idx = tri_index(fr[c], fr[k], m->aug);
        } else idx = tri_index(fr[e - nt], m->rc, m->aug);
        double s = 0.0;
        for (uint32_t j = 0; j < nv; j++)
            if (views[v0 + j].status == A3_CALIB_VIEW_USED) s = s + vs[v0 + j].blk[slot][idx];
        U[e] = s;
    }
}

/* once the views have their status: the free parameters, the counts, OK or TOO_FEW */
static inline void calib_begin(const CalModel *m, const a3_calib_camera *C, const a3_calib_view *views, CalState *s) {
    memset(s, 0, sizeof *s);
    for (int i = 0; i < m->np; i++)
        if (m->is_free(C->flags, i)) s->fr[s->nf++] = i;
    for (uint32_t j = 0; j < C->n_views; j++) {
        const a3_calib_view *rec = &views[C->first_view + j];
        if (rec->status == A3_CALIB_VIEW_USED) { s->vu++; s->n += rec->points; }
    }
    s->status = s->vu == 0 || 2ll * s->n - s->nf - 6ll * s->vu <= 0 ? A3_CALIB_TOO_FEW : A3_CALIB_OK;
}

/* From the start a and the used views' start poses in pose[0]: each view's pose LM, the joint LM over the intrinsics and the poses,
 * the standard deviations.  Nothing happens unless s->status is OK. */
static inline void calib_solve(const CalModel *m, const a3_calib_camera *C, const uint32_t *off, const float *obj, const float *img, View *vs,
                               const a3_calib_view *views, double *a, CalState *s) {
    const uint32_t v0 = C->first_view, nv = C->n_views;
    const int nf = s->nf, *fr = s->fr, cost_at = m->aug * (m->aug + 1) / 2 - 1;
    const int maxit = C->max_iterations ? (int)C->max_iterations : A3_CALIB_DEFAULT_ITERATIONS;
    double cost = 0.0, lambda = 1e-3;
    int iter = 0, conv = 0, cur = 0;
    if (s->status != A3_CALIB_OK) return;
    for (uint32_t j = 0; j < nv; j++) {
        const uint32_t v = v0 + j;
        if (views[v].status != A3_CALIB_VIEW_USED) continue;
        const CalView c = {m, a, NULL, {obj, img, off[v], off[v + 1] - off[v]}};
        pose_lm(cal_block, &c, m->po, m->aug, vs[v].pose[0]);
    }
    for (uint32_t j = 0; j < nv; j++)
        if (views[v0 + j].status == A3_CALIB_VIEW_USED) view_block(m, a, vs[v0 + j].pose[0], off, obj, img, v0 + j, vs[v0 + j].blk[0]);
    for (uint32_t j = 0; j < nv; j++)
        if (views[v0 + j].status == A3_CALIB_VIEW_USED) cost = cost + vs[v0 + j].blk[0][cost_at];
    if (!fin(cost)) { s->status = A3_CALIB_NOT_FINITE; return; }
    double U[MAX_NP * (MAX_NP + 1) / 2 + MAX_NP], S[MAX_NP][MAX_NP], rhs[MAX_NP], Dg[MAX_NP], da[MAX_NP], an[MAX_NP];
    int stop = 0, sums = 1;
    if (cost == 0.0) { stop = 1; conv = 1; }
    while (!stop) {
        if (sums) camera_sums(m, vs, views, v0, nv, cur, nf, fr, U);
        int bad = !schur_terms(m, vs, views, v0, nv, cur, nf, fr, lambda);
        if (!bad) schur_matrix(vs, views, v0, nv, nf, U, lambda, S, rhs);
        if (!bad) bad = !ldl_n(&S[0][0], MAX_NP, nf, Dg);
        sums = 0;
        if (bad) {
            lambda = lambda * 10.0;
            iter = iter + 1;
            if (iter >= maxit) stop = 1;
            continue;
        }
        ldl_n_solve(&S[0][0], MAX_NP, nf, Dg, rhs, da, 0);
        memcpy(an, a, (size_t)m->np * sizeof(double));
        for (int c = 0; c < nf; c++) an[fr[c]] = a[fr[c]] + da[c];
        for (uint32_t j = 0; j < nv; j++) {
            const uint32_t v = v0 + j;
            if (views[v].status != A3_CALIB_VIEW_USED) continue;
            View *V = &vs[v];
            const double *blk = V->blk[cur];
            double L[6][6], D[6], b[6], d[6];
            ldl6_at(blk, m->po, m->aug, lambda, L, D);
            for (int q = 0; q < 6; q++) {
                double t = 0.0;
                for (int k = 0; k < nf; k++) t = t + blk[tri_index(fr[k], m->po + q, m->aug)] * da[k];
                b[q] = -blk[tri_index(m->po + q, m->rc, m->aug)] - t;
            }
            ldl6_solve(L, D, b, d);
            pose_update(V->pose[cur], d, V->pose[1 - cur]);
            view_block(m, an, V->pose[1 - cur], off, obj, img, v, V->blk[1 - cur]);
        }
        double c2 = 0.0;
        for (uint32_t j = 0; j < nv; j++)
            if (views[v0 + j].status == A3_CALIB_VIEW_USED) c2 = c2 + vs[v0 + j].blk[1 - cur][cost_at];
        iter = iter + 1;
        if (c2 < cost) {
            const double rel = (cost - c2) / cost;
            cur = 1 - cur;
            memcpy(a, an, (size_t)m->np * sizeof(double));
            cost = c2;
            lambda = lambda / 10.0;
            sums = 1;
            if (rel < A3_CALIB_REL_TOL || c2 == 0.0) { conv = 1; stop = 1; }
        } else lambda = lambda * 10.0;
        if (iter >= maxit) stop = 1;
    }
    /* the standard deviations */
    if (sums) camera_sums(m, vs, views, v0, nv, cur, nf, fr, U);
    int pd = schur_terms(m, vs, views, v0, nv, cur, nf, fr, 0.0);
    if (pd) schur_matrix(vs, views, v0, nv, nf, U, 0.0, S, rhs);
    pd = pd && ldl_n(&S[0][0], MAX_NP, nf, Dg);
    const double sigma2 = cost / (double)(2ll * s->n - nf - 6ll * s->vu);
    for (int i = 0; i < nf; i++) {
        double dv = INFINITY;
        if (pd) {
            double e[MAX_NP], x[MAX_NP];
            for (int k = 0; k < nf; k++) e[k] = k == i ? 1.0 : 0.0;
            ldl_n_solve(&S[0][0], MAX_NP, nf, Dg, e, x, 0);
            dv = sqrt(sigma2 * x[i]);
        }
        s->std[fr[i]] = dv;
    }
    s->cost = cost; s->iter = iter; s->conv = conv; s->cur = cur;
}

/* the result fields that do not depend on the model, and the used views' records; -> whether the model's own are to follow */
static inline int calib_results(const CalModel *m, const a3_calib_camera *C, const CalState *s, const double *a, const View *vs,
                                a3_calib_result *res, a3_calib_view *views) {
    const int cost_at = m->aug * (m->aug + 1) / 2 - 1;
    memset(res, 0, sizeof *res);
    res->status = (uint32_t)s->status;
    res->views_used = s->vu;
    res->points_used = s->n;
    if (s->status != A3_CALIB_OK) return 0;
    res->iterations = (uint32_t)s->iter;
    res->converged = (uint32_t)s->conv;
    res->fx = a[0]; res->fy = a[1]; res->cx = a[2]; res->cy = a[3];
    res->rms_px = sqrt(s->cost / (double)s->n);
    res->intrinsics.image_width = C->image_width;
    res->intrinsics.image_height = C->image_height;
    res->intrinsics.focal_x = (float)a[0]; res->intrinsics.focal_y = (float)a[1];
    res->intrinsics.principal_x = (float)a[2]; res->intrinsics.principal_y = (float)a[3];
    res->distortion.iterations = 20;
    res->distortion.max_residual_px = 0.1f;
    for (uint32_t j = 0; j < C->n_views; j++) {
        const uint32_t v = C->first_view + j;
        a3_calib_view *rec = &views[v];
        if (rec->status != A3_CALIB_VIEW_USED) continue;
        rec->rms_px = (float)sqrt(vs[v].blk[s->cur][cost_at] / (double)rec->points);
        for (int q = 0; q < 9; q++) rec->rotation[q] = (float)vs[v].pose[s->cur][q];
        for (int q = 0; q < 3; q++) rec->translation[q] = (float)vs[v].pose[s->cur][9 + q];
    }
    return 1;
}

#endif
