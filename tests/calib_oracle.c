/* calib_oracle.c -- the CPU restatement of the camera calibration of include/aruco3_hip.h (a3_calibrate_cameras) that the device kernel
 * k_calibrate is held to bit for bit.  One camera at a time, one view at a time, in the contract's order of operations: every sum over
 * a view's points in point order, every sum over views in view order.  Compiled with -ffp-contract=off (tests/calib_oracle.py).
 * TEST INFRASTRUCTURE ONLY. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../include/aruco3_hip.h"

#define AUG 19
#define NENT 190
#define HAUG 9
#define HENT 45

static int tri_index(int i, int k, int n) { return i * n - (i * (i - 1)) / 2 + (k - i); }

static void tri_ik(int e, int n, int *i, int *k) {
    int r = 0;
    while (e >= n - r) { e -= n - r; r++; }
    *i = r;
    *k = r + e;
}

static int fin(double v) { return isfinite(v) != 0; }

/* the model and its 18 Jacobian columns; column 18 the residual */
static void calib_row(const double a[12], const double R[9], const double t[3], double X, double Y, double ou, double ov, double *au, double *av) {
    const double fx = a[0], fy = a[1], cx = a[2], cy = a[3];
    const double k1 = a[4], k2 = a[5], p1 = a[6], p2 = a[7], k3 = a[8], k4 = a[9], k5 = a[10], k6 = a[11];
    const double qx = R[0] * X + R[1] * Y, qy = R[3] * X + R[4] * Y, qz = R[6] * X + R[7] * Y;
    const double px = qx + t[0], py = qy + t[1], pz = qz + t[2];
    const double ia = 1.0 / pz;
    const double x = px * ia, y = py * ia;
    const double r2 = x * x + y * y;
    const double num = 1.0 + ((k3 * r2 + k2) * r2 + k1) * r2;
    const double den = 1.0 + ((k6 * r2 + k5) * r2 + k4) * r2;
    const double iden = 1.0 / den;
    const double radial = num * iden;
    const double xy2 = 2.0 * x * y;
    const double xx2 = r2 + 2.0 * x * x, yy2 = r2 + 2.0 * y * y;
    const double xd = x * radial + (p1 * xy2 + p2 * xx2);
    const double yd = y * radial + (p1 * yy2 + p2 * xy2);
    au[18] = (fx * xd + cx) - ou;
    av[18] = (fy * yd + cy) - ov;
    const double r4 = r2 * r2, r6 = r4 * r2;
    const double dk1 = r2 * iden, dk2 = r4 * iden, dk3 = r6 * iden;
    const double m = radial * iden;
    const double dk4 = -(m * r2), dk5 = -(m * r4), dk6 = -(m * r6);
    const double gx = fx * x, gy = fy * y;
    au[0] = xd;  au[1] = 0.0; au[2] = 1.0; au[3] = 0.0;
    av[0] = 0.0; av[1] = yd;  av[2] = 0.0; av[3] = 1.0;
    au[4] = gx * dk1; au[5] = gx * dk2; au[8] = gx * dk3; au[9] = gx * dk4; au[10] = gx * dk5; au[11] = gx * dk6;
    av[4] = gy * dk1; av[5] = gy * dk2; av[8] = gy * dk3; av[9] = gy * dk4; av[10] = gy * dk5; av[11] = gy * dk6;
    au[6] = fx * xy2; au[7] = fx * xx2;
    av[6] = fy * yy2; av[7] = fy * xy2;
    const double dnum = (3.0 * k3 * r2 + 2.0 * k2) * r2 + k1;
    const double dden = (3.0 * k6 * r2 + 2.0 * k5) * r2 + k4;
    const double dr = (dnum - radial * dden) * iden;
    const double xxd = ((radial + 2.0 * x * x * dr) + 2.0 * p1 * y) + 6.0 * p2 * x;
    const double xyd = ((2.0 * x * y * dr) + 2.0 * p1 * x) + 2.0 * p2 * y;
    const double yyd = ((radial + 2.0 * y * y * dr) + 6.0 * p1 * y) + 2.0 * p2 * x;
    const double cu = fx * ia, cv = fy * ia;
    const double u0 = cu * xxd, u1 = cu * xyd, u2 = -(cu * (xxd * x + xyd * y));
    const double v0 = cv * xyd, v1 = cv * yyd, v2 = -(cv * (xyd * x + yyd * y));
    const double q2x = 2.0 * qx, q2y = 2.0 * qy, q2z = 2.0 * qz;
    au[12] = u2 * q2y - u1 * q2z; au[13] = u0 * q2z - u2 * q2x; au[14] = u1 * q2x - u0 * q2y;
    av[12] = v2 * q2y - v1 * q2z; av[13] = v0 * q2z - v2 * q2x; av[14] = v1 * q2x - v0 * q2y;
    au[15] = u0; au[16] = u1; au[17] = u2;
    av[15] = v0; av[16] = v1; av[17] = v2;
}

static int ldl6(const double *blk, double lambda, double L[6][6], double D[6]) {
    double A[6][6];
    for (int r = 0; r < 6; r++)
        for (int c = r; c < 6; c++) { const double v = blk[tri_index(12 + r, 12 + c, AUG)]; A[r][c] = v; A[c][r] = v; }
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

static void ldl6_solve(double L[6][6], const double D[6], const double b[6], double x[6]) {
    double y[6];
    for (int i = 0; i < 6; i++) {
        double s = b[i];
        for (int k = 0; k < i; k++) s = s - L[i][k] * y[k];
        y[i] = s;
    }
    for (int i = 5; i >= 0; i--) {
        double s = y[i] / D[i];
        for (int k = i + 1; k < 6; k++) s = s - L[k][i] * x[k];
        x[i] = s;
    }
}

static void cayley_d(const double w[3], const double R[9], double Rn[9]) {
    const double n2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const double k = 2.0 / (1.0 + n2);
    const double W[9] = {0.0, -w[2], w[1], w[2], 0.0, -w[0], -w[1], w[0], 0.0};
    double C[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const double w2 = w[r] * w[c] - (r == c ? n2 : 0.0);
            C[3 * r + c] = (r == c ? 1.0 : 0.0) + k * (W[3 * r + c] + w2);
        }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Rn[3 * r + c] = (C[3 * r] * R[c] + C[3 * r + 1] * R[3 + c]) + C[3 * r + 2] * R[6 + c];
}

static void view_block(const double a[12], const double R[9], const double t[3], const float *obj, const float *img, uint32_t p0, uint32_t np,
                       double out[NENT]) {
    double au[AUG], av[AUG];
    for (int e = 0; e < NENT; e++) out[e] = 0.0;
    for (uint32_t j = 0; j < np; j++) {
        const size_t p = (size_t)p0 + j;
        calib_row(a, R, t, (double)obj[2 * p], (double)obj[2 * p + 1], (double)img[2 * p], (double)img[2 * p + 1], au, av);
        for (int e = 0; e < NENT; e++) {
            int i, k;
            tri_ik(e, AUG, &i, &k);
            out[e] = out[e] + au[i] * au[k];
            out[e] = out[e] + av[i] * av[k];
        }
    }
}

/* step 1: -> 1 and H (row-major, H22 = 1), or 0 (DEGENERATE) */
static int view_homography(const float *obj, const float *img, uint32_t p0, uint32_t np, double H[9]) {
    double sx = 0.0, sy = 0.0, su = 0.0, sv = 0.0;
    for (uint32_t j = 0; j < np; j++) {
        const size_t p = (size_t)p0 + j;
        sx = sx + (double)obj[2 * p];
        sy = sy + (double)obj[2 * p + 1];
        su = su + (double)img[2 * p];
        sv = sv + (double)img[2 * p + 1];
    }
    const double n = (double)np;
    const double mx = sx / n, my = sy / n, mu = su / n, mv = sv / n;
    double dob = 0.0, dim = 0.0;
    for (uint32_t j = 0; j < np; j++) {
        const size_t p = (size_t)p0 + j;
        const double ox = (double)obj[2 * p] - mx, oy = (double)obj[2 * p + 1] - my;
        const double ix = (double)img[2 * p] - mu, iy = (double)img[2 * p + 1] - mv;
        dob = dob + sqrt(ox * ox + oy * oy);
        dim = dim + sqrt(ix * ix + iy * iy);
    }
    const double so = 1.4142135623730951 / (dob / n), si = 1.4142135623730951 / (dim / n);
    double acc[HENT];
    for (int e = 0; e < HENT; e++) acc[e] = 0.0;
    for (uint32_t j = 0; j < np; j++) {
        const size_t p = (size_t)p0 + j;
        const double X = ((double)obj[2 * p] - mx) * so, Y = ((double)obj[2 * p + 1] - my) * so;
        const double U = ((double)img[2 * p] - mu) * si, V = ((double)img[2 * p + 1] - mv) * si;
        const double au[HAUG] = {X, Y, 1.0, 0.0, 0.0, 0.0, -(U * X), -(U * Y), U};
        const double av[HAUG] = {0.0, 0.0, 0.0, X, Y, 1.0, -(V * X), -(V * Y), V};
        for (int e = 0; e < HENT; e++) {
            int i, k;
            tri_ik(e, HAUG, &i, &k);
            acc[e] = acc[e] + au[i] * au[k];
            acc[e] = acc[e] + av[i] * av[k];
        }
    }
    double A[64], b[8], h[8];
    for (int i = 0; i < 8; i++) {
        for (int k = 0; k < 8; k++) A[i * 8 + k] = acc[i <= k ? tri_index(i, k, HAUG) : tri_index(k, i, HAUG)];
        b[i] = acc[tri_index(i, 8, HAUG)];
    }
    double amax = 0.0;
    for (int i = 0; i < 8; i++) {
        const double d = fabs(A[i * 9]);
        if (d > amax) amax = d;
    }
    const double thr = 1e-10 * amax;
    for (int c = 0; c < 8; c++) {
        int piv = c;
        double best = fabs(A[c * 9]);
        for (int r = c + 1; r < 8; r++) {
            const double v = fabs(A[r * 8 + c]);
            if (v > best) { best = v; piv = r; }
        }
        if (!(best > thr) || !fin(best)) return 0;
        if (piv != c) {
            for (int k = 0; k < 8; k++) { const double s = A[piv * 8 + k]; A[piv * 8 + k] = A[c * 8 + k]; A[c * 8 + k] = s; }
            const double s = b[piv]; b[piv] = b[c]; b[c] = s;
        }
        for (int r = c + 1; r < 8; r++) {
            const double f = A[r * 8 + c] / A[c * 9];
            for (int k = c + 1; k < 8; k++) A[r * 8 + k] = A[r * 8 + k] - f * A[c * 8 + k];
            b[r] = b[r] - f * b[c];
        }
    }
    for (int r = 7; r >= 0; r--) {
        double s = b[r];
        for (int k = r + 1; k < 8; k++) s = s - A[r * 8 + k] * h[k];
        h[r] = s / A[r * 9];
    }
    const double Hn[9] = {h[0], h[1], h[2], h[3], h[4], h[5], h[6], h[7], 1.0};
    double M[9], G[9];
    for (int r = 0; r < 3; r++) {
        M[3 * r] = Hn[3 * r] * so;
        M[3 * r + 1] = Hn[3 * r + 1] * so;
        M[3 * r + 2] = Hn[3 * r + 2] - (M[3 * r] * mx + M[3 * r + 1] * my);
    }
    for (int c = 0; c < 3; c++) {
        G[c] = M[c] / si + mu * M[6 + c];
        G[3 + c] = M[3 + c] / si + mv * M[6 + c];
        G[6 + c] = M[6 + c];
    }
    const double h22 = G[8];
    int ok = 1;
    for (int i = 0; i < 9; i++) {
        H[i] = G[i] / h22;
        ok = ok && fin(H[i]);
    }
    return ok;
}

static int ldl_n(double A[12][12], int n, double D[12]) {
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

static void ldl_n_solve(double A[12][12], int n, const double D[12], const double b[12], double x[12]) {
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

typedef struct View {
    double blk[2][NENT];
    double pose[2][12];   /* R (9), t (3) */
    double con[90];
    double H[9];
} View;

static int cal_free(uint32_t flags, int i) {
    if (i == 2 || i == 3) return !(flags & A3_CALIB_FIX_PRINCIPAL_POINT);
    if (i == 6 || i == 7) return !(flags & A3_CALIB_ZERO_TANGENT_DIST);
    if (i == 8) return !(flags & A3_CALIB_FIX_K3);
    if (i >= 9) return (flags & A3_CALIB_RATIONAL_MODEL) != 0;
    return 1;
}

/* the per-view Schur terms at lambda from slot `slot`; -> 0 when a V_j has a bad pivot */
static int schur_terms(View *vs, const a3_calib_view *views, uint32_t v0, uint32_t nv, int slot, int nf, const int *fr, double lambda) {
    const int nt = nf * (nf + 1) / 2;
    int ok = 1;
    for (uint32_t j = 0; j < nv; j++) {
        if (views[v0 + j].status != A3_CALIB_VIEW_USED) continue;
        View *V = &vs[v0 + j];
        const double *blk = V->blk[slot];
        double L[6][6], D[6];
        if (!ldl6(blk, lambda, L, D)) { ok = 0; continue; }
        for (int c = 0; c <= nf; c++) {
            double b[6], y[6];
            for (int m = 0; m < 6; m++) b[m] = c < nf ? blk[tri_index(fr[c], 12 + m, AUG)] : blk[tri_index(12 + m, 18, AUG)];
            ldl6_solve(L, D, b, y);
            for (int k = c < nf ? c : 0; k < nf; k++) {
                double s = 0.0;
                for (int m = 0; m < 6; m++) s = s + blk[tri_index(fr[k], 12 + m, AUG)] * y[m];
                V->con[c < nf ? tri_index(c, k, nf) : nt + k] = s;
            }
        }
    }
    return ok;
}

static void schur_matrix(const View *vs, const a3_calib_view *views, uint32_t v0, uint32_t nv, int nf, const double *U, double lambda,
                         double S[12][12], double rhs[12]) {
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

static void camera_sums(const View *vs, const a3_calib_view *views, uint32_t v0, uint32_t nv, int slot, int nf, const int *fr, double *U) {
    const int nt = nf * (nf + 1) / 2, ne = nt + nf;
    for (int e = 0; e < ne; e++) {
        int idx;
        if (e < nt) {
            int c, k;
            tri_ik(e, nf, &c, &k);
            idx = tri_index(fr[c], fr[k], AUG);
        } else idx = tri_index(fr[e - nt], 18, AUG);
        double s = 0.0;
        for (uint32_t j = 0; j < nv; j++)
            if (views[v0 + j].status == A3_CALIB_VIEW_USED) s = s + vs[v0 + j].blk[slot][idx];
        U[e] = s;
    }
}

static void calibrate_one(const a3_calib_camera *C, uint32_t cam_index, const uint32_t *off, const float *obj, const float *img, View *vs,
                          a3_calib_result *res, a3_calib_view *views) {
    (void)cam_index;
    const uint32_t v0 = C->first_view, nv = C->n_views;
    int fr[12], nf = 0;
    for (int i = 0; i < 12; i++)
        if (cal_free(C->flags, i)) fr[nf++] = i;
    /* 1 */
    for (uint32_t j = 0; j < nv; j++) {
        const uint32_t v = v0 + j, p0 = off[v], np = off[v + 1] - p0;
        a3_calib_view *rec = &views[v];
        memset(rec, 0, sizeof *rec);
        rec->points = np;
        rec->status = np < 4 ? A3_CALIB_VIEW_TOO_FEW_POINTS
                             : view_homography(obj, img, p0, np, vs[v].H) ? A3_CALIB_VIEW_USED : A3_CALIB_VIEW_DEGENERATE;
    }
    /* 2 */
    uint32_t vu = 0, n = 0;
    for (uint32_t j = 0; j < nv; j++)
        if (views[v0 + j].status == A3_CALIB_VIEW_USED) { vu++; n += views[v0 + j].points; }
    int status = A3_CALIB_OK;
    double a[12] = {0};
    if (vu == 0 || 2ll * n - nf - 6ll * vu <= 0) status = A3_CALIB_TOO_FEW;
    else if (C->flags & A3_CALIB_USE_INTRINSIC_GUESS) {
        const a3_distortion *d = &C->guess_distortion;
        a[0] = C->guess.focal_x; a[1] = C->guess.focal_y; a[2] = C->guess.principal_x; a[3] = C->guess.principal_y;
        a[4] = d->k1; a[5] = d->k2; a[6] = d->p1; a[7] = d->p2; a[8] = d->k3; a[9] = d->k4; a[10] = d->k5; a[11] = d->k6;
        if (C->flags & A3_CALIB_ZERO_TANGENT_DIST) { a[6] = 0.0; a[7] = 0.0; }
        if (!(C->flags & A3_CALIB_RATIONAL_MODEL)) { a[9] = 0.0; a[10] = 0.0; a[11] = 0.0; }
    } else {
        const double cx = ((double)C->image_width - 1.0) * 0.5, cy = ((double)C->image_height - 1.0) * 0.5;
        double A00 = 0.0, A01 = 0.0, A11 = 0.0, b0 = 0.0, b1 = 0.0;
        for (uint32_t j = 0; j < nv; j++) {
            if (views[v0 + j].status != A3_CALIB_VIEW_USED) continue;
            const double *H = vs[v0 + j].H;
            double h0 = H[0] - H[6] * cx, h1 = H[3] - H[6] * cy, h2 = H[6];
            double w0 = H[1] - H[7] * cx, w1 = H[4] - H[7] * cy, w2 = H[7];
            double d10 = (h0 + w0) * 0.5, d11 = (h1 + w1) * 0.5, d12 = (h2 + w2) * 0.5;
            double d20 = (h0 - w0) * 0.5, d21 = (h1 - w1) * 0.5, d22 = (h2 - w2) * 0.5;
            const double n0 = 1.0 / sqrt((h0 * h0 + h1 * h1) + h2 * h2), n1 = 1.0 / sqrt((w0 * w0 + w1 * w1) + w2 * w2);
            const double n2 = 1.0 / sqrt((d10 * d10 + d11 * d11) + d12 * d12), n3 = 1.0 / sqrt((d20 * d20 + d21 * d21) + d22 * d22);
            h0 = h0 * n0; h1 = h1 * n0; h2 = h2 * n0;
            w0 = w0 * n1; w1 = w1 * n1; w2 = w2 * n1;
            d10 = d10 * n2; d11 = d11 * n2; d12 = d12 * n2;
            d20 = d20 * n3; d21 = d21 * n3; d22 = d22 * n3;
            const double ra = h0 * w0, rb = h1 * w1, rc = -(h2 * w2);
            const double qa = d10 * d20, qb = d11 * d21, qc = -(d12 * d22);
            A00 = A00 + ra * ra; A00 = A00 + qa * qa;
            A01 = A01 + ra * rb; A01 = A01 + qa * qb;
            A11 = A11 + rb * rb; A11 = A11 + qb * qb;
            b0 = b0 + ra * rc; b0 = b0 + qa * qc;
            b1 = b1 + rb * rc; b1 = b1 + qb * qc;
        }
        const double det = A00 * A11 - A01 * A01;
        const double s0 = (A11 * b0 - A01 * b1) / det, s1 = (A00 * b1 - A01 * b0) / det;
        const double fx = sqrt(1.0 / fabs(s0)), fy = sqrt(1.0 / fabs(s1));
        if (!(det > 1e-9 * (A00 * A11)) || !(fx > 0.0) || !fin(fx) || !(fy > 0.0) || !fin(fy)) status = A3_CALIB_NO_INIT;
        a[0] = fx; a[1] = fy; a[2] = cx; a[3] = cy;
    }
    double cost = 0.0, lambda = 1e-3, std[12] = {0};
    int iter = 0, conv = 0, cur = 0;
    const int maxit = C->max_iterations ? (int)C->max_iterations : A3_CALIB_DEFAULT_ITERATIONS;
    if (status == A3_CALIB_OK) {
        /* 3 */
        for (uint32_t j = 0; j < nv; j++) {
            const uint32_t v = v0 + j;
            if (views[v].status != A3_CALIB_VIEW_USED) continue;
            const uint32_t p0 = off[v], np = off[v + 1] - p0;
            View *V = &vs[v];
            const double *H = V->H;
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
            double R[9] = {r00, r10, r01 * r12 - r02 * r11, r01, r11, r02 * r10 - r00 * r12, r02, r12, r00 * r11 - r01 * r10};
            double t[3] = {(2.0 * m[2][0]) / den, (2.0 * m[2][1]) / den, (2.0 * m[2][2]) / den};
            double *pc = V->blk[0], *po = V->blk[1];
            view_block(a, R, t, obj, img, p0, np, pc);
            double c1 = pc[NENT - 1], lam = 1e-3;
            int evals = 1;
            while (evals < A3_CALIB_POSE_EVALS && c1 > 0.0) {
                double L[6][6], D[6];
                if (!ldl6(pc, lam, L, D)) { lam = lam * 10.0; evals++; continue; }
                double b[6], d[6], Rn[9], tn[3];
                for (int q = 0; q < 6; q++) b[q] = -pc[tri_index(12 + q, 18, AUG)];
                ldl6_solve(L, D, b, d);
                cayley_d(d, R, Rn);
                for (int q = 0; q < 3; q++) tn[q] = t[q] + d[3 + q];
                view_block(a, Rn, tn, obj, img, p0, np, po);
                evals++;
                const double c2 = po[NENT - 1];
                if (c2 < c1) {
                    const double rel = (c1 - c2) / c1;
                    memcpy(R, Rn, sizeof R);
                    memcpy(t, tn, sizeof t);
                    double *s = pc; pc = po; po = s;
                    c1 = c2;
                    lam = lam / 10.0;
                    if (rel < A3_CALIB_REL_TOL) break;
                } else lam = lam * 10.0;
            }
            memcpy(V->pose[0], R, sizeof R);
            memcpy(V->pose[0] + 9, t, sizeof t);
        }
        /* 4 */
        for (uint32_t j = 0; j < nv; j++) {
            const uint32_t v = v0 + j;
            if (views[v].status != A3_CALIB_VIEW_USED) continue;
            view_block(a, vs[v].pose[0], vs[v].pose[0] + 9, obj, img, off[v], off[v + 1] - off[v], vs[v].blk[0]);
        }
        for (uint32_t j = 0; j < nv; j++)
            if (views[v0 + j].status == A3_CALIB_VIEW_USED) cost = cost + vs[v0 + j].blk[0][NENT - 1];
        if (!fin(cost)) status = A3_CALIB_NOT_FINITE;
    }
    if (status == A3_CALIB_OK) {
        double U[90], S[12][12], rhs[12], Dg[12], da[12], an[12];
        int stop = 0, sums = 1;
        if (cost == 0.0) { stop = 1; conv = 1; }
        while (!stop) {
            if (sums) camera_sums(vs, views, v0, nv, cur, nf, fr, U);
            int bad = !schur_terms(vs, views, v0, nv, cur, nf, fr, lambda);
            if (!bad) schur_matrix(vs, views, v0, nv, nf, U, lambda, S, rhs);
            if (!bad) bad = !ldl_n(S, nf, Dg);
            sums = 0;
            if (bad) {
                lambda = lambda * 10.0;
                iter = iter + 1;
                if (iter >= maxit) stop = 1;
                continue;
            }
            ldl_n_solve(S, nf, Dg, rhs, da);
            memcpy(an, a, sizeof an);
            for (int c = 0; c < nf; c++) an[fr[c]] = a[fr[c]] + da[c];
            for (uint32_t j = 0; j < nv; j++) {
                const uint32_t v = v0 + j;
                if (views[v].status != A3_CALIB_VIEW_USED) continue;
                View *V = &vs[v];
                const double *blk = V->blk[cur];
                double L[6][6], D[6], b[6], d[6], Rn[9], tn[3];
                ldl6(blk, lambda, L, D);
                for (int q = 0; q < 6; q++) {
                    double s = 0.0;
                    for (int k = 0; k < nf; k++) s = s + blk[tri_index(fr[k], 12 + q, AUG)] * da[k];
                    b[q] = -blk[tri_index(12 + q, 18, AUG)] - s;
                }
                ldl6_solve(L, D, b, d);
                cayley_d(d, V->pose[cur], Rn);
                for (int q = 0; q < 3; q++) tn[q] = V->pose[cur][9 + q] + d[3 + q];
                memcpy(V->pose[1 - cur], Rn, sizeof Rn);
                memcpy(V->pose[1 - cur] + 9, tn, sizeof tn);
                view_block(an, Rn, tn, obj, img, off[v], off[v + 1] - off[v], V->blk[1 - cur]);
            }
            double c2 = 0.0;
            for (uint32_t j = 0; j < nv; j++)
                if (views[v0 + j].status == A3_CALIB_VIEW_USED) c2 = c2 + vs[v0 + j].blk[1 - cur][NENT - 1];
            iter = iter + 1;
            if (c2 < cost) {
                const double rel = (cost - c2) / cost;
                cur = 1 - cur;
                memcpy(a, an, sizeof a);
                cost = c2;
                lambda = lambda / 10.0;
                sums = 1;
                if (rel < A3_CALIB_REL_TOL || c2 == 0.0) { conv = 1; stop = 1; }
            } else lambda = lambda * 10.0;
            if (iter >= maxit) stop = 1;
        }
        /* 5 */
        if (sums) camera_sums(vs, views, v0, nv, cur, nf, fr, U);
        int pd = schur_terms(vs, views, v0, nv, cur, nf, fr, 0.0);
        if (pd) schur_matrix(vs, views, v0, nv, nf, U, 0.0, S, rhs);
        pd = pd && ldl_n(S, nf, Dg);
        const double sigma2 = cost / (double)(2ll * n - nf - 6ll * vu);
        for (int i = 0; i < nf; i++) {
            double dv = INFINITY;
            if (pd) {
                double e[12], x[12];
                for (int k = 0; k < nf; k++) e[k] = k == i ? 1.0 : 0.0;
                ldl_n_solve(S, nf, Dg, e, x);
                dv = sqrt(sigma2 * x[i]);
            }
            std[fr[i]] = dv;
        }
    }
    const int ok = status == A3_CALIB_OK;
    memset(res, 0, sizeof *res);
    res->status = (uint32_t)status;
    res->views_used = vu;
    res->points_used = n;
    if (ok) {
        res->iterations = (uint32_t)iter;
        res->converged = (uint32_t)conv;
        res->fx = a[0]; res->fy = a[1]; res->cx = a[2]; res->cy = a[3];
        for (int i = 0; i < 8; i++) res->dist[i] = a[4 + i];
        for (int i = 0; i < 12; i++) res->std_dev[i] = std[i];
        res->rms_px = sqrt(cost / (double)n);
        res->intrinsics.image_width = C->image_width;
        res->intrinsics.image_height = C->image_height;
        res->intrinsics.focal_x = (float)a[0]; res->intrinsics.focal_y = (float)a[1];
        res->intrinsics.principal_x = (float)a[2]; res->intrinsics.principal_y = (float)a[3];
        res->distortion.model = A3_DIST_RATIONAL;
        res->distortion.iterations = 20;
        res->distortion.k1 = (float)a[4]; res->distortion.k2 = (float)a[5]; res->distortion.p1 = (float)a[6]; res->distortion.p2 = (float)a[7];
        res->distortion.k3 = (float)a[8]; res->distortion.k4 = (float)a[9]; res->distortion.k5 = (float)a[10]; res->distortion.k6 = (float)a[11];
        res->distortion.max_residual_px = 0.1f;
        for (uint32_t j = 0; j < nv; j++) {
            a3_calib_view *rec = &views[v0 + j];
            if (rec->status != A3_CALIB_VIEW_USED) continue;
            rec->rms_px = (float)sqrt(vs[v0 + j].blk[cur][NENT - 1] / (double)rec->points);
            for (int q = 0; q < 9; q++) rec->rotation[q] = (float)vs[v0 + j].pose[cur][q];
            for (int q = 0; q < 3; q++) rec->translation[q] = (float)vs[v0 + j].pose[cur][9 + q];
        }
    }
}

/* a3_calibrate_cameras on valid input (the argument checks are the library's); views must hold n_views records */
int a3o_calibrate(const a3_calib_camera *cams, size_t n_cams, const uint32_t *view_offsets, size_t n_views, const float *object_xy,
                  const float *image_xy, a3_calib_result *results, a3_calib_view *views) {
    View *vs = (View *)calloc(n_views, sizeof(View));
    if (!vs) return -1;
    for (size_t c = 0; c < n_cams; c++) calibrate_one(&cams[c], (uint32_t)c, view_offsets, object_xy, image_xy, vs, &results[c], views);
    free(vs);
    return 0;
}

/* the forward model in f64 (test data): n board points (x, y) -> pixels through a (12 intrinsics) and (R, t) */
void a3o_calib_project(const double *a, const double *R, const double *t, const double *xy, size_t n, double *out) {
    double au[AUG], av[AUG];
    for (size_t i = 0; i < n; i++) {
        calib_row(a, R, t, xy[2 * i], xy[2 * i + 1], 0.0, 0.0, au, av);
        out[2 * i] = au[18];
        out[2 * i + 1] = av[18];
    }
}

/* layout of the ABI structs as this compiler sees the header */
void a3o_calib_layout(size_t *out) {
    out[0] = sizeof(a3_calib_camera); out[1] = offsetof(a3_calib_camera, guess); out[2] = offsetof(a3_calib_camera, guess_distortion);
    out[3] = sizeof(a3_calib_result); out[4] = offsetof(a3_calib_result, fx); out[5] = offsetof(a3_calib_result, dist);
    out[6] = offsetof(a3_calib_result, std_dev); out[7] = offsetof(a3_calib_result, rms_px); out[8] = offsetof(a3_calib_result, intrinsics);
    out[9] = offsetof(a3_calib_result, distortion); out[10] = sizeof(a3_calib_view); out[11] = offsetof(a3_calib_view, rms_px);
    out[12] = offsetof(a3_calib_view, rotation); out[13] = offsetof(a3_calib_view, translation);
}
