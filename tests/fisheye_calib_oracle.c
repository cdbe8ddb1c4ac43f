/* fisheye_calib_oracle.c -- the CPU restatement of the fisheye camera calibration of include/aruco3_hip.h
 * (a3_calibrate_fisheye_cameras) that the device kernel k_calibrate_fisheye is held to bit for bit.  One camera at a time, one view at
 * a time, in the contract's order of operations: every sum over a view's points in point order, every sum over views in view order.
 * Compiled with -ffp-contract=off (tests/fisheye_calib_oracle.py).  No math function but sqrt and fabs: the arctangent is a64 below.
 * TEST INFRASTRUCTURE ONLY. */
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../include/aruco3_hip.h"

#define AUG 15    /* 8 intrinsics (fx fy cx cy k1 k2 k3 k4), w, t, the residual */
#define NENT 120
#define PO 8      /* first pose column */
#define RC 14     /* the residual's column */
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

/* A64: Cephes' double atan, written out */
static double a64(double t) {
    const double MOREBITS = 6.123233995736765886130e-17;
    double y0, z, m;
    if (t > 2.41421356237309504880) { y0 = 1.5707963267948966; z = -(1.0 / t); m = MOREBITS; }
    else if (t <= 0.66) { y0 = 0.0; z = t; m = 0.0; }
    else { y0 = 0.7853981633974483; z = (t - 1.0) / (t + 1.0); m = 0.5 * MOREBITS; }
    const double w = z * z;
    const double p = (((-8.750608600031904122785e-1 * w + -1.615753718733365076637e1) * w + -7.500855792314704667340e1) * w +
                      -1.228866684490136173410e2) * w + -6.485021904942025371773e1;
    const double q = ((((w + 2.485846490142306297962e1) * w + 1.650270098316988542046e2) * w + 4.328810604912902668951e2) * w +
                      4.853903996359136964868e2) * w + 1.945506571482613964425e2;
    return y0 + ((z * (w * p / q) + z) + m);
}

/* the forward lens F(x, y) in the normalised plane */
static void fe_forward(const double a[8], double x, double y, double *xd, double *yd) {
    const double k1 = a[4], k2 = a[5], k3 = a[6], k4 = a[7];
    const double r = sqrt(x * x + y * y);
    const double th = a64(r), t2 = th * th;
    const double thd = th * (1.0 + (((k4 * t2 + k3) * t2 + k2) * t2 + k1) * t2);
    const double s = r > 0.0 ? thd / r : 1.0;
    *xd = x * s;
    *yd = y * s;
}

/* step 2's undistortion of one image point at the start parameters: -> kept for the start, and the normalised point */
static int fe_start_point(const double a[8], double u, double v, double *xo, double *yo) {
    const double fx = a[0], fy = a[1], cx = a[2], cy = a[3], k1 = a[4], k2 = a[5], k3 = a[6], k4 = a[7];
    const double x0 = (u - cx) / fx, y0 = (v - cy) / fy;
    const double rd = sqrt(x0 * x0 + y0 * y0);
    double r = rd;
    for (int it = 0; it < 20; it++) {
        const double th = a64(r), t2 = th * th;
        const double g = th * (1.0 + (((k4 * t2 + k3) * t2 + k2) * t2 + k1) * t2);
        const double dg = 1.0 + (((9.0 * k4 * t2 + 7.0 * k3) * t2 + 5.0 * k2) * t2 + 3.0 * k1) * t2;
        r = r - (g - rd) * (1.0 + r * r) / dg;
    }
    const double s = rd > 0.0 ? r / rd : 1.0;
    const double x = x0 * s, y = y0 * s;
    double xd, yd;
    fe_forward(a, x, y, &xd, &yd);
    const double ex = (xd - x0) * fx, ey = (yd - y0) * fy;
    const double res = sqrt(ex * ex + ey * ey);
    *xo = x;
    *yo = y;
    return fin(r) && r <= A3_FISHEYE_START_MAX_R && res <= 0.1;
}

/* the model and its 14 Jacobian columns; column 14 the residual */
static void fisheye_row(const double a[8], const double R[9], const double t[3], double X, double Y, double ou, double ov, double *au, double *av) {
    const double fx = a[0], fy = a[1], cx = a[2], cy = a[3], k1 = a[4], k2 = a[5], k3 = a[6], k4 = a[7];
    const double qx = R[0] * X + R[1] * Y, qy = R[3] * X + R[4] * Y, qz = R[6] * X + R[7] * Y;
    const double px = qx + t[0], py = qy + t[1], pz = qz + t[2];
    const double ia = 1.0 / pz;
    const double x = px * ia, y = py * ia;
    const double r2 = x * x + y * y;
    const double r = sqrt(r2);
    const double th = a64(r), t2 = th * th;
    const double poly = 1.0 + (((k4 * t2 + k3) * t2 + k2) * t2 + k1) * t2;
    const double thd = th * poly;
    const double s = r > 0.0 ? thd / r : 1.0;
    const double xd = x * s, yd = y * s;
    au[14] = (fx * xd + cx) - ou;
    av[14] = (fy * yd + cy) - ov;
    const double e = r > 0.0 ? th / r : 1.0;
    const double gx = fx * x * e, gy = fy * y * e;
    const double t4 = t2 * t2, t6 = t4 * t2, t8 = t6 * t2;
    au[0] = xd;  au[1] = 0.0; au[2] = 1.0; au[3] = 0.0;
    av[0] = 0.0; av[1] = yd;  av[2] = 0.0; av[3] = 1.0;
    au[4] = gx * t2; au[5] = gx * t4; au[6] = gx * t6; au[7] = gx * t8;
    av[4] = gy * t2; av[5] = gy * t4; av[6] = gy * t6; av[7] = gy * t8;
    const double dpoly = 1.0 + (((9.0 * k4 * t2 + 7.0 * k3) * t2 + 5.0 * k2) * t2 + 3.0 * k1) * t2;
    const double c = r > 0.0 ? (dpoly / (1.0 + r2) - s) / r2 : 0.0;
    const double xxd = s + x * x * c, xyd = x * y * c, yyd = s + y * y * c;
    const double cu = fx * ia, cv = fy * ia;
    const double u0 = cu * xxd, u1 = cu * xyd, u2 = -(cu * (xxd * x + xyd * y));
    const double v0 = cv * xyd, v1 = cv * yyd, v2 = -(cv * (xyd * x + yyd * y));
    const double q2x = 2.0 * qx, q2y = 2.0 * qy, q2z = 2.0 * qz;
    au[8] = u2 * q2y - u1 * q2z; au[9] = u0 * q2z - u2 * q2x; au[10] = u1 * q2x - u0 * q2y;
    av[8] = v2 * q2y - v1 * q2z; av[9] = v0 * q2z - v2 * q2x; av[10] = v1 * q2x - v0 * q2y;
    au[11] = u0; au[12] = u1; au[13] = u2;
    av[11] = v0; av[12] = v1; av[13] = v2;
}

static int ldl6(const double *blk, double lambda, double L[6][6], double D[6]) {
    double A[6][6];
    for (int r = 0; r < 6; r++)
        for (int c = r; c < 6; c++) { const double v = blk[tri_index(PO + r, PO + c, AUG)]; A[r][c] = v; A[c][r] = v; }
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

static void view_block(const double a[8], const double R[9], const double t[3], const float *obj, const float *img, uint32_t p0, uint32_t np,
                       double out[NENT]) {
    double au[AUG], av[AUG];
    for (int e = 0; e < NENT; e++) out[e] = 0.0;
    for (uint32_t j = 0; j < np; j++) {
        const size_t p = (size_t)p0 + j;
        fisheye_row(a, R, t, (double)obj[2 * p], (double)obj[2 * p + 1], (double)img[2 * p], (double)img[2 * p + 1], au, av);
        for (int e = 0; e < NENT; e++) {
            int i, k;
            tri_ik(e, AUG, &i, &k);
            out[e] = out[e] + au[i] * au[k];
            out[e] = out[e] + av[i] * av[k];
        }
    }
}

/* step 1 of the calibration contract: -> 1 and H (row-major, H22 = 1), or 0 (DEGENERATE) */
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

static int ldl_n(double A[8][8], int n, double D[8]) {
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

static void ldl_n_solve(double A[8][8], int n, const double D[8], const double b[8], double x[8]) {
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
    double con[44];
    double H[9];
} View;

static int fe_free(uint32_t flags, int i) {
    if (i == 2 || i == 3) return !(flags & A3_FISHEYE_FIX_PRINCIPAL_POINT);
    if (i >= 4) return !(flags & (A3_FISHEYE_FIX_K1 << (i - 4)));
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
            for (int m = 0; m < 6; m++) b[m] = c < nf ? blk[tri_index(fr[c], PO + m, AUG)] : blk[tri_index(PO + m, RC, AUG)];
            ldl6_solve(L, D, b, y);
            for (int k = c < nf ? c : 0; k < nf; k++) {
                double s = 0.0;
                for (int m = 0; m < 6; m++) s = s + blk[tri_index(fr[k], PO + m, AUG)] * y[m];
                V->con[c < nf ? tri_index(c, k, nf) : nt + k] = s;
            }
        }
    }
    return ok;
}

static void schur_matrix(const View *vs, const a3_calib_view *views, uint32_t v0, uint32_t nv, int nf, const double *U, double lambda,
                         double S[8][8], double rhs[8]) {
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
        } else idx = tri_index(fr[e - nt], RC, AUG);
        double s = 0.0;
        for (uint32_t j = 0; j < nv; j++)
            if (views[v0 + j].status == A3_CALIB_VIEW_USED) s = s + vs[v0 + j].blk[slot][idx];
        U[e] = s;
    }
}

/* where parameter i (fx fy cx cy k1 k2 k3 k4) sits in a3_calib_result.std_dev and, less 4, in .dist */
static int out_index(int i) { return i < 6 ? i : i + 2; }

static void calibrate_one(const a3_calib_camera *C, const uint32_t *off, const float *obj, const float *img, float *sobj, float *simg, View *vs,
                          a3_calib_result *res, a3_calib_view *views) {
    const uint32_t v0 = C->first_view, nv = C->n_views;
    int fr[8], nf = 0;
    for (int i = 0; i < 8; i++)
        if (fe_free(C->flags, i)) fr[nf++] = i;
    /* 1: the start */
    double a[8] = {0};
    if (C->flags & A3_FISHEYE_USE_INTRINSIC_GUESS) {
        const a3_distortion *d = &C->guess_distortion;
        a[0] = C->guess.focal_x; a[1] = C->guess.focal_y; a[2] = C->guess.principal_x; a[3] = C->guess.principal_y;
        a[4] = d->k1; a[5] = d->k2; a[6] = d->k3; a[7] = d->k4;
    } else {
        const double W = (double)C->image_width, Hh = (double)C->image_height;
        const double f = (W > Hh ? W : Hh) / 3.141592653589793;
        a[0] = f; a[1] = f; a[2] = (W - 1.0) * 0.5; a[3] = (Hh - 1.0) * 0.5;
    }
    /* 2: per view, the start's points, the homography to the normalised plane */
    for (uint32_t j = 0; j < nv; j++) {
        const uint32_t v = v0 + j, p0 = off[v], np = off[v + 1] - p0;
        a3_calib_view *rec = &views[v];
        memset(rec, 0, sizeof *rec);
        rec->points = np;
        if (np < 4) { rec->status = A3_CALIB_VIEW_TOO_FEW_POINTS; continue; }
        uint32_t nk = 0;
        for (uint32_t q = 0; q < np; q++) {
            const size_t p = (size_t)p0 + q;
            double x, y;
            if (!fe_start_point(a, (double)img[2 * p], (double)img[2 * p + 1], &x, &y)) continue;
            const size_t o = (size_t)p0 + nk;
            sobj[2 * o] = obj[2 * p]; sobj[2 * o + 1] = obj[2 * p + 1];
            simg[2 * o] = (float)x; simg[2 * o + 1] = (float)y;
            nk++;
        }
        rec->status = nk >= 4 && view_homography(sobj, simg, p0, nk, vs[v].H) ? A3_CALIB_VIEW_USED : A3_CALIB_VIEW_DEGENERATE;
    }
    uint32_t vu = 0, n = 0;
    for (uint32_t j = 0; j < nv; j++)
        if (views[v0 + j].status == A3_CALIB_VIEW_USED) { vu++; n += views[v0 + j].points; }
    int status = A3_CALIB_OK;
    if (vu == 0 || 2ll * n - nf - 6ll * vu <= 0) status = A3_CALIB_TOO_FEW;
    double cost = 0.0, lambda = 1e-3, std[8] = {0};
    int iter = 0, conv = 0, cur = 0;
    const int maxit = C->max_iterations ? (int)C->max_iterations : A3_CALIB_DEFAULT_ITERATIONS;
    if (status == A3_CALIB_OK) {
        for (uint32_t j = 0; j < nv; j++) {
            const uint32_t v = v0 + j;
            if (views[v].status != A3_CALIB_VIEW_USED) continue;
            const uint32_t p0 = off[v], np = off[v + 1] - p0;
            View *V = &vs[v];
            const double *H = V->H;
            double m[3][3];
            for (int c = 0; c < 3; c++) { m[c][0] = H[c]; m[c][1] = H[3 + c]; m[c][2] = H[6 + c]; }
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
                for (int q = 0; q < 6; q++) b[q] = -pc[tri_index(PO + q, RC, AUG)];
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
        /* 3 */
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
        double U[44], S[8][8], rhs[8], Dg[8], da[8], an[8];
        int stop = 0, sums = 1;
        if (cost == 0.0) { stop = 1; conv = 1; }
        /* 4 */
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
                    for (int k = 0; k < nf; k++) s = s + blk[tri_index(fr[k], PO + q, AUG)] * da[k];
                    b[q] = -blk[tri_index(PO + q, RC, AUG)] - s;
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
                double e[8], x[8];
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
        for (int i = 4; i < 8; i++) res->dist[out_index(i) - 4] = a[i];
        for (int i = 0; i < 8; i++) res->std_dev[out_index(i)] = std[i];
        res->rms_px = sqrt(cost / (double)n);
        res->intrinsics.image_width = C->image_width;
        res->intrinsics.image_height = C->image_height;
        res->intrinsics.focal_x = (float)a[0]; res->intrinsics.focal_y = (float)a[1];
        res->intrinsics.principal_x = (float)a[2]; res->intrinsics.principal_y = (float)a[3];
        res->distortion.model = A3_DIST_FISHEYE;
        res->distortion.iterations = 20;
        res->distortion.k1 = (float)a[4]; res->distortion.k2 = (float)a[5]; res->distortion.k3 = (float)a[6]; res->distortion.k4 = (float)a[7];
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

/* a3_calibrate_fisheye_cameras on valid input (the argument checks are the library's); views must hold n_views records */
int a3o_calibrate_fisheye(const a3_calib_camera *cams, size_t n_cams, const uint32_t *view_offsets, size_t n_views, const float *object_xy,
                          const float *image_xy, a3_calib_result *results, a3_calib_view *views) {
    const size_t n_pts = view_offsets[n_views];
    View *vs = (View *)calloc(n_views, sizeof(View));
    float *start = (float *)calloc(4 * n_pts + 1, sizeof(float));
    if (!vs || !start) { free(vs); free(start); return -1; }
    memset(views, 0, n_views * sizeof *views);
    for (size_t c = 0; c < n_cams; c++)
        calibrate_one(&cams[c], view_offsets, object_xy, image_xy, start, start + 2 * n_pts, vs, &results[c], views);
    free(vs);
    free(start);
    return 0;
}

double a3o_a64(double t) { return a64(t); }

/* one point's two augmented rows (15 each) */
void a3o_fisheye_calib_row(const double *a, const double *R, const double *t, double X, double Y, double u, double v, double *au, double *av) {
    fisheye_row(a, R, t, X, Y, u, v, au, av);
}

/* the forward model in f64 (test data): n board points (x, y) -> pixels through a (8 intrinsics) and (R, t) */
void a3o_fisheye_calib_project(const double *a, const double *R, const double *t, const double *xy, size_t n, double *out) {
    double au[AUG], av[AUG];
    for (size_t i = 0; i < n; i++) {
        fisheye_row(a, R, t, xy[2 * i], xy[2 * i + 1], 0.0, 0.0, au, av);
        out[2 * i] = au[RC];
        out[2 * i + 1] = av[RC];
    }
}

/* step 2's start points of one view: n image points -> kept flags and normalised points (as float) */
void a3o_fisheye_calib_start(const double *a, const float *img, size_t n, int *kept, float *xy) {
    for (size_t i = 0; i < n; i++) {
        double x, y;
        kept[i] = fe_start_point(a, (double)img[2 * i], (double)img[2 * i + 1], &x, &y);
        xy[2 * i] = (float)x;
        xy[2 * i + 1] = (float)y;
    }
}

/* layout of the ABI structs as this compiler sees the header */
void a3o_fisheye_calib_layout(size_t *out) {
    out[0] = sizeof(a3_calib_camera); out[1] = offsetof(a3_calib_camera, guess); out[2] = offsetof(a3_calib_camera, guess_distortion);
    out[3] = sizeof(a3_calib_result); out[4] = offsetof(a3_calib_result, fx); out[5] = offsetof(a3_calib_result, dist);
    out[6] = offsetof(a3_calib_result, std_dev); out[7] = offsetof(a3_calib_result, rms_px); out[8] = offsetof(a3_calib_result, intrinsics);
    out[9] = offsetof(a3_calib_result, distortion); out[10] = sizeof(a3_calib_view); out[11] = offsetof(a3_calib_view, rms_px);
    out[12] = offsetof(a3_calib_view, rotation); out[13] = offsetof(a3_calib_view, translation);
}
