/* solve_oracle.h -- what the f64 solver oracles (calib_, fisheye_calib_, rig_, map_ and handeye_oracle.c) share, each piece once: the
 * CPU counterpart of aruco3_amd/csrc/a3_solve.h.  The contract is "every expression in the order the public header states", so the
 * order of operations in here is part of what the device kernels are held to bit for bit; compile with -ffp-contract=off
 * (tests/oracle_build.py).  Functions are static inline so that an oracle that does not use one stays free of warnings.
 * TEST INFRASTRUCTURE ONLY. */
#ifndef A3_SOLVE_ORACLE_H
#define A3_SOLVE_ORACLE_H
#include <math.h>
#include <stddef.h>
#include <stdint.h>
#include <stdlib.h>
#include <string.h>

#include "../include/aruco3_hip.h"

#define MAX_AUG 19    /* the widest augmented row: the rational model's */
#define MAX_NENT 190

/* entry (i, k), i <= k, of the upper triangle of an n x n matrix stored row by row, and back */
static inline int tri_index(int i, int k, int n) { return i * n - (i * (i - 1)) / 2 + (k - i); }

static inline void tri_ik(int e, int n, int *i, int *k) {
    int r = 0;
    while (e >= n - r) { e -= n - r; r++; }
    *i = r;
    *k = r + e;
}

static inline int fin(double v) { return isfinite(v) != 0; }

/* LDL^T of V + lambda diag(V), V the 6 x 6 block at columns off .. off + 5 of an aug-triangle */
static inline int ldl6_at(const double *blk, int off, int aug, double lambda, double L[6][6], double D[6]) {
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

static inline void ldl6_solve(double L[6][6], const double D[6], const double b[6], double x[6]) {
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

/* LDL^T in place in the lower triangle of the n x n matrix A (row-major, `stride` doubles a row); 0 on a bad pivot */
static inline int ldl_n(double *A, int stride, int n, double *D) {
    for (int j = 0; j < n; j++)
        for (int i = j; i < n; i++) {
            double s = A[(size_t)i * stride + j];
            for (int k = 0; k < j; k++) s = s - A[(size_t)i * stride + k] * A[(size_t)j * stride + k] * D[k];
            if (i == j) {
                if (!(s > 0.0) || !fin(s)) return 0;
                D[j] = s;
            } else A[(size_t)i * stride + j] = s / D[j];
        }
    return 1;
}

/* x may be b.  `down`: the back substitution subtracts its terms from column n - 1 down to i + 1 (the marker map's contract);
 * otherwise from i + 1 up (every other solver's) */
static inline void ldl_n_solve(const double *A, int stride, int n, const double *D, const double *b, double *x, int down) {
    for (int i = 0; i < n; i++) {
        double s = b[i];
        for (int k = 0; k < i; k++) s = s - A[(size_t)i * stride + k] * x[k];
        x[i] = s;
    }
    for (int i = n - 1; i >= 0; i--) {
        double s = x[i] / D[i];
        if (down)
            for (int k = n - 1; k > i; k--) s = s - A[(size_t)k * stride + i] * x[k];
        else
            for (int k = i + 1; k < n; k++) s = s - A[(size_t)k * stride + i] * x[k];
        x[i] = s;
    }
}

/* Rn = cay(w) R */
static inline void cayley_d(const double w[3], const double R[9], double Rn[9]) {
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

/* poses are 12 doubles: R row-major (9), t (3).  Tn = T moved by the step d = (w, dt) */
static inline void pose_update(const double *T, const double d[6], double *Tn) {
    cayley_d(d, T, Tn);
    for (int q = 0; q < 3; q++) Tn[9 + q] = T[9 + q] + d[3 + q];
}

/* a range of planar correspondences: points p0 .. p0 + np - 1 of obj (x, y) and img (u, v) */
typedef struct Points {
    const float *obj, *img;
    uint32_t p0, np;
} Points;

/* the calibration contract's step 1: -> 1 and H (row-major, H22 = 1), or 0 (DEGENERATE) */
static inline int view_homography(const float *obj, const float *img, uint32_t p0, uint32_t np, double H[9]) {
    enum { HAUG = 9, HENT = 45 };
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

/* m[c] = column c of K^-1 H for the pinhole K of a = (fx, fy, cx, cy, ...) */
static inline void h_columns(const double *a, const double H[9], double m[3][3]) {
    for (int c = 0; c < 3; c++) {
        m[c][0] = (H[c] - a[2] * H[6 + c]) / a[0];
        m[c][1] = (H[3 + c] - a[3] * H[6 + c]) / a[1];
        m[c][2] = H[6 + c];
    }
}

/* the pose start from the columns of a homography to the normalised plane */
static inline void pose_from_h(double m[3][3], double R[9], double t[3]) {
    const double n0 = sqrt((m[0][0] * m[0][0] + m[0][1] * m[0][1]) + m[0][2] * m[0][2]);
    const double r00 = m[0][0] / n0, r01 = m[0][1] / n0, r02 = m[0][2] / n0;
    const double dd = (r00 * m[1][0] + r01 * m[1][1]) + r02 * m[1][2];
    const double e0 = m[1][0] - dd * r00, e1 = m[1][1] - dd * r01, e2 = m[1][2] - dd * r02;
    const double ne = sqrt((e0 * e0 + e1 * e1) + e2 * e2);
    const double r10 = e0 / ne, r11 = e1 / ne, r12 = e2 / ne;
    const double n1 = sqrt((m[1][0] * m[1][0] + m[1][1] * m[1][1]) + m[1][2] * m[1][2]);
    const double den = n0 + n1;
    const double Rs[9] = {r00, r10, r01 * r12 - r02 * r11, r01, r11, r02 * r10 - r00 * r12, r02, r12, r00 * r11 - r01 * r10};
    memcpy(R, Rs, sizeof Rs);
    for (int q = 0; q < 3; q++) t[q] = (2.0 * m[2][q]) / den;
}

/* one point's two augmented rows (aug entries each, the last the residual) from a model in ctx */
typedef void (*row_fn)(const void *ctx, double X, double Y, double ou, double ov, double *au, double *av);

/* out = the upper triangle (row by row) of the sum over the points, in point order, of au au^T then av av^T */
static inline void aug_block(row_fn row, const void *ctx, int aug, const Points *P, double *out) {
    const int nent = aug * (aug + 1) / 2;
    double au[MAX_AUG], av[MAX_AUG];
    for (int e = 0; e < nent; e++) out[e] = 0.0;
    for (uint32_t j = 0; j < P->np; j++) {
        const size_t p = (size_t)P->p0 + j;
        row(ctx, (double)P->obj[2 * p], (double)P->obj[2 * p + 1], (double)P->img[2 * p], (double)P->img[2 * p + 1], au, av);
        for (int e = 0; e < nent; e++) {
            int i, k;
            tri_ik(e, aug, &i, &k);
            out[e] = out[e] + au[i] * au[k];
            out[e] = out[e] + av[i] * av[k];
        }
    }
}

/* the aug-triangle of the problem in ctx at `pose` */
typedef void (*block_fn)(const void *ctx, const double *pose, double *out);

/* The pose-only Levenberg-Marquardt loop: at most A3_CALIB_POSE_EVALS evaluations (a failed factorisation counts as one) of
 * `block`, whose pose columns are off .. off + 5 and whose residual column is aug - 1.  pose in / out -> its cost.  The two blocks
 * the loop swaps between are its own: every caller evaluates again at the pose it gets back. */
static inline double pose_lm(block_fn block, const void *ctx, int off, int aug, double *pose) {
    const int cost_at = aug * (aug + 1) / 2 - 1;
    double b0[MAX_NENT], b1[MAX_NENT], *pc = b0, *po = b1;
    block(ctx, pose, pc);
    double c1 = pc[cost_at], lam = 1e-3;
    int evals = 1;
    while (evals < A3_CALIB_POSE_EVALS && c1 > 0.0) {
        double L[6][6], D[6];
        if (!ldl6_at(pc, off, aug, lam, L, D)) { lam = lam * 10.0; evals++; continue; }
        double b[6], d[6], Tn[12];
        for (int q = 0; q < 6; q++) b[q] = -pc[tri_index(off + q, aug - 1, aug)];
        ldl6_solve(L, D, b, d);
        pose_update(pose, d, Tn);
        block(ctx, Tn, po);
        evals++;
        const double c2 = po[cost_at];
        if (c2 < c1) {
            const double rel = (c1 - c2) / c1;
            memcpy(pose, Tn, sizeof Tn);
            double *s = pc; pc = po; po = s;
            c1 = c2;
            lam = lam / 10.0;
            if (rel < A3_CALIB_REL_TOL) break;
        } else lam = lam * 10.0;
    }
    return c1;
}

#endif
