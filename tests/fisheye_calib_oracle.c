/* fisheye_calib_oracle.c -- the CPU restatement of the fisheye camera calibration of include/aruco3_hip.h
 * (a3_calibrate_fisheye_cameras) that the device kernel k_calibrate_fisheye is held to bit for bit.  One camera at a time, one view at
 * a time, in the contract's order of operations: every sum over a view's points in point order, every sum over views in view order.
 * The solver pieces are solve_oracle.h's and the pose and joint LM are calib_driver.h's; what is written out here is the fisheye
 * model's row, the start with its kept-point rule and the model's result fields.  Compiled with -ffp-contract=off
 * (tests/oracle_build.py).  No math function but sqrt and fabs: the arctangent is a64 below.  TEST INFRASTRUCTURE ONLY. */
#include "calib_driver.h"

#define AUG 15    /* 8 intrinsics (fx fy cx cy k1 k2 k3 k4), w, t, the residual */
#define PO 8      /* first pose column */
#define RC 14     /* the residual's column */

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

static int fe_free(uint32_t flags, int i) {
    if (i == 2 || i == 3) return !(flags & A3_FISHEYE_FIX_PRINCIPAL_POINT);
    if (i >= 4) return !(flags & (A3_FISHEYE_FIX_K1 << (i - 4)));
    return 1;
}

static const CalModel FISHEYE = {8, AUG, PO, RC, fisheye_row, fe_free};

/* where parameter i (fx fy cx cy k1 k2 k3 k4) sits in a3_calib_result.std_dev and, less 4, in .dist */
static int out_index(int i) { return i < 6 ? i : i + 2; }

static void calibrate_one(const a3_calib_camera *C, const uint32_t *off, const float *obj, const float *img, float *sobj, float *simg, View *vs,
                          a3_calib_result *res, a3_calib_view *views) {
    const uint32_t v0 = C->first_view, nv = C->n_views;
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
    CalState s;
    calib_begin(&FISHEYE, C, views, &s);
    /* 3 to 5; the homography already maps to the normalised plane, so its columns are the pose start's m */
    for (uint32_t j = 0; j < nv && s.status == A3_CALIB_OK; j++) {
        if (views[v0 + j].status != A3_CALIB_VIEW_USED) continue;
        const double *H = vs[v0 + j].H;
        double m[3][3];
        for (int c = 0; c < 3; c++) { m[c][0] = H[c]; m[c][1] = H[3 + c]; m[c][2] = H[6 + c]; }
        pose_from_h(m, vs[v0 + j].pose[0], vs[v0 + j].pose[0] + 9);
    }
    calib_solve(&FISHEYE, C, off, obj, img, vs, views, a, &s);
    if (!calib_results(&FISHEYE, C, &s, a, vs, res, views)) return;
    for (int i = 4; i < 8; i++) res->dist[out_index(i) - 4] = a[i];
    for (int i = 0; i < 8; i++) res->std_dev[out_index(i)] = s.std[i];
    res->distortion.model = A3_DIST_FISHEYE;
    res->distortion.k1 = (float)a[4]; res->distortion.k2 = (float)a[5]; res->distortion.k3 = (float)a[6]; res->distortion.k4 = (float)a[7];
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
