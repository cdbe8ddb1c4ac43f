/* calib_oracle.c -- the CPU restatement of the camera calibration of include/aruco3_hip.h (a3_calibrate_cameras) that the device kernel
 * k_calibrate is held to bit for bit.  One camera at a time, one view at a time, in the contract's order of operations: every sum over
 * a view's points in point order, every sum over views in view order.  The solver pieces are solve_oracle.h's, the rational model's
 * row is calib_model.h's and the pose and joint LM are calib_driver.h's; what is written out here is the closed-form start, the guess
 * handling and the model's result fields.  Compiled with -ffp-contract=off (tests/oracle_build.py).  TEST INFRASTRUCTURE ONLY. */
#include "calib_driver.h"
#include "calib_model.h"

static int cal_free(uint32_t flags, int i) {
    if (i == 2 || i == 3) return !(flags & A3_CALIB_FIX_PRINCIPAL_POINT);
    if (i == 6 || i == 7) return !(flags & A3_CALIB_ZERO_TANGENT_DIST);
    if (i == 8) return !(flags & A3_CALIB_FIX_K3);
    if (i >= 9) return (flags & A3_CALIB_RATIONAL_MODEL) != 0;
    return 1;
}

static const CalModel RATIONAL = {12, AUG, 12, 18, calib_row, cal_free};

/* the closed-form focal lengths from the used views' homographies, the principal point at the centre; -> 0 (NO_INIT) */
static int focal_start(const a3_calib_camera *C, const View *vs, const a3_calib_view *views, double *a) {
    const double cx = ((double)C->image_width - 1.0) * 0.5, cy = ((double)C->image_height - 1.0) * 0.5;
    double A00 = 0.0, A01 = 0.0, A11 = 0.0, b0 = 0.0, b1 = 0.0;
    for (uint32_t j = 0; j < C->n_views; j++) {
        if (views[C->first_view + j].status != A3_CALIB_VIEW_USED) continue;
        const double *H = vs[C->first_view + j].H;
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
    a[0] = fx; a[1] = fy; a[2] = cx; a[3] = cy;
    return det > 1e-9 * (A00 * A11) && fx > 0.0 && fin(fx) && fy > 0.0 && fin(fy);
}

static void calibrate_one(const a3_calib_camera *C, const uint32_t *off, const float *obj, const float *img, View *vs, a3_calib_result *res,
                          a3_calib_view *views) {
    const uint32_t v0 = C->first_view, nv = C->n_views;
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
    CalState s;
    calib_begin(&RATIONAL, C, views, &s);
    double a[12] = {0};
    if (s.status == A3_CALIB_OK && (C->flags & A3_CALIB_USE_INTRINSIC_GUESS)) {
        const a3_distortion *d = &C->guess_distortion;
        a[0] = C->guess.focal_x; a[1] = C->guess.focal_y; a[2] = C->guess.principal_x; a[3] = C->guess.principal_y;
        a[4] = d->k1; a[5] = d->k2; a[6] = d->p1; a[7] = d->p2; a[8] = d->k3; a[9] = d->k4; a[10] = d->k5; a[11] = d->k6;
        if (C->flags & A3_CALIB_ZERO_TANGENT_DIST) { a[6] = 0.0; a[7] = 0.0; }
        if (!(C->flags & A3_CALIB_RATIONAL_MODEL)) { a[9] = 0.0; a[10] = 0.0; a[11] = 0.0; }
    } else if (s.status == A3_CALIB_OK && !focal_start(C, vs, views, a)) s.status = A3_CALIB_NO_INIT;
    /* 3 to 5 */
    for (uint32_t j = 0; j < nv && s.status == A3_CALIB_OK; j++) {
        if (views[v0 + j].status != A3_CALIB_VIEW_USED) continue;
        double m[3][3];
        h_columns(a, vs[v0 + j].H, m);
        pose_from_h(m, vs[v0 + j].pose[0], vs[v0 + j].pose[0] + 9);
    }
    calib_solve(&RATIONAL, C, off, obj, img, vs, views, a, &s);
    if (!calib_results(&RATIONAL, C, &s, a, vs, res, views)) return;
    for (int i = 0; i < 8; i++) res->dist[i] = a[4 + i];
    for (int i = 0; i < 12; i++) res->std_dev[i] = s.std[i];
    res->distortion.model = A3_DIST_RATIONAL;
    res->distortion.k1 = (float)a[4]; res->distortion.k2 = (float)a[5]; res->distortion.p1 = (float)a[6]; res->distortion.p2 = (float)a[7];
    res->distortion.k3 = (float)a[8]; res->distortion.k4 = (float)a[9]; res->distortion.k5 = (float)a[10]; res->distortion.k6 = (float)a[11];
}

/* a3_calibrate_cameras on valid input (the argument checks are the library's); views must hold n_views records */
int a3o_calibrate(const a3_calib_camera *cams, size_t n_cams, const uint32_t *view_offsets, size_t n_views, const float *object_xy,
                  const float *image_xy, a3_calib_result *results, a3_calib_view *views) {
    View *vs = (View *)calloc(n_views, sizeof(View));
    if (!vs) return -1;
    for (size_t c = 0; c < n_cams; c++) calibrate_one(&cams[c], view_offsets, object_xy, image_xy, vs, &results[c], views);
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
