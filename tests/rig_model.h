/* rig_model.h -- the rig's pose algebra and its row of 13 through E . T, which the marker map and the hand-eye oracles build on too,
 * and the step all three share: one observation's pose from its homography and the pose LM.  TEST INFRASTRUCTURE ONLY. */
#ifndef A3_RIG_MODEL_H
#define A3_RIG_MODEL_H
#include "calib_model.h"

#define RAUG 13    /* 6 columns of the left pose, 6 of the right, the residual */
#define RENT 91

static const double POSE_ID[12] = {1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0, 1.0, 0.0, 0.0, 0.0};

static inline void pose_mul(const double *A, const double *B, double *O) {   /* poses as R (9), t (3) */
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) O[3 * r + c] = (A[3 * r] * B[c] + A[3 * r + 1] * B[3 + c]) + A[3 * r + 2] * B[6 + c];
        O[9 + r] = ((A[3 * r] * B[9] + A[3 * r + 1] * B[10]) + A[3 * r + 2] * B[11]) + A[9 + r];
    }
}

static inline void pose_inv(const double *A, double *O) {
    for (int r = 0; r < 3; r++) {
        for (int c = 0; c < 3; c++) O[3 * r + c] = A[3 * c + r];
        O[9 + r] = -((A[r] * A[9] + A[3 + r] * A[10]) + A[6 + r] * A[11]);
    }
}

static inline void rig_cols(const double u[3], const double Rc[9], const double qc[3], const double qf[3], double res, double *o) {
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
typedef struct RigAt {
    const double *a, *E, *T, *G;
} RigAt;

static inline void rig_row(const void *ctx, double X, double Y, double ou, double ov, double *au, double *av) {
    const RigAt *g = (const RigAt *)ctx;
    const double *E = g->E, *T = g->T;
    double cu[AUG], cv[AUG];
    calib_row(g->a, g->G, g->G + 9, X, Y, ou, ov, cu, cv);
    const double qf[3] = {T[0] * X + T[1] * Y, T[3] * X + T[4] * Y, T[6] * X + T[7] * Y};
    const double y[3] = {qf[0] + T[9], qf[1] + T[10], qf[2] + T[11]};
    double qc[3];
    for (int r = 0; r < 3; r++) qc[r] = (E[3 * r] * y[0] + E[3 * r + 1] * y[1]) + E[3 * r + 2] * y[2];
    rig_cols(cu + 15, E, qc, qf, cu[18], au);
    rig_cols(cv + 15, E, qc, qf, cv[18], av);
}

static inline void obs_block(const double *a, const double *E, const double *T, const double *G, const float *obj, const float *img, uint32_t p0,
                             uint32_t np, double *out) {
    const RigAt g = {a, E, T, G};
    const Points P = {obj, img, p0, np};
    aug_block(rig_row, &g, RAUG, &P, out);
}

/* one observation on its own: E the identity, so the pose sits in columns 6-11 */
typedef struct ObsAlone {
    const double *a;
    Points pts;
} ObsAlone;

static inline void obs_alone_block(const void *ctx, const double *T, double *out) {
    const ObsAlone *o = (const ObsAlone *)ctx;
    obs_block(o->a, POSE_ID, T, T, o->pts.obj, o->pts.img, o->pts.p0, o->pts.np, out);
}

/* the pose start of step 1 from the observation's homography */
static inline void obs_pose_start(const double *a, const double H[9], double *T) {
    double m[3][3];
    h_columns(a, H, m);
    pose_from_h(m, T, T + 9);
}

/* the pose LM of step 1: T in / out -> the cost */
static inline double obs_pose_lm(const double *a, const float *obj, const float *img, uint32_t p0, uint32_t np, double *T) {
    const ObsAlone o = {a, {obj, img, p0, np}};
    return pose_lm(obs_alone_block, &o, 6, RAUG, T);
}

#endif
