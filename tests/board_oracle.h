/* tests/board_oracle.h -- what board_oracle.c shares with charuco_oracle.c, which is compiled beside it: the records, one frame's
 * view of a board, the residual sums of one correspondence, the 64-lane reduction and the LM loop.  TEST INFRASTRUCTURE ONLY. */
#ifndef A3_BOARD_ORACLE_H
#define A3_BOARD_ORACLE_H
#include <stdint.h>

#define A3O_MAX_EVALS 30
#define A3O_REL_TOL 1e-6f
#define A3O_MAX_MARKERS 1024

typedef struct a3o_pose { float error; float rotation[9]; float translation[3]; } a3o_pose;
typedef struct a3o_board_rec {   /* the layout of a3_board_pose */
    uint32_t status, markers_used, markers_rejected, iterations;
    float rms_px, alt_rms_px, rotation[9], translation[3];
} a3o_board_rec;
typedef struct a3o_slot { float x[4], y[4], side, cs, sn, cx, cy; } a3o_slot;

typedef struct {
    const uint32_t* ids; const float* px; uint32_t cnt;   /* the frame's markers, batch order; pixel corners */
    const uint32_t* board_ids; a3o_slot* slots; uint32_t n_slots;
    const uint8_t* dup;
    int has_intr; float iw, ih, fx, fy, cx, cy, sx, sy;
} frame_t;

typedef struct { float h[21], g[6], cost, pix; } acc_t;

/* the sums of a frame's correspondences at (R, t), from the problem in ctx */
typedef void (*a3o_eval_fn)(const void* ctx, const float R[9], const float t[3], acc_t* out);

void a3o_slot_from(const float xy[8], a3o_slot* s);
void a3o_normalise(const frame_t* F, float x, float y, float* u, float* v);
void a3o_accum(acc_t* s, const float R[9], const float t[3], float bx, float by, float mx, float my, float sx, float sy);
void a3o_reduce64(acc_t lanes[64], acc_t* out);
void a3o_cayley(const float w[3], const float R[9], float Rn[9]);
uint32_t a3o_lm(a3o_eval_fn eval, const void* ctx, float R[9], float t[3], float* cost, float* pix);
int a3o_board_pose(const uint32_t* board_ids, const float* board_xy, uint32_t n_board, const uint32_t* ids, const float* px, uint32_t cnt,
                   const float* intr, uint32_t w, uint32_t h, a3o_board_rec* out, float* start_out);

#endif
