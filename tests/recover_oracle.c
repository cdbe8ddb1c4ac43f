/* recover_oracle.c -- the CPU restatement of the board-aided marker recovery (a3_set_board_recovery / a3_recover_markers,
 * include/aruco3_hip.h) that the device kernel k_recover_frames is held to, bit for bit: steps 1-5 of the contract for one frame, in
 * the contract's order of operations.  The homography is the calibration contract's step 1 (solve_oracle.h view_homography).
 * Compile with -ffp-contract=off (tests/oracle_build.py).  TEST INFRASTRUCTURE ONLY. */
#include "calib_model.h"

#define NO_SLOT 0xFFFFFFFFu
#define NO_PICK 0xFFFFFFFFu

static uint32_t slot_of(const uint32_t *board_ids, uint32_t nb, uint32_t id) {
    for (uint32_t s = 0; s < nb; s++)
        if (board_ids[s] == id) return s;
    return NO_SLOT;
}

static int popcount64(uint64_t v) {
    int n = 0;
    while (v) { v &= v - 1; n++; }
    return n;
}

/* step 1: seen[s] = instances of slot s in the frame; -> 1 and H, or 0 (fewer than min_markers usable markers, or DEGENERATE) */
static int frame_homography(const uint32_t *board_ids, const float *board_xy, uint32_t nb, const uint32_t *det_ids, const uint32_t *det_xy,
                            uint32_t nd, uint32_t min_markers, uint32_t *seen, double H[9]) {
    for (uint32_t s = 0; s < nb; s++) seen[s] = 0;
    for (uint32_t i = 0; i < nd; i++) {
        const uint32_t s = slot_of(board_ids, nb, det_ids[i]);
        if (s != NO_SLOT) seen[s]++;
    }
    float *obj = (float *)malloc(sizeof(float) * 8 * (size_t)(nb ? nb : 1)), *img = (float *)malloc(sizeof(float) * 8 * (size_t)(nb ? nb : 1));
    uint32_t k = 0;
    for (uint32_t i = 0; i < nd; i++) {
        const uint32_t s = slot_of(board_ids, nb, det_ids[i]);
        if (s == NO_SLOT || seen[s] != 1) continue;
        for (int j = 0; j < 8; j++) { obj[8 * k + j] = board_xy[8 * (size_t)s + j]; img[8 * k + j] = (float)det_xy[8 * (size_t)i + j]; }
        k++;
    }
    int ok = 0;
    if (k >= 1 && k >= min_markers) ok = view_homography(obj, img, 0, 4 * k, H);
    free(obj); free(img);
    return ok;
}

/* step 2 */
static int expected_corners(const double H[9], const float *xy, double e[8]) {
    int ok = 1;
    for (int j = 0; j < 4; j++) {
        const double X = (double)xy[2 * j], Y = (double)xy[2 * j + 1];
        const double u = (H[0] * X + H[1] * Y) + H[2];
        const double v = (H[3] * X + H[4] * Y) + H[5];
        const double w = (H[6] * X + H[7] * Y) + H[8];
        const double ex = u / w, ey = v / w;
        ok = ok && w > 0.0 && fin(w) && fin(ex) && fin(ey);
        e[2 * j] = ex; e[2 * j + 1] = ey;
    }
    return ok;
}

/* step 3: d2(m, c, r) */
static double pair_d2(const double e[8], const uint32_t *q, int r) {
    double d2 = 0.0;
    for (int j = 0; j < 4; j++) {
        const int s = (j + r) & 3;
        const double dx = e[2 * j] - (double)q[2 * s], dy = e[2 * j + 1] - (double)q[2 * s + 1];
        const double d = dx * dx + dy * dy;
        if (d > d2) d2 = d;
    }
    return d2;
}

/* Steps 1-2 alone, for the tests that place a quad at a chosen distance: ok[s] = 1 and e[8 s ..] for every missing board slot whose
 * expected corners exist.  -> 1 when the frame has a homography. */
int a3o_recover_expected(const uint32_t *board_ids, const float *board_xy, uint32_t nb, const uint32_t *det_ids, const uint32_t *det_xy,
                         uint32_t nd, uint32_t min_markers, double *e, uint8_t *ok) {
    double H[9];
    uint32_t *seen = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(nb ? nb : 1));
    for (uint32_t s = 0; s < nb; s++) ok[s] = 0;
    const int have = frame_homography(board_ids, board_xy, nb, det_ids, det_xy, nd, min_markers, seen, H);
    if (have)
        for (uint32_t s = 0; s < nb; s++)
            if (seen[s] == 0) ok[s] = (uint8_t)expected_corners(H, board_xy + 8 * (size_t)s, e + 8 * (size_t)s);
    free(seen);
    return have;
}

/* One frame.  board: nb ids and 8 floats each; dict: the dictionary's codes; detected: nd ids and 8 integer corners each, in list
 * order; candidates: nc quads (8 integer corners), 4 codes and a has-codes flag each, every one eligible.  out: room for min(nb, nc)
 * records, in candidate order; -> their number. */
uint32_t a3o_recover_markers(const uint32_t *board_ids, const float *board_xy, uint32_t nb, const uint64_t *dict, const uint32_t *det_ids,
                             const uint32_t *det_xy, uint32_t nd, const uint32_t *cand_xy, const uint64_t *codes4, const uint8_t *has_codes,
                             uint32_t nc, uint32_t min_markers, float max_distance_px, uint32_t max_hamming, uint32_t frame, a3_marker *out) {
    double H[9];
    uint32_t *seen = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(nb ? nb : 1));
    uint32_t *pick = (uint32_t *)malloc(sizeof(uint32_t) * (size_t)(nb ? nb : 1));
    double *pd2 = (double *)malloc(sizeof(double) * (size_t)(nb ? nb : 1));
    uint32_t n_out = 0;
    if (frame_homography(board_ids, board_xy, nb, det_ids, det_xy, nd, min_markers, seen, H)) {
        const double bound = (double)max_distance_px * (double)max_distance_px;
        const int compare_bits = max_hamming != 255u;
        /* step 4a: every missing marker's feasible pair of smallest d2; ties the lowest c, then the lowest r */
        for (uint32_t s = 0; s < nb; s++) {
            pick[s] = NO_PICK; pd2[s] = 0.0;
            double e[8];
            if (seen[s] != 0 || !expected_corners(H, board_xy + 8 * (size_t)s, e)) continue;
            const uint64_t want = dict[board_ids[s]];
            for (uint32_t c = 0; c < nc; c++) {
                if (compare_bits && !has_codes[c]) continue;
                for (int r = 0; r < 4; r++) {
                    if (compare_bits && (uint32_t)popcount64(codes4[4 * (size_t)c + r] ^ want) > max_hamming) continue;
                    const double d2 = pair_d2(e, cand_xy + 8 * (size_t)c, r);
                    if (d2 <= bound && (pick[s] == NO_PICK || d2 < pd2[s])) { pick[s] = (c << 2) | (uint32_t)r; pd2[s] = d2; }
                }
            }
        }
        /* step 4b and the records, in candidate order: candidate c goes to the taker of smallest d2, ties the lowest slot */
        for (uint32_t c = 0; c < nc; c++) {
            uint32_t winner = NO_SLOT;
            for (uint32_t s = 0; s < nb; s++)
                if (pick[s] != NO_PICK && (pick[s] >> 2) == c && (winner == NO_SLOT || pd2[s] < pd2[winner])) winner = s;
            if (winner == NO_SLOT) continue;
            const uint32_t r = pick[winner] & 3u, id = board_ids[winner];
            a3_marker m;
            memset(&m, 0, sizeof m);
            m.frame = frame;
            m.id = id;
            m.code = has_codes[c] ? codes4[4 * (size_t)c + r] : 0;
            for (uint32_t i = 0; i < 4; i++) {
                const uint32_t q = (i + r) & 3u;
                m.corners[2 * i] = cand_xy[8 * (size_t)c + 2 * q]; m.corners[2 * i + 1] = cand_xy[8 * (size_t)c + 2 * q + 1];
            }
            m.hamming_distance = compare_bits ? (uint8_t)popcount64(codes4[4 * (size_t)c + r] ^ dict[id]) : (uint8_t)255;
            m.rotation = (uint8_t)r;
            m.candidate_index = (uint16_t)c;
            out[n_out++] = m;
        }
    }
    free(seen); free(pick); free(pd2);
    return n_out;
}
