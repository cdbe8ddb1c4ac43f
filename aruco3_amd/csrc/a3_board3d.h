// a3_board3d.h -- the 3-D board's pieces of include/aruco3_hip.h (a3_set_board3d) that a3_board.h's planar ones do not cover: the slot
// record with three coordinates per corner and the marker's own frame, the correspondence of one corner, the residual / Jacobian
// sums with q = R (X, Y, Z), and Board3Markers, the model that hands them to a3_board.h's board_pose_body.  Everything else (BoardArgs,
// the frame run, the duplicates, the start marker, the image side of a correspondence, board_lm, the counts) is a3_board.h's, used as
// it stands.  Built with -ffp-contract=off.
#pragma once
#include "a3_board.h"

namespace a3 {

struct Board3Slot {   // per board marker, built by a3_set_board3d (host, float: board3d_slot_from)
    float x[4], y[4], z[4];
    float side, ex[3], ey[3], ez[3], c[3], pad[7];   // the marker's frame in the board's: x right, y up, z out of the printed face; its centre
};
static_assert(sizeof(Board3Slot) == 128, "Board3Slot is 128 bytes");

__device__ __forceinline__ const Board3Slot* board3_slots(const BoardArgs& a) { return reinterpret_cast<const Board3Slot*>(a.slots); }

// corner c of the frame (marker first + c / 4, corner c % 4): board point b[3] and normalised image point; false when not used
__device__ __forceinline__ bool board3_corner(const BoardArgs& a, const uint32_t* s_dup, uint32_t first, uint32_t c, float b[3], float* mx, float* my) {
    const uint32_t m = first + (c >> 2);
    const int k = (int)(c & 3u);
    const uint32_t slot = board_slot(a, m);
    if (slot == kNoSlot || board_dup(s_dup, slot)) return false;
    const Board3Slot& s = board3_slots(a)[slot];
    b[0] = s.x[k]; b[1] = s.y[k]; b[2] = s.z[k];
    float x, y;
    board_image_px(a, m, k, &x, &y);
    board_normalise(a, x, y, mx, my);
    return true;
}

// board_accum with q = R (X, Y, Z): from q on, its arithmetic term for term
__device__ __forceinline__ void board3_accum(BoardAcc& s, const float R[9], const float t[3], const float b[3], float mx, float my, float sx, float sy) {
    const float qx = (R[0] * b[0] + R[1] * b[1]) + R[2] * b[2], qy = (R[3] * b[0] + R[4] * b[1]) + R[5] * b[2], qz = (R[6] * b[0] + R[7] * b[1]) + R[8] * b[2];
    const float px = qx + t[0], py = qy + t[1], pz = qz + t[2];
    const float zz = pz > 1e-5f ? pz : 1e-5f;
    const float u = px / zz, v = py / zz;
    const float a = 1.0f / zz, a2 = 2.0f * a;
    const float ru = u - mx, rv = v - my;
    const float ju[6] = {-(a2 * u) * qy, a2 * (qz + u * qx), -a2 * qy, a, 0.0f, -(a * u)};
    const float jv[6] = {-a2 * (qz + v * qy), (a2 * v) * qx, a2 * qx, 0.0f, a, -(a * v)};
    int idx = 0;
    for (int r = 0; r < 6; r++) {
        for (int c = r; c < 6; c++) { s.h[idx] += ju[r] * ju[c] + jv[r] * jv[c]; idx++; }
        s.g[r] += ju[r] * ru + jv[r] * rv;
    }
    s.cost += ru * ru + rv * rv;
    const float eu = ru * sx, ev = rv * sy;
    s.pix += eu * eu + ev * ev;
}

struct Board3Markers : BoardMarkerRun {   // a3_set_board3d: k_board3d_pose (a3_board.h board_pose_body)
    using Slot = Board3Slot;
    struct Corr { float b[3], mx, my; };
    __device__ static const Board3Slot* slots(const BoardArgs& a) { return board3_slots(a); }
    __device__ bool corner(const BoardArgs& a, uint32_t c, Corr& o) const { return board3_corner(a, s_dup, first, c, o.b, &o.mx, &o.my); }
    __device__ static void accum(BoardAcc& s, const float R[9], const float t[3], const Corr& o, float sx, float sy) {
        board3_accum(s, R, t, o.b, o.mx, o.my, sx, sy);
    }
    // the start marker's IPPE pose carried through the marker's own frame (e_x, e_y, e_z, c) into the board's
    __device__ static void start(const Board3Slot& bs, const a3_pose& pm, float R[9], float t[3]) {
        const float* Rm = pm.rotation;
        for (int r = 0; r < 3; r++)
            for (int j = 0; j < 3; j++) R[3 * r + j] = (Rm[3 * r] * bs.ex[j] + Rm[3 * r + 1] * bs.ey[j]) + Rm[3 * r + 2] * bs.ez[j];
        for (int r = 0; r < 3; r++) t[r] = pm.translation[r] - ((R[3 * r] * bs.c[0] + R[3 * r + 1] * bs.c[1]) + R[3 * r + 2] * bs.c[2]);
    }
};

}  // namespace a3
