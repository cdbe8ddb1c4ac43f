// k_board3d.hip -- one pose per frame of a board whose markers are not coplanar (a3_set_board3d; a3_get_board_poses /
// a3_estimate_board_pose serve it as they serve a planar board).  Not part of the reference: an extension stated in
// include/aruco3_hip.h and restated on the CPU by tests/board3d_oracle.c (a3o_board3d_pose), in the same order of operations.
//
// The kernel is a3_board.h's board_pose_body with the 3-D marker model (a3_board3d.h Board3Markers): a corner has three board
// coordinates (Board3Slot), the start carries the marker's IPPE pose through the marker's own frame (e_x, e_y, e_z, c) instead of an
// in-plane rotation, and the sums take q = R (X, Y, Z) (board3_accum).
#include <algorithm>
#include <cmath>

#include "a3_board3d.h"
#include "a3_common.h"
#include "a3_launch.h"

namespace a3 {

__global__ __launch_bounds__(128) void k_board3d_pose(BoardArgs a) { board_pose_body(a, Board3Markers{}, a.out); }

size_t board3d_slot_bytes() { return sizeof(Board3Slot); }

// (the contract's float arithmetic; tests/board3d_oracle.c a3o_board3d_slot)
void board3d_slot_from(const float xyz[12], void* out) {
    Board3Slot s{};
    for (int k = 0; k < 4; k++) { s.x[k] = xyz[3 * k]; s.y[k] = xyz[3 * k + 1]; s.z[k] = xyz[3 * k + 2]; }
    const float d[3] = {s.x[1] - s.x[0], s.y[1] - s.y[0], s.z[1] - s.z[0]};
    s.side = sqrtf((d[0] * d[0] + d[1] * d[1]) + d[2] * d[2]);
    for (int j = 0; j < 3; j++) s.ex[j] = d[j] / s.side;
    const float v[3] = {s.x[0] - s.x[3], s.y[0] - s.y[3], s.z[0] - s.z[3]};
    const float k = (v[0] * s.ex[0] + v[1] * s.ex[1]) + v[2] * s.ex[2];
    float w[3];
    for (int j = 0; j < 3; j++) w[j] = v[j] - k * s.ex[j];
    const float wn = sqrtf((w[0] * w[0] + w[1] * w[1]) + w[2] * w[2]);
    for (int j = 0; j < 3; j++) s.ey[j] = w[j] / wn;
    s.ez[0] = s.ex[1] * s.ey[2] - s.ex[2] * s.ey[1];
    s.ez[1] = s.ex[2] * s.ey[0] - s.ex[0] * s.ey[2];
    s.ez[2] = s.ex[0] * s.ey[1] - s.ex[1] * s.ey[0];
    s.c[0] = 0.25f * ((s.x[0] + s.x[1]) + (s.x[2] + s.x[3]));
    s.c[1] = 0.25f * ((s.y[0] + s.y[1]) + (s.y[2] + s.y[3]));
    s.c[2] = 0.25f * ((s.z[0] + s.z[1]) + (s.z[2] + s.z[3]));
    *reinterpret_cast<Board3Slot*>(out) = s;
}

hipError_t launch_board3d_pose(hipStream_t st, const BoardPoseLaunch& b) {
    if (b.board.slot_kind != kBoardSlots3D) return hipErrorInvalidValue;   // (planar BoardSlot records are half the size)
    if (b.m.n_frames == 0) return hipSuccess;
    BoardArgs a = board_args(b.m, b.board, b.intr, b.W, b.H);
    a.out = b.out;
    hipLaunchKernelGGL(k_board3d_pose, dim3(b.m.n_frames), dim3(128), 0, st, a);
    return hipGetLastError();
}

}  // namespace a3
