// k_board.hip -- one board pose per frame (a3_set_board / a3_get_board_poses / a3_estimate_board_pose).  Not part of the reference:
// an extension stated in include/aruco3_hip.h and restated on the CPU by tests/board_oracle.c (a3o_board_pose), in the same order
// of operations.
//
// The kernel is a3_board.h's board_pose_body with the planar marker model (PlanarMarkers): the four corners of every board marker of the
// frame that is not duplicated, each with its slot's board point.
#include <algorithm>
#include <cmath>

#include "a3_board.h"
#include "a3_common.h"
#include "a3_launch.h"

namespace a3 {

__global__ __launch_bounds__(128) void k_board_pose(BoardArgs a) { board_pose_body(a, PlanarMarkers{}, a.out); }

size_t board_slot_bytes() { return sizeof(BoardSlot); }

// (the contract's float arithmetic; tests/board_oracle.c a3o_board_slot)
void board_slot_from(const float xy[8], void* out) {
    BoardSlot s{};
    for (int k = 0; k < 4; k++) { s.x[k] = xy[2 * k]; s.y[k] = xy[2 * k + 1]; }
    const float ex = s.x[1] - s.x[0], ey = s.y[1] - s.y[0];
    s.side = sqrtf(ex * ex + ey * ey);
    s.cs = ex / s.side; s.sn = ey / s.side;
    s.cx = 0.25f * ((s.x[0] + s.x[1]) + (s.x[2] + s.x[3]));
    s.cy = 0.25f * ((s.y[0] + s.y[1]) + (s.y[2] + s.y[3]));
    *reinterpret_cast<BoardSlot*>(out) = s;
}

hipError_t launch_board_pose(hipStream_t st, const BoardPoseLaunch& b) {
    if (b.m.n_frames == 0) return hipSuccess;
    BoardArgs a = board_args(b.m, b.board, b.intr, b.W, b.H);
    a.out = b.out;
    hipLaunchKernelGGL(k_board_pose, dim3(b.m.n_frames), dim3(128), 0, st, a);
    return hipGetLastError();
}

}  // namespace a3
