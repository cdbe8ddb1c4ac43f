// k_undistort.hip -- lens undistortion of marker corners (a3_set_distortion / a3_undistort_points).  Not part of the reference, whose
// poses assume an ideal pinhole camera: an extension stated in include/aruco3_hip.h, restated on the CPU by tests/lens_oracle.c
// (a3o_undistort) and, for the fisheye model, by tests/fisheye_oracle.c (a3o_fisheye_undistort), which this kernel matches bit for bit.
//
// One lane per corner.  A batch's corners are those of the device-resident marker list (min(marker_cap, *n_dev) markers), read as
// the refined floats (8 per marker) when refinement ran, else as the integer a3_marker corners; the stand-alone call passes n points.
// Output: out_xy, 2 floats per corner (8 per marker: the layout k_pose modes 3 / 4 and k_board_pose's refined corners read), and
// out_res, 1 float per corner.  A few MFLOP per 256-frame batch: the launch is the cost.
#include <algorithm>
#include <cmath>

#include "a3_common.h"
#include "a3_launch.h"
#include "a3_undistort.h"

namespace a3 {

__global__ __launch_bounds__(256) void k_undistort_corners(const a3_marker* __restrict__ markers, const float* __restrict__ pts,
                                                           const unsigned int* __restrict__ n_dev, uint32_t n, UndistortParams p,
                                                           float* __restrict__ out_xy, float* __restrict__ out_res) {
    const uint32_t corners = n_dev ? min(n, *n_dev) * 4u : n;   // (n: markers with n_dev, points without)
    for (uint32_t c = blockIdx.x * blockDim.x + threadIdx.x; c < corners; c += gridDim.x * blockDim.x) {
        float u, v;
        if (pts) { u = pts[2 * (size_t)c]; v = pts[2 * (size_t)c + 1]; }
        else { const uint32_t* q = markers[c >> 2].corners; u = (float)q[2 * (c & 3u)]; v = (float)q[2 * (c & 3u) + 1]; }
        float x, y, r;
        undistort_corner(p, u, v, &x, &y, &r);
        out_xy[2 * (size_t)c] = x;
        out_xy[2 * (size_t)c + 1] = y;
        out_res[c] = r;
    }
}

hipError_t launch_undistort_corners(hipStream_t st, const a3_marker* markers, const float* pts, const unsigned int* n_dev, uint32_t n,
                                    const a3_intrinsics& in, const a3_distortion& d, float* out_xy, float* out_res) {
    const uint64_t corners = n_dev ? (uint64_t)n * 4u : n;
    if (corners == 0) return hipSuccess;
    const UndistortParams p{in.focal_x, in.focal_y, in.principal_x, in.principal_y, d.k1, d.k2, d.p1, d.p2, d.k3, d.k4, d.k5, d.k6,
                            d.max_residual_px, d.iterations, d.model};
    // (grid-stride: a batch's marker_cap is an upper bound -- the blocks past the real count find nothing and leave at once)
    const uint32_t blocks = (uint32_t)std::min<uint64_t>((corners + 255) / 256, 1024);
    hipLaunchKernelGGL(k_undistort_corners, dim3(blocks), dim3(256), 0, st, markers, pts, n_dev, n, p, out_xy, out_res);
    return hipGetLastError();
}

}  // namespace a3
