// a3_undistort.h -- the per-corner undistortion of include/aruco3_hip.h (a3_set_distortion), shared by the batch launch and the
// stand-alone a3_undistort_points: both go through k_undistort_corners, and this routine is all that kernel computes per lane.
// Every expression is written in the contract's order; the library is built with -ffp-contract=off, so nothing is fused.
#pragma once
#include <cstdint>

namespace a3 {

// a3_intrinsics + a3_distortion, as the kernel takes them (by value)
struct UndistortParams {
    float fx, fy, cx, cy;
    float k1, k2, p1, p2, k3, k4, k5, k6;
    float max_residual;
    uint32_t iterations;
};

// (u, v) pixels -> undistorted pixels (*ox, *oy) and the residual in pixels; a failed corner keeps (u, v) and reports +inf
__device__ __forceinline__ void undistort_corner(const UndistortParams& p, float u, float v, float* ox, float* oy, float* res_px) {
    const float x0 = (u - p.cx) / p.fx, y0 = (v - p.cy) / p.fy;
    float x = x0, y = y0;
    for (uint32_t it = 0; it < p.iterations; it++) {
        const float r2 = x * x + y * y;
        const float icdist = (1.0f + ((p.k6 * r2 + p.k5) * r2 + p.k4) * r2) / (1.0f + ((p.k3 * r2 + p.k2) * r2 + p.k1) * r2);
        const float dx = 2.0f * p.p1 * x * y + p.p2 * (r2 + 2.0f * x * x);
        const float dy = p.p1 * (r2 + 2.0f * y * y) + 2.0f * p.p2 * x * y;
        x = (x0 - dx) * icdist;
        y = (y0 - dy) * icdist;
    }
    const float r2 = x * x + y * y;
    const float radial = (1.0f + ((p.k3 * r2 + p.k2) * r2 + p.k1) * r2) / (1.0f + ((p.k6 * r2 + p.k5) * r2 + p.k4) * r2);
    const float xd = x * radial + (2.0f * p.p1 * x * y + p.p2 * (r2 + 2.0f * x * x));
    const float yd = y * radial + (p.p1 * (r2 + 2.0f * y * y) + 2.0f * p.p2 * x * y);
    const float ex = (xd - x0) * p.fx, ey = (yd - y0) * p.fy;
    const float res = sqrtf(ex * ex + ey * ey);
    const bool ok = isfinite(x) && isfinite(y) && isfinite(res) && res <= p.max_residual;
    *ox = ok ? x * p.fx + p.cx : u;
    *oy = ok ? y * p.fy + p.cy : v;
    *res_px = ok ? res : __builtin_inff();
}

}  // namespace a3
