// a3_undistort.h -- the per-corner undistortion of include/aruco3_hip.h (a3_set_distortion), shared by the batch launch and the
// stand-alone a3_undistort_points: both go through k_undistort_corners, and this routine is all that kernel computes per lane.
// Two models, uniform per launch: the rational one and the fisheye one (whose forward model k_rectify's map shares).
// Every expression is written in the contract's order; the library is built with -ffp-contract=off, so nothing is fused.
#pragma once
#include <cstdint>

#include "a3_common.h"

namespace a3 {

// a3_intrinsics + a3_distortion, as the kernel takes them (by value)
struct UndistortParams {
    float fx, fy, cx, cy;
    float k1, k2, p1, p2, k3, k4, k5, k6;
    float max_residual;
    uint32_t iterations;
    uint32_t model;   // A3_DIST_RATIONAL or A3_DIST_FISHEYE: uniform per launch
};

// the contract's A(t), its arctangent: the three ranges as selects (both quotients are always evaluated; a lane keeps one), so a wave
// never diverges here and the rectification kernel's map holds no branch
__device__ __forceinline__ float fisheye_atan(float t) {
    const bool hi = t > 2.414213562373095f, mid = t > 0.4142135623730950f;
    const float zh = -(1.0f / t), zm = (t - 1.0f) / (t + 1.0f);
    const float y0 = hi ? 1.5707963267948966f : (mid ? 0.7853981633974483f : 0.0f);
    const float z = hi ? zh : (mid ? zm : t);
    const float w = z * z;
    return y0 + ((((8.05374449538e-2f * w - 1.38776856032e-1f) * w + 1.99777106478e-1f) * w - 3.33329491539e-1f) * w * z + z);
}

// the contract's forward model F: ideal normalised (x, y) -> distorted normalised (*xd, *yd)
__device__ __forceinline__ void fisheye_forward(float k1, float k2, float k3, float k4, float x, float y, float* xd, float* yd) {
    const float r = sqrtf(x * x + y * y);
    const float th = fisheye_atan(r), t2 = th * th;
    const float thd = th * (1.0f + (((k4 * t2 + k3) * t2 + k2) * t2 + k1) * t2);
    const float s = r > 0.0f ? thd / r : 1.0f;
    *xd = x * s;
    *yd = y * s;
}

// (u, v) pixels -> undistorted pixels (*ox, *oy) and the residual in pixels; a failed corner keeps (u, v) and reports +inf
__device__ __forceinline__ void undistort_corner(const UndistortParams& p, float u, float v, float* ox, float* oy, float* res_px) {
    const float x0 = (u - p.cx) / p.fx, y0 = (v - p.cy) / p.fy;
    if (p.model == A3_DIST_FISHEYE) {   // Newton on r = tan(theta): no tangent needed
        const float rd = sqrtf(x0 * x0 + y0 * y0);
        float r = rd;
        for (uint32_t it = 0; it < p.iterations; it++) {
            const float th = fisheye_atan(r), t2 = th * th;
            const float g = th * (1.0f + (((p.k4 * t2 + p.k3) * t2 + p.k2) * t2 + p.k1) * t2);
            const float dg = 1.0f + (((9.0f * p.k4 * t2 + 7.0f * p.k3) * t2 + 5.0f * p.k2) * t2 + 3.0f * p.k1) * t2;
            r = r - (g - rd) * (1.0f + r * r) / dg;
        }
        const float s = rd > 0.0f ? r / rd : 1.0f;
        const float x = x0 * s, y = y0 * s;
        float xd, yd;
        fisheye_forward(p.k1, p.k2, p.k3, p.k4, x, y, &xd, &yd);
        const float ex = (xd - x0) * p.fx, ey = (yd - y0) * p.fy;
        const float res = sqrtf(ex * ex + ey * ey);
        const bool ok = isfinite(x) && isfinite(y) && isfinite(res) && res <= p.max_residual;
        *ox = ok ? x * p.fx + p.cx : u;
        *oy = ok ? y * p.fy + p.cy : v;
        *res_px = ok ? res : __builtin_inff();
        return;
    }
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
