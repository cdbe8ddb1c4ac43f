// k_refine.hip -- sub-pixel corner refinement (a3_set_corner_refinement / a3_refine_corners).  Not part of the reference, which
// keeps the integer contour corners: an extension stated in include/aruco3_hip.h, restated on the CPU by tests/refine_oracle.c
// (a3o_refine_corners), which this kernel matches bit for bit.
//
// One wave64 per corner, four per workgroup (the four corners of one marker, or four consecutive caller corners); the tile load and
// the iteration are a3_subpix.h's subpix_load_tile / subpix_iterate, as the ChArUco corner stage calls them.
#include <algorithm>
#include <cmath>

#include "a3_common.h"
#include "a3_launch.h"
#include "a3_subpix.h"

namespace a3 {

// markers != nullptr: the accepted markers of a batch (min(n, *n_dev) of them), 4 corners each, window from the quad's cell size.
// markers == nullptr: n caller corners `pts` of frame 0, window from cell_px[k] (nullable).  out: x, y per corner, in corner order.
__global__ __launch_bounds__(256) void k_refine_corners(PixelSrc src, uint32_t W, uint32_t H, const a3_marker* __restrict__ markers,
                                                        const unsigned int* __restrict__ n_dev, const float* __restrict__ pts,
                                                        const float* __restrict__ cell_px, uint32_t n, RefineParams p, float* __restrict__ out) {
    __shared__ uint8_t s_tile[4][kRefineTile * kRefineTile];
    __shared__ float s_g[4][2 * kRefineMaxWin + 1];
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const uint32_t units = markers ? min(n, *n_dev) : (n + 3u) / 4u;
    const float eps2 = p.min_shift * p.min_shift;
    for (uint32_t u = blockIdx.x; u < units; u += gridDim.x) {   // (uniform over the workgroup: the barriers below are safe)
        const uint32_t k = u * 4u + (uint32_t)wave;
        const bool live = markers || k < n;
        float q0x = 0.0f, q0y = 0.0f, cell = __builtin_nanf("");
        uint32_t frame = 0;
        if (markers) {
            const uint32_t* c = markers[u].corners;
            float best = 0.0f;
            for (int e = 0; e < 4; e++) {   // shortest side (a3o_quad_cell_px)
                const int e2 = (e + 1) & 3;
                const float dx = (float)c[2 * e2] - (float)c[2 * e], dy = (float)c[2 * e2 + 1] - (float)c[2 * e + 1];
                const float len = sqrtf(dx * dx + dy * dy);
                if (e == 0 || len < best) best = len;
            }
            cell = best / (float)p.cells;
            q0x = (float)c[2 * wave]; q0y = (float)c[2 * wave + 1];
            frame = markers[u].frame;
        } else if (live) {
            q0x = pts[2 * k]; q0y = pts[2 * k + 1];
            if (cell_px) cell = cell_px[k];
        }
        const int w = markers || cell_px ? refine_window(p, cell) : (int)p.win_half;
        const int T = 4 * w + 6;
        const int ox = (int)floorf(q0x) - 2 * w - 2, oy = (int)floorf(q0y) - 2 * w - 2;
        if (live) subpix_load_tile(src, src.base + (size_t)frame * src.frame_stride, W, H, T, ox, oy, p, w, lane, s_tile[wave], s_g[wave]);
        __syncthreads();
        if (live) {
            const float2 q = subpix_iterate(s_tile[wave], T, ox, oy, s_g[wave], w, q0x, q0y, p, eps2, lane);
            if (lane == 0) { out[2 * (size_t)k] = q.x; out[2 * (size_t)k + 1] = q.y; }
        }
        __syncthreads();   // (the next unit overwrites the tiles)
    }
}

void refine_params(void* out, const a3_refine_config& cfg, uint32_t cells) {
    RefineParams* p = reinterpret_cast<RefineParams*>(out);
    p->win_half = cfg.win_half; p->max_iterations = cfg.max_iterations; p->cells = cells;
    p->relative_win = cfg.relative_win; p->min_shift = cfg.min_shift;
    for (int w = 0; w <= kRefineMaxWin; w++)
        for (int k = 0; k <= 2 * kRefineMaxWin; k++) {
            const int i = k - w;
            p->g[w][k] = w > 0 && k <= 2 * w ? (float)exp(-(double)(i * i) / (double)(w * w)) : 0.0f;
        }
}

size_t refine_params_bytes() { return sizeof(RefineParams); }

hipError_t launch_refine_corners(hipStream_t st, const RefineLaunch& r) {
    const uint32_t units = r.markers ? r.n : (r.n + 3u) / 4u;
    if (units == 0) return hipSuccess;
    hipLaunchKernelGGL(k_refine_corners, dim3(std::min<uint32_t>(units, 1024u)), dim3(256), 0, st, r.src, r.W, r.H, r.markers, r.n_dev, r.pts, r.cell_px, r.n,
                       *reinterpret_cast<const RefineParams*>(r.params), r.out);
    return hipGetLastError();
}

}  // namespace a3
