// a3_subpix.h -- the cornerSubPix iteration of include/aruco3_hip.h (a3_refine_config), shared by k_refine_corners (k_refine.hip) and the
// ChArUco corner stage (k_charuco.hip): one wave64 per corner, the integer grey levels any allowed estimate can touch in an LDS tile,
// every iteration LDS and VALU only.  The estimate and the five sums are wave-uniform (the xor butterfly leaves the same bits in every
// lane), so the iteration loop never diverges.  Built with -ffp-contract=off: nothing is fused.
#pragma once
#include <cmath>

#include "a3_common.h"

namespace a3 {

constexpr int kRefineMaxWin = 10;
// Estimates stay within w of the start q0 (the revert rule), samples lie within w + 1 of an estimate, and a bilinear sample reads
// floor(x) and floor(x) + 1: 4w + 4 columns from floor(q0.x) - 2w - 1.  One guard column / row on each side absorbs the rounding
// of c + i in float: 4w + 6, 46 at w = 10 (2116 bytes per wave).
constexpr int kRefineTile = 4 * kRefineMaxWin + 6;

struct RefineParams {
    uint32_t win_half, max_iterations, cells;
    float relative_win, min_shift;
    float g[kRefineMaxWin + 1][2 * kRefineMaxWin + 1];   // g[w][i + w] = (float)exp(-(double)(i*i) / (double)(w*w)), host libm
};

// the contract's window: win_half, or min(win_half, max(2, floor(relative_win * cell_px))) (NaN -> 2)
__device__ __forceinline__ int refine_window(const RefineParams& p, float cell_px) {
    const int wh = (int)p.win_half;
    if (!(p.relative_win > 0.0f)) return wh;
    const float t = floorf(p.relative_win * cell_px);
    const int v = t >= 2.0f ? (t >= (float)wh ? wh : (int)t) : 2;
    return min(v, wh);
}

// into_luma8 grey level of pixel (x, y) of a frame (the grey plane K1 wrote, or the caller's pixel: same integers)
__device__ __forceinline__ uint32_t refine_grey(const uint8_t* __restrict__ frame, unsigned long long row_stride, int fmt, uint32_t x, uint32_t y) {
    const uint8_t* row = frame + (size_t)y * row_stride;
    if (fmt == A3_FMT_L8 || fmt == kFmtGreyPlane) return row[x];
    if (fmt == A3_FMT_YUYV8 || fmt == A3_FMT_UYVY8) return row[2u * (size_t)x + (fmt == A3_FMT_UYVY8 ? 1u : 0u)];   // packed 4:2:2: the luma byte as it stands
    if (fmt == A3_FMT_RGB8) { const uint8_t* q = row + 3u * (size_t)x; return luma_of(q[0], q[1], q[2]); }
    const uint8_t* q = row + 4u * (size_t)x;
    return fmt == A3_FMT_BGRA8 ? luma_of(q[2], q[1], q[0]) : luma_of(q[0], q[1], q[2]);
}

// bilinear sample at (x, y) from the wave's tile (origin ox, oy; border replicate is baked into the tile), the contract's order
__device__ __forceinline__ float refine_sample(const uint8_t* __restrict__ tile, int T, int ox, int oy, float x, float y) {
    const float x0f = floorf(x), y0f = floorf(y);
    const float fx = x - x0f, fy = y - y0f;
    const int tx = min(max((int)x0f - ox, 0), T - 2), ty = min(max((int)y0f - oy, 0), T - 2);   // (a guard: never active, see kRefineTile)
    const uint8_t* r = tile + ty * T + tx;
    const float i00 = (float)r[0], i01 = (float)r[1], i10 = (float)r[T], i11 = (float)r[T + 1];
    return (1.0f - fy) * ((1.0f - fx) * i00 + fx * i01) + fy * ((1.0f - fx) * i10 + fx * i11);
}

// the wave's tile (T x T, origin ox, oy) of frame `fb` with the border replicated, and the window's weights g[0 .. 2w]
__device__ __forceinline__ void subpix_load_tile(const PixelSrc& src, const uint8_t* fb, uint32_t W, uint32_t H, int T, int ox, int oy,
                                                 const RefineParams& p, int w, int lane, uint8_t* tile, float* g) {
    for (int t = lane; t < T * T; t += 64) {
        const int x = min(max(ox + t % T, 0), (int)W - 1), y = min(max(oy + t / T, 0), (int)H - 1);
        tile[t] = (uint8_t)refine_grey(fb, src.row_stride, src.fmt, (uint32_t)x, (uint32_t)y);
    }
    if (lane <= 2 * w) g[lane] = p.g[w][lane];
}

// the iteration from q0 with half-width w over the wave's tile (after a barrier behind subpix_load_tile) -> the corner
__device__ __forceinline__ float2 subpix_iterate(const uint8_t* tile, int T, int ox, int oy, const float* g, int w, float q0x, float q0y,
                                                 const RefineParams& p, float eps2, int lane) {
    const int side = 2 * w + 1, npx = side * side;
    float cx = q0x, cy = q0y;
    for (uint32_t it = 0; it < p.max_iterations; it++) {
        float a = 0.0f, b = 0.0f, c2 = 0.0f, bb1 = 0.0f, bb2 = 0.0f;
        for (int q = lane; q < npx; q += 64) {   // lane l: pixels l, l + 64, ... of the window, row-major
            const int i = q % side - w, j = q / side - w;
            const float m = g[i + w] * g[j + w];
            const float gx = refine_sample(tile, T, ox, oy, cx + (float)(i + 1), cy + (float)j) -
                             refine_sample(tile, T, ox, oy, cx + (float)(i - 1), cy + (float)j);
            const float gy = refine_sample(tile, T, ox, oy, cx + (float)i, cy + (float)(j + 1)) -
                             refine_sample(tile, T, ox, oy, cx + (float)i, cy + (float)(j - 1));
            const float fi = (float)i, fj = (float)j;
            a += gx * gx * m;
            b += gx * gy * m;
            c2 += gy * gy * m;
            bb1 += gx * gx * m * fi + gx * gy * m * fj;
            bb2 += gx * gy * m * fi + gy * gy * m * fj;
        }
        for (int o = 32; o >= 1; o >>= 1) {   // xor butterfly: a + b == b + a, so every lane ends with the same bits
            a += __shfl_xor(a, o); b += __shfl_xor(b, o); c2 += __shfl_xor(c2, o);
            bb1 += __shfl_xor(bb1, o); bb2 += __shfl_xor(bb2, o);
        }
        const float det = a * c2 - b * b;
        if (det == 0.0f || !isfinite(det)) break;
        const float s = 1.0f / det;
        const float nx = cx + (c2 * s * bb1 - b * s * bb2), ny = cy + (-b * s * bb1 + a * s * bb2);
        if (!(fabsf(nx - q0x) <= (float)w && fabsf(ny - q0y) <= (float)w)) { cx = q0x; cy = q0y; break; }
        const float dx = nx - cx, dy = ny - cy;
        cx = nx; cy = ny;
        if (dx * dx + dy * dy <= eps2) break;
    }
    return make_float2(cx, cy);
}

}  // namespace a3
