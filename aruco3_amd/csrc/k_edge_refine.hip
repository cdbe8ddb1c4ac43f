// k_edge_refine.hip -- edge-fit corner refinement (a3_refine_config.method A3_REFINE_EDGES).  Not part of the reference: an extension
// stated in include/aruco3_hip.h, restated on the CPU by tests/edge_refine_oracle.c (a3o_refine_quads), which this kernel matches bit
// for bit.  Built with -ffp-contract=off: nothing is fused.
//
// One wave64 per marker, four markers per workgroup.  Lane l works on side l >> 4 of the quad, station l & 15 of that side: it walks
// its station's 4r + 5 bilinear samples along the side's outward normal straight from the frame (the perimeter of a marker fits no LDS
// tile, and the four bytes of a sample are the only reuse), keeping the last four in registers for the central difference.  The five
// sums of a side's line fit stay inside the side's DPP row (row_ror 8, 4, 2, 1: after the step by 8 the values have period 8 in the
// row, so a rotation by 4 brings what an xor by 4 brings, and so on down -- the bits of the xor butterfly the contract states).  The
// four lines cross sides by v_readlane from lanes 0, 16, 32, 48; from there on every lane holds the same corners, so the pass loop
// and every revert verdict are wave-uniform.  No LDS, no barrier: a wave that has no marker leaves.
#include <algorithm>
#include <cmath>

#include "a3_common.h"
#include "a3_launch.h"
#include "a3_subpix.h"

namespace a3 {

constexpr float kEdgeLiveLevel = (float)A3_REFINE_EDGES_LIVE_LEVEL;
constexpr float kEdgeMinSide = 4.0f;
constexpr float kEdgeMinLive = 12.0f;

struct EdgeParams {
    uint32_t win_half, max_iterations, cells;
    float relative_win, min_shift;
};

// the search range: a3_subpix.h's refine_window on this kernel's parameters
__device__ __forceinline__ int edge_range(const EdgeParams& p, float cell_px) {
    const int wh = (int)p.win_half;
    if (!(p.relative_win > 0.0f)) return wh;
    const float t = floorf(p.relative_win * cell_px);
    const int v = t >= 2.0f ? (t >= (float)wh ? wh : (int)t) : 2;
    return min(v, wh);
}

// x + (x of lane (l + R) & 15 of the same row of 16), R = 8, 4, 2, 1
template <int R>
__device__ __forceinline__ float row_add_ror(float x) {
    return x + __builtin_bit_cast(float, __builtin_amdgcn_update_dpp(0, __builtin_bit_cast(int, x), 0x120 + R, 0xf, 0xf, false));
}
__device__ __forceinline__ float row_sum16(float x) {
    x = row_add_ror<8>(x); x = row_add_ror<4>(x); x = row_add_ror<2>(x); x = row_add_ror<1>(x);
    return x;
}
__device__ __forceinline__ float lane_bcast(float x, int lane) {   // (lane: a constant)
    return __builtin_bit_cast(float, __builtin_amdgcn_readlane(__builtin_bit_cast(int, x), lane));
}

// Where a pixel's grey level lies (a3_subpix.h's refine_grey with the format's tests taken out of the sample loop, so that the loads of
// the loop is straight code): bpp bytes per pixel.  kKind 0: the byte at `off` is the grey level (L8, the grey plane, the luma byte of
// packed 4:2:2); 1: bytes 0, 1, 2 are R, G, B of luma_of (RGB8, RGBA8); 2: B, G, R (BGRA8).
struct EdgePixel { uint32_t bpp, off; };
template <int kKind>
__device__ __forceinline__ uint32_t edge_grey(const uint8_t* __restrict__ fb, unsigned long long row_stride, EdgePixel f, uint32_t x, uint32_t y) {
    const uint8_t* q = fb + (size_t)y * row_stride + (size_t)(f.bpp * x + f.off);
    if constexpr (kKind == 1) return luma_of(q[0], q[1], q[2]);
    if constexpr (kKind == 2) return luma_of(q[2], q[1], q[0]);
    return q[0];
}

// the contract's bilinear sample at (x, y) of frame fb, image coordinates clamped to the frame
template <int kKind>
__device__ __forceinline__ float edge_sample(const uint8_t* __restrict__ fb, unsigned long long row_stride, EdgePixel fmt, int W, int H, float x, float y) {
    const float x0f = floorf(x), y0f = floorf(y);
    const float fx = x - x0f, fy = y - y0f;
    const int x0 = (int)x0f, y0 = (int)y0f;
    const uint32_t xa = (uint32_t)min(max(x0, 0), W - 1), xb = (uint32_t)min(max(x0 + 1, 0), W - 1);
    const uint32_t ya = (uint32_t)min(max(y0, 0), H - 1), yb = (uint32_t)min(max(y0 + 1, 0), H - 1);
    const float i00 = (float)edge_grey<kKind>(fb, row_stride, fmt, xa, ya), i01 = (float)edge_grey<kKind>(fb, row_stride, fmt, xb, ya);
    const float i10 = (float)edge_grey<kKind>(fb, row_stride, fmt, xa, yb), i11 = (float)edge_grey<kKind>(fb, row_stride, fmt, xb, yb);
    return (1.0f - fy) * ((1.0f - fx) * i00 + fx * i01) + fy * ((1.0f - fx) * i10 + fx * i11);
}

// markers != nullptr: the accepted markers of a batch (min(n, *n_dev) of them), range from the quad's cell size.
// markers == nullptr: n / 4 caller quads `pts` of frame 0, range from cell_px[4 u] (nullable).  out: 8 floats per quad.
// flags (with markers; nullable): the list's flag words -- a3_set_marker_polarity's A3_POLARITY_BOTH.
template <int kKind>
__global__ __launch_bounds__(256) void k_refine_edges(PixelSrc src, EdgePixel pix, uint32_t W, uint32_t H, const a3_marker* __restrict__ markers,
                                                      const unsigned int* __restrict__ n_dev, const float* __restrict__ pts,
                                                      const float* __restrict__ cell_px, uint32_t n, EdgeParams p, float* __restrict__ out,
                                                      const uint32_t* __restrict__ flags /*nullable: every quad dark inside*/) {
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const int side = lane >> 4, station = lane & 15;
    const uint32_t quads = markers ? min(n, *n_dev) : n / 4u;
    const uint32_t groups = (quads + 3u) / 4u;
    const float s = 0.125f + 0.75f * (((float)station + 0.5f) / 16.0f);
    for (uint32_t g = blockIdx.x; g < groups; g += gridDim.x) {
        const uint32_t u = g * 4u + (uint32_t)wave;
        if (u >= quads) break;   // (only the last group is short; no barrier anywhere)
        float q0x, q0y, q1x, q1y, q2x, q2y, q3x, q3y, cell = __builtin_nanf("");
        uint32_t frame = 0;
        bool have_cell;
        if (markers) {
            const uint32_t* c = markers[u].corners;
            q0x = (float)c[0]; q0y = (float)c[1]; q1x = (float)c[2]; q1y = (float)c[3];
            q2x = (float)c[4]; q2y = (float)c[5]; q3x = (float)c[6]; q3y = (float)c[7];
            float best = 0.0f;
            for (int e = 0; e < 4; e++) {   // shortest side (a3o_quad_cell_px)
                const int e2 = (e + 1) & 3;
                const float dx = (float)c[2 * e2] - (float)c[2 * e], dy = (float)c[2 * e2 + 1] - (float)c[2 * e + 1];
                const float len = sqrtf(dx * dx + dy * dy);
                if (e == 0 || len < best) best = len;
            }
            cell = best / (float)p.cells;
            frame = markers[u].frame;
            have_cell = true;
        } else {
            const float* c = pts + 8 * (size_t)u;
            q0x = c[0]; q0y = c[1]; q1x = c[2]; q1y = c[3]; q2x = c[4]; q2y = c[5]; q3x = c[6]; q3y = c[7];
            have_cell = cell_px != nullptr;
            if (have_cell) cell = cell_px[4 * (size_t)u];
        }
        // a marker flagged A3_MARKER_INVERTED is bright inside: g_j = S_(j-2) - S_(j+2), the exact negation (wave-uniform)
        const bool inverted = markers && flags && (flags[u] & A3_MARKER_INVERTED) != 0u;
        const int r = have_cell ? edge_range(p, cell) : (int)p.win_half;
        const float reach = (float)(2 * r);
        const uint8_t* fb = src.base + (size_t)frame * src.frame_stride;
        float c0x = q0x, c0y = q0y, c1x = q1x, c1y = q1y, c2x = q2x, c2y = q2y, c3x = q3x, c3y = q3y;
        bool revert = false;
        for (uint32_t it = 0; it < p.max_iterations; it++) {
            // this lane's side a -> b
            const float ax = side == 0 ? c0x : side == 1 ? c1x : side == 2 ? c2x : c3x, ay = side == 0 ? c0y : side == 1 ? c1y : side == 2 ? c2y : c3y;
            const float bx = side == 0 ? c1x : side == 1 ? c2x : side == 2 ? c3x : c0x, by = side == 0 ? c1y : side == 1 ? c2y : side == 2 ? c3y : c0y;
            const float dx = bx - ax, dy = by - ay;
            const float L = sqrtf(dx * dx + dy * dy);
            const bool shrt = !(L >= kEdgeMinSide);
            if (__any(shrt)) { revert = true; break; }   // (the corners are the same in every lane: so is each side's L)
            const float Nx = dy / L, Ny = -(dx / L);
            const float px = ax + s * dx, py = ay + s * dy;
            // samples S_i = P(p + (i / 2) N), i = -2r - 2 .. 2r + 2; g_j = S_(j+2) - S_(j-2), j = -2r .. 2r, with the last four samples kept
            float s0 = 0.0f, s1 = 0.0f, s2 = 0.0f, s3 = 0.0f, gmax = 0.0f, sw = 0.0f, swo = 0.0f;
            for (int i = -2 * r - 2; i <= 2 * r + 2; i++) {
                const float o = (float)i * 0.5f;
                const float v = edge_sample<kKind>(fb, src.row_stride, pix, (int)W, (int)H, px + o * Nx, py + o * Ny);
                if (i >= -2 * r + 2) {   // s0 = S_(i-4)
                    const float gj = inverted ? s0 - v : v - s0, oj = (float)(i - 2) * 0.5f;
                    const float wj = gj > 0.0f ? gj * gj : 0.0f;
                    gmax = gj > gmax ? gj : gmax;
                    sw += wj;
                    swo += wj * oj;
                }
                s0 = s1; s1 = s2; s2 = s3; s3 = v;
            }
            const bool live = gmax >= kEdgeLiveLevel;
            const float m = live ? swo / sw : 0.0f, one = live ? 1.0f : 0.0f, sl = live ? s : 0.0f;
            const float fn = row_sum16(one), Ss = row_sum16(sl), Sss = row_sum16(sl * sl), Sm = row_sum16(m), Ssm = row_sum16(sl * m);
            const float det = fn * Sss - Ss * Ss;
            const bool bad = !(fn >= kEdgeMinLive) || det == 0.0f || !isfinite(det);
            if (__any(bad)) { revert = true; break; }
            const float alpha = (Sm * Sss - Ss * Ssm) / det, beta = (fn * Ssm - Ss * Sm) / det;
            const float Ox = ax + alpha * Nx, Oy = ay + alpha * Ny, Dx = dx + beta * Nx, Dy = dy + beta * Ny;
            const float O0x = lane_bcast(Ox, 0), O0y = lane_bcast(Oy, 0), D0x = lane_bcast(Dx, 0), D0y = lane_bcast(Dy, 0);
            const float O1x = lane_bcast(Ox, 16), O1y = lane_bcast(Oy, 16), D1x = lane_bcast(Dx, 16), D1y = lane_bcast(Dy, 16);
            const float O2x = lane_bcast(Ox, 32), O2y = lane_bcast(Oy, 32), D2x = lane_bcast(Dx, 32), D2y = lane_bcast(Dy, 32);
            const float O3x = lane_bcast(Ox, 48), O3y = lane_bcast(Oy, 48), D3x = lane_bcast(Dx, 48), D3y = lane_bcast(Dy, 48);
            // corner e: line e - 1 (O_p, D_p) meets line e (O_c, D_c) at O_c + v D_c
            float nx[4], ny[4];
            bool off = false;
#define A3_EDGE_MEET(e, Opx, Opy, Dpx, Dpy, Ocx, Ocy, Dcx, Dcy, qx, qy)                                        \
            {                                                                                                  \
                const float wx = Ocx - Opx, wy = Ocy - Opy, dd = Dpx * Dcy - Dpy * Dcx;                         \
                const float v = (wx * Dpy - wy * Dpx) / dd;                                                     \
                nx[e] = Ocx + v * Dcx; ny[e] = Ocy + v * Dcy;                                                   \
                off = off || dd == 0.0f || !(fabsf(nx[e] - qx) <= reach && fabsf(ny[e] - qy) <= reach);         \
            }
            A3_EDGE_MEET(0, O3x, O3y, D3x, D3y, O0x, O0y, D0x, D0y, q0x, q0y)
            A3_EDGE_MEET(1, O0x, O0y, D0x, D0y, O1x, O1y, D1x, D1y, q1x, q1y)
            A3_EDGE_MEET(2, O1x, O1y, D1x, D1y, O2x, O2y, D2x, D2y, q2x, q2y)
            A3_EDGE_MEET(3, O2x, O2y, D2x, D2y, O3x, O3y, D3x, D3y, q3x, q3y)
#undef A3_EDGE_MEET
            if (off) { revert = true; break; }
            const float ms = p.min_shift;
            const bool moved = fabsf(nx[0] - c0x) > ms || fabsf(ny[0] - c0y) > ms || fabsf(nx[1] - c1x) > ms || fabsf(ny[1] - c1y) > ms ||
                               fabsf(nx[2] - c2x) > ms || fabsf(ny[2] - c2y) > ms || fabsf(nx[3] - c3x) > ms || fabsf(ny[3] - c3y) > ms;
            c0x = nx[0]; c0y = ny[0]; c1x = nx[1]; c1y = ny[1]; c2x = nx[2]; c2y = ny[2]; c3x = nx[3]; c3y = ny[3];
            if (!moved) break;
        }
        if (revert) { c0x = q0x; c0y = q0y; c1x = q1x; c1y = q1y; c2x = q2x; c2y = q2y; c3x = q3x; c3y = q3y; }
        if (lane < 8) {
            const float v = lane == 0 ? c0x : lane == 1 ? c0y : lane == 2 ? c1x : lane == 3 ? c1y : lane == 4 ? c2x : lane == 5 ? c2y : lane == 6 ? c3x : c3y;
            out[8 * (size_t)u + lane] = v;
        }
    }
}

hipError_t launch_refine_edges(hipStream_t st, const RefineLaunch& r) {
    const uint32_t quads = r.markers ? r.n : r.n / 4u;
    if (quads == 0) return hipSuccess;
    const RefineParams* rp = reinterpret_cast<const RefineParams*>(r.params);
    const EdgeParams p{rp->win_half, rp->max_iterations, rp->cells, rp->relative_win, rp->min_shift};
    const int fmt = r.src.fmt;
    // (the library's own grey plane: one byte per pixel, which is its grey level; format_bpp has 0 for it on purpose)
    const bool plane = fmt == kFmtGreyPlane;
    const EdgePixel px{plane ? 1u : (uint32_t)format_bpp(fmt), plane ? 0u : (uint32_t)std::max(format_luma_offset(fmt), 0)};
    const dim3 grid(std::min<uint32_t>((quads + 3u) / 4u, 1024u));
#define A3_EDGE_LAUNCH(kind) hipLaunchKernelGGL(k_refine_edges<kind>, grid, dim3(256), 0, st, r.src, px, r.W, r.H, r.markers, r.n_dev, r.pts, r.cell_px, r.n, p, r.out, r.flags)
    if (fmt == A3_FMT_RGB8 || fmt == A3_FMT_RGBA8) A3_EDGE_LAUNCH(1);
    else if (fmt == A3_FMT_BGRA8) A3_EDGE_LAUNCH(2);
    else A3_EDGE_LAUNCH(0);
#undef A3_EDGE_LAUNCH
    return hipGetLastError();
}

}  // namespace a3
