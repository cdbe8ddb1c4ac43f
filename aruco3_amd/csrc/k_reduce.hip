// k_reduce.hip -- detection on reduced frames (a3_reduce_frames, a3_set_reduction): the box-filtered grey plane of full-size frames, and
// the map of a marker list's integer corners back to full size.  Not part of the reference: an extension stated in include/aruco3_hip.h,
// restated in numpy by tests/reduced_cases.py (reduce), which k_reduce_frames matches byte for byte.
//
// k_reduce_frames<FMT, F>: output byte (j, i) = (S + F*F/2) / (F*F), S the sum of luma_of over the F x F source block at (F j, F i).
// Like the threshold kernel it reads whole row segments: a lane owns kRun = T_LPX = 16 consecutive source pixels of the F source rows of
// one output row, fetched with k_threshold_k1.h's loaders (load_vec: 16-byte loads where base and strides are 16-byte aligned and the
// run lies inside the block columns; load_raw's byte gather otherwise, i.e. in the lane that holds a row's end and on unaligned
// frames) and turned into 16 grey bytes per row by grey_row.  The F rows are summed column-wise as packed u16 pairs (even bytes and odd
// bytes of each grey dword apart: at most 4 x 255 per half, no carries).  Columns at and behind F * w -- the W mod F trailing ones --
// belong to no block: a lane never loads them (the loaders see a row of F * w pixels), and rows at and behind F * h are never addressed.
//   F = 2, 4: F divides the run, so a lane forms its 16 / F block sums in registers: even + odd sums are the horizontal pairs (F = 2:
//     two outputs per dword, 8 bytes per lane), and low + high half of those the fours (F = 4: 4 bytes per lane).  A workgroup is
//     kTileH waves, one output row each; a wave's row piece is 512 / 256 contiguous bytes.
//   F = 3 does not divide the run: the plainer path, through LDS.  A workgroup is kWaves3 = 3 waves side by side on ONE output row,
//     3 x 1024 = 3072 source columns = 1024 whole blocks; every lane parks its 16 column sums (u16) in LDS, and behind a barrier lane t
//     (and t + 192, for t < 64) adds three neighbours for each of the 4 outputs 4 t .. 4 t + 3 and divides by 9.  The workgroup walks
//     its kTileH rows one after another, two LDS buffers in turn so that one barrier per row suffices.  (What it costs: DESIGN.md 4.17.)
// Stores: a lane's 4 or 8 output bytes leave as whole dwords where the destination address is dword-aligned and the row holds them;
// the last lane of a row stores its remaining bytes one by one, as does every lane of a row that is not dword-aligned; nothing past a
// row's w bytes is written.  Frames: the grid's z axis in chunks of kChunk, walked by the workgroup.
//
// k_scale_markers: one lane per marker of a device-resident list (count on the device): corners[8] -> F c + F / 2, in place.
#include <algorithm>

#include "a3_common.h"
#include "a3_launch.h"
#include "k_threshold_k1.h"

namespace a3 {

constexpr int kRun = 16;                // consecutive source pixels of a lane
static_assert(kRun == T_LPX, "a lane's run is what the threshold kernels' loaders fetch (a3_threshold_plan.h)");
constexpr int kWaveRun = WAVE * kRun;   // source pixels of a wave: one row segment
constexpr int kTileH = 4;               // output rows of a workgroup
constexpr int kChunk = 4;               // frames a workgroup walks
constexpr int kWaves3 = 3;              // factor 3: waves of a workgroup, side by side on one row (3 * kWaveRun source columns = kWaveRun whole blocks)

struct ReduceParams {
    uint32_t w, h, n_frames;            // the reduced size
    int aligned;                        // src base and both src strides are multiples of 16
    unsigned long long src_row, src_frame, dst_row, dst_frame;
};

// a lane's output bytes (NW dwords, `nout` of them inside the row) -> d
template <int NW>
__device__ __forceinline__ void store_run(uint8_t* d, const uint32_t (&o)[NW], uint32_t nout) {
    const bool dword = (reinterpret_cast<uintptr_t>(d) & 3u) == 0;
#pragma unroll
    for (int k = 0; k < NW; k++) {
        if (dword && nout >= 4u * (k + 1)) {
            *reinterpret_cast<uint32_t*>(d + 4 * k) = o[k];
        } else {
#pragma unroll
            for (int b = 0; b < 4; b++)
                if ((uint32_t)(4 * k + b) < nout) d[4 * k + b] = (uint8_t)(o[k] >> (8 * b));
        }
    }
}

// the column sums of F source rows of the lane's run: E[i] = sums of pixels 4 i (low half) and 4 i + 2, O[i] = of 4 i + 1 and 4 i + 3.
// x0: the run's first column; Wc = F * w, the columns that belong to blocks; y0: the first of the F rows
template <int FMT, int F>
__device__ __forceinline__ void column_sums(const uint8_t* __restrict__ frame, size_t row_stride, int x0, int y0, int Wc, int Hc, bool aligned,
                                            uint32_t (&E)[T_NG], uint32_t (&O)[T_NG]) {
    RawRow<FMT> raw[F];
#pragma unroll
    for (int r = 0; r < F; r++) load_raw<FMT>(frame, row_stride, x0, y0 + r, Wc, Hc, aligned, raw[r]);
#pragma unroll
    for (int i = 0; i < T_NG; i++) { E[i] = 0u; O[i] = 0u; }
#pragma unroll
    for (int r = 0; r < F; r++) {
        uint32_t g[T_NG];
        grey_row<FMT>(raw[r], g);
#pragma unroll
        for (int i = 0; i < T_NG; i++) { E[i] += g[i] & 0x00FF00FFu; O[i] += (g[i] >> 8) & 0x00FF00FFu; }
    }
}

template <int FMT, int F>
__global__ __launch_bounds__(F == 3 ? WAVE * kWaves3 : WAVE * kTileH) void k_reduce_frames(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst,
                                                                                         const ReduceParams p) {
    static_assert(F == 2 || F == 3 || F == 4, "factors 2, 3 and 4");
    const int Wc = (int)p.w * F, Hc = (int)p.h * F;
    const uint32_t f0 = blockIdx.z * kChunk, f1 = min(f0 + (uint32_t)kChunk, p.n_frames);
    if constexpr (F != 3) {
        constexpr int NOUT = kRun / F, NW = NOUT / 4;   // output bytes / dwords of a lane
        const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
        const uint32_t i = blockIdx.y * kTileH + wave;
        const int x0 = (int)blockIdx.x * kWaveRun + (int)lane * kRun;
        if (i >= p.h || x0 >= Wc) return;
        const uint32_t j0 = (uint32_t)x0 / F, nout = min((uint32_t)NOUT, p.w - j0);
        for (uint32_t f = f0; f < f1; f++) {
            uint32_t E[T_NG], O[T_NG], o[NW];
            column_sums<FMT, F>(src + (unsigned long long)f * p.src_frame, p.src_row, x0, (int)i * F, Wc, Hc, p.aligned != 0, E, O);
            if constexpr (F == 2) {
                // T = E + O: the sums of blocks 2 q (low half) and 2 q + 1; (T + 2) >> 2 per half, then four bytes to a dword
                uint32_t v[T_NG];
#pragma unroll
                for (int q = 0; q < T_NG; q++) v[q] = ((E[q] + O[q] + 0x00020002u) >> 2) & 0x00FF00FFu;
#pragma unroll
                for (int k = 0; k < NW; k++) o[k] = __builtin_amdgcn_perm(v[2 * k + 1], v[2 * k], 0x06040200u);
            } else {
                o[0] = 0u;
#pragma unroll
                for (int q = 0; q < T_NG; q++) {
                    const uint32_t t = E[q] + O[q];
                    o[0] |= ((((t & 0xFFFFu) + (t >> 16)) + 8u) >> 4) << (8 * q);
                }
            }
            store_run<NW>(dst + (unsigned long long)f * p.dst_frame + (unsigned long long)i * p.dst_row + j0, o, nout);
        }
    } else {
        __shared__ alignas(16) uint32_t s_cs[2][kWaves3 * kWaveRun / 2];   // column sums of the workgroup's 3072 columns, two u16 to a word
        const uint32_t tid = threadIdx.x;
        const int x0 = (int)blockIdx.x * (kWaves3 * kWaveRun) + (int)tid * kRun;
        const uint32_t jb = blockIdx.x * (uint32_t)kWaveRun;   // the workgroup's first output column
        int buf = 0;
        for (uint32_t f = f0; f < f1; f++) {
            for (uint32_t ti = 0; ti < (uint32_t)kTileH; ti++) {
                const uint32_t i = blockIdx.y * kTileH + ti;
                if (i >= p.h) break;   // (the same for the whole workgroup)
                uint32_t E[T_NG], O[T_NG];
                column_sums<FMT, 3>(src + (unsigned long long)f * p.src_frame, p.src_row, x0, (int)i * 3, Wc, Hc, p.aligned != 0, E, O);
                uint4* park = reinterpret_cast<uint4*>(&s_cs[buf][tid * (kRun / 2)]);
                park[0] = make_uint4((E[0] & 0xFFFFu) | (O[0] << 16), (E[0] >> 16) | (O[0] & 0xFFFF0000u),
                                     (E[1] & 0xFFFFu) | (O[1] << 16), (E[1] >> 16) | (O[1] & 0xFFFF0000u));
                park[1] = make_uint4((E[2] & 0xFFFFu) | (O[2] << 16), (E[2] >> 16) | (O[2] & 0xFFFF0000u),
                                     (E[3] & 0xFFFFu) | (O[3] << 16), (E[3] >> 16) | (O[3] & 0xFFFF0000u));
                __syncthreads();
                // 256 runs of 4 outputs for 192 lanes.  (The buffer read here is written again two rows on, behind the next row's barrier.)
                for (uint32_t t = tid; t < (uint32_t)kWaveRun / 4; t += WAVE * kWaves3) {
                    const uint32_t j0 = jb + 4u * t;
                    if (j0 >= p.w) break;
                    const uint2* cs = reinterpret_cast<const uint2*>(&s_cs[buf][6u * t]);   // 12 u16 from byte 24 t
                    const uint2 a = cs[0], b = cs[1], c = cs[2];
                    const uint32_t s0 = (a.x & 0xFFFFu) + (a.x >> 16) + (a.y & 0xFFFFu), s1 = (a.y >> 16) + (b.x & 0xFFFFu) + (b.x >> 16);
                    const uint32_t s2 = (b.y & 0xFFFFu) + (b.y >> 16) + (c.x & 0xFFFFu), s3 = (c.x >> 16) + (c.y & 0xFFFFu) + (c.y >> 16);
                    const uint32_t o[1] = {(s0 + 4u) / 9u | ((s1 + 4u) / 9u) << 8 | ((s2 + 4u) / 9u) << 16 | ((s3 + 4u) / 9u) << 24};
                    store_run<1>(dst + (unsigned long long)f * p.dst_frame + (unsigned long long)i * p.dst_row + j0, o, min(4u, p.w - j0));
                }
                buf ^= 1;
            }
        }
    }
}

template <int FMT>
static void launch_reduce_fmt(hipStream_t st, uint32_t factor, const uint8_t* src, uint8_t* dst, const ReduceParams& p) {
    const uint32_t ty = (p.h + kTileH - 1) / kTileH, tz = (p.n_frames + kChunk - 1) / kChunk;
    if (factor == 3) {
        const dim3 grid((p.w + kWaveRun - 1) / kWaveRun, ty, tz), block(WAVE * kWaves3);
        hipLaunchKernelGGL((k_reduce_frames<FMT, 3>), grid, block, 0, st, src, dst, p);
    } else {
        const dim3 grid((p.w * factor + kWaveRun - 1) / kWaveRun, ty, tz), block(WAVE * kTileH);
        if (factor == 2) hipLaunchKernelGGL((k_reduce_frames<FMT, 2>), grid, block, 0, st, src, dst, p);
        else hipLaunchKernelGGL((k_reduce_frames<FMT, 4>), grid, block, 0, st, src, dst, p);
    }
}

hipError_t launch_reduce_frames(hipStream_t st, const ReduceLaunch& l) {
    ReduceParams p{};
    p.w = l.W / l.factor; p.h = l.H / l.factor; p.n_frames = l.n_frames;
    p.aligned = (reinterpret_cast<uintptr_t>(l.src) % 16 == 0) && (l.src_row % 16 == 0) && (l.src_frame % 16 == 0);
    p.src_row = l.src_row; p.src_frame = l.src_frame; p.dst_row = l.dst_row; p.dst_frame = l.dst_frame;
    // (packed 4:2:2: grey_row keeps the luma bytes)
    return with_format(l.fmt, [&](auto F) { launch_reduce_fmt<decltype(F)::value>(st, l.factor, l.src, l.dst, p); return hipGetLastError(); });
}

__global__ __launch_bounds__(256) void k_scale_markers(a3_marker* __restrict__ markers, const unsigned int* __restrict__ n_dev, uint32_t cap, uint32_t factor) {
    const uint32_t m = blockIdx.x * blockDim.x + threadIdx.x;
    if (m >= min(*n_dev, cap)) return;
#pragma unroll
    for (int c = 0; c < 8; c++) markers[m].corners[c] = factor * markers[m].corners[c] + factor / 2u;
}

hipError_t launch_scale_markers(hipStream_t st, const ScaleMarkersLaunch& s) {
    if (s.n == 0) return hipSuccess;
    hipLaunchKernelGGL(k_scale_markers, dim3((s.n + 255u) / 256u), dim3(256), 0, st, s.markers, s.n_dev, s.n, s.factor);
    return hipGetLastError();
}

}  // namespace a3
