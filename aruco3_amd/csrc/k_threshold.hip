// k_threshold.hip -- K1: pixels -> grey (into_luma8) -> 15x15 adaptive threshold, fused.
//
// Replaces `image.into_luma8()` + `imageproc::contrast::adaptive_threshold(&grey, 7)`
// (src/aruco.rs:60-61).  Pure integer, so every output byte must equal the oracle's.
//
//   grey  L = (2126 R + 7152 G + 722 B) / 10000          (u32, truncating)
//   white iff L >= floor(sum / area) over the window clipped to the image
//         <=> sum < (L + 1) * area                        (no division)
//
// What must move per pixel: 3 B read (RGB8) + 1/8 B written -- the thresholded image leaves the kernel bit-packed
// (a3_common.h: words_per_row), which is all the contour stage reads, and no grey plane is written unless somebody asks
// for Detection.grey (debug taps).  No LDS, no barriers: one wave walks down a strip of 1024 columns, lane l owns 16
// consecutive columns, and everything between the 48-byte row slice it loads and the 16 bits it stores stays in
// registers (k_grey_threshold7 below).  The arithmetic is laid out for instruction count -- the first register-resident
// version spent 21 VALU lane-instructions per pixel and was issue-bound at 0.56 of the HBM roofline:
//   grey        two v_dot4_u32_u8 + one v_mul_hi_u32_u24 per pixel, the >> 5 writes the byte into place (SDWA dst_sel)
//   horizontal  15-wide sums of the NEW grey row first, on bytes: four v_sad_u8 start two chains (pixels 0 and 8), each
//               slide step advances both chains with two packed-u16 instructions (byte pairs come from v_perm_b32)
//   vertical    15-row sliding sums of those row sums as packed u16 pairs: v_pk_add_u16 / v_pk_sub_u16 against a ring of
//               the last 15 rows of row sums (15 * 255 * 15 < 2^16)
//   compare     sum < (L + 1) * area on pairs: v_pk_mad_u16, saturating v_pk_sub_u16, v_pk_min_u16, bits shifted in by
//               another v_pk_mad_u16
// Out-of-image pixels count as 0, which makes the unclipped sum equal the clipped one; the area is the clipped window.
#include "k_threshold_k1.h"

namespace a3 {

// ---- generic radius: plain kernels (correct for any threshold_window and any alignment, not tuned): what is left for them are
// radii above 31 and radius 0 (a3_threshold_plan.h: threshold_path) ----
// four consecutive pixels per thread: dword loads and one dword store where the row is 4-byte aligned, bytes otherwise
template <int FMT>
__global__ void k_grey_generic(const uint8_t* __restrict__ pixels, size_t row_stride, size_t frame_stride, int W, int H,
                               uint8_t* __restrict__ grey) {
    const int x = 4 * (blockIdx.x * blockDim.x + threadIdx.x), y = blockIdx.y;
    if (x >= W) return;
    const uint32_t f = blockIdx.z;
    constexpr int BPP = RawRow<FMT>::BPP;
    constexpr int LO = FMT == A3_FMT_UYVY8 ? 1 : 0;   // packed 4:2:2: the luma byte of a pixel's two (the grey level as it stands)
    const uint8_t* p = pixels + (size_t)f * frame_stride + (size_t)y * row_stride + (size_t)x * BPP;
    uint8_t* out = grey + (size_t)f * W * H + (size_t)y * W + x;
    auto luma = [](uint32_t b0, uint32_t b1, uint32_t b2) -> uint32_t { return FMT == A3_FMT_BGRA8 ? luma_of(b2, b1, b0) : luma_of(b0, b1, b2); };
    if (x + 3 < W && (reinterpret_cast<uintptr_t>(p) & 3) == 0 && (reinterpret_cast<uintptr_t>(out) & 3) == 0) {
        uint32_t d[BPP];
#pragma unroll
        for (int i = 0; i < BPP; i++) d[i] = reinterpret_cast<const uint32_t*>(p)[i];
        uint32_t g = 0;
#pragma unroll
        for (int i = 0; i < 4; i++) {
            uint32_t v;
            if (BPP == 1) v = (d[0] >> (8 * i)) & 0xFFu;
            else if (BPP == 2) v = (d[i >> 1] >> (8 * (2 * (i & 1) + LO))) & 0xFFu;
            else {
                const int b = i * BPP;   // byte offset of pixel i inside d[]
                auto byte = [&](int k) -> uint32_t { return (d[k >> 2] >> (8 * (k & 3))) & 0xFFu; };
                v = luma(byte(b), byte(b + 1), byte(b + 2));
            }
            g |= v << (8 * i);
        }
        *reinterpret_cast<uint32_t*>(out) = g;
        return;
    }
    for (int i = 0; i < 4 && x + i < W; i++) {
        const uint8_t* q = p + (size_t)i * BPP;
        out[i] = BPP == 1 ? q[0] : (BPP == 2 ? q[LO] : (uint8_t)luma(q[0], q[1], q[2]));
    }
}

// one wave per packed word: 64 consecutive pixels, result gathered with a ballot
__global__ __launch_bounds__(64) void k_threshold_generic(const uint8_t* __restrict__ grey, int W, int H, int radius, uint64_t* __restrict__ bits) {
    const int x = blockIdx.x * 64 + threadIdx.x, y = blockIdx.y;
    const uint8_t* g = grey + (size_t)blockIdx.z * W * H;
    bool white = false;
    if (x < W) {
        const int ylo = y > radius ? y - radius : 0, yhi = (long long)y + radius < H - 1 ? y + radius : H - 1;
        const int xlo = x > radius ? x - radius : 0, xhi = (long long)x + radius < W - 1 ? x + radius : W - 1;
        unsigned long long sum = 0;
        for (int yy = ylo; yy <= yhi; yy++)
            for (int xx = xlo; xx <= xhi; xx++) sum += g[(size_t)yy * W + xx];
        const unsigned long long area = (unsigned long long)(yhi - ylo + 1) * (unsigned long long)(xhi - xlo + 1);
        const unsigned long long gv = g[(size_t)y * W + x];
        white = sum < (gv + 1) * area;
    }
    const unsigned long long m = __ballot(white);
    const size_t wpr = words_per_row((uint32_t)W);
    if (threadIdx.x == 0) bits[(size_t)blockIdx.z * wpr * H + (size_t)y * wpr + blockIdx.x] = m;
}

// Radii 32..128, separable: horizontal sums of the grey plane into a u16 plane (2R+1 <= 257 values of at most 255), then a
// vertical running sum per column with the compare.  Plain kernels (no register ring: (2R+1)^2 * 256 no longer fits 16 bits), but
// the work per pixel no longer grows with the window's AREA as in k_threshold_generic.
// k_hsum_generic: a workgroup covers 1024 columns of one row, four consecutive outputs per thread (a sliding sum: 2R + 4 byte reads for
// four results); the row segment is staged in LDS with dword loads.
constexpr int kHsumCols = 1024;
__global__ __launch_bounds__(256) void k_hsum_generic(const uint8_t* __restrict__ grey, int W, int H, int radius, uint16_t* __restrict__ hsum) {
    extern __shared__ uint8_t s_row[];   // grey bytes of columns x0 - R4 .. of this row, R4 = R rounded up to 4 (zeros outside the image)
    const int x0 = blockIdx.x * kHsumCols, y = blockIdx.y;
    const size_t base = ((size_t)blockIdx.z * H + y) * W;
    const int r4 = (radius + 3) & ~3, span = kHsumCols + 2 * r4;
    const bool row_aligned = ((base & 3) == 0) && ((W & 3) == 0);
    for (int i = threadIdx.x * 4; i < span; i += 1024) {
        const int x = x0 - r4 + i;
        uint32_t v = 0;
        if (row_aligned && x >= 0 && x + 3 < W) v = *reinterpret_cast<const uint32_t*>(grey + base + x);
        else {
#pragma unroll
            for (int b = 0; b < 4; b++) if (x + b >= 0 && x + b < W) v |= (uint32_t)grey[base + x + b] << (8 * b);
        }
        *reinterpret_cast<uint32_t*>(s_row + i) = v;
    }
    __syncthreads();
    const int x = x0 + 4 * (int)threadIdx.x;
    if (x >= W) return;
    const uint8_t* p = s_row + r4 + 4 * threadIdx.x - radius;   // p[k] = grey(x - R + k)
    uint32_t sum = 0;
    for (int k = 0; k <= 2 * radius; k++) sum += p[k];
    uint32_t out[4];
    out[0] = sum;
#pragma unroll
    for (int j = 1; j < 4; j++) { sum += p[2 * radius + j]; sum -= p[j - 1]; out[j] = sum; }
#pragma unroll
    for (int j = 0; j < 4; j++) if (x + j < W) hsum[base + x + j] = (uint16_t)out[j];
}

// one wave per 64 columns and strip of rows: lane = column, V = sum of hsum over the rows y - R .. y + R inside the image; the loads of
// eight rows are issued together (they do not depend on V), then the eight rows are finished in order
constexpr int kVsumRows = 128;
__global__ __launch_bounds__(64) void k_vsum_threshold_generic(const uint8_t* __restrict__ grey, const uint16_t* __restrict__ hsum, int W, int H, int radius,
                                                               uint64_t* __restrict__ bits) {
    const int x = blockIdx.x * 64 + threadIdx.x, y0 = blockIdx.y * kVsumRows, y1 = min(H, y0 + kVsumRows);
    const size_t plane = (size_t)blockIdx.z * W * H;
    const bool in = x < W;
    const int xc = in ? x : W - 1;
    const uint16_t* hs = hsum + plane + xc;
    const uint8_t* g = grey + plane + xc;
    const uint32_t ax = in ? (uint32_t)(min(x + radius, W - 1) - max(x - radius, 0) + 1) : 0u;
    uint32_t V = 0;
    for (int yy = max(y0 - radius, 0); yy <= min(y0 + radius, H - 1); yy++) V += hs[(size_t)yy * W];
    const size_t wpr = words_per_row((uint32_t)W);
    uint64_t* brow = bits + (size_t)blockIdx.z * wpr * H + blockIdx.x;
    constexpr int B = 8;
    for (int yb = y0; yb < y1; yb += B) {
        uint32_t gv[B], add[B], sub[B];
#pragma unroll
        for (int u = 0; u < B; u++) {   // unconditional loads from clamped rows, masked afterwards
            const int y = yb + u, ya = y + radius + 1, ys = y - radius;
            gv[u] = g[(size_t)min(y, H - 1) * W];
            add[u] = hs[(size_t)min(ya, H - 1) * W] & (0u - (uint32_t)(ya < H));
            sub[u] = hs[(size_t)max(ys, 0) * W] & (0u - (uint32_t)(ys >= 0));
        }
#pragma unroll
        for (int u = 0; u < B; u++) {
            const int y = yb + u;
            if (y >= y1) break;
            const uint32_t ay = (uint32_t)(min(y + radius, H - 1) - max(y - radius, 0) + 1);
            const bool white = in && V < (gv[u] + 1u) * (ax * ay);     // sum < (L + 1) * area  <=>  L >= floor(sum / area)
            const unsigned long long m = __ballot(white);
            if (threadIdx.x == 0) brow[(size_t)y * wpr] = m;
            V += add[u]; V -= sub[u];
        }
    }
}

// ---- host launcher -------------------------------------------------------------------------
// one launcher per path of a3_threshold_plan.h's threshold_path; the fused kernels of radii 1..3 and 4..6 are instantiated in
// translation units of their own (k_threshold_r1.hip, _r2.hip), the ring kernel's in k_threshold_big.hip
hipError_t launch_grey_threshold(hipStream_t st, const ThresholdLaunch& t) {
    const int W = t.W, H = t.H, radius = (int)t.radius; const uint32_t n = t.n;
    auto grey_plane = [&] {   // what the two plain paths read
        return with_format(t.fmt, [&](auto F) {
            hipLaunchKernelGGL(k_grey_generic<decltype(F)::value>, dim3((W + 255) / 256, H, n), dim3(64), 0, st, t.pixels, t.row_stride, t.frame_stride, W, H, t.grey);
            return hipGetLastError();
        });
    };
    switch (threshold_path(t.radius)) {
        case ThresholdPath::K1: return t.radius <= 3 ? launch_k1_r1(st, t) : t.radius <= 6 ? launch_k1_r2(st, t) : launch_k1<7>(st, t);
        case ThresholdPath::Ring: return launch_ring_threshold(st, t);
        case ThresholdPath::Separable:   // row sums (<= 257 * 255 fit a u16), then a running column sum with the compare
            if (t.hsum_tmp) {
                if (hipError_t e = grey_plane(); e != hipSuccess) return e;
                hipLaunchKernelGGL(k_hsum_generic, dim3((W + kHsumCols - 1) / kHsumCols, H, n), dim3(256), kHsumCols + 2 * ((t.radius + 3) & ~3u) + 16, st, t.grey, W, H, radius, t.hsum_tmp);
                hipLaunchKernelGGL(k_vsum_threshold_generic, dim3(words_per_row((uint32_t)W), (H + kVsumRows - 1) / kVsumRows, n), dim3(64), 0, st, t.grey, t.hsum_tmp,
                                   W, H, radius, t.bits);
                return hipGetLastError();
            }
            [[fallthrough]];   // no plane of row sums: brute force, as ever
        case ThresholdPath::Brute:
            if (hipError_t e = grey_plane(); e != hipSuccess) return e;
            hipLaunchKernelGGL(k_threshold_generic, dim3(words_per_row((uint32_t)W), H, n), dim3(64), 0, st, t.grey, W, H, radius, t.bits);
            return hipGetLastError();
    }
    return hipErrorInvalidValue;
}

}  // namespace a3
