// k_rectify.hip -- frame rectification (a3_rectify_frames): whole frames seen through a lens -> the frames of an ideal pinhole view.
// Not part of the reference: an extension stated in include/aruco3_hip.h, restated on the CPU by tests/rectify_oracle.c (a3o_rectify),
// which this kernel matches byte for byte; with the fisheye lens model (k_rectify<BPP, A3_DIST_FISHEYE>) tests/fisheye_oracle.c
// (a3o_fisheye_rectify).  The two models differ in rectify_map's forward model only.
//
// The map output pixel -> source position is the same for every frame of a call and is never written to memory: a lane computes it
// once for the kRun consecutive output pixels of one row that it owns, keeps per pixel the byte offset of the top-left tap, the two
// blend weights and three flag bits in registers, and then walks the kChunk frames of its workgroup (frame chunks are the grid's z
// axis).  A wave owns 64 * kRun = 256 consecutive pixels of one output row, a workgroup kTileH such rows, so a wave's stores are one
// contiguous piece of 256 / 768 / 1024 bytes made of 4- / 12- / 16-byte lane pieces; the last lane of a row stores its pixels byte by
// byte (as does every lane of a destination row that is not dword-aligned), and nothing past a row's pixels is written.
// Loads: the two taps of a source row are neighbours, so one load fetches both -- 2 / 6 / 8 bytes at the pixel pair's own address
// (any alignment; never aligned down, so never a byte outside the row), as a ushort, a dword + a ushort, or two dwords.  The pair
// starts at column min(x0, sw - 2): in the last column x1 = x0 and the pair's second pixel serves both taps.  A one-column source is
// read pixel by pixel.  Pixels that see nothing read the pair at (0, 0) and select `fill`; a wave none of whose pixels sees anything
// loads nothing.
// The grey form (a3_set_rectification, launch_rectify_grey) is the same kernel with another last step: per pixel the blended bytes go
// through luma_of in the source format's channel order and ONE byte is kept, so a lane's kRun pixels are one dword, a wave's row
// piece 256 contiguous bytes, and the two store rules above hold unchanged.  RGBA8 and BGRA8 are the same work in the pixel form and
// different work here, so the grey form is instantiated per format; the pixel-form instantiations compile as before.
// Packed 4:2:2 (A3_FMT_YUYV8, A3_FMT_UYVY8) has the grey form only: the pair load is one dword (Y U Y V or U Y V Y), the luma byte is the
// only one blended and is the output byte, so the result is the L8 form's on a plane of those luma bytes; a3_rectify_frames uses it too.
#include <algorithm>
#include <cstring>

#include "a3_common.h"
#include "a3_launch.h"
#include "a3_undistort.h"

namespace a3 {

constexpr int kRun = 4;              // consecutive output pixels of a lane
constexpr int kTileW = WAVE * kRun;  // output pixels of a wave: one row segment
constexpr int kTileH = 4;            // rows of a workgroup, one wave each
constexpr int kChunk = 16;           // frames a workgroup walks with one evaluation of the map

struct RectifyParams {
    float dfx, dfy, dcx, dcy, sfx, sfy, scx, scy;
    float R[9];
    float k1, k2, p1, p2, k3, k4, k5, k6;
    uint32_t sw, sh, dw, dh, n_frames, fill;
    unsigned long long src_row, src_frame, dst_row, dst_frame;
};

constexpr uint32_t kTapSecond = 1u, kTapNextRow = 2u, kTapInside = 4u;

// the contract's map for output pixel (j, i) -> whether it sees the source, and where.  MODEL: A3_DIST_RATIONAL (which serves
// A3_DIST_NONE with every coefficient 0) or A3_DIST_FISHEYE; the two differ in the forward model only.
template <int MODEL>
__device__ inline bool rectify_map(const RectifyParams& p, uint32_t j, uint32_t i, float* u_out, float* v_out) {
    const float a = ((float)j - p.dcx) / p.dfx, b = ((float)i - p.dcy) / p.dfy;
    const float X = (p.R[0]*a + p.R[3]*b) + p.R[6], Y = (p.R[1]*a + p.R[4]*b) + p.R[7], Wz = (p.R[2]*a + p.R[5]*b) + p.R[8];
    const float x = X / Wz, y = Y / Wz;
    float xd, yd;
    if constexpr (MODEL == A3_DIST_FISHEYE) {
        fisheye_forward(p.k1, p.k2, p.k3, p.k4, x, y, &xd, &yd);
    } else {
        const float r2 = x*x + y*y;
        const float radial = (1.0f + ((p.k3*r2 + p.k2)*r2 + p.k1)*r2) / (1.0f + ((p.k6*r2 + p.k5)*r2 + p.k4)*r2);
        xd = x*radial + (2.0f*p.p1*x*y + p.p2*(r2 + 2.0f*x*x));
        yd = y*radial + (p.p1*(r2 + 2.0f*y*y) + 2.0f*p.p2*x*y);
    }
    const float u = xd*p.sfx + p.scx, v = yd*p.sfy + p.scy;
    *u_out = u;
    *v_out = v;
    // (a NaN fails every comparison, an infinity the bounds: "finite" needs no test of its own)
    return Wz > 0.0f && u >= 0.0f && u <= (float)(p.sw - 1u) && v >= 0.0f && v <= (float)(p.sh - 1u);
}

template <int N> struct alignas(4) Words { uint32_t v[N]; };

// two neighbouring pixels of a row, 2 * BPP bytes from q (any alignment), the first pixel in the low bytes
template <int BPP> __device__ inline uint64_t load_pair(const uint8_t* q) {
    if constexpr (BPP == 1) {
        uint16_t t;
        memcpy(&t, q, 2);
        return t;
    } else if constexpr (BPP == 2) {   // (packed 4:2:2: Y U Y V or U Y V Y, the pair's two luma bytes among them)
        uint32_t t;
        memcpy(&t, q, 4);
        return t;
    } else if constexpr (BPP == 3) {
        uint32_t lo;
        uint16_t hi;
        memcpy(&lo, q, 4);
        memcpy(&hi, q + 4, 2);
        return (uint64_t)lo | ((uint64_t)hi << 32);
    } else {
        uint64_t t;
        memcpy(&t, q, 8);
        return t;
    }
}

// a one-column source: the pixel, twice
template <int BPP> __device__ inline uint64_t load_single(const uint8_t* q) {
    uint64_t t = 0;
#pragma unroll
    for (int c = 0; c < BPP; c++) t |= (uint64_t)q[c] << (8 * c);
    return t | (t << (8 * BPP));
}

// GREY: kPixelForm -- the output pixel in the input's format -- or the A3_FMT_* of the source, the grey form: the same map, taps and
// blend, then one byte per pixel, luma_of the pixel's rounded output bytes in that format's channel order (L8: the byte; alpha is never
// blended).  dst is then a plane of dst_row = dw, and a lane's kRun pixels are one dword.
constexpr int kPixelForm = -1;

template <int BPP, int MODEL, int GREY = kPixelForm>
__global__ __launch_bounds__(256) void k_rectify(const uint8_t* __restrict__ src, uint8_t* __restrict__ dst, const RectifyParams p) {
    constexpr bool grey = GREY != kPixelForm;
    constexpr int OBPP = grey ? 1 : BPP;   // bytes of an output pixel
    // packed 4:2:2 has the grey form only: of a pixel's two bytes the luma byte (C0) alone is blended, and it is the output byte as it
    // stands -- what the L8 form makes of a plane of those luma bytes
    constexpr bool yuv422 = GREY == A3_FMT_YUYV8 || GREY == A3_FMT_UYVY8;
    static_assert(BPP != 2 || yuv422, "two bytes per pixel: packed 4:2:2, the grey form");
    static_assert(!grey || BPP == (int)format_bpp(GREY), "the grey form's BPP is its format's");
    constexpr int C0 = GREY == A3_FMT_UYVY8 ? 1 : 0, C1 = yuv422 ? C0 + 1 : (grey && BPP == 4 ? 3 : BPP);   // the bytes of a pixel that are blended
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    const uint32_t i = blockIdx.y * kTileH + wave, j0 = blockIdx.x * kTileW + lane * kRun;
    if (i >= p.dh || j0 >= p.dw) return;
    const uint32_t run = min((uint32_t)kRun, p.dw - j0);
    const bool single = p.sw == 1u;

    unsigned long long off[kRun];
    float ax[kRun], ay[kRun];
    uint32_t flags[kRun];
    bool sees = false;
#pragma unroll
    for (int q = 0; q < kRun; q++) {
        off[q] = 0; ax[q] = 0.0f; ay[q] = 0.0f; flags[q] = 0;
        float u, v;
        if ((uint32_t)q < run && rectify_map<MODEL>(p, j0 + q, i, &u, &v)) {
            const float fx0 = floorf(u), fy0 = floorf(v);
            const uint32_t x0 = (uint32_t)fx0, y0 = (uint32_t)fy0;   // (0 <= u <= sw - 1, 0 <= v <= sh - 1)
            const uint32_t xb = single ? 0u : min(x0, p.sw - 2u);
            ax[q] = u - fx0;
            ay[q] = v - fy0;
            off[q] = (unsigned long long)y0 * p.src_row + (unsigned long long)xb * BPP;
            flags[q] = kTapInside | (x0 != xb ? kTapSecond : 0u) | (y0 + 1u <= p.sh - 1u ? kTapNextRow : 0u);
            sees = true;
        }
    }
    const bool wave_sees = __any(sees);

    const uint32_t f0 = blockIdx.z * kChunk, f1 = min(f0 + (uint32_t)kChunk, p.n_frames);
    for (uint32_t f = f0; f < f1; f++) {
        const uint8_t* s = src + (unsigned long long)f * p.src_frame;
        uint8_t* d = dst + (unsigned long long)f * p.dst_frame + (unsigned long long)i * p.dst_row + (unsigned long long)j0 * OBPP;
        uint32_t w[OBPP] = {};   // the lane's kRun * OBPP output bytes
        if (wave_sees) {
            uint64_t top[kRun], bot[kRun];
#pragma unroll
            for (int q = 0; q < kRun; q++) {
                const uint8_t* t0 = s + off[q];
                const uint8_t* t1 = t0 + ((flags[q] & kTapNextRow) ? p.src_row : 0ull);
                top[q] = single ? load_single<BPP>(t0) : load_pair<BPP>(t0);
                bot[q] = single ? load_single<BPP>(t1) : load_pair<BPP>(t1);
            }
#pragma unroll
            for (int q = 0; q < kRun; q++) {
                const int sh0 = (flags[q] & kTapSecond) ? 8 * BPP : 0;
                const float bx = 1.0f - ax[q], by = 1.0f - ay[q];
                uint32_t ch[3] = {};   // (the grey form: the pixel's colour bytes)
#pragma unroll
                for (int c = C0; c < C1; c++) {
                    const float i00 = (float)((uint32_t)(top[q] >> (sh0 + 8 * c)) & 0xFFu), i01 = (float)((uint32_t)(top[q] >> (8 * (BPP + c))) & 0xFFu);
                    const float i10 = (float)((uint32_t)(bot[q] >> (sh0 + 8 * c)) & 0xFFu), i11 = (float)((uint32_t)(bot[q] >> (8 * (BPP + c))) & 0xFFu);
                    const float val = by*(bx*i00 + ax[q]*i01) + ay[q]*(bx*i10 + ax[q]*i11);
                    const uint32_t out = (flags[q] & kTapInside) ? (uint32_t)fminf(floorf(val + 0.5f), 255.0f) : p.fill;
                    if constexpr (grey) {
                        ch[c - C0] = out;
                    } else {
                        const int byte = q * BPP + c;
                        w[byte >> 2] |= out << (8 * (byte & 3));
                    }
                }
                if constexpr (grey)
                    w[0] |= (BPP == 1 || yuv422 ? ch[0] : (GREY == A3_FMT_BGRA8 ? luma_of(ch[2], ch[1], ch[0]) : luma_of(ch[0], ch[1], ch[2]))) << (8 * q);
            }
        } else {
#pragma unroll
            for (int k = 0; k < OBPP; k++) w[k] = (grey && BPP != 1 && !yuv422 ? luma_of(p.fill, p.fill, p.fill) : p.fill) * 0x01010101u;
        }
        if (run == (uint32_t)kRun && (reinterpret_cast<uintptr_t>(d) & 3u) == 0) {
            Words<OBPP> o;
#pragma unroll
            for (int k = 0; k < OBPP; k++) o.v[k] = w[k];
            *reinterpret_cast<Words<OBPP>*>(d) = o;   // one 4- / 12- / 16-byte store
        } else {   // the end of a row, or a destination row that is not dword-aligned
#pragma unroll
            for (int byte = 0; byte < kRun * OBPP; byte++)
                if ((uint32_t)byte < run * OBPP) d[byte] = (uint8_t)(w[byte >> 2] >> (8 * (byte & 3)));
        }
    }
}

void rectify_grid(uint32_t dw, uint32_t dh, uint32_t n_frames, uint32_t* tiles_x, uint32_t* tiles_y, uint32_t* chunks) {
    *tiles_x = (dw + kTileW - 1) / kTileW;
    *tiles_y = (dh + kTileH - 1) / kTileH;
    *chunks = (n_frames + kChunk - 1) / kChunk;
}

// the kernel's parameters for r on frames of these strides (lens coefficients taken as 0 with A3_DIST_NONE)
static RectifyParams rectify_params(const a3_rectify& r, uint32_t n_frames, size_t src_row, size_t src_frame, size_t dst_row, size_t dst_frame) {
    const bool lens = r.distortion.model == A3_DIST_FISHEYE || r.distortion.model == A3_DIST_RATIONAL;
    const a3_distortion& k = r.distortion;
    RectifyParams p{};
    p.dfx = r.dst.focal_x; p.dfy = r.dst.focal_y; p.dcx = r.dst.principal_x; p.dcy = r.dst.principal_y;
    p.sfx = r.src.focal_x; p.sfy = r.src.focal_y; p.scx = r.src.principal_x; p.scy = r.src.principal_y;
    for (int m = 0; m < 9; m++) p.R[m] = r.rotation[m];
    p.k1 = lens ? k.k1 : 0.0f; p.k2 = lens ? k.k2 : 0.0f; p.p1 = lens ? k.p1 : 0.0f; p.p2 = lens ? k.p2 : 0.0f;
    p.k3 = lens ? k.k3 : 0.0f; p.k4 = lens ? k.k4 : 0.0f; p.k5 = lens ? k.k5 : 0.0f; p.k6 = lens ? k.k6 : 0.0f;
    p.sw = r.src.image_width; p.sh = r.src.image_height; p.dw = r.dst.image_width; p.dh = r.dst.image_height;
    p.n_frames = n_frames; p.fill = r.fill;
    p.src_row = src_row; p.src_frame = src_frame; p.dst_row = dst_row; p.dst_frame = dst_frame;
    return p;
}

hipError_t launch_rectify(hipStream_t st, const RectifyLaunch& l) {
    const a3_rectify& r = *l.r;
    const uint8_t* const src = l.src; uint8_t* const dst = l.dst; const int bpp = l.bpp;
    const bool fisheye = r.distortion.model == A3_DIST_FISHEYE;
    const RectifyParams p = rectify_params(r, l.n_frames, l.src_row, l.src_frame, l.dst_row, l.dst_frame);
    uint32_t tx, ty, tz;
    rectify_grid(p.dw, p.dh, l.n_frames, &tx, &ty, &tz);
    const dim3 grid(tx, ty, tz), block(WAVE * kTileH);
    if (fisheye) {   // (p1 p2 k5 k6 are 0 there: a3_rectify_frames checked)
        if (bpp == 1) hipLaunchKernelGGL((k_rectify<1, A3_DIST_FISHEYE>), grid, block, 0, st, src, dst, p);
        else if (bpp == 3) hipLaunchKernelGGL((k_rectify<3, A3_DIST_FISHEYE>), grid, block, 0, st, src, dst, p);
        else hipLaunchKernelGGL((k_rectify<4, A3_DIST_FISHEYE>), grid, block, 0, st, src, dst, p);
    } else {
        if (bpp == 1) hipLaunchKernelGGL((k_rectify<1, A3_DIST_RATIONAL>), grid, block, 0, st, src, dst, p);
        else if (bpp == 3) hipLaunchKernelGGL((k_rectify<3, A3_DIST_RATIONAL>), grid, block, 0, st, src, dst, p);
        else hipLaunchKernelGGL((k_rectify<4, A3_DIST_RATIONAL>), grid, block, 0, st, src, dst, p);
    }
    return hipGetLastError();
}

template <int MODEL> static hipError_t launch_grey_form(hipStream_t st, dim3 grid, dim3 block, int fmt, const uint8_t* src, uint8_t* grey, const RectifyParams& p) {
    return with_format(fmt, [&](auto F) {
        constexpr int FMT = decltype(F)::value;
        hipLaunchKernelGGL((k_rectify<(int)format_bpp(FMT), MODEL, FMT>), grid, block, 0, st, src, grey, p);
        return hipGetLastError();
    });
}

hipError_t launch_rectify_grey(hipStream_t st, const RectifyGreyLaunch& l) {
    const a3_rectify& r = *l.r;
    const size_t dw = r.dst.image_width, dh = r.dst.image_height;
    const RectifyParams p = rectify_params(r, l.n_frames, l.src_row, l.src_frame, l.dst_row ? l.dst_row : dw, l.dst_row ? l.dst_frame : dw * dh);
    uint32_t tx, ty, tz;
    rectify_grid(p.dw, p.dh, l.n_frames, &tx, &ty, &tz);
    const dim3 grid(tx, ty, tz), block(WAVE * kTileH);
    return r.distortion.model == A3_DIST_FISHEYE ? launch_grey_form<A3_DIST_FISHEYE>(st, grid, block, l.fmt, l.src, l.grey, p)
                                                 : launch_grey_form<A3_DIST_RATIONAL>(st, grid, block, l.fmt, l.src, l.grey, p);
}

}  // namespace a3
