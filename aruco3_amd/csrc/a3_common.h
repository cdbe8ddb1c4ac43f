// a3_common.h -- shared device/host declarations for libaruco3_hip.so (gfx950 only).
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "../../include/aruco3_hip.h"
#include "a3_batch_head.h"   // DeviceCounters, the kErr* flags, the scratch words of a batch, kMaxChunkFrames, the shard counts

namespace a3 {

constexpr int WAVE = 64;

// ---- contour graph ("darts") ------------------------------------------------------------
// A dart is (pixel, direction of a foreground 8-neighbour).  Directions are numbered
// clockwise on screen starting at west, the ring order of the border follower the
// reference calls (imageproc find_contours, src/aruco.rs:64): W NW N NE E SE S SW.
__device__ __constant__ const int8_t kDX[8] = {-1, -1, 0, 1, 1, 1, 0, -1};
__device__ __constant__ const int8_t kDY[8] = {0, -1, -1, -1, 0, 1, 1, 1};

constexpr uint32_t kNoKey = 0xFFFFFFFFu;  // "this dart is not a start event"
constexpr uint32_t kNone = 0xFFFFFFFFu;

// dart info byte: bits 0-2 = incoming direction, bit 3 = W-event dart, bit 4 = E-event dart,
// bit 5 = successor missing (chain end; only face cycles of the 8-neighbour graph do this)
constexpr uint8_t kInfoW = 1u << 3;
constexpr uint8_t kInfoE = 1u << 4;
constexpr uint8_t kInfoBroken = 1u << 5;

// per-dart record, one u64: bits 0-15 x, 16-31 y, 32-39 foreground-neighbour mask F of the pixel, 40-47 info byte,
// 48-63 frame index inside the chunk (chunks hold at most kMaxChunkFrames = 65536 frames)
__host__ __device__ inline uint64_t dart_rec(uint32_t xy, uint32_t F, uint32_t info, uint32_t frame) {
    return (uint64_t)xy | ((uint64_t)(F & 0xFFu) << 32) | ((uint64_t)(info & 0xFFu) << 40) | ((uint64_t)(frame & 0xFFFFu) << 48);
}
__host__ __device__ inline uint32_t rec_frame(uint64_t r) { return (uint32_t)(r >> 48); }
__host__ __device__ inline uint32_t rec_xy(uint64_t r) { return (uint32_t)r; }
__host__ __device__ inline uint32_t rec_F(uint64_t r) { return (uint32_t)(r >> 32) & 0xFFu; }
__host__ __device__ inline uint32_t rec_info(uint64_t r) { return (uint32_t)(r >> 40) & 0xFFu; }

// The thresholded image is kept bit-packed: row y of a frame is `words_per_row(W)` little-endian u64 words,
// bit i of word j is pixel x = 64 j + i (1 = white / foreground); bits past the image width are 0.
__host__ __device__ inline uint32_t words_per_row(uint32_t W) { return (W + 63u) / 64u; }

// Directions k whose dart (p,k) can lie on a border the reference follows, from the foreground-neighbour mask F
// of p: neighbour k foreground, neighbour k-1 background (the counter-clockwise sweep is not empty), and for a
// 4-neighbour direction (k even) neighbour k-2 background as well; every other dart only belongs to a
// triangular face cycle of the 8-neighbour graph (tests/dart_model.py, rule "pdart").
__host__ __device__ inline uint32_t pdart_mask(uint32_t F) {
    const uint32_t rot1 = ((F << 1) | (F >> 7)) & 0xFFu, rot2 = ((F << 2) | (F >> 6)) & 0xFFu;
    return F & ~rot1 & (0xAAu | ~rot2) & 0xFFu;
}

// Where the decode stage reads grey levels from: the caller's frames (grey is recomputed per tap, so K1 need not write a
// grey plane at all) or, with debug taps / other threshold windows, the grey plane K1 wrote (fmt = kFmtGreyPlane).
constexpr int kFmtGreyPlane = 4;
struct PixelSrc {
    const uint8_t* base;
    unsigned long long row_stride, frame_stride;
    int fmt;   // A3_FMT_* or kFmtGreyPlane
};

// image::DynamicImage::into_luma8 for one pixel: (2126 R + 7152 G + 722 B) / 10000, truncating
__host__ __device__ inline uint32_t luma_of(uint32_t r, uint32_t g, uint32_t b) { return (2126u * r + 7152u * g + 722u * b) / 10000u; }

// one border that survived the size pruning and gets its points written out
struct ContourRec {
    uint32_t frame;
    uint32_t start_key;   // 2*raster(start pixel) (+1 when started as a hole border): the reference's contour order
    uint32_t point_base;  // into the point pool
    uint32_t n;           // number of points
};

// a quad candidate (contours_to_candidates + enforce_clockwise, src/aruco.rs:124-185)
struct CandRec {
    uint32_t start_key;
    uint16_t xy[8];
};

// what k_decode leaves per final candidate slot (k_decode.hip writes it; the marker gather and k_recover.hip read it)
struct DecodeOut {
    uint64_t code;
    uint64_t codes[4];
    uint32_t id;
    uint8_t valid, rotation, hamming, hom_ok;
    int32_t decode_ok;
    uint32_t patch;   // debug taps: index of this candidate's warped patch in the patch buffer, kNone if it was not kept
};

}  // namespace a3
