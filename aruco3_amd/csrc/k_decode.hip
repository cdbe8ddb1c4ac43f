// k_decode.hip -- K5..K7: candidate ordering + discard_too_near, homography warp + Otsu +
// triangle resize + bit decode + dictionary lookup + marker accept, IPPE pose, dictionary utilities.
//
// Replaces src/aruco.rs:69-113 (discard_too_near, extract_homographies,
// homography_to_code_permutations, the find_nearest loop and the accept test),
// src/dictionaries.rs:129-138,160-196 and src/pose.rs:52-348.
//
// Floating point follows the reference operation by operation (f64 for the 8x8 solve and
// Otsu, f32 elsewhere); the library is built with -ffp-contract=off so that no a*b+c is
// fused, exactly like the Rust reference and the CPU oracle.

#include "a3_common.h"
#include "a3_launch.h"
#include "a3_ippe.h"

namespace a3 {

// ---------------------------------------------------------------------------------------
// per frame: order candidates as the reference found them, then discard_too_near
// ---------------------------------------------------------------------------------------
__device__ __forceinline__ float perimeter4(const uint16_t* q) {  // src/aruco.rs:328-338
    float p = 0.0f;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int j = (i + 1) & 3;
        const float dx = (float)q[2 * i] - (float)q[2 * j];
        const float dy = (float)q[2 * i + 1] - (float)q[2 * j + 1];
        p += sqrtf((dx * dx) + (dy * dy));
    }
    return p;
}

struct __attribute__((aligned(8))) ProjRec { float inv[9]; int ok; };
__device__ bool solve_projection(const float* from, float S, float* inv_out);

// discard_too_near's distance between quad i and quad j: the reference's sum of the four corner distances (src/aruco.rs:187-232); across
// threshold windows (include/aruco3_hip.h, a3_set_threshold_windows step 3) the minimum over the four rotations of j, r = 0 first, a
// later r only when strictly smaller.  A constant cross == false leaves the r = 0 sum and nothing else.
__device__ __forceinline__ float merge_distance(const float* xi, const float* xj, bool cross) {
    float best = 0.0f;
#pragma unroll
    for (int r = 0; r < 4; r++) {
        float distance = 0.0f;
#pragma unroll
        for (int p = 0; p < 4; p++) {
            const int q = (p + r) & 3;
            const float dx = xi[2 * p] - xj[2 * q];
            const float dy = xi[2 * p + 1] - xj[2 * q + 1];
            distance += sqrtf((dx * dx) + (dy * dy));
        }
        if (r == 0) best = distance;
        else if (cross && distance < best) best = distance;
    }
    return best;
}

// One wave per frame: the body of k_frame_candidates (MERGE == false: one table per frame, K == 1, plane_cand == max_cand) and of
// k_merge_candidates (MERGE: K = 2..4 planes per frame, plane (k, f) at index k * n_frames + f with plane_cand slots).  Frame f's list
// is the concatenation over k of plane (k, f)'s quads in start-key order: rank = (quads of the frame's earlier planes) + (keys of the
// same plane below this one).  MERGE carries the window index with the quad (a byte per slot), which selects the distance, and writes
// merged_count and kErrCandTable; nothing else differs.
// proj != nullptr: the wave also solves the projection of every surviving candidate (one lane each: the 8x8 system needs
// ~200 VGPRs, affordable in a one-wave workgroup) into proj[work index], which saves the separate k_projection launch.
// BIG (tables beyond kFrameCandLds slots per frame -- a frame tiled with thousands of small squares; no camera frame gets there): the
// sorted quads live where they end up anyway (pre_xy), keys and perimeters in a scratch plane of the caller's, and only the dead flags
// (and window bytes) in LDS (a byte each per slot: 64 KB at the format's limit of 65 536 -- a3_marker.candidate_index is 16 bits).
// Same walk, same order, every LDS access of the small form a trip to the L2 instead: correct, not fast (0.1 s for 7 000 quads, all
// of them far apart).
constexpr uint32_t kFrameCandLds = 6144;   // 21 bytes of LDS per slot in the small form (22 with the window byte): 129 KB of the CU's 160
constexpr int kFcWaves = 1;   // occupancy bound of k_frame_candidates and k_projection (the 8x8 solve needs ~200 VGPRs)
template <bool BIG, bool MERGE>
__device__ __forceinline__ void frame_candidates(const CandRec* __restrict__ cands, const uint32_t* __restrict__ cand_count,
                                                 uint32_t n_frames, uint32_t K, uint32_t plane_cand, uint32_t max_cand,
                                                 float min_distance, uint16_t* pre_xy, uint16_t* __restrict__ fin_xy,
                                                 uint32_t* __restrict__ fin_count, uint32_t* __restrict__ work,
                                                 unsigned int* __restrict__ work_count, uint32_t S, ProjRec* __restrict__ proj,
                                                 float* big_scratch /* BIG: frames x max_cand */, uint32_t* __restrict__ merged_count,
                                                 unsigned int* __restrict__ err_flags) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint16_t* s_xy = BIG ? pre_xy + (size_t)blockIdx.x * max_cand * 8 : reinterpret_cast<uint16_t*>(smem);                      // max_cand * 8
    float* s_per = BIG ? big_scratch + (size_t)blockIdx.x * max_cand : reinterpret_cast<float*>(smem + (size_t)max_cand * 16);   // max_cand
    uint8_t* s_dead = BIG ? smem : smem + (size_t)max_cand * 20;                                                                // max_cand
    [[maybe_unused]] uint8_t* s_win = s_dead + max_cand;                                                                        // max_cand, MERGE only
    // (BIG: what one lane wrote to memory another reads after the barrier -- the fence makes the wave's stores visible and drops stale lines)
#define FC_SYNC() do { if (BIG) __threadfence(); __syncthreads(); } while (0)
    constexpr uint32_t kPlanes = MERGE ? 4 : 1;
    const uint32_t f = blockIdx.x;
    const int lane = threadIdx.x;
    uint32_t cnt[kPlanes], off[kPlanes];   // a plane's quads and where they start in the frame's list
    uint32_t c;
    if constexpr (MERGE) {
        // merged_count[f]: the length of the concatenated list; for a frame with a plane beyond plane_cand (flagged by k_contour_quads:
        // the batch is re-run) the fullest plane's count, and for a frame whose planes sum beyond max_cand (raised here) the sum --
        // either way what the marker gather reports as the fullest count -- and the frame is left empty.
        uint32_t sum = 0, most = 0;
        bool plane_over = false;
#pragma unroll
        for (uint32_t k = 0; k < kPlanes; k++) {
            const uint32_t ck = k < K ? cand_count[(size_t)k * n_frames + f] : 0u;
            plane_over |= ck > plane_cand;
            most = max(most, ck);
            cnt[k] = ck; off[k] = sum;
            sum += min(ck, plane_cand);   // (no wrap: at most 4 x 65536)
        }
        const bool merged_over = !plane_over && sum > max_cand;
        c = plane_over || merged_over ? 0u : sum;
        if (lane == 0) {
            merged_count[f] = plane_over ? most : sum;
            if (merged_over) atomicOr(err_flags, kErrCandTable);
        }
        if (!c) for (uint32_t k = 0; k < kPlanes; k++) cnt[k] = 0;
    } else {
        // a frame that overflowed its table: k_contour_quads has flagged it, the host re-runs the batch with larger tables and nothing
        // of this pass is used -- no point in ordering the slots that did fit (seconds, at the large end of the through-memory form)
        c = cand_count[f] > max_cand ? 0u : cand_count[f];
        cnt[0] = c; off[0] = 0;
    }
    // rank sort by start key within a plane (keys are unique: one border starts per pixel visit).  The keys go to LDS first: ranking
    // straight from global memory was a chain of c dependent loads per lane (s_per doubles as the key buffer until the
    // perimeters are written).
    uint32_t* s_key = reinterpret_cast<uint32_t*>(s_per);
#pragma unroll
    for (uint32_t k = 0; k < kPlanes; k++) {
        const CandRec* src = cands + ((size_t)k * n_frames + f) * plane_cand;
        for (uint32_t i = lane; i < cnt[k]; i += 64) s_key[off[k] + i] = src[i].start_key;
    }
    FC_SYNC();
#pragma unroll
    for (uint32_t k = 0; k < kPlanes; k++) {
        const CandRec* src = cands + ((size_t)k * n_frames + f) * plane_cand;
        for (uint32_t i = lane; i < cnt[k]; i += 64) {
            const uint32_t key = s_key[off[k] + i];
            const CandRec r = src[i];   // in flight while the rank is counted
            uint32_t rank = off[k];
            for (uint32_t j = 0; j < cnt[k]; j++) rank += s_key[off[k] + j] < key;
            for (int q = 0; q < 8; q++) s_xy[rank * 8 + q] = r.xy[q];
            if constexpr (MERGE) s_win[rank] = (uint8_t)k;
        }
    }
    FC_SYNC();
    for (uint32_t i = lane; i < c; i += 64) {
        s_per[i] = perimeter4(&s_xy[i * 8]);
        s_dead[i] = 0;
        if (!BIG) for (int k = 0; k < 8; k++) pre_xy[((size_t)f * max_cand + i) * 8 + k] = s_xy[i * 8 + k];
    }
    FC_SYNC();
    // discard_too_near, src/aruco.rs:187-232: i ascending; for j > i ascending, a close pair kills the smaller
    // perimeter; once i itself is dead the rest of its row is a no-op.
    if (c >= 2 && c <= 64) {
        // The usual case (a frame holds a few dozen quads): the same walk with everything in registers -- lane j holds quad j (and its
        // window), row i's quad comes through v_readlane (i is uniform), the dead set is a 64-bit mask every lane carries -- so a row
        // is four square roots, a division and two ballots, without LDS traffic or a barrier.  (s_memtime stamps: the LDS version
        // below spent 850 cycles per live row, half of the kernel's 20 us on BASELINE config 2.)
        const uint32_t j = min((uint32_t)lane, c - 1u);
        float xj[8];
#pragma unroll
        for (int k = 0; k < 8; k++) xj[k] = (float)s_xy[j * 8 + k];
        const float per_j = s_per[j];
        int win_j = 0;
        if constexpr (MERGE) win_j = (int)s_win[j];
        unsigned long long dead = 0;
        for (uint32_t i = 0; i + 1 < c; i++) {
            if ((dead >> i) & 1ull) continue;   // uniform
            float xi[8];
#pragma unroll
            for (int k = 0; k < 8; k++) xi[k] = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(xj[k]), (int)i));
            const float per_i = __int_as_float(__builtin_amdgcn_readlane(__float_as_int(per_j), (int)i));
            bool cross = false;
            if constexpr (MERGE) cross = __builtin_amdgcn_readlane(win_j, (int)i) != win_j;
            const float distance = merge_distance(xi, xj, cross);
            const bool cand = (uint32_t)lane > i && (uint32_t)lane < c && !((dead >> lane) & 1ull);
            const bool close_alive = cand && (distance / 4.0f) < min_distance;
            const bool bigger = close_alive && !(per_i >= per_j);
            const unsigned long long m_close = __ballot(close_alive), m_big = __ballot(bigger);
            unsigned long long kill = m_close;
            if (m_big) {
                kill = m_close & ((1ull << (__ffsll((long long)m_big) - 1)) - 1ull);
                dead |= 1ull << i;
            }
            dead |= kill;
        }
        if ((uint32_t)lane < c) s_dead[lane] = (uint8_t)((dead >> lane) & 1ull);
    } else
    for (uint32_t i = 0; i + 1 < c; i++) {
        if (s_dead[i]) continue;  // uniform: LDS value
        const float per_i = s_per[i];
        bool i_dead = false;
        for (uint32_t j0 = i + 1; j0 < c && !i_dead; j0 += 64) {
            const uint32_t j = j0 + lane;
            bool close_alive = false, bigger = false;
            if (j < c && !s_dead[j]) {
                float xi[8], xj[8];
#pragma unroll
                for (int k = 0; k < 8; k++) { xi[k] = (float)s_xy[i * 8 + k]; xj[k] = (float)s_xy[j * 8 + k]; }
                bool cross = false;
                if constexpr (MERGE) cross = s_win[i] != s_win[j];
                const float distance = merge_distance(xi, xj, cross);
                close_alive = (distance / 4.0f) < min_distance;
                bigger = close_alive && !(per_i >= s_per[j]);
            }
            const unsigned long long m_close = __ballot(close_alive), m_big = __ballot(bigger);
            unsigned long long kill = m_close;
            if (m_big) {
                const int first = __ffsll((long long)m_big) - 1;
                kill = m_close & ((1ull << first) - 1ull);
                i_dead = true;
            }
            if ((kill >> lane) & 1ull) s_dead[j] = 1;
        }
        if (i_dead && lane == 0) s_dead[i] = 1;
        __syncthreads();   // (only s_dead changes inside this loop, and s_dead lives in LDS in both forms: no memory fence per row)
    }
    FC_SYNC();
    // survivors, order preserved: count them, take a range of the work list, then write quads, work items and projections
    uint32_t total = 0;
    for (uint32_t i0 = 0; i0 < c; i0 += 64) {
        const uint32_t i = i0 + lane;
        total += (uint32_t)__popcll(__ballot(i < c && !s_dead[i]));
    }
    uint32_t w0 = 0;
    if (lane == 0) {
        fin_count[f] = total;
        if (total) w0 = atomicAdd(work_count, total);
    }
    w0 = __shfl(w0, 0);
    uint32_t base = 0;
    for (uint32_t i0 = 0; i0 < c; i0 += 64) {
        const uint32_t i = i0 + lane;
        const bool alive = i < c && !s_dead[i];
        const unsigned long long m = __ballot(alive);
        if (alive) {
            const uint32_t pos = base + __popcll(m & ((1ull << lane) - 1ull));
            float from[8];
            for (int k = 0; k < 8; k++) { const uint16_t v = s_xy[i * 8 + k]; fin_xy[((size_t)f * max_cand + pos) * 8 + k] = v; from[k] = (float)v; }
            work[w0 + pos] = f * max_cand + pos;
            if (proj) {
                ProjRec r;
                r.ok = solve_projection(from, (float)S, r.inv) ? 1 : 0;
                proj[w0 + pos] = r;
            }
        }
        base += __popcll(m);
    }
#undef FC_SYNC
}

// cands: unordered CandRec[max_cand] per frame (as k_contour_quads appended them), 21 bytes of LDS per slot (BIG: 1).
template <bool BIG>
__global__ __launch_bounds__(64, kFcWaves) void k_frame_candidates(const CandRec* __restrict__ cands, const uint32_t* __restrict__ cand_count,
                                                         uint32_t max_cand, float min_distance, uint16_t* pre_xy,
                                                         uint16_t* __restrict__ fin_xy, uint32_t* __restrict__ fin_count,
                                                         uint32_t* __restrict__ work, unsigned int* __restrict__ work_count,
                                                         uint32_t S, ProjRec* __restrict__ proj, float* big_scratch /* BIG: frames x max_cand */) {
    frame_candidates<BIG, false>(cands, cand_count, 0u, 1u, max_cand, max_cand, min_distance, pre_xy, fin_xy, fin_count, work, work_count, S, proj,
                                 big_scratch, nullptr, nullptr);
}

// Several threshold windows (a3_set_threshold_windows), K = 2..4: cands is CandRec[plane_cand] per PLANE with cand_count per plane, and
// all merged tables (pre_xy, fin_xy, work, proj, big_scratch) have merged_cap = merged_cand_capacity(K, plane_cand) slots per frame;
// 22 bytes of LDS per slot (BIG: 2).
template <bool BIG>
__global__ __launch_bounds__(64, kFcWaves) void k_merge_candidates(const CandRec* __restrict__ cands, const uint32_t* __restrict__ cand_count,
                                                         uint32_t n_frames, uint32_t K, uint32_t plane_cand, uint32_t merged_cap,
                                                         float min_distance, uint16_t* pre_xy, uint16_t* __restrict__ fin_xy,
                                                         uint32_t* __restrict__ fin_count, uint32_t* __restrict__ work,
                                                         unsigned int* __restrict__ work_count, uint32_t S, ProjRec* __restrict__ proj,
                                                         float* big_scratch, uint32_t* __restrict__ merged_count,
                                                         unsigned int* __restrict__ err_flags) {
    frame_candidates<BIG, true>(cands, cand_count, n_frames, K, plane_cand, merged_cap, min_distance, pre_xy, fin_xy, fin_count, work, work_count, S,
                                proj, big_scratch, merged_count, err_flags);
}

// ---------------------------------------------------------------------------------------
// decode one candidate per workgroup
// ---------------------------------------------------------------------------------------
// (DecodeOut, one per final candidate slot: a3_common.h -- k_recover.hip reads the records too)

// imageproc Projection::from_control_points: 8x8 system in f64, LU with partial pivoting (nalgebra order of
// operations), cast to f32, adjugate inverse normalised by its last element.  Single lane.
__device__ bool solve_projection(const float* from, float S, float* inv_out) {
    double A[8][8], b[8];
    const float to[8] = {0.0f, 0.0f, S, 0.0f, S, S, 0.0f, S};
    for (int i = 0; i < 4; i++) {
        const double xf = from[2 * i], yf = from[2 * i + 1], x = to[2 * i], y = to[2 * i + 1];
        A[2 * i][0] = 0.0; A[2 * i][1] = 0.0; A[2 * i][2] = 0.0; A[2 * i][3] = -xf; A[2 * i][4] = -yf; A[2 * i][5] = -1.0;
        A[2 * i][6] = y * xf; A[2 * i][7] = y * yf;
        A[2 * i + 1][0] = xf; A[2 * i + 1][1] = yf; A[2 * i + 1][2] = 1.0; A[2 * i + 1][3] = 0.0; A[2 * i + 1][4] = 0.0; A[2 * i + 1][5] = 0.0;
        A[2 * i + 1][6] = -x * xf; A[2 * i + 1][7] = -x * yf;
        b[2 * i] = -y; b[2 * i + 1] = x;
    }
    // Every index below is a compile-time constant after unrolling (the pivot row is exchanged by predicated moves over the
    // candidate rows, b follows its rows instead of replaying the permutation afterwards): A and b live in registers.  With
    // A[piv][c] indexed at run time they lived in scratch memory and this kernel took 24 us for 2.5 k candidates.
#pragma unroll
    for (int i = 0; i < 8; i++) {
        int piv = i; double best = fabs(A[i][i]);
#pragma unroll
        for (int r = i + 1; r < 8; r++) { const double v = fabs(A[r][i]); if (v > best) { best = v; piv = r; } }
        double diag = A[i][i];
#pragma unroll
        for (int r = i + 1; r < 8; r++) diag = piv == r ? A[r][i] : diag;
        if (diag == 0.0) continue;
#pragma unroll
        for (int r = i + 1; r < 8; r++) {
            const bool sw = piv == r;
#pragma unroll
            for (int c = 0; c < 8; c++) { const double x = A[i][c], y = A[r][c]; A[i][c] = sw ? y : x; A[r][c] = sw ? x : y; }
            const double x = b[i], y = b[r]; b[i] = sw ? y : x; b[r] = sw ? x : y;
        }
        const double inv_diag = 1.0 / diag;
#pragma unroll
        for (int r = i + 1; r < 8; r++) A[r][i] *= inv_diag;
#pragma unroll
        for (int c = i + 1; c < 8; c++) {
            const double pr = -A[i][c];
#pragma unroll
            for (int r = i + 1; r < 8; r++) A[r][c] = pr * A[r][i] + A[r][c];
        }
    }
#pragma unroll
    for (int i = 0; i < 7; i++) {
        const double coeff = -b[i];
#pragma unroll
        for (int r = i + 1; r < 8; r++) b[r] = coeff * A[r][i] + b[r];
    }
    bool singular = false;
#pragma unroll
    for (int i = 7; i >= 0; i--) {
        const double diag = A[i][i];
        if (diag == 0.0) singular = true;
        const double coeff = b[i] / diag;
        b[i] = coeff;
        const double nc = -coeff;
#pragma unroll
        for (int r = 0; r < i; r++) b[r] = nc * A[r][i] + b[r];
    }
    if (singular) return false;
    float t[9];
    for (int i = 0; i < 8; i++) t[i] = (float)b[i];
    t[8] = 1.0f;
    const float t00 = t[0], t01 = t[1], t02 = t[2], t10 = t[3], t11 = t[4], t12 = t[5], t20 = t[6], t21 = t[7], t22 = t[8];
    const float m00 = t11 * t22 - t12 * t21;
    const float m01 = t10 * t22 - t12 * t20;
    const float m02 = t10 * t21 - t11 * t20;
    const float det = t00 * m00 - t01 * m01 + t02 * m02;
    if (fabsf(det) < 1e-10f) return false;
    const float m10 = t01 * t22 - t02 * t21;
    const float m11 = t00 * t22 - t02 * t20;
    const float m12 = t00 * t21 - t01 * t20;
    const float m20 = t01 * t12 - t02 * t11;
    const float m21 = t00 * t12 - t02 * t10;
    const float m22 = t00 * t11 - t01 * t10;
    const float r[9] = {m00 / det, -m10 / det, m20 / det, -m01 / det, m11 / det, -m21 / det, m02 / det, -m12 / det, m22 / det};
    for (int i = 0; i < 8; i++) inv_out[i] = r[i] / r[8];
    inv_out[8] = 1.0f;
    return true;
}

// v_cvt_u32_f32 truncates, saturates (negative -> 0, >= 2^32 -> 0xFFFFFFFF) and turns NaN into 0: Rust's `as u32` in one
// instruction (written as asm because a C++ cast is undefined outside the range, i.e. free to be anything after optimisation).
__device__ __forceinline__ uint32_t sat_u32(float x) {
    uint32_t r;
    asm("v_cvt_u32_f32_e32 %0, %1" : "=v"(r) : "v"(x));
    return r;
}

// imageproc's Clamp for u8: x < 255 ? (x > 0 ? x as u8 : 0) : 255 -- so NaN gives 255.  Branch-free: the sampling loop runs
// this three times per sample, and the nested ifs became three exec-mask regions each.
__device__ __forceinline__ uint8_t clamp_u8(float x) {
    const uint32_t r = min(sat_u32(x), 255u);
    return (uint8_t)(x != x ? 255u : r);
}

// grey level of pixel x in a frame row: the plane K1 wrote, or into_luma8 of the caller's pixel (same integers).
// Y422: the frames are packed 4:2:2 (A3_FMT_YUYV8 / A3_FMT_UYVY8) -- the luma byte as it stands.  A template parameter of the sampler
// and of k_decode, not one more run-time case: the instantiations for the other formats then compile exactly as they did (one more
// case in grey_tap alone cost k_decode two spilled VGPRs), and the 4:2:2 ones carry no luma arithmetic at all.
template <bool Y422 = false>
__device__ __forceinline__ float grey_tap(const uint8_t* __restrict__ row, uint32_t x, int fmt) {
    if constexpr (Y422) return (float)row[2u * (size_t)x + (fmt == A3_FMT_UYVY8 ? 1u : 0u)];
    if (fmt == A3_FMT_L8 || fmt == kFmtGreyPlane) return (float)row[x];
    if (fmt == A3_FMT_RGB8) { const uint8_t* p = row + 3u * (size_t)x; return (float)luma_of(p[0], p[1], p[2]); }
    const uint8_t* p = row + 4u * (size_t)x;
    return (float)(fmt == A3_FMT_BGRA8 ? luma_of(p[2], p[1], p[0]) : luma_of(p[0], p[1], p[2]));
}

// grey of one pixel in the low bytes of px (byte 0 = R, or B when bgr): byte-wise dot products with the split weights
// 2126 = 8*256+78, 7152 = 27*256+240, 722 = 2*256+210 and the exact /10000 (same integers as luma_of, as in K1)
__device__ __forceinline__ uint32_t luma_px(uint32_t px, bool bgr) {
    const uint32_t lo = __builtin_amdgcn_udot4(px, bgr ? 0x004EF0D2u : 0x00D2F04Eu, 0u, false);
    const uint32_t hi = __builtin_amdgcn_udot4(px, bgr ? 0x00081B02u : 0x00021B08u, 0u, false);
    const uint32_t l = lo + (hi << 8);   // <= 10000 * 255 < 2^22
    __builtin_assume(l < (1u << 22));     // both factors below 2^24: the full-rate v_mul_hi_u32_u24 instead of the quarter-rate v_mul_hi_u32
    return (uint32_t)(((uint64_t)l * 13743896ull) >> 37);
}

// imageproc interpolate_bilinear: default (0) outside, the two horizontal lerps truncated to u8 first.
// Split in two so that a lane can have the loads of several samples in flight before it converts any of them:
// issue() decides the case and starts the two 12-byte row reads, finish() turns them into the sample.
// The reads are UNCONDITIONAL -- a sample that falls outside the frame, or so close to its end that a 12-byte read would run
// past it, reads the frame's first bytes instead and ignores them -- and the case is data (`mode`), not control flow: with the
// loads behind an `if`, the compiler threads the case through to finish() and ends up with issue + wait + finish per sample,
// i.e. one round trip to memory per sample instead of one per kU samples.
struct TapLoad {
    uint32_t top[3], bot[3];
    float rw, bw;
    uint32_t sh;         // byte misalignment of the first tap, in bits (top row | bottom row << 8)
    int mode;            // 0 outside (sample = 0), 1 wide loads hold the taps, 2 near the end of the frame: byte loads in finish()
    uint32_t l, t;       // first tap (mode 2 only)
};

// The frame as 4-byte words in the GLOBAL address space: a pointer that went through uintptr_t arithmetic is a generic one to the
// compiler, and loads through it are flat_load (LDS / scratch aperture checks, and every LDS wait of the loop then waits for
// them as well); with the base uniform per workgroup and the offset 32 bits wide the tap loads are global_load ... s[base]
// with no 64-bit address arithmetic per sample.
typedef const uint32_t __attribute__((address_space(1)))* a3_gptr;

// OffT: uint32_t when the frame's bytes (+ 16) fit 32 bits and a row's stride 24, else uint64_t.  base4 = the frame's first byte rounded down to 4
// bytes (`mis` = what was rounded off), or any 16 readable bytes when the frame is smaller than one wide read (`tiny`: no
// sample then takes the wide path).  wide_limit = frame bytes - 12: the last offset at which a 12-byte read ends inside the frame.
template <typename OffT>
__device__ __forceinline__ void sample_issue(TapLoad& tl, a3_gptr base4, uint32_t mis, OffT row_stride, OffT wide_limit, bool tiny,
                                             uint32_t bpp, uint32_t w, uint32_t h, float x, float y, bool valid) {
    const float left = floorf(x), right = left + 1.0f, top = floorf(y), bottom = top + 1.0f;
    tl.rw = x - left; tl.bw = y - top;
    // (bitwise, not short-circuit: no branches)
    const bool inside = valid & !((left < 0.0f) | (right >= (float)w) | (top < 0.0f) | (bottom >= (float)h));
    // (converted unconditionally, selected afterwards: with the conversion inside the ternary each became an exec-mask region)
    const uint32_t lc = sat_u32(left), tc = sat_u32(top), bc = sat_u32(bottom);
    const uint32_t l = inside ? lc : 0u, t = inside ? tc : 0u, b = inside ? bc : 0u;
    tl.l = l; tl.t = t;
    OffT ot, ob;
    if constexpr (sizeof(OffT) == 4) {   // row index < 2^16, row_stride < 2^24 (the caller's condition for this path), products < 2^32: full-rate 24-bit multiplies
        const uint32_t xl = __umul24(bpp, l);
        ot = __umul24(t, (uint32_t)row_stride) + xl; ob = __umul24(b, (uint32_t)row_stride) + xl;
    } else {
        ot = (OffT)t * row_stride + (OffT)(bpp * l); ob = (OffT)b * row_stride + (OffT)(bpp * l);
    }
    // the wide read of the bottom row must end inside this frame (running on into the next row is fine)
    const bool wide = inside & !tiny & (ob <= wide_limit);
    tl.mode = inside ? (wide ? 1 : 2) : 0;
    const OffT at = (wide ? ot : (OffT)0) + (OffT)mis, ab = (wide ? ob : (OffT)0) + (OffT)mis;
    const a3_gptr qt = base4 + (at >> 2), qb = base4 + (ab >> 2);
    tl.top[0] = qt[0]; tl.top[1] = qt[1]; tl.top[2] = qt[2];
    tl.bot[0] = qb[0]; tl.bot[1] = qb[1]; tl.bot[2] = qb[2];
    // both rows start at the same misalignment only if row_stride % 4 == 0; keep one shift per row in sh's halves
    tl.sh = ((uint32_t)(at & 3u) * 8u) | (((uint32_t)(ab & 3u) * 8u) << 8);
}

template <bool Y422 = false>
__device__ __forceinline__ void pair_from(const uint32_t d[3], uint32_t sh, int fmt, uint32_t bpp, float* g0, float* g1) {
    const uint32_t w0 = __builtin_amdgcn_alignbit(d[1], d[0], sh), w1 = __builtin_amdgcn_alignbit(d[2], d[1], sh);   // bytes p .. p+7
    if constexpr (Y422) {   // bpp 2: the two taps of a row are the luma bytes o and o + 2 of the window (o = 1 for UYVY)
        const uint32_t y = fmt == A3_FMT_UYVY8 ? w0 >> 8 : w0;
        *g0 = (float)(y & 0xFFu); *g1 = (float)((y >> 16) & 0xFFu);
        return;
    }
    if (bpp == 1u) { *g0 = (float)(w0 & 0xFFu); *g1 = (float)((w0 >> 8) & 0xFFu); return; }
    const bool bgr = fmt == A3_FMT_BGRA8;
    const uint32_t px1 = bpp == 3u ? ((w0 >> 24) | (w1 << 8)) : w1;   // the dot products ignore byte 3
    *g0 = (float)luma_px(w0, bgr);
    *g1 = (float)luma_px(px1, bgr);
}

template <bool Y422 = false>
__device__ __forceinline__ uint8_t sample_finish(const TapLoad& tl, const uint8_t* __restrict__ img, size_t row_stride, int fmt, uint32_t bpp) {
    float a, b, c, d;
    pair_from<Y422>(tl.top, tl.sh & 0xFFu, fmt, bpp, &a, &b);
    pair_from<Y422>(tl.bot, tl.sh >> 8, fmt, bpp, &c, &d);
    if (tl.mode == 2) {   // the last few pixels of a frame: byte loads
        const uint8_t* rt = img + (size_t)tl.t * row_stride;
        const uint8_t* rb = rt + row_stride;
        a = grey_tap<Y422>(rt, tl.l, fmt); b = grey_tap<Y422>(rt, tl.l + 1u, fmt); c = grey_tap<Y422>(rb, tl.l, fmt); d = grey_tap<Y422>(rb, tl.l + 1u, fmt);
    }
    const uint8_t tv = clamp_u8((1.0f - tl.rw) * a + tl.rw * b);
    const uint8_t bv = clamp_u8((1.0f - tl.rw) * c + tl.rw * d);
    const uint8_t v = clamp_u8((1.0f - tl.bw) * (float)tv + tl.bw * (float)bv);
    return tl.mode == 0 ? (uint8_t)0 : v;
}

__device__ __forceinline__ float triangle_kernel(float x) { return fabsf(x) < 1.0f ? 1.0f - fabsf(x) : 0.0f; }

// image::imageops::resize weights for output index o (in_len -> out_len), normalised; returns left, sets count
__device__ uint32_t resize_weights(uint32_t in_len, uint32_t out_len, uint32_t o, float* ws, uint32_t* count) {
    const float ratio = (float)in_len / (float)out_len;
    const float sratio = ratio < 1.0f ? 1.0f : ratio;
    const float src_support = 1.0f * sratio;
    float input = ((float)o + 0.5f) * ratio;
    long long left = (long long)floorf(input - src_support);
    left = left < 0 ? 0 : (left > (long long)in_len - 1 ? (long long)in_len - 1 : left);
    long long right = (long long)ceilf(input + src_support);
    right = right < left + 1 ? left + 1 : (right > (long long)in_len ? (long long)in_len : right);
    input = input - 0.5f;
    float sum = 0.0f;
    uint32_t n = 0;
    for (long long i = left; i < right; i++) {
        const float w = triangle_kernel(((float)i - input) / sratio);
        ws[n++] = w;
        sum += w;
    }
    for (uint32_t i = 0; i < n; i++) ws[i] /= sum;
    *count = n;
    return (uint32_t)left;
}

// The 8x8 solve needs ~200 VGPRs for one lane's work; inside k_decode it would cap that kernel's occupancy, so it runs
// first, one lane per candidate (inside k_frame_candidates; k_projection is the stand-alone form the tuning probe uses), and
// leaves 9 floats + a flag per candidate.

// The triangle-resize weights of a full patch (S -> n) are the same for every candidate of a context: a table computed once
// (k_weight_table, at a3_create) replaces seven lanes of every decode workgroup computing them while the other 249 waited
// (~30 f32 divisions in a row: ~4 us on the critical path of each candidate).  Row o of the table: left, count, weights.
constexpr size_t kWeightTableBytes = 16384;   // n <= 10 rows of (2 + max_taps <= 202) floats
__global__ void k_weight_table(uint32_t S, uint32_t n, uint32_t max_taps, float* __restrict__ wtab) {
    if (threadIdx.x >= n) return;
    float* row = wtab + (size_t)threadIdx.x * (max_taps + 2);
    uint32_t cnt;
    const uint32_t left = resize_weights(S, n, threadIdx.x, row + 2, &cnt);
    row[0] = __uint_as_float(left); row[1] = __uint_as_float(cnt);
}
__global__ __launch_bounds__(64, kFcWaves) void k_projection(const uint16_t* __restrict__ fin_xy, const uint32_t* __restrict__ work,
                                                   const unsigned int* __restrict__ work_count, uint32_t S, ProjRec* __restrict__ proj) {
    const uint32_t n_work = *work_count;
    for (uint32_t wi = blockIdx.x * blockDim.x + threadIdx.x; wi < n_work; wi += gridDim.x * blockDim.x) {
        const uint32_t slot = work[wi];
        const uint16_t* q = fin_xy + (size_t)slot * 8;
        float from[8];
        for (int i = 0; i < 8; i++) from[i] = (float)q[i];
        ProjRec r;
        r.ok = solve_projection(from, (float)S, r.inv) ? 1 : 0;
        proj[wi] = r;
    }
}

// rotate_bit_matrix (src/aruco.rs:315-326: new[a][b] = old[b][n-1-a], 90 degrees counter-clockwise) applied r times:
// cell (y, x) of the rotated matrix comes from the original at
//   r=0 (y,x)  r=1 (x,n-1-y)  r=2 (n-1-y,n-1-x)  r=3 (n-1-x,y)
__device__ __forceinline__ void rotated_source(uint32_t r, uint32_t n, uint32_t y, uint32_t x, uint32_t* sy, uint32_t* sx) {
    if (r == 0) { *sy = y; *sx = x; }
    else if (r == 1) { *sy = x; *sx = n - 1 - y; }
    else if (r == 2) { *sy = n - 1 - y; *sx = n - 1 - x; }
    else { *sy = n - 1 - x; *sx = y; }
}

// grid-stride over the work list; block = NT threads; dynamic LDS:
//   patch S*S | tmp n*S f32 | wtab n*max_taps f32 | wleft n u32 | wcnt n u32 | bits n*n
constexpr int kDecodeKU = 2;        // samples per lane and trip whose row reads are in flight together
constexpr int kDecodeThreads = 256;  // threads that sample one candidate
constexpr int kDecodeWaves = 5;      // workgroups of 256 threads per CU-quarter (= waves per SIMD)
constexpr int kDecodeDB = 8;         // dictionary codes per lane and trip in the nearest-code scan
// Wave-wide scans and reductions by DPP row shifts (row_shr:1,2,4,8 inside rows of 16 lanes) and row broadcasts (row_bcast:15 into
// rows 1 and 3, row_bcast:31 into rows 2 and 3): pure VALU, the result of a reduction ends up in lane 63.  The shuffle ladders
// they replace are six ds_bpermute round trips each.  `OLD` is what a lane without a source combines with: the identity.
#define A3_DPP_STEPS(STEP) STEP(0x111, 0xF) STEP(0x112, 0xF) STEP(0x114, 0xF) STEP(0x118, 0xF) STEP(0x142, 0xA) STEP(0x143, 0xC)
__device__ __forceinline__ uint32_t wave_incl_add(uint32_t v) {
#define A3_S(CTRL, RM) v += (uint32_t)__builtin_amdgcn_update_dpp(0, (int)v, CTRL, RM, 0xF, false);
    A3_DPP_STEPS(A3_S)
#undef A3_S
    return v;
}
__device__ __forceinline__ unsigned long long wave_min_u64_to63(unsigned long long v) {
#define A3_S(CTRL, RM)                                                                                                  \
    {                                                                                                                    \
        const uint32_t lo_ = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)(uint32_t)v, CTRL, RM, 0xF, false);           \
        const uint32_t hi_ = (uint32_t)__builtin_amdgcn_update_dpp(-1, (int)(uint32_t)(v >> 32), CTRL, RM, 0xF, false);    \
        const unsigned long long o_ = ((unsigned long long)hi_ << 32) | lo_;                                             \
        v = o_ < v ? o_ : v;                                                                                             \
    }
    A3_DPP_STEPS(A3_S)
#undef A3_S
    return v;
}
// largest variance, lowest threshold among equals (the Otsu scan's first strict maximum); identity: (-1.0, INT_MAX)
__device__ __forceinline__ void wave_best_var_to63(double& var, int& best_t) {
#define A3_S(CTRL, RM)                                                                                                  \
    {                                                                                                                    \
        const unsigned long long vb_ = (unsigned long long)__double_as_longlong(var);                                    \
        const uint32_t lo_ = (uint32_t)__builtin_amdgcn_update_dpp(0, (int)(uint32_t)vb_, CTRL, RM, 0xF, false);           \
        const uint32_t hi_ = (uint32_t)__builtin_amdgcn_update_dpp((int)0xBFF00000u, (int)(uint32_t)(vb_ >> 32), CTRL, RM, 0xF, false); \
        const int ot_ = __builtin_amdgcn_update_dpp(0x7FFFFFFF, best_t, CTRL, RM, 0xF, false);                             \
        const double ov_ = __longlong_as_double((long long)(((unsigned long long)hi_ << 32) | lo_));                     \
        if (ov_ > var || (ov_ == var && ot_ < best_t)) { var = ov_; best_t = ot_; }                                      \
    }
    A3_DPP_STEPS(A3_S)
#undef A3_S
}

// gather the accepted markers of frame f, candidate order preserved, by ONE WAVE (per_frame[] holds the number of accepted candidates
// of every frame: k_decode counted them; a frame's first output slot is the sum over the frames before it)
__device__ __forceinline__ void compact_frame_wave(uint32_t f, int lane, const DecodeOut* __restrict__ outs, const uint16_t* __restrict__ fin_xy,
                                                   const uint32_t* __restrict__ fin_count, uint32_t n_frames, uint32_t max_cand,
                                                   a3_marker* __restrict__ markers, uint32_t marker_cap, const uint32_t* __restrict__ per_frame,
                                                   unsigned int* __restrict__ marker_total, unsigned int* __restrict__ err_flags,
                                                   const uint32_t* __restrict__ cand_count, unsigned int* __restrict__ cand_pre_total) {
    uint32_t base = 0;
    for (uint32_t g = lane; g < f; g += 64) base += per_frame[g];
    for (int o = 32; o > 0; o >>= 1) base += __shfl_xor(base, o);
    if (f + 1 == n_frames && lane == 0) *marker_total = base + per_frame[f];
    if (f + 1 == n_frames) {   // a3_stats.candidates_pre: quads after contours_to_candidates, summed over the batch
        uint32_t pre = 0, most = 0;   // BatchScratch::cand_most: the largest number of quads any frame produced (beyond its table's slots: what the host grows the tables to)
        for (uint32_t g = lane; g < n_frames; g += 64) { pre += min(cand_count[g], max_cand); most = max(most, cand_count[g]); }
        for (int o = 32; o > 0; o >>= 1) { pre += __shfl_xor(pre, o); most = max(most, (uint32_t)__shfl_xor(most, o)); }
        if (lane == 0) { *cand_pre_total = pre; cand_pre_total[kCandMostFromPre] = most; }
    }
    const uint32_t c = fin_count[f];
    uint32_t pos = base;
    for (uint32_t k0 = 0; k0 < c; k0 += 64) {
        const uint32_t k = k0 + lane;
        DecodeOut o;
        o.valid = 0;
        if (k < c) o = outs[(size_t)f * max_cand + k];
        const unsigned long long m = __ballot(o.valid != 0);
        if (o.valid) {
            const uint32_t p = pos + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));
            if (p < marker_cap) {
                a3_marker mk;
                mk.frame = f;
                mk.id = o.id;
                mk.code = o.code;
                const uint16_t* q = fin_xy + ((size_t)f * max_cand + k) * 8;
                for (int i = 0; i < 4; i++) {  // corners.rotate_left(min_rotation), src/aruco.rs:103
                    const int s2 = (i + o.rotation) & 3;
                    mk.corners[2 * i] = q[2 * s2];
                    mk.corners[2 * i + 1] = q[2 * s2 + 1];
                }
                mk.hamming_distance = o.hamming;
                mk.rotation = o.rotation;
                mk.candidate_index = (uint16_t)k;
                markers[p] = mk;
            } else atomicOr(err_flags, kErrMarkerCap);
        }
        pos += (uint32_t)__popcll(m);
    }
}

// NT threads sample one candidate, PT of them (64, or all) run the stages after the sampling.  History of the shape, on the
// 2.5 k candidates of BASELINE config 2 (round 2, docs/HISTORY.md): 256 threads throughout, 4 samples "in flight" per lane, row-major
// sample order (round 1): 116 us; 64 threads, 8 x 8 blocked order: 98 us; 256 threads sampling, the first wave doing the rest:
// 94 us -- and 7 us less than the 64-thread version inside the pipeline, where the frames are not in any cache.
// Y422: the frames are packed 4:2:2 (src.fmt A3_FMT_YUYV8 / A3_FMT_UYVY8; see grey_tap)
// BOTH: a3_set_marker_polarity's A3_POLARITY_BOTH (include/aruco3_hip.h): a bit matrix whose perimeter is lit all round is read
// complemented, and DecodeOut.decode_ok is 2 for it.  A template parameter for Y422's reason: with BOTH == false nothing below differs
// from the kernel without it, so the default instantiations compile to what they were.
template <int NT, int PT, bool Y422 = false, bool BOTH = false>
__global__ __launch_bounds__(NT, kDecodeWaves) void k_decode(PixelSrc src, int W, int H, uint32_t first_frame,
                                                const uint16_t* __restrict__ fin_xy, const uint32_t* __restrict__ work,
                                                const unsigned int* __restrict__ work_count, uint32_t max_cand, uint32_t S, uint32_t n,
                                                uint32_t max_taps, const uint64_t* __restrict__ dict, uint32_t n_codes, uint32_t tau,
                                                int filter, const ProjRec* __restrict__ proj, const float* __restrict__ wtab, DecodeOut* __restrict__ outs,
                                                uint8_t* __restrict__ patches /*nullable*/, uint32_t patch_cap, uint32_t* __restrict__ per_frame /*nullable*/, int dbg) {
    // dbg (a3_debug_kernel_time only, 0 in the product path): 1 = no sampling, 2 / 3 / 4 = stop after sampling / Otsu / bits
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    uint8_t* s_patch = smem;
    size_t o = ((size_t)S * S + 15) & ~(size_t)15;
    float* s_tmp = reinterpret_cast<float*>(smem + o); o += (size_t)n * S * 4;
    float* s_w = reinterpret_cast<float*>(smem + o); o += (size_t)n * max_taps * 4;
    uint32_t* s_left = reinterpret_cast<uint32_t*>(smem + o); o += (size_t)n * 4;
    uint32_t* s_cnt = reinterpret_cast<uint32_t*>(smem + o); o += (size_t)n * 4;
    uint8_t* s_bits = smem + o;
    __shared__ uint32_t s_hist[256];
    __shared__ float s_inv[9];
    __shared__ int s_ok, s_have;
    __shared__ uint32_t s_otsu;
    __shared__ uint64_t s_codes[4];
    __shared__ unsigned long long s_best[NT / 64][4];
    constexpr int NW = NT / 64;   // waves per candidate
    __shared__ uint32_t s_scan_w[NW], s_scan_s[NW];
    __shared__ double s_var[NW];
    __shared__ int s_vt[NW];

    const int tid = threadIdx.x;
    const uint32_t n_work = *work_count;
    for (uint32_t wi = blockIdx.x; wi < n_work; wi += gridDim.x) {
        const uint32_t slot = work[wi];
        const uint32_t fl = slot / max_cand;
        const uint8_t* img = src.base + (size_t)(first_frame + fl) * src.frame_stride;
        __syncthreads();
        if (tid < 9) s_inv[tid] = proj[wi].inv[tid];
        if (tid == 9) s_ok = proj[wi].ok;
        for (int i = tid; i < 256; i += NT) s_hist[i] = 0;
        __syncthreads();
        const bool ok = s_ok != 0;
        const uint32_t pw = ok ? S : 1u, ph = pw;
        // resize weights (same table for both passes: the patch and the grid are square): the launch-wide table for a full
        // patch, computed in place for the 1x1 stand-in of a failed projection (quirk Q4).  Fetched here, ahead of the
        // sampling, so that the trip to the table is not on the path between the Otsu level and the resize.
        if (ok) {
            for (uint32_t i = tid; i < n * (max_taps + 2); i += NT) {
                const uint32_t oi = i / (max_taps + 2), k = i - oi * (max_taps + 2);
                const float v = wtab[i];
                if (k == 0) s_left[oi] = __float_as_uint(v);
                else if (k == 1) s_cnt[oi] = __float_as_uint(v);
                else if (k - 2 < __float_as_uint(wtab[(size_t)oi * (max_taps + 2) + 1])) s_w[(size_t)oi * max_taps + (k - 2)] = v;
            }
        } else if (tid < (int)n) {
            const uint32_t oi = tid;
            uint32_t cnt;
            s_left[oi] = resize_weights(pw, n, oi, s_w + (size_t)oi * max_taps, &cnt);
            s_cnt[oi] = cnt;
        }
        // warp_into: integer output coordinates, no centre offset, mapping = the projection's inverse
        if (ok && dbg == 1) {
            for (uint32_t i = tid; i < S * S; i += NT) { s_patch[i] = (uint8_t)(i * 7u); atomicAdd(&s_hist[(i * 7u) & 255u], 1u); }
        } else if (ok) {
            const float t0 = s_inv[0], t1 = s_inv[1], t2 = s_inv[2], t3 = s_inv[3], t4 = s_inv[4], t5 = s_inv[5], t6 = s_inv[6],
                        t7 = s_inv[7], t8 = s_inv[8];
            // kU samples per lane per trip: all their row reads (one 12-byte load per row and sample: the two taps of a row
            // are adjacent) are in flight before the first is converted
            constexpr int kU = kDecodeKU;
            // Sample order: blocks of 8 x 8 output pixels, one block per wave instruction (lane = 8 * (y & 7) + (x & 7)).  Taps
            // of a block lie in a compact patch of the frame whatever the marker's rotation, so the 64 lanes of a load touch
            // a few dozen cache lines; a row-major order puts the 64 samples of an instruction on a slanted line that crosses
            // a new image row -- a new cache line -- at almost every sample of a rotated marker.
            const uint32_t bpp = Y422 ? 2u : ((src.fmt == A3_FMT_RGB8) ? 3u : ((src.fmt == A3_FMT_RGBA8 || src.fmt == A3_FMT_BGRA8) ? 4u : 1u));
            // (a frame smaller than one wide read cannot hold a candidate; the weight table is merely something of 16 KB to read)
            const unsigned long long frame_bytes = (unsigned long long)(H - 1) * src.row_stride + (unsigned long long)W * bpp;
            const bool tiny = frame_bytes < 16ull, off32 = frame_bytes < 0xFFFFFFE0ull && src.row_stride < (1ull << 24);
            const uintptr_t img_u = reinterpret_cast<uintptr_t>(img);
            const uint32_t mis = tiny ? 0u : (uint32_t)(img_u & 3u);
            const a3_gptr base4 = reinterpret_cast<a3_gptr>(tiny ? reinterpret_cast<uintptr_t>(wtab) : img_u - mis);
            const uint32_t nbx = (S + 7u) / 8u, n_slots = nbx * nbx * 64u;
            // slot -> (x, y); blk / nbx as (blk * Mb) >> 16, Mb = 2^16 / nbx + 1: exact while blk * nbx < 2^16 (blk < nbx^2 <= 625,
            // nbx <= 25), and full rate
            const uint32_t Mb = 65536u / nbx + 1u;
            auto slot_xy = [&](uint32_t slot, uint32_t* x, uint32_t* y) -> bool {
                const uint32_t blk = slot >> 6, l = slot & 63u, by = __umul24(min(blk, 1023u), Mb) >> 16, bx = blk - __umul24(by, nbx);
                *x = bx * 8u + (l & 7u); *y = by * 8u + (l >> 3);
                return slot < n_slots && *x < S && *y < S;
            };
            for (uint32_t i0 = tid; i0 < n_slots; i0 += NT * kU) {
                TapLoad tl[kU];
#pragma unroll
                for (int u = 0; u < kU; u++) {
                    uint32_t x, y;
                    const bool valid = slot_xy(i0 + (uint32_t)NT * u, &x, &y);
                    const float fx = (float)x, fy = (float)y;
                    const float d = t6 * fx + t7 * fy + t8;
                    const float px = (t0 * fx + t1 * fy + t2) / d;
                    const float py = (t3 * fx + t4 * fy + t5) / d;
                    if (off32) sample_issue<uint32_t>(tl[u], base4, mis, (uint32_t)src.row_stride, (uint32_t)(frame_bytes - 12ull), tiny, bpp, (uint32_t)W, (uint32_t)H, px, py, valid);
                    else sample_issue<unsigned long long>(tl[u], base4, mis, src.row_stride, frame_bytes - 12ull, tiny, bpp, (uint32_t)W, (uint32_t)H, px, py, valid);
                }
#pragma unroll
                for (int u = 0; u < kU; u++) {
                    uint32_t x, y;
                    if (slot_xy(i0 + (uint32_t)NT * u, &x, &y)) {
                        const uint8_t v = sample_finish<Y422>(tl[u], img, (size_t)src.row_stride, src.fmt, bpp);
                        s_patch[__umul24(y, S) + x] = v;
                        atomicAdd(&s_hist[v], 1u);
                    }
                }
            }
        } else if (tid == 0) {  // GrayImage::new(1, 1): one black pixel (quirk Q4)
            s_patch[0] = 0;
            s_hist[0] = 1;
        }
        __syncthreads();
        if (dbg == 2) continue;
        // PT = 64: everything after the sampling is the work of ONE wave, whatever the number of waves that sampled: its stages are short
        // loops over 64 .. 400 items separated by synchronisation points, which for a single wave cost nothing (LDS operations
        // of a wave complete in order; POST_SYNC only keeps the compiler from moving accesses across it), while four waves pay
        // a barrier -- and the wait for every outstanding memory access that comes with it -- at each of them.  The other waves
        // go on to the top of the loop.
        static_assert(PT == 64 || PT == NT, "the stages after the sampling run on one wave or on all");
        constexpr int NWP = PT / 64;
#define POST_SYNC() { if constexpr (PT == NT) __syncthreads(); else { __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront"); __builtin_amdgcn_wave_barrier(); } }
        if (PT == NT || tid < PT) {
            // debug taps: the patch buffer holds patch_cap patches, one per work item (NOT per candidate slot: slots are
            // frame * max_cand + k and would run past the buffer for frames beyond patch_cap / max_cand)
            const bool keep_patch = patches != nullptr && wi < patch_cap;
            if (keep_patch) {
                uint8_t* dst = patches + (size_t)wi * S * S;
                for (uint32_t i = tid; i < S * S; i += PT) dst[i] = ok ? s_patch[i] : 0;
            }
            // otsu_level (imageproc): the reference scans thresholds 0..255 keeping running integer sums and the first strict
            // maximum of w_b * w_f * (mean_b - mean_f)^2 in f64.  The running sums are exact integers, so every threshold can
            // be evaluated independently from prefix sums with the very same f64 operations; the first strict maximum is the
            // largest variance, lowest threshold among equals, and it must exceed the initial 0.0.
            {
                constexpr int B = 256 / PT;                 // thresholds per lane: t = tid * B + k
                uint32_t cw[B], cs[B];                      // inclusive prefix sums inside the lane's run of thresholds
                uint32_t rw = 0, rs = 0;
    #pragma unroll
                for (int k = 0; k < B; k++) {
                    const uint32_t t = (uint32_t)tid * B + k, hcnt = s_hist[t];
                    rw += hcnt; rs += t * hcnt;
                    cw[k] = rw; cs[k] = rs;
                }
                uint32_t bw = wave_incl_add(rw), bs = wave_incl_add(rs);   // inclusive prefix sums over lanes
                if ((tid & 63) == 63) { s_scan_w[tid >> 6] = bw; s_scan_s[tid >> 6] = bs; }
                POST_SYNC();
                uint32_t total_sum_u = 0;
                for (int w = 0; w < NWP; w++) {
                    if (w < (tid >> 6)) { bw += s_scan_w[w]; bs += s_scan_s[w]; }
                    total_sum_u += s_scan_s[w];
                }
                const uint32_t before_w = bw - rw, before_s = bs - rs;   // everything below this lane's first threshold
                const uint32_t total_weight = pw * ph;
                const double total_pixel_sum = (double)total_sum_u;
                double var = -1.0;   // "not a candidate"
                int best_t = tid * B;
    #pragma unroll
                for (int k = 0; k < B; k++) {
                    const uint32_t bwk = before_w + cw[k], bsk = before_s + cs[k];
                    const uint32_t fw = total_weight - bwk;
                    if (bwk != 0 && fw != 0) {
                        const double background_pixel_sum = (double)bsk;
                        const double foreground_pixel_sum = total_pixel_sum - background_pixel_sum;
                        const double background_mean = background_pixel_sum / (double)bwk;
                        const double foreground_mean = foreground_pixel_sum / (double)fw;
                        const double diff = background_mean - foreground_mean;
                        const double mean_diff_squared = diff * diff;
                        const double v = (double)bwk * (double)fw * mean_diff_squared;
                        if (v > var) { var = v; best_t = tid * B + k; }   // ascending k: the first strict maximum of the run
                    }
                }
                wave_best_var_to63(var, best_t);
                if ((tid & 63) == 63) { s_var[tid >> 6] = var; s_vt[tid >> 6] = best_t; }
                POST_SYNC();
                if (tid == 0) {
                    double bv = s_var[0]; int bt = s_vt[0];
                    for (int w = 1; w < NWP; w++) if (s_var[w] > bv || (s_var[w] == bv && s_vt[w] < bt)) { bv = s_var[w]; bt = s_vt[w]; }
                    s_otsu = bv > 0.0 ? (uint32_t)bt : 0u;
                }
            }
            if (dbg == 3) continue;
            // threshold(.., Binary) is applied where the patch is read: a pixel counts as 255 iff it is above the Otsu level
            POST_SYNC();   // s_otsu (and, long ago, the weights)
            const uint32_t otsu = s_otsu;
            if (pw == n) {  // resize() copies when the size already matches
                for (uint32_t i = tid; i < n * n; i += PT) s_bits[i] = s_patch[i] > otsu;   // (255 or 0) > 127
            } else {
                for (uint32_t i = tid; i < n * pw; i += PT) {  // vertical pass into f32
                    const uint32_t oy = i / pw, x = i - oy * pw;
                    const float* ws = s_w + (size_t)oy * max_taps;
                    const uint32_t left = s_left[oy], cnt = s_cnt[oy];
                    float t = 0.0f;
                    for (uint32_t k = 0; k < cnt; k++) t += (s_patch[(left + k) * pw + x] > otsu ? 255.0f : 0.0f) * ws[k];
                    s_tmp[oy * pw + x] = t;
                }
                POST_SYNC();
                for (uint32_t i = tid; i < n * n; i += PT) {  // horizontal pass, clamp, round to nearest
                    const uint32_t y = i / n, ox = i - y * n;
                    const float* ws = s_w + (size_t)ox * max_taps;
                    const uint32_t left = s_left[ox], cnt = s_cnt[ox];
                    float t = 0.0f;
                    for (uint32_t k = 0; k < cnt; k++) t += s_tmp[y * pw + left + k] * ws[k];
                    const float c = t < 0.0f ? 0.0f : (t > 255.0f ? 255.0f : t);
                    s_bits[y * n + ox] = (uint8_t)roundf(c) > 127;
                }
            }
            POST_SYNC();
            if (dbg == 4) continue;
            // border test + 4 rotated codes, src/aruco.rs:287-310.  One lane per (rotation, cell): the bit goes to its place in
            // the code with an LDS atomic (row-major, first cell = most significant bit).
            if (tid < 4) s_codes[tid] = 0;
            {   // the marker's border must be black all round: one lane per border cell (left, right, top, bottom x n)
                const uint32_t end = n ? n - 1 : 0;
                int lit = 0;
                [[maybe_unused]] int all_lit = 1;
                for (uint32_t t = (uint32_t)tid; t < 4u * n; t += PT) {
                    const uint32_t side = t / n, i = t - side * n;
                    const int cell = s_bits[side == 0 ? i * n : (side == 1 ? i * n + end : (side == 2 ? i : end * n + i))];
                    lit |= cell;
                    if constexpr (BOTH) all_lit &= cell;
                }
                const int any_lit = (PT == NT ? __syncthreads_or(lit) : (int)(__ballot(lit) != 0ull));
                if constexpr (BOTH) {   // no cell lit: read dark (this test first); every cell lit: read inverted; else no codes
                    const int every_lit = (PT == NT ? __syncthreads_and(all_lit) : (int)(__ballot(!all_lit) == 0ull));
                    if (tid == 0) s_have = !any_lit ? 1 : (every_lit ? 2 : 0);
                } else
                if (tid == 0) s_have = !any_lit;
            }
            POST_SYNC();
            {
                const uint32_t inner = n >= 2 ? n - 2 : 0, cells = inner * inner;   // <= 64 cells, 4 rotations
                [[maybe_unused]] const uint8_t flip = BOTH ? (uint8_t)(s_have == 2) : (uint8_t)0;
                if (s_have) {
                    for (uint32_t t = (uint32_t)tid; t < 4u * cells; t += PT) {
                        const uint32_t r = t / cells, idx = t - r * cells;
                        const uint32_t y = 1 + idx / inner, x = 1 + idx % inner;
                        // rotation r of the bit matrix, read row-major
                        uint32_t sy, sx;
                        rotated_source(r, n, y, x, &sy, &sx);
                        if (BOTH ? (s_bits[sy * n + sx] ^ flip) != 0 : s_bits[sy * n + sx] != 0) atomicOr(reinterpret_cast<unsigned long long*>(&s_codes[r]), 1ull << (cells - 1 - idx));
                    }
                }
            }
            POST_SYNC();
            const int have = s_have;
            // find_nearest for the 4 codes: strict '<' => lowest index among equal distances
            unsigned long long best[4] = {~0ull, ~0ull, ~0ull, ~0ull};
            if (have) {
                const uint64_t c0 = s_codes[0], c1 = s_codes[1], c2 = s_codes[2], c3 = s_codes[3];
                // eight codes per lane and trip, their loads issued together (unconditional, clamped index): one code per trip is a
                // chain of n_codes / 64 round trips to the table -- 16 for a 1024-code dictionary
                constexpr int DB = kDecodeDB;
                for (uint32_t i0 = tid; i0 < n_codes; i0 += PT * DB) {
                    uint64_t cw[DB];
    #pragma unroll
                    for (int u = 0; u < DB; u++) cw[u] = dict[min(i0 + (uint32_t)(u * PT), n_codes - 1u)];
    #pragma unroll
                    for (int u = 0; u < DB; u++) {
                        const uint32_t i = i0 + (uint32_t)(u * PT);
                        const unsigned long long past = 0ull - (unsigned long long)(i >= n_codes);   // all ones: never the minimum
                        const uint64_t c = cw[u];
                        const unsigned long long k0 = (((unsigned long long)__popcll(c ^ c0) << 32) | i) | past;
                        const unsigned long long k1 = (((unsigned long long)__popcll(c ^ c1) << 32) | i) | past;
                        const unsigned long long k2 = (((unsigned long long)__popcll(c ^ c2) << 32) | i) | past;
                        const unsigned long long k3 = (((unsigned long long)__popcll(c ^ c3) << 32) | i) | past;
                        best[0] = k0 < best[0] ? k0 : best[0];
                        best[1] = k1 < best[1] ? k1 : best[1];
                        best[2] = k2 < best[2] ? k2 : best[2];
                        best[3] = k3 < best[3] ? k3 : best[3];
                    }
                }
    #pragma unroll
                for (int r = 0; r < 4; r++) best[r] = wave_min_u64_to63(best[r]);
                if ((tid & 63) == 63)
                    for (int r = 0; r < 4; r++) s_best[tid >> 6][r] = best[r];
            }
            POST_SYNC();
            if (tid == 0) {
                DecodeOut out;
                out.valid = 0; out.id = 0; out.code = 0; out.rotation = 0; out.hamming = 0; out.patch = keep_patch ? wi : kNone;
                out.hom_ok = ok; out.decode_ok = have;
                for (int r = 0; r < 4; r++) out.codes[r] = have ? s_codes[r] : 0;
                int found_any = 0;
                uint32_t min_code_distance = 0x7FFFFFFFu, min_rotation = 0, min_code_id = 0x7FFFFFFFu;
                uint64_t min_code = 0x7FFFFFFFull;
                if (have) {
                    for (uint32_t r = 0; r < 4; r++) {
                        unsigned long long b = s_best[0][r];
                        for (int w = 1; w < NWP; w++) b = s_best[w][r] < b ? s_best[w][r] : b;
                        // empty dictionary: find_nearest returns (0, 0xFF)
                        const uint32_t nearest_dist = n_codes ? (uint32_t)(b >> 32) : 0xFFu;
                        const uint32_t nearest_id = n_codes ? (uint32_t)b : 0u;
                        if (nearest_dist < min_code_distance) {
                            min_code = s_codes[r]; min_code_distance = nearest_dist; min_code_id = nearest_id; min_rotation = r; found_any = 1;
                        }
                    }
                }
                if (found_any && (!filter || min_code_distance < tau)) {
                    out.valid = 1; out.id = min_code_id; out.code = min_code; out.rotation = (uint8_t)min_rotation;
                    out.hamming = (uint8_t)min_code_distance;
                }
                outs[slot] = out;
                if (out.valid && per_frame) atomicAdd(&per_frame[first_frame + fl], 1u);   // one address per frame: no contention to speak of
            }
        }
#undef POST_SYNC
    }
}

// gather the accepted markers, frame by frame, candidate order preserved: one wave per frame.  per_frame[] already holds
// the number of accepted candidates of every frame (k_decode counted them), so a frame's first output slot is a sum over
// the frames before it, which every wave forms for itself (n_frames is a few hundred; the single-workgroup kernel below
// takes over beyond kCompactParMax frames).
constexpr uint32_t kCompactParMax = 4096;
__global__ __launch_bounds__(256) void k_compact_markers_par(const DecodeOut* __restrict__ outs, const uint16_t* __restrict__ fin_xy,
                                                             const uint32_t* __restrict__ fin_count, uint32_t n_frames, uint32_t max_cand,
                                                             a3_marker* __restrict__ markers, uint32_t marker_cap,
                                                             const uint32_t* __restrict__ per_frame, unsigned int* __restrict__ marker_total,
                                                             unsigned int* __restrict__ err_flags, const uint32_t* __restrict__ cand_count,
                                                             unsigned int* __restrict__ cand_pre_total) {
    const uint32_t f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= n_frames) return;
    compact_frame_wave(f, threadIdx.x & 63, outs, fin_xy, fin_count, n_frames, max_cand, markers, marker_cap, per_frame, marker_total, err_flags, cand_count,
                       cand_pre_total);
}

// The same with one workgroup and no pre-computed counts (any number of frames).
__global__ __launch_bounds__(256) void k_compact_markers(const DecodeOut* __restrict__ outs, const uint16_t* __restrict__ fin_xy,
                                                         const uint32_t* __restrict__ fin_count, uint32_t n_frames, uint32_t first_frame,
                                                         uint32_t max_cand, a3_marker* __restrict__ markers, uint32_t marker_cap,
                                                         uint32_t* __restrict__ per_frame, unsigned int* __restrict__ marker_total,
                                                         unsigned int* __restrict__ err_flags, const uint32_t* __restrict__ cand_count,
                                                         unsigned int* __restrict__ cand_pre_total) {
    __shared__ uint32_t s_scan[256];
    __shared__ uint32_t s_base;
    const int tid = threadIdx.x;
    if (tid == 0) s_base = *marker_total;
    {
        uint32_t pre = 0, most = 0;
        for (uint32_t g = tid; g < n_frames; g += 256) { pre += min(cand_count[g], max_cand); most = max(most, cand_count[g]); }
        if (pre) atomicAdd(cand_pre_total, pre);
        if (most) atomicMax(cand_pre_total + kCandMostFromPre, most);
    }
    __syncthreads();
    for (uint32_t f0 = 0; f0 < n_frames; f0 += 256) {
        const uint32_t f = f0 + tid;
        uint32_t cnt = 0;
        if (f < n_frames) {
            const uint32_t c = fin_count[f];
            for (uint32_t k = 0; k < c; k++) cnt += outs[(size_t)f * max_cand + k].valid;
        }
        s_scan[tid] = cnt;
        __syncthreads();
        for (int o = 1; o < 256; o <<= 1) {
            const uint32_t v = tid >= o ? s_scan[tid - o] : 0;
            __syncthreads();
            s_scan[tid] += v;
            __syncthreads();
        }
        const uint32_t excl = s_scan[tid] - cnt, tile_total = s_scan[255];
        const uint32_t base = s_base;
        if (f < n_frames) {
            per_frame[first_frame + f] = cnt;
            uint32_t pos = base + excl;
            const uint32_t c = fin_count[f];
            for (uint32_t k = 0; k < c; k++) {
                const DecodeOut o = outs[(size_t)f * max_cand + k];
                if (!o.valid) continue;
                if (pos < marker_cap) {
                    a3_marker m;
                    m.frame = first_frame + f;
                    m.id = o.id;
                    m.code = o.code;
                    const uint16_t* q = fin_xy + ((size_t)f * max_cand + k) * 8;
                    for (int i = 0; i < 4; i++) {  // corners.rotate_left(min_rotation), src/aruco.rs:103
                        const int s = (i + o.rotation) & 3;
                        m.corners[2 * i] = q[2 * s];
                        m.corners[2 * i + 1] = q[2 * s + 1];
                    }
                    m.hamming_distance = o.hamming;
                    m.rotation = o.rotation;
                    m.candidate_index = (uint16_t)k;
                    markers[pos] = m;
                } else atomicOr(err_flags, kErrMarkerCap);
                pos++;
            }
        }
        __syncthreads();
        if (tid == 0) s_base = base + tile_total;
        __syncthreads();
    }
    if (tid == 0) *marker_total = s_base;
}

// Fixed-capacity detection records for the multi-GPU gather: one record per frame,
//   u32 count | u32 global frame index | maxm x a3_marker | (with poses: maxm x 2 x a3_pose, the pair of marker k at 2k, 2k+1)
// (marker.frame rewritten to the global index, unused slots zero), written straight from the device-resident marker (and pose)
// list of the last batch: one wave per frame.  A frame with more than maxm markers raises *overflow (the host turns it into
// A3_ERR_CAPACITY: records are never clipped silently).
__global__ __launch_bounds__(256) void k_pack_detections(const a3_marker* __restrict__ markers, const a3_pose* __restrict__ poses /*nullable*/,
                                                         const uint32_t* __restrict__ per_frame,
                                                         uint32_t n_frames, uint32_t first_frame_global, uint32_t maxm,
                                                         uint32_t* __restrict__ dst, unsigned int* __restrict__ overflow) {
    const int lane = threadIdx.x & 63;
    const uint32_t f = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (f >= n_frames) return;
    uint32_t base = 0;
    for (uint32_t g = lane; g < f; g += 64) base += per_frame[g];
    for (int o = 32; o > 0; o >>= 1) base += __shfl_xor(base, o);
    const uint32_t cnt = per_frame[f];
    constexpr uint32_t kMarkerWords = sizeof(a3_marker) / 4, kPoseWords = 2 * sizeof(a3_pose) / 4;
    const uint32_t rec_words = 2u + maxm * (kMarkerWords + (poses ? kPoseWords : 0u));
    uint32_t* rec = dst + (size_t)f * rec_words;
    if (cnt > maxm) { if (lane == 0) atomicOr(overflow, 1u); }
    const uint32_t kept = min(cnt, maxm);
    if (lane == 0) { rec[0] = kept; rec[1] = first_frame_global + f; }
    const uint32_t* src = reinterpret_cast<const uint32_t*>(markers + base);
    for (uint32_t w = lane; w < maxm * kMarkerWords; w += 64) {
        uint32_t v = 0u;
        if (w < kept * kMarkerWords) v = (w % kMarkerWords == 0u) ? first_frame_global + f : src[w];   // word 0 of a marker = .frame
        rec[2u + w] = v;
    }
    if (poses) {
        const uint32_t* ps = reinterpret_cast<const uint32_t*>(poses + 2 * (size_t)base);
        uint32_t* pd = rec + 2u + maxm * kMarkerWords;
        for (uint32_t w = lane; w < maxm * kPoseWords; w += 64) pd[w] = w < kept * kPoseWords ? ps[w] : 0u;
    }
}

// Detection.homographies of one frame in one piece (debug taps): the frame's candidates keep their patches wherever their work
// items fell in the tap; one workgroup per candidate copies its patch into a dense array that leaves in a single D2H copy
// (a copy per patch was a blocking hipMemcpy per candidate).  A candidate whose patch was not kept gets zeros and sets *missing.
__global__ __launch_bounds__(256) void k_gather_patches(const DecodeOut* __restrict__ outs, uint32_t n_cand, const uint8_t* __restrict__ patches,
                                                        uint32_t patch_cap, uint32_t S2, uint8_t* __restrict__ dst, unsigned int* __restrict__ missing) {
    const uint32_t k = blockIdx.x;
    if (k >= n_cand) return;
    const uint32_t slot = outs[k].patch;
    const bool have = slot < patch_cap;
    if (!have && threadIdx.x == 0) atomicOr(missing, 1u);
    const uint8_t* src = patches + (size_t)(have ? slot : 0u) * S2;
    for (uint32_t i = threadIdx.x; i < S2; i += blockDim.x) dst[(size_t)k * S2 + i] = have ? src[i] : (uint8_t)0;
}

hipError_t launch_gather_patches(hipStream_t st, const void* outs_frame, uint32_t n_cand, const uint8_t* patches, uint32_t patch_cap, uint32_t S2,
                                 uint8_t* dst, unsigned int* missing) {
    if (n_cand == 0) return hipSuccess;
    hipLaunchKernelGGL(k_gather_patches, dim3(n_cand), dim3(256), 0, st, reinterpret_cast<const DecodeOut*>(outs_frame), n_cand, patches, patch_cap, S2,
                       dst, missing);
    return hipGetLastError();
}

// the bit-matrix rotation of the decode kernel on its own (reference vectors: src/aruco.rs:414-444)
__global__ void k_debug_rotate_bits(const uint8_t* __restrict__ in, uint32_t n, uint32_t r, uint8_t* __restrict__ out) {
    const uint32_t i = threadIdx.x;
    if (i >= n * n) return;
    uint32_t sy, sx;
    rotated_source(r, n, i / n, i % n, &sy, &sx);
    out[i] = in[sy * n + sx];
}

// ---------------------------------------------------------------------------------------
// IPPE pose, one lane per marker (solve_normalized: a3_ippe.h)
// ---------------------------------------------------------------------------------------
// mode 0: pts = corners / (w,h) (solve_with_undistorted_points); 1: unproject through intrinsics; 2: already normalised;
// 3 / 4: as 0 / 1 from float corners in norm_pts (8 per marker: the refined corners of a3_set_corner_refinement)
// corner_stride: u32 words between the corner lists of consecutive markers (8 for a packed list, 14 inside a3_marker[]);
// n_dev (optional): marker count produced on the device by k_compact_markers.
__global__ void k_pose(const uint32_t* __restrict__ corners, uint32_t corner_stride, const float* __restrict__ norm_pts, uint32_t n,
                       const unsigned int* __restrict__ n_dev, int mode, float marker_size_mm,
                       float iw, float ih, float fx, float fy, float cx, float cy, a3_pose* __restrict__ out) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (n_dev) n = min(n, *n_dev);
    if (i >= n) return;
    float pts[8];
    for (int k = 0; k < 4; k++) {
        if (mode == 2) { pts[2 * k] = norm_pts[8 * i + 2 * k]; pts[2 * k + 1] = norm_pts[8 * i + 2 * k + 1]; continue; }
        const float x = mode >= 3 ? norm_pts[8 * i + 2 * k] : (float)corners[(size_t)corner_stride * i + 2 * k];
        const float y = mode >= 3 ? norm_pts[8 * i + 2 * k + 1] : (float)corners[(size_t)corner_stride * i + 2 * k + 1];
        if (mode == 0 || mode == 3) { pts[2 * k] = x / iw; pts[2 * k + 1] = y / ih; }   // src/pose.rs:60
        else { pts[2 * k] = (x - cx) / fx; pts[2 * k + 1] = (y - cy) / fy; }         // src/pinhole.rs:88-93
    }
    a3_pose p1, p2;
    solve_normalized(pts, marker_size_mm, &p1, &p2);
    out[2 * i] = p1;
    out[2 * i + 1] = p2;
}

// ---------------------------------------------------------------------------------------
// dictionary utilities
// ---------------------------------------------------------------------------------------
__global__ void k_find_nearest(const uint64_t* __restrict__ dict, uint32_t n_codes, const uint64_t* __restrict__ bits, uint32_t n,
                               uint32_t* __restrict__ idx, uint8_t* __restrict__ dist) {
    // one wave per query
    const int lane = threadIdx.x & 63;
    const uint32_t qi = (blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    if (qi >= n) return;
    const uint64_t b = bits[qi];
    unsigned long long best = ~0ull;
    for (uint32_t i = lane; i < n_codes; i += 64) {
        const unsigned long long k = ((unsigned long long)__popcll(dict[i] ^ b) << 32) | i;
        best = k < best ? k : best;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long other = __shfl_xor(best, o);
        best = other < best ? other : best;
    }
    if (lane == 0) {
        idx[qi] = n_codes ? (uint32_t)best : 0u;
        dist[qi] = n_codes ? (uint8_t)(best >> 32) : 0xFF;
    }
}

__global__ void k_calc_tau(const uint64_t* __restrict__ dict, uint32_t n_codes, unsigned int* __restrict__ tau) {
    unsigned int best = 255;
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < n_codes; i += gridDim.x * blockDim.x) {
        const uint64_t c = dict[i];
        for (uint32_t j = i + 1; j < n_codes; j++) {
            const unsigned int d = __popcll(c ^ dict[j]);
            best = d < best ? d : best;
        }
    }
    for (int o = 32; o > 0; o >>= 1) { const unsigned int other = __shfl_xor(best, o); best = other < best ? other : best; }
    if ((threadIdx.x & 63) == 0) atomicMin(tau, best);
}

__global__ void k_selftest_ieee(const double* __restrict__ a, const double* __restrict__ b, uint32_t n, double* __restrict__ sq,
                                double* __restrict__ dv, float* __restrict__ sqf, float* __restrict__ dvf) {
    const uint32_t i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    sq[i] = sqrt(a[i]);
    dv[i] = a[i] / b[i];
    sqf[i] = sqrtf((float)a[i]);
    dvf[i] = (float)a[i] / (float)b[i];
}

// ---------------------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------------------
size_t decode_lds_bytes(uint32_t S, uint32_t n, uint32_t max_taps) {
    size_t o = ((size_t)S * S + 15) & ~(size_t)15;
    o += (size_t)n * S * 4 + (size_t)n * max_taps * 4 + (size_t)n * 8 + (size_t)n * n;
    return (o + 15) & ~(size_t)15;
}

// k_frame_candidates or k_merge_candidates, one wave per frame: the BIG choice, the LDS bytes (20 per slot for quads and perimeters in
// the small form, flag_bytes per slot in both), the dynamic-LDS attribute and the launch
template <typename... P, typename... A>
static hipError_t launch_candidates(hipStream_t st, const DecodeStage& f, void (*small)(P...), void (*through_memory)(P...), uint32_t flag_bytes, A... args) {
    const bool big = f.max_cand > kFrameCandLds;
    if (big && !f.big_scratch) return hipErrorInvalidValue;
    void (*const kernel)(P...) = big ? through_memory : small;
    const size_t lds = (size_t)f.max_cand * (flag_bytes + (big ? 0u : 20u)) + 16;
    if (lds > 48 * 1024) {   // tables grown past the default
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
        if (e != hipSuccess) return e;
    }
    hipLaunchKernelGGL(kernel, dim3(f.n_frames), dim3(64), lds, st, args...);
    return hipGetLastError();
}
hipError_t launch_frame_candidates(hipStream_t st, const DecodeStage& f) {
    return launch_candidates(st, f, k_frame_candidates<false>, k_frame_candidates<true>, 1, f.cands, f.cand_count, f.max_cand, f.min_distance, f.pre_xy,
                             f.fin_xy, f.fin_count, f.work, f.work_count, f.S, reinterpret_cast<ProjRec*>(f.proj), f.big_scratch);
}
hipError_t launch_merge_candidates(hipStream_t st, const DecodeStage& f) {
    if (f.windows < 2 || f.windows > 4 || !f.merged_count || f.plane_cand == 0 || f.max_cand > kMaxCandLimit ||
        (uint64_t)f.windows * f.plane_cand < f.max_cand)
        return hipErrorInvalidValue;
    return launch_candidates(st, f, k_merge_candidates<false>, k_merge_candidates<true>, 2, f.cands, f.cand_count, f.n_frames, f.windows, f.plane_cand,
                             f.max_cand, f.min_distance, f.pre_xy, f.fin_xy, f.fin_count, f.work, f.work_count, f.S, reinterpret_cast<ProjRec*>(f.proj),
                             f.big_scratch, f.merged_count, f.err_flags);
}
uint32_t frame_cand_lds_slots() { return kFrameCandLds; }

size_t proj_rec_bytes() { return sizeof(ProjRec); }
size_t weight_table_bytes() { return kWeightTableBytes; }
hipError_t launch_weight_table(hipStream_t st, uint32_t S, uint32_t n, uint32_t max_taps, float* wtab) {
    if ((size_t)n * (max_taps + 2) * 4 > kWeightTableBytes || n > 64) return hipErrorInvalidValue;
    hipLaunchKernelGGL(k_weight_table, dim3(1), dim3(64), 0, st, S, n, max_taps, wtab);
    return hipGetLastError();
}

hipError_t launch_decode(hipStream_t st, const DecodeStage& d) {
    ProjRec* recs = reinterpret_cast<ProjRec*>(d.proj);
    if (d.projection) hipLaunchKernelGGL(k_projection, dim3(256), dim3(64), 0, st, d.fin_xy, d.work, d.work_count, d.S, recs);
    // Four waves sample a candidate: a candidate is a chain of round trips to the frame (19 of them for one wave: 65 us for a lone
    // candidate however idle the chip is, 33 us with four waves).  What follows the sampling runs on all four waves when the
    // batch is small and every microsecond of that chain shows (`few`: at most 64 frames; 36 us for the 337 candidates of 32
    // frames against 39), and on one wave -- no workgroup barriers -- when thousands of candidates are in flight and only the
    // throughput counts (BASELINE config 2: decode stage 0.123 ms against 0.130 with one wave per candidate throughout).
    const size_t lds = decode_lds_bytes(d.S, d.n, d.max_taps);
    // (packed 4:2:2: the samplers' instantiation of their own, grey_tap; inverted: a3_set_marker_polarity's A3_POLARITY_BOTH)
    const bool y422 = d.src.fmt == A3_FMT_YUYV8 || d.src.fmt == A3_FMT_UYVY8;
    auto launch = [&](auto kernel, int threads) {
        hipLaunchKernelGGL(kernel, dim3(d.grid_blocks), dim3(threads), lds, st, d.src, d.W, d.H, d.first_frame, d.fin_xy, d.work, d.work_count, d.max_cand, d.S,
                           d.n, d.max_taps, d.dict, d.n_codes, d.tau, d.filter, recs, d.wtab, reinterpret_cast<DecodeOut*>(d.outs), d.patches, d.patch_cap,
                           d.per_frame, d.variant);
    };
    auto pick = [&](auto y, auto both) {
        constexpr bool Y = decltype(y)::value, B = decltype(both)::value;
        if (d.few) launch(k_decode<256, 256, Y, B>, 256);
        else launch(k_decode<kDecodeThreads, 64, Y, B>, kDecodeThreads);
    };
    if (d.inverted) { if (y422) pick(std::true_type{}, std::true_type{}); else pick(std::false_type{}, std::true_type{}); }
    else { if (y422) pick(std::true_type{}, std::false_type{}); else pick(std::false_type{}, std::false_type{}); }
    return hipGetLastError();
}

size_t decode_out_bytes() { return sizeof(DecodeOut); }

hipError_t launch_compact_markers(hipStream_t st, const DecodeStage& c) {
    const DecodeOut* outs = reinterpret_cast<const DecodeOut*>(c.outs);
    if (c.first_frame == 0 && c.n_frames <= kCompactParMax)
        hipLaunchKernelGGL(k_compact_markers_par, dim3((c.n_frames + 3) / 4), dim3(256), 0, st, outs, c.fin_xy, c.fin_count, c.n_frames, c.max_cand, c.markers,
                           c.marker_cap, c.per_frame, c.marker_total, c.err_flags, c.cand_count, c.cand_pre_total);
    else
        hipLaunchKernelGGL(k_compact_markers, dim3(1), dim3(256), 0, st, outs, c.fin_xy, c.fin_count, c.n_frames, c.first_frame, c.max_cand, c.markers,
                           c.marker_cap, c.per_frame, c.marker_total, c.err_flags, c.cand_count, c.cand_pre_total);
    return hipGetLastError();
}

// a3_get_marker_flags: one lane per marker of the final list (behind the gather and the recovery merge): A3_MARKER_INVERTED iff the
// candidate the marker names was read inverted (decode_ok == 2).  A marker that names no slot of the tables gets 0.
__global__ __launch_bounds__(256) void k_marker_flags(const a3_marker* __restrict__ markers, const unsigned int* __restrict__ n_dev, uint32_t cap,
                                                      const DecodeOut* __restrict__ outs, uint32_t n_frames, uint32_t max_cand,
                                                      uint32_t* __restrict__ flags) {
    const uint32_t total = min(cap, *n_dev);
    for (uint32_t i = blockIdx.x * blockDim.x + threadIdx.x; i < total; i += gridDim.x * blockDim.x) {
        const uint32_t f = markers[i].frame, k = markers[i].candidate_index;
        const bool in_table = f < n_frames && k < max_cand;
        flags[i] = in_table && outs[(size_t)f * max_cand + k].decode_ok == 2 ? A3_MARKER_INVERTED : 0u;
    }
}

hipError_t launch_marker_flags(hipStream_t st, const MarkerFlagsLaunch& m) {
    if (m.n == 0) return hipSuccess;
    const uint32_t want = (m.n + 255u) / 256u, blocks = want < 1024u ? want : 1024u;
    hipLaunchKernelGGL(k_marker_flags, dim3(blocks), dim3(256), 0, st, m.markers, m.n_dev, m.n, reinterpret_cast<const DecodeOut*>(m.outs), m.n_frames,
                       m.max_cand, m.flags);
    return hipGetLastError();
}

hipError_t launch_pack_detections(hipStream_t st, const a3_marker* markers, const a3_pose* poses, const uint32_t* per_frame, uint32_t n_frames,
                                  uint32_t first_frame_global, uint32_t maxm, void* dst, unsigned int* overflow) {
    hipLaunchKernelGGL(k_pack_detections, dim3((n_frames + 3) / 4), dim3(256), 0, st, markers, poses, per_frame, n_frames, first_frame_global, maxm,
                       reinterpret_cast<uint32_t*>(dst), overflow);
    return hipGetLastError();
}

hipError_t launch_debug_rotate_bits(hipStream_t st, const uint8_t* in, uint32_t n, uint32_t r, uint8_t* out) {
    hipLaunchKernelGGL(k_debug_rotate_bits, dim3(1), dim3(256), 0, st, in, n, r, out);
    return hipGetLastError();
}

hipError_t launch_pose(hipStream_t st, const PoseLaunch& p) {
    hipLaunchKernelGGL(k_pose, dim3((p.n + 63) / 64), dim3(64), 0, st, p.corners, p.corner_stride, p.norm_pts, p.n, p.n_dev, p.mode, p.marker_size_mm, p.iw, p.ih,
                       p.fx, p.fy, p.cx, p.cy, p.out);
    return hipGetLastError();
}

hipError_t launch_find_nearest(hipStream_t st, const uint64_t* dict, uint32_t n_codes, const uint64_t* bits, uint32_t n, uint32_t* idx,
                               uint8_t* dist) {
    hipLaunchKernelGGL(k_find_nearest, dim3((n * 64 + 255) / 256), dim3(256), 0, st, dict, n_codes, bits, n, idx, dist);
    return hipGetLastError();
}

hipError_t launch_calc_tau(hipStream_t st, const uint64_t* dict, uint32_t n_codes, unsigned int* tau) {
    hipLaunchKernelGGL(k_calc_tau, dim3(64), dim3(256), 0, st, dict, n_codes, tau);
    return hipGetLastError();
}

hipError_t launch_selftest(hipStream_t st, const double* a, const double* b, uint32_t n, double* sq, double* dv, float* sqf, float* dvf) {
    hipLaunchKernelGGL(k_selftest_ieee, dim3((n + 255) / 256), dim3(256), 0, st, a, b, n, sq, dv, sqf, dvf);
    return hipGetLastError();
}

}  // namespace a3
