// k_recover.hip -- board-aided recovery of markers the decoder rejected (a3_set_board_recovery / a3_recover_markers).  Not part of the
// reference: an extension stated in include/aruco3_hip.h and restated on the CPU by tests/recover_oracle.c (a3o_recover_markers), in
// the same order of operations.
//
// k_recover_frames, one workgroup of four waves per frame.  Wave 0 lists the frame's usable board markers in list order (a ballot per 64
// markers keeps the order) as float correspondences in LDS and solves the frame homography with the calibration's view_homography; wave 1
// lists the missing board slots meanwhile.  The pair search gives every missing marker to one wave, whose lanes walk the candidates: a
// lane keeps the smallest (d2, candidate, shift) it met, the wave combines the lanes by an xor butterfly over that key -- a minimum over
// an order-independent key, so no result depends on which lane or wave came first.  The two-level assignment compares the missing
// markers pairwise in LDS (a candidate table would not fit: 65 536 candidates).  Nothing is accumulated through global atomics; the
// workgroup owns its frame's output records.
// k_recover_merge, one workgroup per frame, copies the detected markers and the recovered ones into the merged list; a frame's place is
// the sum of the counts before it, which every workgroup forms for itself.
#include <cmath>

#include "a3_board.h"
#include "a3_calib.h"
#include "a3_common.h"
#include "a3_launch.h"

namespace a3 {

constexpr int kRecThreads = 256, kRecWaves = kRecThreads / 64;
constexpr int kRecRowDoubles = 64 * 2 * kHomAug;
static_assert(kRecRowDoubles >= 64 + 64 + 8 + 8, "the homography works in the row buffer");
static_assert(A3_CALIB_MAX_POINTS >= 4 * A3_BOARD_MAX_MARKERS, "a frame's correspondences are one calibration view");
constexpr uint32_t kNoPick = 0xFFFFFFFFu;

struct RecCand {
    uint32_t xy[8];
    uint64_t codes[4];
    bool has;
};

__device__ __forceinline__ uint32_t rec_marker_slot(const RecoverLaunch& a, uint32_t m) {
    const uint32_t id = a.markers ? a.markers[m].id : a.ids[m];
    return id < a.board.n_codes ? (uint32_t)a.board.slot_of[id] : (uint32_t)kNoSlot;
}

// candidate c of frame f -> whether it is eligible (it did not become a marker)
__device__ __forceinline__ bool rec_load_cand(const RecoverLaunch& a, uint32_t f, uint32_t c, RecCand* q) {
    if (a.outs) {
        const size_t slot = (size_t)f * a.max_cand + c;
        const DecodeOut* o = reinterpret_cast<const DecodeOut*>(a.outs) + slot;
        if (o->valid) return false;
        q->has = o->hom_ok != 0 && o->decode_ok != 0;
        for (int r = 0; r < 4; r++) q->codes[r] = o->codes[r];
        const uint16_t* p = a.fin_xy + slot * 8;
        for (int k = 0; k < 8; k++) q->xy[k] = p[k];
    } else {
        q->has = a.has_codes[c] != 0;
        for (int r = 0; r < 4; r++) q->codes[r] = a.codes4[4 * (size_t)c + r];
        for (int k = 0; k < 8; k++) q->xy[k] = a.cand_xy[8 * (size_t)c + k];
    }
    return true;
}

// step 2: the four expected corners of a board slot through H; false: the marker is skipped
__device__ __forceinline__ bool rec_expected(const double* H, const BoardSlot& s, double e[8]) {
    bool ok = true;
    for (int j = 0; j < 4; j++) {
        const double X = (double)s.x[j], Y = (double)s.y[j];
        const double u = (H[0] * X + H[1] * Y) + H[2];
        const double v = (H[3] * X + H[4] * Y) + H[5];
        const double w = (H[6] * X + H[7] * Y) + H[8];
        const double ex = u / w, ey = v / w;
        ok = ok && w > 0.0 && fin(w) && fin(ex) && fin(ey);
        e[2 * j] = ex; e[2 * j + 1] = ey;
    }
    return ok;
}

// step 3: d2(m, c, r)
__device__ __forceinline__ double rec_d2(const double e[8], const uint32_t xy[8], int r) {
    double d2 = 0.0;
    for (int j = 0; j < 4; j++) {
        const int s = (j + r) & 3;
        const double dx = e[2 * j] - (double)xy[2 * s], dy = e[2 * j + 1] - (double)xy[2 * s + 1];
        const double d = dx * dx + dy * dy;
        d2 = d > d2 ? d : d2;
    }
    return d2;
}

__global__ __launch_bounds__(kRecThreads) void k_recover_frames(RecoverLaunch a) {
    __shared__ double s_rows[kRecRowDoubles];
    __shared__ double s_wv[8], s_H[9];
    __shared__ float s_obj[8 * A3_BOARD_MAX_MARKERS], s_img[8 * A3_BOARD_MAX_MARKERS];   // the frame's correspondences (step 1)
    __shared__ double s_d2[A3_BOARD_MAX_MARKERS];      // per missing marker: its pick's d2 ...
    __shared__ uint32_t s_pick[A3_BOARD_MAX_MARKERS];  // ... and (c << 2) | r, kNoPick: none
    __shared__ uint16_t s_miss[A3_BOARD_MAX_MARKERS];  // the missing slots, ascending
    __shared__ uint8_t s_win[A3_BOARD_MAX_MARKERS];
    __shared__ uint32_t s_seen[A3_BOARD_MAX_MARKERS / 32], s_dup[A3_BOARD_MAX_MARKERS / 32];
    __shared__ uint32_t s_ok, s_nmiss, s_nrec;
    const uint32_t f = blockIdx.x;
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const uint32_t nb = min(a.n_slots, (uint32_t)A3_BOARD_MAX_MARKERS);
    const BoardSlot* slots = reinterpret_cast<const BoardSlot*>(a.board.slots);
    uint32_t first, cnt;   // the frame's run of the marker list (every wave)
    board_frame_run(a.markers != nullptr, a.per_frame, a.n, a.n_dev, f, lane, &first, &cnt);
    const uint32_t n_cand = a.outs ? min(a.fin_count[f], a.max_cand) : a.n_cand;
    if (tid == 0) { s_ok = 0; s_nmiss = 0; s_nrec = 0; }
    board_mark_duplicates(s_seen, s_dup, cnt, true, (uint32_t)tid, (uint32_t)kRecThreads, [&](uint32_t i) {
        const uint32_t slot = rec_marker_slot(a, first + i);
        return slot >= nb ? (uint32_t)kNoSlot : slot;   // (a slot past the board's does not count)
    });
    if (wave == 0) {   // ---- step 1: correspondences in list order, then the homography ----
        uint32_t k = 0;
        for (uint32_t i0 = 0; i0 < cnt; i0 += 64) {
            const uint32_t i = i0 + (uint32_t)lane;
            uint32_t slot = kNoSlot;
            if (i < cnt) slot = rec_marker_slot(a, first + i);
            const bool use = slot < nb && !board_dup(s_dup, slot);
            const unsigned long long mask = __ballot(use);
            const uint32_t u = k + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
            if (use && u < (uint32_t)A3_BOARD_MAX_MARKERS) {
                const BoardSlot& bs = slots[slot];
                for (int j = 0; j < 4; j++) {
                    s_obj[8 * u + 2 * j] = bs.x[j]; s_obj[8 * u + 2 * j + 1] = bs.y[j];
                    const uint32_t px = a.markers ? a.markers[first + i].corners[2 * j] : a.corners[8 * (size_t)(first + i) + 2 * j];
                    const uint32_t py = a.markers ? a.markers[first + i].corners[2 * j + 1] : a.corners[8 * (size_t)(first + i) + 2 * j + 1];
                    s_img[8 * u + 2 * j] = (float)px; s_img[8 * u + 2 * j + 1] = (float)py;
                }
            }
            k += (uint32_t)__popcll(mask);
        }
        k = min(k, (uint32_t)A3_BOARD_MAX_MARKERS);   // (unique slots: never more)
        wave_sync();
        bool ok = false;
        if (k >= 1 && k >= a.cfg.min_markers) ok = view_homography(s_obj, s_img, 0, 4 * k, s_rows, s_wv, lane, s_H);   // (k: wave-uniform)
        if (lane == 0) s_ok = ok ? 1u : 0u;
    } else if (wave == 1) {   // ---- the missing slots, ascending ----
        uint32_t k = 0;
        for (uint32_t s0 = 0; s0 < nb; s0 += 64) {
            const uint32_t s = s0 + (uint32_t)lane;
            const bool miss = s < nb && !((s_seen[s >> 5] >> (s & 31)) & 1u);
            const unsigned long long mask = __ballot(miss);
            if (miss) s_miss[k + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull))] = (uint16_t)s;
            k += (uint32_t)__popcll(mask);
        }
        if (lane == 0) s_nmiss = k;
    }
    __syncthreads();
    const uint32_t nmiss = s_ok ? s_nmiss : 0u;
    if (nmiss == 0 || n_cand == 0) {   // (uniform over the workgroup)
        if (tid == 0) a.rec_count[f] = 0;
        return;
    }
    const double bound = (double)a.cfg.max_distance_px * (double)a.cfg.max_distance_px;
    const uint32_t max_hamming = a.cfg.max_hamming;
    const bool compare_bits = max_hamming != 255u;
    // ---- steps 2-4a: every missing marker's best feasible (c, r); one wave per marker, lanes over the candidates ----
    for (uint32_t mi = (uint32_t)wave; mi < nmiss; mi += kRecWaves) {
        const uint32_t slot = s_miss[mi];
        double e[8];
        double best_d2 = INFINITY;
        uint32_t best_key = kNoPick;
        if (rec_expected(s_H, slots[slot], e)) {   // (uniform over the wave)
            const uint64_t want = a.dict[a.slot_ids[slot]];
            for (uint32_t c = (uint32_t)lane; c < n_cand; c += 64) {
                RecCand q;
                if (!rec_load_cand(a, f, c, &q)) continue;
                if (compare_bits && !q.has) continue;
                for (int r = 0; r < 4; r++) {
                    if (compare_bits && (uint32_t)__popcll(q.codes[r] ^ want) > max_hamming) continue;
                    const double d2 = rec_d2(e, q.xy, r);
                    if (d2 <= bound && d2 < best_d2) { best_d2 = d2; best_key = (c << 2) | (uint32_t)r; }   // (c, r ascend: ties keep the first)
                }
            }
            for (int o = 32; o >= 1; o >>= 1) {
                const double od = __shfl_xor(best_d2, o);
                const uint32_t ok = (uint32_t)__shfl_xor((int)best_key, o);
                if (od < best_d2 || (od == best_d2 && ok < best_key)) { best_d2 = od; best_key = ok; }
            }
        }
        if (lane == 0) { s_pick[mi] = best_key; s_d2[mi] = best_d2; }
    }
    __syncthreads();
    // ---- step 4b: a candidate taken by several markers goes to the smallest d2, then the lowest slot ----
    for (uint32_t mi = (uint32_t)tid; mi < nmiss; mi += kRecThreads) {
        const uint32_t pick = s_pick[mi];
        bool win = pick != kNoPick;
        if (win) {
            const double d2 = s_d2[mi];
            for (uint32_t mj = 0; mj < nmiss; mj++) {
                const uint32_t pj = s_pick[mj];
                if (mj == mi || pj == kNoPick || (pj >> 2) != (pick >> 2)) continue;
                const double dj = s_d2[mj];
                if (dj < d2 || (dj == d2 && mj < mi)) win = false;
            }
        }
        s_win[mi] = win ? 1 : 0;
    }
    __syncthreads();
    // ---- steps 5-6: the winners' records, in candidate order ----
    for (uint32_t mi = (uint32_t)tid; mi < nmiss; mi += kRecThreads) {
        if (!s_win[mi]) continue;
        const uint32_t pick = s_pick[mi], c = pick >> 2, r = pick & 3u;
        uint32_t rank = 0;
        for (uint32_t mj = 0; mj < nmiss; mj++) rank += (s_win[mj] && (s_pick[mj] >> 2) < c) ? 1u : 0u;
        atomicAdd(&s_nrec, 1u);
        RecCand q;
        if (rank >= a.rec_cap || !rec_load_cand(a, f, c, &q)) continue;   // (never: winners <= min(slots, candidates) <= rec_cap)
        const uint32_t id = a.slot_ids[s_miss[mi]];
        a3_marker m;
        m.frame = f;
        m.id = id;
        m.code = q.has ? q.codes[r] : 0ull;
        for (int i = 0; i < 4; i++) {
            const int s = (i + (int)r) & 3;
            m.corners[2 * i] = q.xy[2 * s]; m.corners[2 * i + 1] = q.xy[2 * s + 1];
        }
        m.hamming_distance = compare_bits ? (uint8_t)__popcll(q.codes[r] ^ a.dict[id]) : (uint8_t)255;
        m.rotation = (uint8_t)r;
        m.candidate_index = (uint16_t)c;
        a.rec[(size_t)f * a.rec_cap + rank] = m;
    }
    __syncthreads();
    if (tid == 0) a.rec_count[f] = min(s_nrec, a.rec_cap);
}

__global__ __launch_bounds__(kRecThreads) void k_recover_merge(RecoverMergeLaunch a) {
    __shared__ uint32_t s_det[kRecThreads], s_rec[kRecThreads];
    const uint32_t f = blockIdx.x;
    const int tid = threadIdx.x;
    uint32_t db = 0, rb = 0;
    for (uint32_t g = (uint32_t)tid; g < f; g += kRecThreads) { db += a.det_per_frame[g]; rb += a.rec_count[g]; }
    s_det[tid] = db; s_rec[tid] = rb;
    __syncthreads();
    for (int o = kRecThreads / 2; o >= 1; o >>= 1) {
        if (tid < o) { s_det[tid] += s_det[tid + o]; s_rec[tid] += s_rec[tid + o]; }
        __syncthreads();
    }
    const uint32_t det_first = s_det[0], base = s_det[0] + s_rec[0];
    const uint32_t dcnt = a.det_per_frame[f], rcnt = min(a.rec_count[f], a.rec_cap);
    for (uint32_t i = (uint32_t)tid; i < dcnt + rcnt; i += kRecThreads) {
        const uint32_t pos = base + i;
        if (pos >= a.out_cap) continue;
        if (i < dcnt) {
            if (det_first + i < a.det_cap) a.out[pos] = a.det[det_first + i];   // (a short gather has raised kErrMarkerCap already)
        } else a.out[pos] = a.rec[(size_t)f * a.rec_cap + (i - dcnt)];
    }
    if (tid == 0) {
        a.per_frame[f] = dcnt + rcnt;
        if (f + 1 == a.n_frames) {   // the list's total: this workgroup alone writes it (the kernels ahead on the stream are done)
            const uint32_t total = base + dcnt + rcnt;
            *a.marker_total = total;
            if (total > a.out_cap) *a.err_flags = *a.err_flags | kErrMarkerCap;
        }
    }
}

hipError_t launch_recover_frames(hipStream_t st, const RecoverLaunch& r) {
    if (r.n_frames == 0) return hipSuccess;
    hipLaunchKernelGGL(k_recover_frames, dim3(r.n_frames), dim3(kRecThreads), 0, st, r);
    return hipGetLastError();
}

hipError_t launch_recover_merge(hipStream_t st, const RecoverMergeLaunch& m) {
    if (m.n_frames == 0) return hipSuccess;
    hipLaunchKernelGGL(k_recover_merge, dim3(m.n_frames), dim3(kRecThreads), 0, st, m);
    return hipGetLastError();
}

}  // namespace a3
