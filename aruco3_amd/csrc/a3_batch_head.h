// The head of a batch's zero block and what the host makes of it -- the one definition: the 64 scratch words the kernels and the host
// share (BatchScratch), the per-chunk DeviceCounters behind them, the verdict finish_batch reaches from both (batch_verdict: deliver,
// re-run with a hint or a pool grown, or fail) and the plan arithmetic enqueue_chain launches by (chunks, frame bases, rounds, the zero
// block's layout, pool sizes).  Plain arithmetic on values -- no HIP, no context -- so a plain C++ program walks every branch
// (tests/batch_verdict.cpp); a3_common.h includes this file, so the kernels see the same declarations.
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/aruco3_hip.h"

namespace a3 {

template <typename T> constexpr T min_of(T a, T b) { return b < a ? b : a; }
template <typename T> constexpr T max_of(T a, T b) { return a < b ? b : a; }

// ---- what the device writes -----------------------------------------------------------------------------------------------------------
constexpr uint32_t kMaxChunkFrames = 65536u;   // a dart record holds its frame's index inside the chunk in 16 bits (dart_rec)
constexpr int kResolveItersMax = 16;           // start-resolution passes a launch sequence can hold
// slot counters spread over this many addresses, picked by blockIdx.x (or the leader's tile) & (shards - 1)
constexpr uint32_t kLeaderShards = 16, kEntryShards = 16, kDeadShards = 16;

struct DeviceCounters {
    unsigned long long darts;       // per chunk: next free dart
    unsigned long long points;      // next free point
    unsigned int contours;          // next free ContourRec
    unsigned int traced;            // cycles with a start event (stat)
    unsigned int err_flags;         // kErr*
    unsigned int resolve_needed;    // set by k_resolve_fast: some border's first start event does not fire -> run the fixpoint passes
    unsigned int jump_changed[32];     // per doubling round: darts whose key changed
    unsigned int resolve_changed[16];  // per start-resolution pass: cycles whose start moved
    unsigned int entry_overflow;    // k_entry_frame: a frame has more entries than fit in LDS -> re-run with the global doubling rounds
    unsigned int pad[1];
};
static_assert(sizeof(DeviceCounters::resolve_changed) / sizeof(unsigned int) == kResolveItersMax, "one resolve_changed slot per pass");

constexpr unsigned kErrBrokenEvent = 1u,   // an event dart on a broken chain
                   kErrPointPool = 2u, kErrContourTable = 4u, kErrCandTable = 8u,   // a pool or table overflowed
                   kErrResolve = 16u,      // the start-resolution passes launched did not converge
                   kErrMarkerCap = 32u,    // more markers than the list holds
                   kErrScatter = 64u;      // k_scatter_points / k_cycle_select: a store's index failed its bounds check (nothing was stored)

// k_tile_scan's plan workgroup (plan_frames) writes these for a device-planned batch
struct PlanWords {
    uint32_t darts;             // the batch's dart total; 0 when it exceeds the capacity the batch was launched with
    uint32_t overflow;          // ... 1 then: every later kernel is a no-op and the host plans the re-run itself
    uint32_t max_frame_darts;   // the largest frame
    uint32_t total_clamped;     // the dart total whether it fits or not, at most 2^32 - 1
};
// The 256 bytes at the head of the zero block: zeroed with it once per batch, read back with the counters and the markers in one copy.
struct BatchScratch {
    unsigned int work_count;       // k_frame_candidates: work items = quads that survived discard_too_near
    unsigned int marker_total;     // the marker gather (k_compact_markers*)
    unsigned int cand_pre_total;   // ... quads after contours_to_candidates, each frame's clipped to its table
    unsigned int pack_overflow;    // a3_pack_detections: a frame holds more markers than its record
    unsigned int err_flags;        // kErr* of the contour stage's quads and the decode stage (each chunk's DeviceCounters holds its own)
    unsigned int cand_most;        // the marker gather: the fullest frame's quad count, beyond its table's slots too
    unsigned int unused6[2];
    PlanWords plan;
    unsigned int unused12[4];
    unsigned int leader_count[kLeaderShards];   // per chunk (zeroed between chunks with entry_count): leaders of cycles with a start event
    unsigned int entry_count[kEntryShards];     // ... entries: darts whose predecessor lies in another tile
    unsigned int dead_count[kDeadShards];       // all chunks: borders k_local_contract finished with (traced, never listed)
};
static_assert(offsetof(BatchScratch, work_count) == 0 && offsetof(BatchScratch, marker_total) == 4 && offsetof(BatchScratch, cand_pre_total) == 8 &&
              offsetof(BatchScratch, pack_overflow) == 12 && offsetof(BatchScratch, err_flags) == 16 && offsetof(BatchScratch, cand_most) == 20 &&
              offsetof(BatchScratch, plan) == 32 && offsetof(PlanWords, darts) == 0 && offsetof(PlanWords, overflow) == 4 &&
              offsetof(PlanWords, max_frame_darts) == 8 && offsetof(PlanWords, total_clamped) == 12 && offsetof(BatchScratch, leader_count) == 64 &&
              offsetof(BatchScratch, entry_count) == 128 && offsetof(BatchScratch, dead_count) == 192 && sizeof(BatchScratch) == 256,
              "the scratch words' offsets are part of the read-back head");
static_assert(offsetof(BatchScratch, entry_count) == offsetof(BatchScratch, leader_count) + sizeof(BatchScratch::leader_count),
              "leader and entry counts are cleared by one memset");
// the marker gather is handed &cand_pre_total and writes the fullest frame's count this many words behind it
constexpr unsigned kCandMostFromPre = (offsetof(BatchScratch, cand_most) - offsetof(BatchScratch, cand_pre_total)) / sizeof(unsigned int);

// ---- limits and the hints a context carries from batch to batch -------------------------------------------------------------------------
// Quad candidates kept per frame.  The reference is unbounded (src/aruco.rs:124-166 pushes into a Vec); here the tables start at
// kMaxCandDefault per frame and a batch that overflows them is re-run with tables twice the size (1024, 2048, 4096, 6144 -- as far as the
// per-frame ordering + discard_too_near kernel keeps a frame's candidates in LDS, 21 bytes each -- then 12 288 ... through memory), up
// to kMaxCandLimit = 65 536, where a3_marker.candidate_index (16 bits) ends; beyond that: A3_ERR_LIMIT.
constexpr uint32_t kMaxCandDefault = 1024, kMaxCandLimit = A3_MAX_CANDIDATES_PER_FRAME;
static_assert(kMaxCandLimit == 65536, "a3_marker.candidate_index is a uint16_t");
constexpr uint32_t kMaxContoursDefault = 1u << 20;
constexpr uint64_t kMaxDartsDefault = 48ull << 20;
constexpr uint64_t kMaxPointsDefault = 64ull << 20;
// dart indices and entry slots (at most 32 k above the darts) stay below 2^30: a pending FinState holds a 30-bit slot beside its
// marker bit (k_contours.hip)
constexpr uint64_t kHardMaxDarts = (1ull << 30) - (1ull << 16);
constexpr uint64_t kHardMaxPoints = 3ull << 30;

struct BatchHints {
    // launch-count hints (every pass past convergence is an empty launch of ~5 us): start low, retry the batch with the
    // maximum if a pass count turns out too small
    int jump_rounds_hint = 10, resolve_iters_hint = 4;
    int resolve_full_ttl = 0;   // > 0: launch the fixpoint passes over all darts too (a recent batch needed them); else only k_resolve_fast
    int entry_global_ttl = 0;   // > 0: a recent batch had a frame whose entry list did not fit LDS: use the global doubling rounds
    // device-side planning: the previous batch of this shape fitted one chunk with plan_darts darts, so this one is enqueued
    // without reading the dart counts back first (k_plan); an overflow falls back to the host plan once (force_host_plan)
    bool plan_valid = false, force_host_plan = false;
    uint32_t plan_n = 0, plan_W = 0, plan_H = 0;
    uint64_t plan_darts = 0;
    uint64_t max_points = kMaxPointsDefault;
    uint32_t max_contours = kMaxContoursDefault;
    uint32_t max_cand = kMaxCandDefault;   // candidate slots per frame (grows on overflow, see kMaxCandLimit)
};

// ---- the verdict ----------------------------------------------------------------------------------------------------------------------
// what the batch record knows; lds_slots: frame_cand_lds_slots(); slot_bytes: what a candidate slot costs over all per-frame tables
// while a frame's candidates are ordered in LDS
struct BatchFacts {
    uint32_t n, W, H; bool device_plan; size_t n_chunks; uint64_t chunk0_darts; int rounds_max; size_t out_cap; uint32_t lds_slots; size_t slot_bytes;
};
struct Verdict {
    // Rerun: the hints say how.  GrowCands: a re-run with next_cand slots per frame at slot_bytes each, once the caller has found that
    // the tables fit the device and committed BatchHints::max_cand.  Fail: code and message.
    enum Action { Deliver, Rerun, GrowCands, Fail } action = Deliver;
    int code = A3_OK; const char* message = nullptr;
    uint32_t next_cand = 0; size_t slot_bytes = 0;
    // a3_stats (darts: of a device-planned batch), all zero when the device's plan overflowed: nothing else was looked at
    uint64_t darts = 0, contours_traced = 0, contours_materialised = 0; uint32_t jump_rounds = 0, resolve_iterations = 0;
    uint32_t total = 0, n_work = 0, n_pre = 0;             // Deliver: markers, work items, quads before discard_too_near
    uint32_t tap_contours = 0; uint64_t tap_points = 0;    // ... chunk 0's contour table and point pool (debug taps)
};

// The order of the checks is the policy: an earlier one hides every later one until the re-run it asks for has cured it.
inline Verdict batch_verdict(const BatchScratch& hs, const DeviceCounters* hc, const BatchFacts& f, BatchHints& h) {
    Verdict v;
    const auto rerun = [&v]() { v.action = Verdict::Rerun; return v; };
    const auto fail = [&v](int code, const char* message) { v.action = Verdict::Fail; v.code = code; v.message = message; return v; };
    if (f.device_plan) {
        if (hs.plan.overflow) { h.force_host_plan = true; return rerun(); }   // the graph outgrew the hint: plan on the host this once
        v.darts = hs.plan.darts;
        h.plan_darts = hs.plan.darts;
    } else {
        h.plan_valid = f.n_chunks == 1;
        h.plan_n = f.n; h.plan_W = f.W; h.plan_H = f.H;
        h.plan_darts = f.n_chunks == 1 ? f.chunk0_darts : 0;
    }
    unsigned int flags = hs.err_flags;
    for (unsigned int dead : hs.dead_count) v.contours_traced += dead;
    uint64_t need_points = 0; uint32_t need_contours = 0;
    bool jump_short = false, resolve_needed = false, entry_overflow = false;
    for (size_t ci = 0; ci < f.n_chunks; ci++) {
        const DeviceCounters& c = hc[ci];
        flags |= c.err_flags;
        resolve_needed |= c.resolve_needed != 0;
        entry_overflow |= c.entry_overflow != 0;
        need_points = max_of<uint64_t>(need_points, c.points);
        need_contours = max_of(need_contours, c.contours);
        v.contours_traced += c.traced;
        v.contours_materialised += c.contours;
        for (int r = 0; r < 32; r++) if (c.jump_changed[r]) v.jump_rounds = max_of<uint32_t>(v.jump_rounds, r + 1);
        uint32_t it = c.resolve_needed ? 1 : 0;  // 0: k_resolve_fast confirmed the natural starts; pass k+1 ran iff pass k moved something
        for (int r = 0; r < kResolveItersMax - 1; r++) if (c.resolve_changed[r]) it = r + 2;
        v.resolve_iterations = max_of(v.resolve_iterations, it);
        if (f.rounds_max > 0 && f.rounds_max < 32 && c.jump_changed[f.rounds_max - 1] != 0) jump_short = true;
    }
    if (entry_overflow) { h.entry_global_ttl = 64; h.jump_rounds_hint = max_of(h.jump_rounds_hint, 12); return rerun(); }   // a frame's entry list outgrew LDS: re-run with the global rounds
    if (h.entry_global_ttl > 0) h.entry_global_ttl--;
    if (jump_short && h.jump_rounds_hint < 32) { h.jump_rounds_hint = 32; return rerun(); }   // re-run with all rounds
    if (resolve_needed) {
        const bool ran = h.resolve_full_ttl > 0;
        h.resolve_full_ttl = 64;        // keep the full passes in the launch sequence for the next batches
        if (!ran) return rerun();       // they were not launched this time
    } else if (h.resolve_full_ttl > 0) h.resolve_full_ttl--;
    if ((flags & kErrResolve) && h.resolve_iters_hint < kResolveItersMax) { h.resolve_iters_hint = kResolveItersMax; return rerun(); }
    h.jump_rounds_hint = max_of(4, min_of(32, (int)v.jump_rounds + 2));   // follow the workload, both ways (one round of slack: a short launch costs a re-run)
    if (flags & (kErrPointPool | kErrContourTable)) {   // grow and re-run
        if (need_points > h.max_points) h.max_points = min_of<uint64_t>(kHardMaxPoints, max_of(need_points, h.max_points * 2));
        if (need_contours > h.max_contours) h.max_contours = max_of(need_contours, h.max_contours * 2);
        return rerun();
    }
    if (flags & kErrBrokenEvent) return fail(A3_ERR_INTERNAL, "contour graph: a start event lies on an open chain");
    if (flags & kErrScatter) return fail(A3_ERR_INTERNAL, "contour points: a border slot, rank or point index out of range");
    if (flags & kErrResolve) return fail(A3_ERR_INTERNAL, "contour start resolution did not converge");
    if (flags & kErrCandTable) {   // a frame has more quad candidates than its table: twice the table and again
        // straight to the table that holds the fullest frame: 2048, 4096, 6144 (the last that k_frame_candidates works in LDS),
        // 12 288, 24 576, 49 152, 65 536
        const uint32_t need = max_of(hs.cand_most, h.max_cand + 1u);
        if (need > kMaxCandLimit) return fail(A3_ERR_LIMIT, "a frame holds more than 65536 quad candidates (A3_MAX_CANDIDATES_PER_FRAME)");
        uint32_t next = h.max_cand;
        while (next < need) next = next < f.lds_slots ? min_of(f.lds_slots, next * 2) : min_of(kMaxCandLimit, next * 2);
        if ((uint64_t)f.n * next > 0xFFFFFFFFull) return fail(A3_ERR_LIMIT, "frames x candidate slots per frame exceeds 2^32: fewer frames per call");
        v.action = Verdict::GrowCands; v.next_cand = next; v.slot_bytes = f.slot_bytes + (next > f.lds_slots ? 4 : 0);
        return v;
    }
    if (flags & kErrMarkerCap) return fail(A3_ERR_CAPACITY, "out_cap is smaller than the number of markers found");
    v.total = hs.marker_total;
    if (v.total > f.out_cap) return fail(A3_ERR_CAPACITY, "out_cap is smaller than the number of markers found");
    v.n_work = hs.work_count; v.n_pre = hs.cand_pre_total;
    if (f.n_chunks) { v.tap_contours = hc[0].contours; v.tap_points = hc[0].points; }
    return v;
}

// ---- the plan -------------------------------------------------------------------------------------------------------------------------
// A batch shaped like the previous one, which fitted one chunk, is planned on the device (no read-back of the dart counts before
// the contour stage).  -> the dart capacity such a batch is launched with; 0: this batch must be planned by the host.
inline uint64_t device_plan_capacity(const BatchHints& h, uint64_t max_darts, uint32_t n, uint32_t W, uint32_t H) {
    if (!(h.plan_valid && !h.force_host_plan && h.plan_n == n && h.plan_W == W && h.plan_H == H && n <= kMaxChunkFrames)) return 0;
    const uint64_t cap_d = h.plan_darts + h.plan_darts / 4 + 65536;
    return cap_d > max_darts ? 0 : cap_d;
}
// One allocation for everything small: [frame_cursor | cand_count | (device plan: frame_darts) | HEAD | markers], HEAD =
// [BatchScratch | counters | per_frame]: what the host reads back ahead of the markers.
struct ZeroLayout { size_t ctr_bytes, head_bytes, head_off, total; };
inline ZeroLayout zero_layout(size_t n_chunks, uint32_t chunk_frames, uint32_t n, uint32_t marker_cap) {
    ZeroLayout z;
    z.ctr_bytes = sizeof(DeviceCounters) * n_chunks;
    z.head_bytes = (sizeof(BatchScratch) + z.ctr_bytes + (size_t)n * 4 + 7) & ~(size_t)7;
    const size_t fd_off = ((size_t)chunk_frames * 4 + (size_t)n * 4 + 15) & ~(size_t)15;
    z.head_off = (fd_off + 255) & ~(size_t)255;
    z.total = z.head_off + z.head_bytes + (size_t)marker_cap * sizeof(a3_marker);
    return z;
}
inline uint32_t marker_cap_of(uint32_t max_cand, uint32_t n, size_t out_cap) {
    return (uint32_t)min_of<size_t>(max_of<size_t>(out_cap, 1), (size_t)n * max_cand);
}
// markers read back speculatively with the head: a quarter more than the last batch had
inline uint32_t marker_guess_of(uint32_t last_marker_total, uint32_t marker_cap) {
    return (uint32_t)min_of<size_t>(marker_cap, (size_t)last_marker_total + last_marker_total / 4 + 64);
}
// a single-chunk batch is followed by device-planned ones sized darts * 1.25 + 64k: the pool is allocated for that at once
inline uint64_t pool_darts_of(uint64_t max_darts, uint64_t max_chunk_darts, size_t n_chunks) {
    uint64_t pool_darts = max_of<uint64_t>(max_chunk_darts, 1);
    if (n_chunks == 1) {
        pool_darts = min_of<uint64_t>(max_of<uint64_t>(max_darts, pool_darts), pool_darts + pool_darts / 2 + 131072);
        // in steps of an eighth of an octave: a stream of batches whose graphs differ by a percent or two (consecutive batches of one
        // camera) must not re-allocate the pool -- a dozen hipFree + hipMalloc in the middle of a batch, ~2 ms -- at every new maximum
        uint64_t step = 1ull << 17;
        while (step * 16 < pool_darts) step <<= 1;
        pool_darts = min_of<uint64_t>((pool_darts + step - 1) / step * step, max_of<uint64_t>(kHardMaxDarts, pool_darts));
    }
    return pool_darts;
}

struct Chunk { uint32_t first, count; uint64_t darts; uint32_t max_frame_darts; };
struct ChunkSplit {
    bool refused;        // a frame above kHardMaxDarts: nothing else is filled in
    uint64_t max_darts;  // the caller's, grown to the largest frame: one frame must fit
    uint64_t total_darts, max_chunk_darts; uint32_t n_chunks, max_chunk_frames;
};
// Frames fd[0..n) in order into chunks of at most max_darts darts and max_frames frames each; chunks: room for n.
inline ChunkSplit split_chunks(const uint64_t* fd, uint32_t n, uint64_t max_darts, uint32_t max_frames, Chunk* chunks) {
    ChunkSplit s{false, max_darts, 0, 0, 0, 0};
    uint64_t biggest = 0;
    for (uint32_t f = 0; f < n; f++) { biggest = max_of(biggest, fd[f]); s.total_darts += fd[f]; }
    if (biggest > kHardMaxDarts) { s.refused = true; return s; }
    s.max_darts = max_of(max_darts, biggest);
    Chunk c{0, 0, 0, 0};
    const auto close = [&]() {
        chunks[s.n_chunks++] = c;
        s.max_chunk_frames = max_of(s.max_chunk_frames, c.count); s.max_chunk_darts = max_of(s.max_chunk_darts, c.darts);
    };
    for (uint32_t f = 0; f < n; f++) {
        if (c.count && (c.darts + fd[f] > s.max_darts || c.count >= max_frames)) { close(); c = Chunk{f, 0, 0, 0}; }
        c.count++; c.darts += fd[f]; c.max_frame_darts = (uint32_t)max_of<uint64_t>(c.max_frame_darts, fd[f]);
    }
    if (c.count) close();
    return s;
}
// frame bases of chunk c: bases[0..stride), stride = the batch's max_chunk_frames + 1 (past the chunk's frames: its dart total)
inline void chunk_frame_bases(const uint64_t* fd, const Chunk& c, uint32_t stride, uint32_t* bases) {
    uint32_t acc = 0;
    for (uint32_t i = 0; i < stride; i++) {
        bases[i] = acc;
        if (i < c.count) acc += (uint32_t)fd[c.first + i];
    }
}
// Global doubling rounds of a chunk whose largest frame has max_frame_darts darts: enough for a cycle through all of them plus the
// round that observes "nothing moved", at most the hint; debug_cap (a3_debug_set_jump_rounds, 0: none): too few on purpose, except
// in the re-run with all rounds that a short launch asks for.
inline int chunk_rounds(uint32_t max_frame_darts, int jump_rounds_hint, int debug_cap) {
    int rounds = 1;
    while ((1ull << rounds) < (uint64_t)max_frame_darts && rounds < 31) rounds++;
    rounds = min_of(rounds + 1, jump_rounds_hint);
    return debug_cap > 0 && jump_rounds_hint < 32 ? min_of(rounds, debug_cap) : rounds;
}

}  // namespace a3
