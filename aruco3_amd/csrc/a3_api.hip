// a3_api.hip -- host side of libaruco3_hip.so: context, device pools, the batch pipeline and the C ABI
// declared in include/aruco3_hip.h.  No CPU fallback of any stage lives here: without a HIP device
// a3_create fails with A3_ERR_NO_DEVICE.
#include <algorithm>
#include <atomic>
#include <cmath>
#include <chrono>
#include <cstddef>
#include <cstdio>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "a3_board3d_check.h"
#include "a3_common.h"
#include "a3_format.h"
#include "a3_internal.h"
#include "a3_launch.h"
#include "a3_readback.h"
#include "a3_rectify_check.h"
#include "a3_reduce_check.h"
#include "a3_solve_check.h"
#include "a3_windows_check.h"

using namespace a3;

namespace {

// message of the last failed context-less call (a3_create, a3_calculate_tau) ON THIS THREAD: contexts for different GPUs may be
// created concurrently from different threads
thread_local std::string g_create_error;

// (The pool and table limits, the hints a context carries between batches and the device's verdict on a batch: a3_batch_head.h.)
// debug taps: warped patches kept per batch (one per candidate that reaches the decode stage).  The tap holds a patch for every
// candidate the batch can have (frames x kMaxCand) up to kPatchCapMax patches (2.4 GB at 49 x 49); a binding that populates
// Detection.homographies for more than 1024 frames per call splits the call (integration/aruco3_hip.rs does).
constexpr uint32_t kPatchCapMin = 32768, kPatchCapMax = 1u << 20;

// grow-only device buffer
struct DevBuf {
    void* p = nullptr;
    size_t cap = 0;
    hipError_t ensure(size_t bytes) {
        if (bytes <= cap) return hipSuccess;
        if (p) { hipError_t e = hipFree(p); p = nullptr; cap = 0; if (e != hipSuccess) return e; }
        hipError_t e = hipMalloc(&p, bytes);
        if (e == hipSuccess) cap = bytes;
        return e;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; cap = 0; }
    template <typename T> T* as() const { return reinterpret_cast<T*>(p); }
};

// Consecutive 256-byte-aligned segments of one DevBuf, for the solver entry points: each segment is declared once (add: n elements
// of T, or n records of `elem` bytes seen as T) and then addressed by the handle that add returned, so no offset sum is written twice.
// The copies and the memset go to the layout's stream.
template <typename T> struct Seg { size_t off, n; };
struct Layout {
    DevBuf& buf;
    hipStream_t stream;
    size_t end = 0;
    template <typename T> Seg<T> add(size_t n, size_t elem = sizeof(T)) {
        const size_t off = (end + 255) & ~(size_t)255;
        end = off + n * elem;
        return {off, n};
    }
    hipError_t ensure() { return buf.ensure((end + 255) & ~(size_t)255); }   // (the last segment padded like the others)
    template <typename T> T* at(Seg<T> s) const { return reinterpret_cast<T*>(buf.as<uint8_t>() + s.off); }
    template <typename T> hipError_t upload(Seg<T> s, const T* src, size_t n) const {   // n: what the caller has, may be 0
        return n ? hipMemcpyAsync(at(s), src, n * sizeof(T), hipMemcpyHostToDevice, stream) : hipSuccess;
    }
    template <typename T> hipError_t download(Seg<T> s, T* dst) const {   // dst: nullable
        return dst ? hipMemcpyAsync(dst, at(s), s.n * sizeof(T), hipMemcpyDeviceToHost, stream) : hipSuccess;
    }
    template <typename T> hipError_t zero_from(Seg<T> s) const { return hipMemsetAsync(at(s), 0, end - s.off, stream); }   // s and all behind it
};

// One batch: the call and every setting it runs with, captured once when it starts (begin_batch) -- a setter called while the batch
// is in flight applies to the next one -- and what its enqueue decided.  enqueue_front, enqueue_chain, enqueue_back (also when it is
// deferred), finish_batch and the synchronous re-run read this record, never the context's live settings.
struct Batch {
    // the call (pixels: on the device)
    const uint8_t* pixels = nullptr; int fmt = 0;
    uint32_t W = 0, H = 0, n = 0;
    size_t row_stride = 0, frame_stride = 0, out_cap = 0;
    // settings
    bool want_pose = false, pose_has_intr = false;   // a3_detect_batch_pose*: poses of every marker, solved on the device
    float pose_size_mm = 0.0f;
    a3_intrinsics pose_intr{};
    a3_refine_config refine{};   // corner refinement (method NONE: none)
    bool refined = false;        // ... is on: 8 floats per marker
    bool board = false;          // a pose batch with a board set: k_board_pose runs behind k_pose
    a3_distortion dist{};        // lens distortion (model NONE: none)
    bool undist = false;         // ... is on, on a pose batch: 8 corner floats + 4 residuals per marker
    bool charuco = false;        // ChArUco set: the corner stage runs behind the refinement (and k_charuco_pose behind k_board_pose)
    a3_charuco_config charuco_cfg{};
    uint32_t charuco_nc = 0, charuco_guess = 0;   // chessboard corners; records in the speculative read-back
    // a3_set_board_recovery in force: the marker gather writes to a side list and k_recover_frames / k_recover_merge leave the merged
    // list where every later stage and the read-back expect the batch's markers
    bool recover = false;
    a3_recover_config recover_cfg{};
    uint32_t recover_slots = 0, recover_cap = 0;   // board markers; records a frame's recovery can hold (ensure_back_buffers)
    // a3_set_marker_polarity was A3_POLARITY_BOTH when the batch began: k_decode reads an all-lit border complemented, k_marker_flags
    // leaves a flag word per marker for the edge fit and for a3_get_marker_flags
    bool flags = false;
    uint32_t sides = 0;          // the side results all of this turns on, one bit per SideKind (a3_readback.h)
    bool has(int kind) const { return (sides >> kind & 1u) != 0; }
    // The call's frames as staged on the device (frames, of frames_W x frames_H pixels).  With a3_set_rectification or a3_set_reduction in
    // force (they exclude each other) they are the SOURCE of a derived grey plane, and pixels, fmt, W, H, row_stride and frame_stride above
    // describe that plane (A3_FMT_L8, tightly packed), written ahead of the threshold kernel:
    //   Rectified: the frames seen through rect_r, of rect_r.dst's size, by k_rectify's grey form; everything behind that launch sees nothing else
    //   Reduced: frames_W / reduce_f x frames_H / reduce_f, by k_reduce_frames; the front half (threshold ... decode, recovery) sees nothing
    //     else, and the back half (refinement, ChArUco, poses) works on `frames` from the corners k_scale_markers mapped back up
    enum class Plane { None, Rectified, Reduced } plane = Plane::None;
    PixelSrc frames{};
    uint32_t frames_W = 0, frames_H = 0;
    a3_rectify rect_r{};
    uint32_t reduce_f = 0;
    // a3_set_threshold_windows: the radius of the single-window path (the context's threshold_window, or the one radius set), or with
    // K >= 2 the windows of a batch whose front half and contour stage run on planes = n * K planes (plane (k, f) at k * n + f,
    // plane_cand candidate slots each) and whose candidates k_merge_candidates merges into n frames' lists of max_cand slots
    uint32_t K = 1, win[A3_MAX_THRESHOLD_WINDOWS] = {}, radius = 0, planes = 0, plane_cand = 0;
    bool taps = false;           // debug taps: grey plane, patches, contours and the per-frame candidate counts are kept
    bool sample_frames = false;  // a3_debug_sample_frames: a tapped batch still samples the caller's frames wherever an untapped one would
    int profiling = 0, profile_every = 1;   // a3_set_profiling in force
    // enqueue_front
    int prof = 0;                // the profiling level of this enqueue (the sampled threshold-only mode times one batch in profile_every)
    bool need_grey = false;      // the threshold kernel writes the grey plane (taps, or a radius above 31)
    bool grey_src = false;       // ... and the decode stage samples it (always, unless a3_debug_sample_frames keeps a tapped batch on the frames)
    uint32_t max_cand = 0, patch_cap = 0, marker_cap = 0, guess = 0;
    // enqueue_chain
    bool active = false, device_plan = false;
    size_t n_chunks = 0;
    Readback rb;                 // where the results lie in the pinned staging buffer (ensure_back_buffers)
    uint64_t chunk0_darts = 0;
    int rounds_max = 0;
    PixelSrc src{};              // what the decode stage samples: the caller's frames or the grey plane
};

}  // namespace

struct a3_ctx {
    int device = 0;
    hipStream_t own_stream = nullptr, stream = nullptr;
    // host frames (A3_MEM_HOST) are copied on the device's copy stream (shared by the contexts of a device, see DeviceStreams), the
    // compute stream waits for the copy through ev_in: with two contexts in flight (submit / collect) the H2D of batch i+1 runs
    // under the kernels of batch i
    hipEvent_t ev_in = nullptr;
    // Deferred decode (submit / collect with more than one context, see enqueue_chain): the decode stage of a submitted batch
    // runs on the device's decode stream, released from inside the launch sequence of the NEXT submitted batch, so that it shares
    // the GPU with that batch's contour stage (both are latency-bound and leave the chip mostly idle) instead of standing in line.
    hipEvent_t ev_contours = nullptr, ev_k1 = nullptr, ev_k1_done = nullptr, ev_gate = nullptr;
    // Bursts (a3_order_after): a context that declared gates since its last submit is a member of a burst that is not the last
    // one: its submit enqueues the threshold kernel only and HOLDS the rest (contour stage ... read-back) until the burst's last
    // member -- the first submit without gates on the device -- has enqueued its threshold kernel; the held chains are then
    // enqueued behind that kernel.  The threshold kernels of a burst so run back to back with nothing in between.
    bool gates_declared = false;     // a3_order_after was called since the last submit
    bool rest_held = false;          // guarded by g_defer_mu: the chain of the submitted batch has not been enqueued yet
    int held_rc = 0;                 // guarded by g_defer_mu: what enqueueing the held chain returned, whoever did it
    bool back_deferred = false;      // guarded by g_defer_mu
    int back_rc = 0;                 // a failed launch of the deferred half, whoever enqueued it (guarded by g_defer_mu): collect reports it
    bool allow_defer = false;        // set by the submit entry points for the batch being enqueued
    int batch_mode = 0;              // where the decode stage of the batch being submitted is released (batch_mode_of, fixed at submit)
    std::atomic<uint32_t> stepping{0};   // A3_STEP_* of the batch in flight / last finished (a3_stats.stepping); another thread's submit may release this context's held chain
    uint32_t released_others = 0;    // held chains of other contexts this batch's submit released (the burst's last member)
    uint32_t reruns = 0;             // synchronous re-runs the device asked for while the last call's batch was produced (pool growth, more passes, host plan)
    a3_config cfg{};
    uint8_t num_bits = 0, tau = 0;
    uint32_t n_codes = 0, mark_size = 0;
    std::string err;

    uint64_t max_darts = kMaxDartsDefault;
    BatchHints hints;   // launch-count hints, the device plan, the pools and tables that grow: what batch_verdict moves (a3_batch_head.h)
    uint32_t dbg_nd = 0, dbg_frames = 0, dbg_chunks = 0;   // a3_debug_kernel_time: shape of the last batch's contour graph
    PixelSrc dbg_src{};
    // a3_debug_inject_candidates (tests only): quads that replace frame 0's candidate list of the next batch, between the contour
    // stage and k_frame_candidates (quirk Q4: a degenerate quad cannot come out of a convex hull)
    std::vector<CandRec> inject;
    bool inject_armed = false;
    uint32_t inject_count = 0;
    Batch batch;                    // the batch in flight (or the last one)
    bool pending_trivial = false;   // a submitted batch with no frames / empty images
    bool busy() const { return batch.active || pending_trivial; }   // a submitted batch has not been collected
    bool debug_taps = false;   // a3_set_debug_taps: the setting the next batch captures
    bool debug_sample_frames = false;   // a3_debug_sample_frames (tests only): likewise
    uint32_t patch_cap = 0;    // patches the tap of the last tapped batch could hold
    bool grey_valid = false;   // the last batch wrote the grey plane
    // a3_download_contours: the last batch ran with debug taps in one chunk, so its contour table and point pool are whole
    bool contours_valid = false;
    uint32_t tap_contours = 0; uint64_t tap_points = 0;
    // a3_pack_detections: the marker list of the last finished batch is still on the device
    bool markers_valid = false;
    uint32_t last_n = 0, last_max_per_frame = 0;
    // a3_set_profiling, the setting the next batch captures: 0 off, 1 threshold stage only, 2 every stage (an event record between
    // kernels costs ~6 us of device time)
    int profiling = 0;
    int profile_every = 1;   // threshold-only mode: time every k-th batch (A3_PROFILE_THRESHOLD_SAMPLED: 4)
    uint32_t batch_seq = 0;
    hipEvent_t ev[6] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
    double prof_ms[A3_STAGE_COUNT] = {0, 0, 0};
    uint64_t prof_n[A3_STAGE_COUNT] = {0, 0, 0};
    a3_stats stats{};

    // last batch geometry (for the debug downloads): frames = the planes of the front half and the contour stage (the batch's frames
    // times its threshold windows), frames_merged = the batch's frames, cand_stride = slots per frame of the tables behind the candidates,
    // pre_count = the per-frame lengths of the lists before the discard on the device
    uint32_t W = 0, H = 0, frames = 0, frames_merged = 0, cand_stride = 0;
    const uint32_t* pre_count = nullptr;
    // a3_set_threshold_windows: the setting later batches capture (0 windows: off)
    uint32_t n_windows = 0, windows[A3_MAX_THRESHOLD_WINDOWS] = {};

    DevBuf dict, in, grey, bin, frame_darts, frame_darts_dev, frame_base, pix_base, tile_darts;
    DevBuf d_xy, d_succ, fin, t_cur, t_next;
    DevBuf leader_list, leader_keep, entry_list, es_a, es_b;
    DevBuf contours, cyc_start_off, points;
    DevBuf cands, pre_xy, fin_xy, fin_count, work, outs, proj, patches, cand_big;
    DevBuf merged_count;   // several threshold windows: the per-frame lengths of the concatenated candidate lists (k_merge_candidates)
    // one allocation zeroed by one memset per batch, its head read back with one copy (zero_layout, a3_batch_head.h)
    DevBuf zero_blk;
    a3_marker* markers_ptr = nullptr;                // the compacted marker list, right behind the read-back head in the zero block
    unsigned long long* frame_darts_ptr = nullptr;   // frame_darts_dev (device plan: kept zero by its reader) or the frame_darts buffer (host plan)
    BatchScratch* head = nullptr; DeviceCounters* counters = nullptr; uint32_t* per_frame = nullptr; uint32_t* frame_cursor = nullptr; uint32_t* cand_count = nullptr;
    uint32_t last_marker_total = 0;   // sizes the speculative marker read-back of the next batch
    DevBuf tmp_a, tmp_b, tmp_c, tmp_d;
    DevBuf hsum;                // row sums of the grey plane (u16): the separable threshold path only (radii 32..128)
    DevBuf wtab;                // triangle-resize weights of a full patch (sample -> mark_size), written once at a3_create
    DevBuf pose_buf;            // a3_detect_batch_pose: both poses of every marker of the last batch (kept for a3_pack_detections)
    // The side results (kSides, a3_readback.h), by kind: where the batch in flight has them on the device (ensure_back_buffers), the copy
    // finish_batch kept for the getters, and whether the last collected batch produced the kind.  (Poses have no kept copy: their flag
    // says that pose_buf holds the last batch's, for a3_pack_detections.)
    // (The marker flags are a per-marker result outside the table -- a3_readback.h says why -- with members of their own below
    // (flags_buf, flags_h, flags_valid): whoever changes how the per-marker kinds are sized, staged, re-fetched, kept or cleared changes
    // the `b.flags` lines beside those loops in ensure_back_buffers, enqueue_back, finish_batch, begin_batch and finish_trivial too.)
    void* side_dev[kSideKinds] = {};
    std::vector<uint8_t> side_h[kSideKinds];
    bool side_valid[kSideKinds] = {};
    // a3_set_corner_refinement: the setting later batches capture; refine_prm holds the kernel parameters (weight tables) built for
    // refine_prm_cfg, rebuilt when a batch brings another setting
    a3_refine_config refine{};
    a3_refine_config refine_prm_cfg{};
    std::vector<float> refine_prm;
    DevBuf refined_buf;          // refined corners of the last batch on the device (8 floats per marker, marker order)
    // a3_set_marker_polarity: the setting later batches capture; the flag words of the batch in flight on the device (marker order), the
    // copy finish_batch kept for a3_get_marker_flags, and whether the last collected batch ran in mode A3_POLARITY_BOTH
    int polarity = A3_POLARITY_DARK;
    DevBuf flags_buf;
    std::vector<uint32_t> flags_h;
    bool flags_valid = false;
    // a3_set_board: the board later batches capture (board_ids; board_slots: one BoardSlot record per marker) and its device tables
    // (id -> slot, slot records), brought up to date at the next submit when board_version moved -- never while a batch of this
    // context is in flight, so a batch keeps the board it was submitted with
    // a3_set_board3d: the same, with Board3Slot records; board_kind says which records board_slots holds (kBoardSlotsPlanar /
    // kBoardSlots3D), board_kind_up which the device tables hold since the last upload
    std::vector<uint32_t> board_ids;
    std::vector<uint8_t> board_slots;
    uint32_t board_kind = kBoardSlotsPlanar, board_kind_up = kBoardSlotsPlanar;
    uint64_t board_version = 0, board_dev_version = 0;
    std::vector<uint16_t> board_slot_up;   // (the sources of the last upload, untouched until the next one)
    std::vector<uint8_t> board_slots_up;
    DevBuf board_slot_of, board_slot_rec, board_buf;   // id -> slot (n_codes x u16), slot records, board poses of the last batch (per frame)
    // a3_set_board_recovery: the setting later batches capture; the board's ids in slot order on the device (brought up to date with the
    // board's tables); the side list the marker gather writes ([total, padded to 16 bytes | per-frame counts | recovered per frame] in
    // recover_counts, the markers in recover_det), the per-frame records of k_recover_frames
    a3_recover_config recover{};
    uint64_t recover_ids_version = 0;
    std::vector<uint32_t> recover_ids_up;
    DevBuf recover_ids, recover_counts, recover_det, recover_tmp;
    // a3_set_distortion: the setting later pose batches capture; undist_buf holds the undistorted corners of the last batch on the
    // device: [marker_cap x 8 floats | marker_cap x 4 residuals]
    a3_distortion dist{};
    DevBuf undist_buf;
    // a3_set_charuco: the chessboard later batches capture (charuco_tab_h: [2 floats per corner | 4 adjacent ids per corner]) and its
    // device copy, brought up to date at the next submit as the board's; charuco_prm: the refinement parameters built for charuco_prm_cfg
    a3_charuco_config charuco_cfg{};
    std::vector<uint32_t> charuco_tab_h;
    uint32_t charuco_nc = 0;
    uint64_t charuco_version = 0, charuco_dev_version = 0;
    std::vector<uint32_t> charuco_tab_up;
    a3_charuco_config charuco_prm_cfg{};
    std::vector<float> charuco_prm;
    // the last batch on the device: per-frame slots [n x nc records | n + 1 counts], the records in (frame, id) order, their undistorted
    // pixels (pose batches with distortion) and the poses
    DevBuf charuco_tab, charuco_tmp, charuco_buf, charuco_und, charuco_pose_buf;
    std::vector<a3_charuco_corner> h_charuco;   // the last collected batch's corner records, and whether it ran with ChArUco
    bool charuco_valid = false;
    // The solver entry points (a3_calibrate_cameras ... a3_build_marker_maps): the call's staged input, the kernel's scratch, the
    // maps' reduced systems (two n x n per map: sized very differently from the rest) and the results.  One set serves them all: each
    // of these calls refuses to start while a batch is in flight and waits for its own work before it returns.
    DevBuf solve_in, solve_scratch, solve_big, solve_out;
    // a3_rectify_frames: host-side source frames and host-side output staged on the device
    DevBuf rect_in, rect_out;
    // a3_set_rectification and a3_set_reduction (factor 0: off): the settings later batches capture, one of them at the most, and the
    // derived grey plane of the batch in flight (Batch::plane; n x w x h bytes, tightly packed): written ahead of the threshold kernel,
    // sampled by the decode stage (rectified: also by the refinement and ChArUco) until collect.  a3_reduce_frames stages host-side
    // frames and output in rect_in / rect_out as a3_rectify_frames does (both calls are synchronous)
    a3_rectify rect{};
    bool rect_on = false;
    a3_reduction reduction{};
    DevBuf plane;
    uint32_t last_charuco_total = 0;   // sizes the speculative record read-back of the next batch
    void* pinned = nullptr;
    size_t pinned_cap = 0;
    // debug taps: per-frame candidate counts of the last batch (before / after discard_too_near), read back with the results so
    // that a3_candidate_count and the a3_download_* calls that start with it need no device round trip of their own
    void* pinned_counts = nullptr;
    size_t pinned_counts_cap = 0;
    std::vector<uint32_t> h_cand_pre, h_cand_fin;
    bool counts_valid = false;
};

namespace {

int fail(a3_ctx* c, int code, const char* what, hipError_t e = hipSuccess) {
    char buf[512];
    if (e != hipSuccess) snprintf(buf, sizeof buf, "%s: %s", what, hipGetErrorString(e));
    else snprintf(buf, sizeof buf, "%s", what);
    if (c) c->err = buf; else g_create_error = buf;
    return code;
}

#define A3_HIP(call)                                                        \
    do {                                                                    \
        hipError_t e_ = (call);                                             \
        if (e_ != hipSuccess) return fail(ctx, A3_ERR_HIP, #call, e_);      \
    } while (0)

// Waiting for a batch that takes about a millisecond: a blocking hipStreamSynchronize wakes the host tens of microseconds
// late, so poll first (with the CPU's spin-wait hint between polls, which leaves the core's other hardware thread its share)
// and block once the work has proved long: after 2 ms the wake-up delay no longer matters.
inline void spin_pause() {
#if defined(__x86_64__) || defined(__i386__)
    __builtin_ia32_pause();
#endif
}
constexpr auto kSpinBudget = std::chrono::milliseconds(2);

hipError_t wait_stream(hipStream_t st) {
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipStreamQuery(st);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > kSpinBudget) return hipStreamSynchronize(st);
        spin_pause();
    }
}

hipError_t wait_event(hipEvent_t ev, hipStream_t st) {
    (void)hipStreamQuery(st);   // makes the runtime hand everything queued so far to the GPU; the event poll alone may not
    const auto t0 = std::chrono::steady_clock::now();
    for (;;) {
        const hipError_t e = hipEventQuery(ev);
        if (e != hipErrorNotReady) return e;
        if (std::chrono::steady_clock::now() - t0 > kSpinBudget) return hipEventSynchronize(ev);
        spin_pause();
    }
}

int ensure_pinned(a3_ctx* ctx, size_t bytes) {
    if (bytes <= ctx->pinned_cap) return A3_OK;
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    ctx->pinned = nullptr; ctx->pinned_cap = 0;
    A3_HIP(hipHostMalloc(&ctx->pinned, bytes, hipHostMallocDefault));
    ctx->pinned_cap = bytes;
    return A3_OK;
}

uint32_t mark_size_of(uint8_t num_bits) {  // src/dictionaries.rs:154-156
    return (uint32_t)((uint8_t)std::ceil(std::sqrt((float)num_bits)) + 2);
}

int ensure_dart_pool(a3_ctx* ctx, uint64_t darts) {
    A3_HIP(ctx->d_xy.ensure(darts * 8));   // dart records (dart_rec)
    A3_HIP(ctx->d_succ.ensure(darts * 4));
    A3_HIP(ctx->fin.ensure(darts * fin_state_bytes()));   // the 8-byte states (leader, hops | flags, or pending) of k_local_contract / k_jump_finalize
    A3_HIP(ctx->t_cur.ensure(darts * 8));
    A3_HIP(ctx->t_next.ensure(darts * 8));
    A3_HIP(ctx->leader_list.ensure(leader_list_bytes((uint32_t)darts)));   // leaders of cycles with a start event, 16 shards
    A3_HIP(ctx->leader_keep.ensure(leader_list_bytes((uint32_t)darts)));   // k_cycle_select: pass-1 verdict per leader slot
    const size_t eslots = entry_slots((uint32_t)darts);   // sharded slot space: darts + at most 16 tiles of padding
    A3_HIP(ctx->entry_list.ensure(eslots * 4));
    // entries are darts whose predecessor lies in another 2048-dart tile; the bound darts is never reached in practice,
    // but an adversarial image can come close, so size for it
    A3_HIP(ctx->es_a.ensure(eslots * entry_state_bytes()));
    A3_HIP(ctx->es_b.ensure(eslots * entry_state_bytes()));
    return A3_OK;
}

// ---- streams ----
// A process has few hardware queues (the runtime multiplexes its streams onto four by default), and two streams that land on one
// queue run in order whatever their events say: a decode stage "released beside the next batch" then simply stands in that
// batch's line -- measured: a second set of contexts, each with three streams of its own, lost 10 % where the first set gained
// 7 %.  So streams are few: ONE decode stream and ONE copy stream per device, shared by all contexts (their work never wants to
// overlap with itself), created on first use; a context's own stream exists only if the caller never passed one (a3_set_stream).
struct DeviceStreams { hipStream_t decode = nullptr, copy = nullptr; };
std::mutex g_streams_mu;
DeviceStreams g_dev_streams[64];
bool g_hold_rests = true;        // a3_debug_set_hold: bursts hold their chains back (see submit_common); 0 for A/B
std::atomic<int> g_jump_rounds_cap{0};   // a3_debug_set_jump_rounds: at most this many global doubling rounds (0: no cap)
enum { kStreamCopy = 0, kStreamDecode = 1 };

hipError_t create_stream(hipStream_t* st) { return hipStreamCreateWithPriority(st, hipStreamNonBlocking, 0); }

hipError_t device_stream(int device, int kind, hipStream_t* out) {
    std::lock_guard<std::mutex> lk(g_streams_mu);
    DeviceStreams& ds = g_dev_streams[device & 63];
    hipStream_t& st = kind == kStreamDecode ? ds.decode : ds.copy;
    if (!st) {
        const hipError_t e = create_stream(&st);
        if (e != hipSuccess) { st = nullptr; return e; }
    }
    *out = st;
    return hipSuccess;
}

// the stream a context enqueues on: the caller's (a3_set_stream) or, created on first need, its own
int need_stream(a3_ctx* ctx);

// ---- deferred decode: contexts whose submitted batch has its contour stage enqueued and its decode stage not yet ----
std::mutex g_defer_mu;
std::vector<a3_ctx*> g_deferred;
// 0: no deferral; 1: release a waiting decode stage behind the next batch's threshold kernel; 2 (default): behind the next batch's
// k_local_contract -- the kernels that follow it (entry resolution, finalize, scatter, quads) are latency-bound like the decode
// stage and share the chip with it, whereas the dart kernels before it are bound by VALU and LDS throughput and only get slower
// in company.  Measured in one process (round 3, docs/HISTORY.md; BASELINE config 2, two contexts): 0.820 / 0.769 / 0.762 ms per step
// for modes 0 / 1 / 2 (0.794 / 0.744 / 0.741 on another box); smaller decode grids (2048 ... 512 workgroups) only lose.  Deferring the second half of the contour stage as well (entry resolution ... quads, released with the
// decode stage behind the next threshold kernel) was built and measured: 0.777 with two contexts, 0.821 with three -- dropped.
// (a3_debug_set_overlap in a3_internal.h switches modes for the A/B measurements of tools/.)
// Since round 5 the mode is decided PER BATCH, by the library, from what the caller did through the public header -- no switch
// selects the stepping any more (g_overlap_force == -1, the default):
//   * a context whose stream no other context of the device uses never defers (mode 0): consecutive batches on such contexts
//     overlap by themselves, and a context that declared burst gates (a3_order_after) holds its chain back (submit_common);
//   * contexts that SHARE one stream (a3_set_stream with the same caller stream) run in order there, whatever they do: the
//     deferred decode stage -- mode 2 -- is the only overlap there is, so they get it.
// a3_debug_set_overlap(0 | 1 | 2) forces one mode on every batch of the process for the A/B measurements of tools/; forced modes
// 1 and 2 also switch the burst hold off, which is what the library did by default until round 4.
std::atomic<int> g_overlap_force{-1};
// the mode of the batch `ctx` is about to submit
std::vector<a3_ctx*> g_contexts;   // every live context of the process (guarded by g_streams_mu)
int batch_mode_of(const a3_ctx* ctx) {
    const int f = g_overlap_force.load(std::memory_order_relaxed);
    if (f >= 0) return f;
    if (!ctx->stream || ctx->stream == ctx->own_stream) return 0;
    std::lock_guard<std::mutex> lk(g_streams_mu);
    for (const a3_ctx* o : g_contexts)
        if (o != ctx && o->device == ctx->device && o->stream == ctx->stream) return 2;
    return 0;
}
// where a batch being enqueued releases the decode stages other contexts have deferred
int release_mode() {
    const int f = g_overlap_force.load(std::memory_order_relaxed);
    return f >= 0 ? f : 2;
}
// (The decode stream has default priority: the lowest one measured the same, and is the wrong thing to hold when two processes
// share a GPU.)

// the refinement kernel's parameters for setting `cfg` (weight tables from libm: built once per setting, not per batch)
const void* refine_params_for(a3_ctx* ctx, const a3_refine_config& cfg) {
    if (ctx->refine_prm.empty() || memcmp(&ctx->refine_prm_cfg, &cfg, sizeof cfg) != 0) {
        ctx->refine_prm.assign((refine_params_bytes() + 3) / 4, 0.0f);
        refine_params(ctx->refine_prm.data(), cfg, ctx->mark_size);
        ctx->refine_prm_cfg = cfg;
    }
    return ctx->refine_prm.data();
}

// ChArUco: the per-frame slot records of charuco_tmp (the counts follow them)
size_t charuco_slot_bytes(const Batch& b) { return ((size_t)b.n * b.charuco_nc * sizeof(a3_charuco_corner) + 255) & ~(size_t)255; }
// what a3_readback.h lays a batch's staging out from
ReadbackShape readback_shape(const Batch& b, size_t head_bytes) { return {b.n, b.guess, b.charuco_guess, head_bytes, b.want_pose, b.refined, b.undist, b.board, b.charuco, b.recover, b.flags}; }
// the refinement kernel's parameters for the ChArUco setting `cfg` (its window and iteration settings; built once per setting)
const void* charuco_params_for(a3_ctx* ctx, const a3_charuco_config& cfg) {
    if (ctx->charuco_prm.empty() || memcmp(&ctx->charuco_prm_cfg, &cfg, sizeof cfg) != 0) {
        ctx->charuco_prm.assign((refine_params_bytes() + 3) / 4, 0.0f);
        const a3_refine_config rc{A3_REFINE_SUBPIX, cfg.win_half, cfg.relative_win, cfg.max_iterations, cfg.min_shift};
        refine_params(ctx->charuco_prm.data(), rc, 0);
        ctx->charuco_prm_cfg = cfg;
    }
    return ctx->charuco_prm.data();
}

// the board's and the ChArUco setting's device tables (upload_board, upload_charuco); nc: the chessboard corners of the setting in force
BoardTables board_tables(const a3_ctx* ctx, uint32_t nc) {
    return {.slot_of = ctx->board_slot_of.as<uint16_t>(), .n_codes = ctx->n_codes, .slots = ctx->board_slot_rec.p, .cxy = ctx->charuco_tab.as<float>(),
            .adj = ctx->charuco_tab.as<uint32_t>() + 2 * (size_t)nc, .nc = nc, .slot_kind = ctx->board_kind_up};
}
// The decode stage on the context's buffers as the last enqueue_front / layout_zero_block left them: what the product path
// (enqueue_back) and the probe (a3_debug_kernel_time) share.  The frames, the table size, the grid and the taps are the caller's.
DecodeStage decode_stage(const a3_ctx* ctx) {
    const uint32_t S = ctx->cfg.homography_sample_size;
    DecodeStage d;
    d.cands = ctx->cands.as<CandRec>(); d.cand_count = ctx->cand_count; d.pre_xy = ctx->pre_xy.as<uint16_t>(); d.fin_xy = ctx->fin_xy.as<uint16_t>();
    d.fin_count = ctx->fin_count.as<uint32_t>(); d.work = ctx->work.as<uint32_t>(); d.S = S; d.proj = ctx->proj.p; d.big_scratch = ctx->cand_big.as<float>();
    d.n = ctx->mark_size; d.max_taps = S; d.dict = ctx->dict.as<uint64_t>(); d.n_codes = ctx->n_codes; d.tau = ctx->tau;
    d.filter = ctx->cfg.filter_high_bit_errors; d.wtab = ctx->wtab.as<float>(); d.outs = ctx->outs.p; d.per_frame = ctx->per_frame; d.markers = ctx->markers_ptr;
    BatchScratch* const head = ctx->head;
    d.work_count = &head->work_count; d.marker_total = &head->marker_total; d.cand_pre_total = &head->cand_pre_total; d.err_flags = &head->err_flags;
    return d;
}

// candidates -> markers -> read-back of one batch, on stream `st` (the context's stream, or its decode stream when deferred)
int enqueue_back(a3_ctx* ctx, hipStream_t st, const Batch& b) {
    const float min_corner_separation = (float)std::min(b.W, b.H) * ctx->cfg.min_corner_separation_factor;   // src/aruco.rs:56
    unsigned int* d_marker_total = &ctx->head->marker_total;
    ctx->pre_count = b.K > 1 ? ctx->merged_count.as<uint32_t>() : ctx->cand_count;
    if (ctx->inject_armed) {   // (test hook; never set by a caller of the public header)
        ctx->inject_armed = false;
        const uint32_t cnt = (uint32_t)ctx->inject.size();
        if (cnt) A3_HIP(hipMemcpyAsync(ctx->cands.p, ctx->inject.data(), cnt * sizeof(CandRec), hipMemcpyHostToDevice, st));
        ctx->inject_count = cnt;
        A3_HIP(hipMemcpyAsync(ctx->cand_count, &ctx->inject_count, 4, hipMemcpyHostToDevice, st));
    }
    // few frames (small batches): all four waves of a workgroup run the stages behind the sampling.  (Round 5 tried folding the marker
    // gather into k_decode for one-frame calls -- its last workgroup, found by a ticket -- to save a launch: the call got 5 us SLOWER,
    // 166 against 161 us in alternating runs, a fence + ticket per workgroup and a serial tail costing more than the launch; removed.)
    DecodeStage dec = decode_stage(ctx);
    dec.n_frames = b.n; dec.max_cand = b.max_cand; dec.min_distance = min_corner_separation; dec.marker_cap = b.marker_cap;
    dec.src = b.src; dec.W = (int)b.W; dec.H = (int)b.H; dec.few = b.n <= 64u; dec.inverted = b.flags;
    if (b.taps) dec.patches = ctx->patches.as<uint8_t>();
    dec.patch_cap = b.patch_cap;
    dec.grid_blocks = (int)std::min<uint32_t>(4096u, b.n * 128u);   // (grid-stride over the work list; 4096 workgroups that find nothing cost a one-frame call ~4 us)
    uint32_t* side_total = nullptr, * side_per_frame = nullptr, * recovered = nullptr;   // recover_counts: [total, padded | per frame | recovered per frame]
    if (b.recover) {
        side_total = ctx->recover_counts.as<uint32_t>(); side_per_frame = side_total + 4; recovered = static_cast<uint32_t*>(ctx->side_dev[kSideRecovered]);   // the gather's list, counts and total go to the side buffers; the batch's own are written by k_recover_merge
        A3_HIP(hipMemsetAsync(side_total, 0, 16 + (size_t)b.n * 4, st));
        dec.markers = ctx->recover_det.as<a3_marker>(); dec.per_frame = side_per_frame; dec.marker_total = side_total;
    }
    if (b.K > 1) {   // the K planes' tables merged into the frames' lists; from here on cand_count is the merged lists'
        dec.windows = b.K; dec.plane_cand = b.plane_cand; dec.merged_count = ctx->merged_count.as<uint32_t>();
        A3_HIP(launch_merge_candidates(st, dec));
        dec.cand_count = dec.merged_count;
    } else A3_HIP(launch_frame_candidates(st, dec));
    A3_HIP(launch_decode(st, dec));
    A3_HIP(launch_compact_markers(st, dec));
    if (b.recover) {
        A3_HIP(launch_recover_frames(st, {.markers = dec.markers, .n_dev = side_total, .per_frame = side_per_frame, .n = b.marker_cap, .n_frames = b.n,
                                          .outs = dec.outs, .fin_xy = dec.fin_xy, .fin_count = dec.fin_count, .max_cand = b.max_cand,
                                          .board = board_tables(ctx, b.charuco_nc), .slot_ids = ctx->recover_ids.as<uint32_t>(), .n_slots = b.recover_slots,
                                          .dict = ctx->dict.as<uint64_t>(), .cfg = b.recover_cfg, .rec = ctx->recover_tmp.as<a3_marker>(),
                                          .rec_cap = b.recover_cap, .rec_count = recovered}));
        A3_HIP(launch_recover_merge(st, {.det = dec.markers, .det_cap = b.marker_cap, .det_per_frame = side_per_frame, .rec = ctx->recover_tmp.as<a3_marker>(),
                                         .rec_cap = b.recover_cap, .rec_count = recovered, .n_frames = b.n, .out = ctx->markers_ptr, .out_cap = b.marker_cap,
                                         .per_frame = ctx->per_frame, .marker_total = d_marker_total, .err_flags = &ctx->head->err_flags}));
    }
    uint32_t* const flags = b.flags ? ctx->flags_buf.as<uint32_t>() : nullptr;
    if (b.flags)   // which markers of the final list were read inverted (ahead of the scaling and the refinement, which reads them)
        A3_HIP(launch_marker_flags(st, {.markers = ctx->markers_ptr, .n_dev = d_marker_total, .n = b.marker_cap, .outs = dec.outs, .n_frames = b.n,
                                        .max_cand = b.max_cand, .flags = flags}));
    // what everything behind the marker list samples and measures by: the decode stage's source, or with a reduction the caller's
    // full-size frames, on which the list's corners lie once k_scale_markers has mapped them up
    const bool reduced = b.plane == Batch::Plane::Reduced;
    const PixelSrc back_src = reduced ? b.frames : b.src;
    const uint32_t back_W = reduced ? b.frames_W : b.W, back_H = reduced ? b.frames_H : b.H;
    if (reduced) A3_HIP(launch_scale_markers(st, {.markers = ctx->markers_ptr, .n_dev = d_marker_total, .n = b.marker_cap, .factor = b.reduce_f}));
    float* const refined = b.refined ? ctx->refined_buf.as<float>() : nullptr;
    if (b.refined) {   // sub-pixel corners of the device-resident marker list, sampled from the same frames / grey plane as the decode stage
        const RefineLaunch rl{.src = back_src, .W = back_W, .H = back_H, .markers = ctx->markers_ptr, .n_dev = d_marker_total, .n = b.marker_cap,
                              .params = refine_params_for(ctx, b.refine), .out = refined, .flags = flags};
        A3_HIP(b.refine.method == A3_REFINE_EDGES ? launch_refine_edges(st, rl) : launch_refine_corners(st, rl));
    }
    if (b.undist)   // undistorted pixel corners of the same markers (of their refined corners with refinement on)
        A3_HIP(launch_undistort_corners(st, ctx->markers_ptr, refined, d_marker_total, b.marker_cap, b.pose_intr, b.dist, ctx->undist_buf.as<float>(),
                                        static_cast<float*>(ctx->side_dev[kSideUndistRes])));
    // the batch's marker list with the float corners the poses are solved from: undistorted, else refined, else none (the integer corners)
    MarkerSrc m{.markers = ctx->markers_ptr, .n_dev = d_marker_total, .per_frame = ctx->per_frame, .corners = b.undist ? ctx->undist_buf.as<float>() : refined,
                .n = b.marker_cap, .n_frames = b.n};
    const BoardTables board = board_tables(ctx, b.charuco_nc);
    const a3_intrinsics* const intr = b.pose_has_intr ? &b.pose_intr : nullptr;
    const uint32_t* charuco_counts = b.charuco ? reinterpret_cast<const uint32_t*>(ctx->charuco_tmp.as<uint8_t>() + charuco_slot_bytes(b)) : nullptr;
    float* charuco_und = b.charuco && b.want_pose && b.undist ? ctx->charuco_und.as<float>() : nullptr;
    if (b.charuco) {   // the chessboard corners of the same markers (their raw refined or integer corners), sampled as the refinement samples
        MarkerSrc raw = m;
        raw.corners = refined;
        A3_HIP(launch_charuco_corners(st, {.src = back_src, .W = back_W, .H = back_H, .m = raw, .board = board, .min_markers = b.charuco_cfg.min_markers,
                                           .refine = b.charuco_cfg.refine, .params = charuco_params_for(ctx, b.charuco_cfg), .intr = &b.pose_intr, .dist = &b.dist,
                                           .slots_tmp = ctx->charuco_tmp.as<a3_charuco_corner>(), .counts = const_cast<uint32_t*>(charuco_counts),
                                           .out = ctx->charuco_buf.as<a3_charuco_corner>(), .und = charuco_und}));
    }
    if (b.want_pose) {   // IPPE on the device-resident marker list (src/pose.rs:52-81), no extra round trip
        const a3_intrinsics& in = b.pose_intr;
        PoseLaunch pose{.n = b.marker_cap, .n_dev = d_marker_total, .marker_size_mm = b.pose_size_mm, .iw = (float)back_W, .ih = (float)back_H, .fx = in.focal_x,
                        .fy = in.focal_y, .cx = in.principal_x, .cy = in.principal_y, .out = ctx->pose_buf.as<a3_pose>()};
        if (m.corners) {   // from float corners (k_pose modes 3 / 4)
            pose.corner_stride = 8u; pose.norm_pts = m.corners; pose.mode = b.pose_has_intr ? 4 : 3;
        } else {
            pose.corners = reinterpret_cast<const uint32_t*>(reinterpret_cast<const uint8_t*>(ctx->markers_ptr) + offsetof(a3_marker, corners));
            pose.corner_stride = (uint32_t)(sizeof(a3_marker) / 4); pose.mode = b.pose_has_intr ? 1 : 0;
        }
        A3_HIP(launch_pose(st, pose));
        if (b.board) {   // one board pose per frame from the same device-resident markers (and refined corners), no extra round trip
            const BoardPoseLaunch bp{.m = m, .board = board, .intr = intr, .W = back_W, .H = back_H, .out = ctx->board_buf.as<a3_board_pose>()};
            A3_HIP(board.slot_kind == kBoardSlots3D ? launch_board3d_pose(st, bp) : launch_board_pose(st, bp));
        }
        if (b.charuco)   // one ChArUco pose per frame from the records just written, the starts as the board pose takes them
            A3_HIP(launch_charuco_pose(st, {.m = m, .board = board, .counts = charuco_counts, .recs = ctx->charuco_buf.as<a3_charuco_corner>(), .und = charuco_und,
                                            .intr = intr, .W = back_W, .H = back_H, .out = ctx->charuco_pose_buf.as<a3_charuco_pose>()}));
    }
    if (b.prof >= 2) A3_HIP(hipEventRecord(ctx->ev[3], st));
    // ---- results: one copy of [head | `guess` markers], then the poses and (taps) the counts ----
    // (every destination from the batch's layout, a3_readback.h; the board and ChArUco poses: one record per frame, whatever the marker count)
    const Readback& rb = b.rb;
    auto stage = [&](const Span& to, const void* from) { return hipMemcpyAsync(at<uint8_t>(ctx->pinned, to), from, to.bytes, hipMemcpyDeviceToHost, st); };
    A3_HIP(hipMemcpyAsync(ctx->pinned, ctx->head, rb.head.bytes + rb.markers.bytes, hipMemcpyDeviceToHost, st));
    for (int k = 0; k < kSideKinds; k++)
        if (b.has(k)) A3_HIP(stage(rb.side[k], ctx->side_dev[k]));
    if (b.flags) A3_HIP(stage(rb.flags, flags));
    if (b.charuco) {
        A3_HIP(hipMemcpyAsync(at<uint8_t>(ctx->pinned, rb.charuco_total), charuco_counts + b.n, 4, hipMemcpyDeviceToHost, st));
        A3_HIP(stage(rb.charuco, ctx->charuco_buf.p));
    }
    if (b.taps) {   // Detection.candidates / .homographies will be asked for frame by frame: their counts travel now
        A3_HIP(hipMemcpyAsync(ctx->pinned_counts, dec.cand_count, (size_t)b.n * 4, hipMemcpyDeviceToHost, st));
        A3_HIP(hipMemcpyAsync((uint8_t*)ctx->pinned_counts + (size_t)b.n * 4, ctx->fin_count.p, (size_t)b.n * 4, hipMemcpyDeviceToHost, st));
    }
    A3_HIP(hipEventRecord(ctx->ev[4], st));
    return A3_OK;
}

// Enqueue the deferred second half of `ctx`'s batch on its decode stream: after its own contour stage and, when `after` is
// given, after that event (the threshold kernel of the batch another context has just submitted).  g_defer_mu is held.
int flush_deferred_impl(a3_ctx* ctx, hipEvent_t after);
int flush_deferred_locked(a3_ctx* ctx, hipEvent_t after) {
    const int rc = flush_deferred_impl(ctx, after);
    if (rc) ctx->back_rc = rc;   // the owner may be another thread's context: its collect must not read a batch that never ran
    return rc;
}
int flush_deferred_impl(a3_ctx* ctx, hipEvent_t after) {
    if (!ctx->back_deferred) return A3_OK;
    ctx->back_deferred = false;
    for (size_t i = 0; i < g_deferred.size(); i++)
        if (g_deferred[i] == ctx) { g_deferred.erase(g_deferred.begin() + (long)i); break; }
    hipStream_t ds = nullptr;
    A3_HIP(device_stream(ctx->device, kStreamDecode, &ds));
    A3_HIP(hipStreamWaitEvent(ds, ctx->ev_contours, 0));
    if (after) A3_HIP(hipStreamWaitEvent(ds, after, 0));
    if (int rc = enqueue_back(ctx, ds, ctx->batch)) return rc;
    (void)hipStreamQuery(ds);   // hands what was just queued to the GPU now (the owner polls an event, not this stream)
    return A3_OK;
}

int need_stream(a3_ctx* ctx) {
    if (ctx->stream) return A3_OK;
    if (!ctx->own_stream) {
        A3_HIP(hipSetDevice(ctx->device));
        A3_HIP(create_stream(&ctx->own_stream));
    }
    {   // (batch_mode_of reads every live context's stream under this lock, possibly from another thread's submit)
        std::lock_guard<std::mutex> lk(g_streams_mu);
        ctx->stream = ctx->own_stream;
    }
    return A3_OK;
}

// ---- bursts: contexts whose submitted batch has its threshold kernel enqueued and the rest held back (see a3_ctx::rest_held) ----
std::vector<a3_ctx*> g_held;   // guarded by g_defer_mu, in submission order
int enqueue_chain(a3_ctx* ctx, Batch& b, bool defer_locked);
// Enqueue the held chain of `ctx`'s batch on its stream, behind `after` when given (the threshold kernel of the burst's last
// member).  g_defer_mu is held; the owner may be another thread's context, so the verdict is kept for its collect.
int flush_held_locked(a3_ctx* ctx, hipEvent_t after, bool by_last_member = false) {
    if (!ctx->rest_held) return A3_OK;
    ctx->rest_held = false;
    ctx->stepping = by_last_member ? A3_STEP_HELD_RELEASED_BY_LAST : A3_STEP_HELD_RELEASED_EARLY;
    for (size_t i = 0; i < g_held.size(); i++)
        if (g_held[i] == ctx) { g_held.erase(g_held.begin() + (long)i); break; }
    int rc = A3_OK;
    if (after && hipStreamWaitEvent(ctx->stream, after, 0) != hipSuccess) rc = fail(ctx, A3_ERR_HIP, "hipStreamWaitEvent (burst gate)");
    if (rc == A3_OK) rc = enqueue_chain(ctx, ctx->batch, /*defer_locked=*/true);
    ctx->held_rc = rc;
    (void)hipStreamQuery(ctx->stream);   // hands what was just queued to the GPU now (the owner may be polling an event)
    return rc;
}

// ---- what a batch's chain needs before it can be enqueued without allocating ----
// (device_plan_capacity, zero_layout, marker_cap_of, marker_guess_of, pool_darts_of: a3_batch_head.h)
// The second half's buffers: poses, refined corners, board poses, undistorted corners, pinned staging for the read-back head and `guess` markers (+ poses
// ...; a longer list is fetched by finish_batch after growing it), pinned staging for the tap counts.
int ensure_back_buffers(a3_ctx* ctx, Batch& b, size_t head_bytes) {
    b.rb = readback_layout(readback_shape(b, head_bytes));   // (guess and charuco_guess are fixed; the head's size is known now)
    void** const side = ctx->side_dev;   // (where each side result of this batch is written: what the read-back copies from)
    if (b.want_pose) { A3_HIP(ctx->pose_buf.ensure((size_t)b.marker_cap * 2 * sizeof(a3_pose))); side[kSidePoses] = ctx->pose_buf.p; }
    if (b.refined) { A3_HIP(ctx->refined_buf.ensure((size_t)b.marker_cap * 8 * sizeof(float))); side[kSideRefined] = ctx->refined_buf.p; }
    if (b.board) { A3_HIP(ctx->board_buf.ensure((size_t)b.n * sizeof(a3_board_pose))); side[kSideBoard] = ctx->board_buf.p; }
    if (b.flags) A3_HIP(ctx->flags_buf.ensure(std::max<size_t>(b.marker_cap, 1) * kFlagsRec));
    if (b.undist) {
        A3_HIP(ctx->undist_buf.ensure((size_t)b.marker_cap * 12 * sizeof(float)));
        side[kSideUndist] = ctx->undist_buf.p; side[kSideUndistRes] = ctx->undist_buf.as<float>() + (size_t)b.marker_cap * 8;
    }
    if (b.charuco) {
        const size_t recs = (size_t)b.n * b.charuco_nc;
        A3_HIP(ctx->charuco_tmp.ensure(charuco_slot_bytes(b) + ((size_t)b.n + 1) * 4));
        A3_HIP(ctx->charuco_buf.ensure(std::max<size_t>(recs, 1) * sizeof(a3_charuco_corner)));
        if (b.want_pose) { A3_HIP(ctx->charuco_pose_buf.ensure((size_t)b.n * sizeof(a3_charuco_pose))); side[kSideCharucoPoses] = ctx->charuco_pose_buf.p; }
        if (b.want_pose && b.undist) A3_HIP(ctx->charuco_und.ensure(std::max<size_t>(recs, 1) * 8));
    }
    if (b.recover) {
        b.recover_cap = std::min(b.recover_slots, b.max_cand);
        A3_HIP(ctx->recover_counts.ensure(16 + (size_t)b.n * 8));
        side[kSideRecovered] = ctx->recover_counts.as<uint32_t>() + 4 + b.n;   // [total, padded | per frame | recovered per frame]
        A3_HIP(ctx->recover_det.ensure((size_t)b.marker_cap * sizeof(a3_marker)));
        A3_HIP(ctx->recover_tmp.ensure((size_t)b.n * b.recover_cap * sizeof(a3_marker)));
    }
    if (int rc = ensure_pinned(ctx, pinned_bytes(b.rb))) return rc;
    if (b.taps && ctx->pinned_counts_cap < (size_t)b.n * 8) {
        if (ctx->pinned_counts) (void)hipHostFree(ctx->pinned_counts);
        ctx->pinned_counts = nullptr; ctx->pinned_counts_cap = 0;
        A3_HIP(hipHostMalloc(&ctx->pinned_counts, (size_t)b.n * 8, hipHostMallocDefault));
        ctx->pinned_counts_cap = (size_t)b.n * 8;
    }
    return A3_OK;
}
// Every buffer the chain (contour stage ... read-back) of a DEVICE-PLANNED batch uses, with a dart capacity of cap_d, allocated
// before anything of the chain is launched -- for a chain that is held back for a burst, at submit: it is enqueued later, by
// whichever thread submits the burst's last member, under the process-wide lock, and must then find nothing left to allocate
// (hipMalloc / hipHostMalloc synchronise the device).  The per-frame dart totals of the device plan live in frame_darts_dev, zeroed
// once here and handed back zeroed by the plan workgroup.
int ensure_chain_buffers(a3_ctx* ctx, hipStream_t st, Batch& b, uint64_t cap_d) {
    const uint32_t n = b.planes;
    const ZeroLayout z = zero_layout(1, n, n, b.marker_cap);
    A3_HIP(ctx->tile_darts.ensure(tile_darts_bytes(b.W, b.H, n)));
    A3_HIP(ctx->zero_blk.ensure(z.total));
    if (ctx->frame_darts_dev.cap < (size_t)n * 8) {
        A3_HIP(ctx->frame_darts_dev.ensure((size_t)n * 8));
        A3_HIP(hipMemsetAsync(ctx->frame_darts_dev.p, 0, ctx->frame_darts_dev.cap, st));
    }
    A3_HIP(ctx->frame_base.ensure((size_t)(n + 1) * 4));
    if (int rc = ensure_dart_pool(ctx, pool_darts_of(ctx->max_darts, cap_d, 1))) return rc;
    A3_HIP(ctx->pix_base.ensure((size_t)n * b.W * b.H * 4));
    A3_HIP(ctx->contours.ensure((size_t)ctx->hints.max_contours * sizeof(ContourRec)));
    A3_HIP(ctx->cyc_start_off.ensure((size_t)ctx->hints.max_contours * 4));
    A3_HIP(ctx->points.ensure(ctx->hints.max_points * 4));
    return ensure_back_buffers(ctx, b, z.head_bytes);
}

// One batch = enqueue_front (buffers, threshold kernel) + enqueue_chain (plan, contour stage, then the second half -- candidates ->
// markers -> read-back, ending in an event -- or its deferral) + finish_batch (wait for the event, check the device's verdict, hand
// out the markers).  a3_detect_batch runs them back to back (enqueue_batch); a3_detect_batch_submit / _collect let the caller
// enqueue the next batch (on another context) before collecting this one, so the GPU never waits for the host; a burst
// (submit_common) enqueues a member's chain later than its front half.  `b.pixels` is a device pointer here.

// `held`: the chain is held back (submit_common holds device-planned batches only): an event goes behind the threshold kernel, which
// the burst's last member's own threshold kernel replaces for the chains it releases, and the chain's buffers are allocated now.
int enqueue_front(a3_ctx* ctx, Batch& b, bool held) {
    hipStream_t st = ctx->stream;
    const uint32_t n = b.n, W = b.W, H = b.H;
    const size_t npx = (size_t)W * H;
    const uint32_t kMaxCand = ctx->hints.max_cand;
    // the grey plane is materialised only for readers outside the fused path: Detection.grey (debug taps) and the generic
    // threshold kernels (radii above 31); the decode stage otherwise samples the caller's frames directly
    const bool big_window = b.K == 1 && threshold_writes_grey_plane(b.radius);   // (a set of two or more holds fused-kernel radii only)
    const uint32_t np = b.planes;   // the planes of the front half: n, or n x K with several threshold windows
    const uint32_t merged_cand = b.K > 1 ? merged_cand_capacity(b.K, kMaxCand) : kMaxCand;
    b.need_grey = b.taps || big_window;
    b.grey_src = big_window || (b.taps && !b.sample_frames);
    if (b.need_grey) A3_HIP(ctx->grey.ensure(npx * n));
    ctx->grey_valid = b.need_grey;
    if (big_window) A3_HIP(ctx->hsum.ensure(npx * n * 2));
    const size_t bits_per_frame = (size_t)words_per_row(W) * 8 * H;   // packed thresholded image
    A3_HIP(ctx->bin.ensure(bits_per_frame * np));
    A3_HIP(ctx->frame_darts.ensure((size_t)np * 8));
    A3_HIP(ctx->cands.ensure((size_t)np * kMaxCand * sizeof(CandRec)));
    if (b.K > 1) A3_HIP(ctx->merged_count.ensure((size_t)n * 4));
    A3_HIP(ctx->pre_xy.ensure((size_t)n * merged_cand * 16));
    A3_HIP(ctx->fin_xy.ensure((size_t)n * merged_cand * 16));
    A3_HIP(ctx->fin_count.ensure((size_t)n * 4));
    A3_HIP(ctx->work.ensure((size_t)n * merged_cand * 4));
    if (merged_cand > frame_cand_lds_slots()) A3_HIP(ctx->cand_big.ensure((size_t)n * merged_cand * 4));   // keys / perimeters of k_frame_candidates' through-memory form
    A3_HIP(ctx->outs.ensure((size_t)n * merged_cand * decode_out_bytes()));
    A3_HIP(ctx->proj.ensure((size_t)n * merged_cand * proj_rec_bytes()));
    b.max_cand = merged_cand; b.plane_cand = kMaxCand;
    b.marker_cap = marker_cap_of(merged_cand, n, b.out_cap);
    b.guess = marker_guess_of(ctx->last_marker_total, b.marker_cap);
    b.patch_cap = (uint32_t)std::min<uint64_t>(kPatchCapMax, std::max<uint64_t>(kPatchCapMin, (uint64_t)n * merged_cand));
    if (b.taps) { A3_HIP(ctx->patches.ensure((size_t)b.patch_cap * ctx->cfg.homography_sample_size * ctx->cfg.homography_sample_size)); ctx->patch_cap = b.patch_cap; }
    ctx->W = W; ctx->H = H; ctx->frames = np; ctx->frames_merged = n; ctx->cand_stride = merged_cand;
    ctx->stats = a3_stats{};
    ctx->contours_valid = false; ctx->markers_valid = false; ctx->side_valid[kSidePoses] = false;

    // ---- K1 ----
    b.prof = b.profiling == 1 && (ctx->batch_seq++ % (uint32_t)b.profile_every) != 0 ? 0 : b.profiling;
    // the frames' derived grey plane, immediately ahead of its reader on the same stream: whatever orders that orders this
    const PixelSrc& fr = b.frames;
    if (b.plane == Batch::Plane::Rectified)
        A3_HIP(launch_rectify_grey(st, {.src = fr.base, .src_row = (size_t)fr.row_stride, .src_frame = (size_t)fr.frame_stride, .n_frames = n, .fmt = fr.fmt,
                                        .r = &b.rect_r, .grey = ctx->plane.as<uint8_t>()}));
    if (b.plane == Batch::Plane::Reduced)
        A3_HIP(launch_reduce_frames(st, {.src = fr.base, .src_row = (size_t)fr.row_stride, .src_frame = (size_t)fr.frame_stride, .n_frames = n, .fmt = fr.fmt,
                                         .W = b.frames_W, .H = b.frames_H, .factor = b.reduce_f, .dst = ctx->plane.as<uint8_t>(), .dst_row = W,
                                         .dst_frame = npx}));
    if (b.prof) A3_HIP(hipEventRecord(ctx->ev[0], st));
    // one launch per window, window k's bits in block k of the packed planes (the grey plane, where wanted, is the first launch's)
    for (uint32_t k = 0; k < b.K; k++)
        A3_HIP(launch_grey_threshold(st, {.pixels = b.pixels, .fmt = b.fmt, .row_stride = b.row_stride, .frame_stride = b.frame_stride, .W = (int)W, .H = (int)H,
                                          .n = n, .radius = b.K > 1 ? b.win[k] : b.radius, .grey = b.need_grey && k == 0 ? ctx->grey.as<uint8_t>() : nullptr,
                                          .bits = ctx->bin.as<uint64_t>() + bits_per_frame / 8 * window_plane(k, 0, n),
                                          .hsum_tmp = big_window ? ctx->hsum.as<uint16_t>() : nullptr}));
    if (b.prof) A3_HIP(hipEventRecord(ctx->ev[1], st));
    if (!held) return A3_OK;
    A3_HIP(hipEventRecord(ctx->ev_k1_done, st));   // (held chains of a burst wait for the last member's)
    const uint64_t cap_d = device_plan_capacity(ctx->hints, ctx->max_darts, np, W, H);
    if (cap_d == 0) return fail(ctx, A3_ERR_INTERNAL, "a chain was held back for a batch that needs a host-side plan");
    return ensure_chain_buffers(ctx, st, b, cap_d);
}

// The contour stage's buffers as the last enqueue_front / layout_zero_block left them, for a chunk of the context's batch: what the
// chunk loop (enqueue_chain) and the probe (a3_debug_kernel_time) share.  The chunk, the settings and n_live are the caller's.
ContourChunk contour_chunk(const a3_ctx* ctx) {
    ContourChunk c;
    c.W = (int)ctx->W; c.H = (int)ctx->H; c.batch_frames = ctx->frames;
    c.bits = ctx->bin.as<uint64_t>(); c.tile_darts = ctx->tile_darts.as<uint32_t>(); c.pix_base = ctx->pix_base.as<uint32_t>();
    c.d_rec = ctx->d_xy.as<uint64_t>(); c.d_succ = ctx->d_succ.as<uint32_t>();
    c.entry_list = ctx->entry_list.as<uint32_t>(); c.es_a = ctx->es_a.p; c.es_b = ctx->es_b.p; c.fin = ctx->fin.p;
    c.leader_count = ctx->head->leader_count; c.entry_count = ctx->head->entry_count;
    c.leader_list = ctx->leader_list.as<uint32_t>(); c.leader_keep = ctx->leader_keep.as<uint32_t>();
    c.t_cur = ctx->t_cur.as<uint64_t>(); c.t_next = ctx->t_next.as<uint64_t>();
    c.contours = ctx->contours.as<ContourRec>(); c.cyc_start_off = ctx->cyc_start_off.as<uint32_t>(); c.points = ctx->points.as<uint32_t>();
    c.max_contours = ctx->hints.max_contours; c.max_points = ctx->hints.max_points;
    c.cands = ctx->cands.as<CandRec>(); c.cand_count = ctx->cand_count;
    c.err_flags = &ctx->head->err_flags;
    return c;
}

// Everything after the threshold kernel.  `defer_locked`: the caller holds g_defer_mu (a held chain released by another context's
// submit, by a gate, by collect): nothing in here may take that lock again, so such a batch neither releases other contexts'
// deferred decode stages nor defers its own -- and, planned on the device with every buffer allocated by its front half
// (ensure_chain_buffers), it neither allocates nor waits for the device.
int enqueue_chain(a3_ctx* ctx, Batch& b, bool defer_locked) {
    hipStream_t st = ctx->stream;
    const uint32_t n = b.planes, W = b.W, H = b.H;   // (the planes: this function is the contour stage's)
    const int rel_mode = defer_locked ? 0 : release_mode();
    const size_t npx = (size_t)W * H;
    const uint32_t minwh = W < H ? W : H;
    const uint32_t min_edge_length = (uint32_t)((float)minwh * ctx->cfg.min_side_length_factor);   // src/aruco.rs:55
    const uint32_t kMaxCand = b.plane_cand;
    // batches of OTHER contexts (same device) that wait with their decode stage are released from inside this batch's launch
    // sequence (see release_mode()): `release_waiting()` records the event they wait for and enqueues them
    bool released = false;
    auto release_waiting = [&]() -> int {
        if (released) return A3_OK;
        std::lock_guard<std::mutex> lk(g_defer_mu);
        bool any = false;
        for (a3_ctx* o : g_deferred) any |= (o != ctx && o->device == ctx->device);
        if (!any) return A3_OK;
        released = true;
        A3_HIP(hipEventRecord(ctx->ev_k1, st));
        const std::vector<a3_ctx*> list = g_deferred;   // (flush edits g_deferred)
        for (a3_ctx* o : list)
            if (o != ctx && o->device == ctx->device)
                if (int rc = flush_deferred_locked(o, ctx->ev_k1)) { ctx->err = "deferred decode of another context: " + o->err; return rc; }
        return A3_OK;
    };
    if (rel_mode == 1) { if (int rc = release_waiting()) return rc; }

    // ---- contour graph size per frame -> chunk plan ----
    // A batch shaped like the previous one is planned on the device: no read-back, no idle GPU while the host thinks.
    const uint64_t cap_d = device_plan_capacity(ctx->hints, ctx->max_darts, n, W, H);
    const bool device_plan = cap_d != 0;
    // The zero block (zero_layout): one memset zeroes it up to the end of HEAD; HEAD and the marker list that follows it come back
    // to the host in one copy.
    size_t head_bytes = 0, head_off = 0;
    void* zero_p = nullptr; size_t zero_bytes = 0;
    auto layout_zero_block = [&](size_t n_chunks, uint32_t chunk_frames, bool launch) -> hipError_t {
        const ZeroLayout zl = zero_layout(n_chunks, chunk_frames, n, b.marker_cap);
        head_bytes = zl.head_bytes; head_off = zl.head_off;
        const hipError_t e = ctx->zero_blk.ensure(zl.total);
        if (e != hipSuccess) return e;
        uint8_t* z = ctx->zero_blk.as<uint8_t>();
        ctx->frame_cursor = reinterpret_cast<uint32_t*>(z);
        ctx->cand_count = ctx->frame_cursor + chunk_frames;
        ctx->head = reinterpret_cast<BatchScratch*>(z + head_off);
        ctx->counters = reinterpret_cast<DeviceCounters*>(ctx->head + 1);
        ctx->per_frame = reinterpret_cast<uint32_t*>(ctx->counters + n_chunks);
        ctx->markers_ptr = reinterpret_cast<a3_marker*>(z + head_off + head_bytes);
        zero_p = z; zero_bytes = (head_off + head_bytes + 15) & ~(size_t)15;   // (may run a few bytes into the marker area: not yet written)
        return launch ? launch_zero(st, zero_p, zero_bytes) : hipSuccess;
    };
    std::vector<Chunk> chunks;
    std::vector<uint64_t> fd;
    if (device_plan) {
        if (int rc = ensure_chain_buffers(ctx, st, b, cap_d)) return rc;
        chunks.push_back(Chunk{0, n, cap_d, (uint32_t)std::min<uint64_t>(cap_d, 0xFFFFFFFFu)});
        // The plan workgroup (last of k_tile_scan's launch) zeroes the block before it writes the plan into it: nothing earlier
        // touches it, and a launch of its own costs 4 us for a few KB.
        A3_HIP(layout_zero_block(1, n, false));
        ctx->frame_darts_ptr = ctx->frame_darts_dev.as<unsigned long long>();
    } else {
        A3_HIP(ctx->tile_darts.ensure(tile_darts_bytes(W, H, n)));
        ctx->frame_darts_ptr = ctx->frame_darts.as<unsigned long long>();
        A3_HIP(hipMemsetAsync(ctx->frame_darts.p, 0, (size_t)n * 8, st));
    }
    // device plan: frame bases and the dart total come out of the same launch sequence (BatchScratch::plan, read back with the results)
    DartCountLaunch count{.bits = ctx->bin.as<uint64_t>(), .W = (int)W, .H = (int)H, .n_frames = n, .frame_darts = ctx->frame_darts_ptr,
                          .tile_darts = ctx->tile_darts.as<uint32_t>(), .plan_cap = cap_d};
    if (device_plan) { count.frame_base = ctx->frame_base.as<uint32_t>(); count.plan = &ctx->head->plan; count.zero_p = zero_p; count.zero_bytes = zero_bytes; }
    A3_HIP(launch_dart_count(st, count));
    const uint32_t* n_live = device_plan ? &ctx->head->plan.darts : nullptr;   // written by the plan workgroup of launch_dart_count
    uint32_t max_chunk_frames = n;
    if (!device_plan) {
        if (int rc = ensure_pinned(ctx, std::max<size_t>((size_t)n * 8, 1 << 16))) return rc;
        A3_HIP(hipMemcpyAsync(ctx->pinned, ctx->frame_darts.p, (size_t)n * 8, hipMemcpyDeviceToHost, st));
        A3_HIP(wait_stream(st));
        fd.assign((uint64_t*)ctx->pinned, (uint64_t*)ctx->pinned + n);
        chunks.resize(n);
        const ChunkSplit split = split_chunks(fd.data(), n, ctx->max_darts, kMaxChunkFrames, chunks.data());
        ctx->stats.darts += split.total_darts;
        if (split.refused) return fail(ctx, A3_ERR_LIMIT, "a frame needs more contour-graph nodes than 32-bit indices allow");
        ctx->max_darts = split.max_darts;   // one frame must fit; grow the pool
        chunks.resize(split.n_chunks);
        max_chunk_frames = split.max_chunk_frames;
        if (int rc = ensure_dart_pool(ctx, pool_darts_of(ctx->max_darts, split.max_chunk_darts, chunks.size()))) return rc;
        A3_HIP(ctx->pix_base.ensure((size_t)max_chunk_frames * npx * 4));
        A3_HIP(ctx->frame_base.ensure((size_t)(max_chunk_frames + 1) * 4 * chunks.size()));
        A3_HIP(layout_zero_block(chunks.size(), max_chunk_frames, true));
        A3_HIP(ctx->contours.ensure((size_t)ctx->hints.max_contours * sizeof(ContourRec)));
        A3_HIP(ctx->cyc_start_off.ensure((size_t)ctx->hints.max_contours * 4));
        A3_HIP(ctx->points.ensure(ctx->hints.max_points * 4));
        // frame bases of every chunk, uploaded once, staged behind fd's place in the pinned buffer
        const size_t stride = max_chunk_frames + 1, n_bases = stride * chunks.size();
        if (int rc = ensure_pinned(ctx, (size_t)n * 8 + n_bases * 4 + (1 << 16))) return rc;
        uint32_t* h_bases = reinterpret_cast<uint32_t*>((uint8_t*)ctx->pinned + (size_t)n * 8);
        for (size_t ci = 0; ci < chunks.size(); ci++) chunk_frame_bases(fd.data(), chunks[ci], (uint32_t)stride, h_bases + ci * stride);
        A3_HIP(hipMemcpyAsync(ctx->frame_base.p, h_bases, n_bases * 4, hipMemcpyHostToDevice, st));
    }
    ctx->stats.chunks = (uint32_t)chunks.size();

    // ---- contour stage, chunk by chunk ----
    ContourChunk cc = contour_chunk(ctx);
    cc.n_live = n_live;
    cc.resolve_iters = ctx->hints.resolve_full_ttl > 0 ? ctx->hints.resolve_iters_hint : 0;
    cc.inline_resolve_W = ctx->hints.resolve_full_ttl > 0 ? 0 : (int)W;
    cc.min_edge_length = min_edge_length;
    cc.eps_factor = ctx->cfg.contour_simplification_epsilon;
    cc.keep_all = b.taps;
    cc.max_cand = kMaxCand;
    int rounds_max = 0;
    for (size_t ci = 0; ci < chunks.size(); ci++) {
        const Chunk& c = chunks[ci];
        const uint32_t nd = (uint32_t)c.darts;
        if (nd == 0) continue;
        if (ci > 0) {   // the batch-wide memset covered chunk 0
            A3_HIP(hipMemsetAsync(cc.leader_count, 0, sizeof(BatchScratch::leader_count) + sizeof(BatchScratch::entry_count), st));
            A3_HIP(hipMemsetAsync(ctx->frame_cursor, 0, (size_t)c.count * 4, st));   // per-frame entry counts
        }
        cc.first_frame = c.first; cc.n_frames = c.count; cc.n_darts = nd;
        cc.frame_base = ctx->frame_base.as<uint32_t>() + ci * (max_chunk_frames + 1);
        cc.ctr = ctx->counters + ci;
        A3_HIP(launch_dart_build(st, cc));
        const int rounds = chunk_rounds(c.max_frame_darts, ctx->hints.jump_rounds_hint, g_jump_rounds_cap.load(std::memory_order_relaxed));
        rounds_max = std::max(rounds_max, rounds);
        cc.max_rounds = rounds;
        cc.frame_entries = ctx->hints.entry_global_ttl > 0 ? nullptr : ctx->frame_cursor;   // per-frame entry counts
        // Short borders are finished with inside k_local_contract (kDead) on DENSE graphs only -- noise-like frames, where nine borders
        // in ten die of their length: there it saves a sixth of the contour stage; on clean frames (a dart per hundred pixels, a few
        // dozen borders per frame) it would only cost its bookkeeping.  Results are the same either way.
        const bool dense_graph = (uint64_t)nd * 10u >= (uint64_t)c.count * npx;
        cc.dead_count = (b.taps || !dense_graph) ? nullptr : ctx->head->dead_count;
        cc.phase = 1;   // first half: the doubling rounds inside LDS tiles
        A3_HIP(launch_rank_cycles(st, cc));
        if (rel_mode == 2) { if (int rc = release_waiting()) return rc; }   // waiting decode stages go out behind this k_local_contract
        ctx->dbg_nd = nd; ctx->dbg_frames = c.count; ctx->dbg_chunks = (uint32_t)chunks.size();
        cc.phase = 2;   // second half: entry resolution, final states (+ border selection), point scatter, quads
        A3_HIP(launch_rank_cycles(st, cc));
        A3_HIP(launch_resolve(st, cc));
        A3_HIP(launch_select_scatter(st, cc));
        A3_HIP(launch_contour_quads(st, cc));
    }
    if (rel_mode != 0) { if (int rc = release_waiting()) return rc; }   // (a batch without a contour graph releases here)
    if (b.prof >= 2) A3_HIP(hipEventRecord(ctx->ev[2], st));

    // ---- candidates -> markers -> read-back: enqueued now, or deferred behind the next submitted batch's threshold kernel ----
    b.src = b.grey_src ? PixelSrc{ctx->grey.as<uint8_t>(), W, (unsigned long long)npx, kFmtGreyPlane}
                        : PixelSrc{b.pixels, b.row_stride, b.frame_stride, b.fmt};
    ctx->dbg_src = b.src;
    if (int rc = ensure_back_buffers(ctx, b, head_bytes)) return rc;   // (device plan: ensure_chain_buffers did, this is a no-op)
    b.device_plan = device_plan; b.n_chunks = chunks.size(); b.chunk0_darts = chunks.empty() ? 0 : chunks[0].darts;
    b.rounds_max = rounds_max;
    ctx->counts_valid = false;
    // Deferral: only for submitted batches (somebody will submit again or collect), and not while every stage is being timed
    // (the stage times are those of stages that run alone).  The decode stage then waits on the context's decode stream until
    // (a) another context submits a batch -- it is released behind that batch's threshold kernel and shares the GPU with its
    // contour stage -- or (b) this batch is collected first.
    if (ctx->allow_defer && !defer_locked && b.profiling < 2 && ctx->batch_mode != 0) {
        A3_HIP(hipEventRecord(ctx->ev_contours, st));
        std::lock_guard<std::mutex> lk(g_defer_mu);
        ctx->back_deferred = true;
        ctx->back_rc = 0;
        ctx->stepping = A3_STEP_DECODE_DEFERRED;
        g_deferred.push_back(ctx);
    } else if (int rc = enqueue_back(ctx, st, b)) return rc;
    b.active = true;
    return A3_OK;
}

// the whole batch at once (a3_detect_batch, a re-run, a submit that is neither held nor a burst's split last member)
int enqueue_batch(a3_ctx* ctx) {
    ctx->stepping = A3_STEP_WHOLE;
    if (int rc = enqueue_front(ctx, ctx->batch, false)) return rc;
    return enqueue_chain(ctx, ctx->batch, false);
}

// `poses`: where a pose batch's poses go (null: not wanted); `out_cap`: the capacity of the caller's `out` (and `poses`)
int finish_batch(a3_ctx* ctx, a3_marker* out, a3_pose* poses, size_t out_cap, uint32_t* per_frame_count, size_t* out_n) {
    Batch& b = ctx->batch;
    if (!b.active) return fail(ctx, A3_ERR_INVALID, "no batch was submitted");
    {   // a chain still held back (no later member of its burst was submitted): it goes out now
        std::lock_guard<std::mutex> lk(g_defer_mu);
        (void)flush_held_locked(ctx, nullptr);
        if (const int rc = ctx->held_rc) { ctx->held_rc = 0; b.active = false; return rc; }
    }
    b.active = false;
    hipStream_t st = ctx->stream;
    const size_t n_chunks = b.n_chunks;
    const uint32_t guess = b.guess, n = b.n;
    uint8_t* hp = (uint8_t*)ctx->pinned;
    Readback rb = b.rb;   // where the results lie behind hp (a3_readback.h)
    {   // nobody submitted behind this batch: its decode stage goes out now
        std::lock_guard<std::mutex> lk(g_defer_mu);
        if (int rc = flush_deferred_locked(ctx, nullptr)) return rc;
        if (const int rc = ctx->back_rc) { ctx->back_rc = 0; return rc; }   // (released by another context's submit, and that failed)
    }
    A3_HIP(wait_event(ctx->ev[4], st));
    // the device's verdict on the batch (a3_batch_head.h): deliver, re-run with the hints it moved, or fail
    const BatchScratch& hs = *reinterpret_cast<const BatchScratch*>(hp);
    const DeviceCounters* hc = reinterpret_cast<const DeviceCounters*>(&hs + 1);
    const size_t slot_bytes = sizeof(CandRec) + 16 + 16 + 4 + decode_out_bytes() + proj_rec_bytes();   // cands, pre_xy, fin_xy, work, outs, proj
    const Verdict v = batch_verdict(hs, hc, {.n = b.planes, .W = b.W, .H = b.H, .device_plan = b.device_plan, .n_chunks = n_chunks, .chunk0_darts = b.chunk0_darts,
                                             .rounds_max = b.rounds_max, .out_cap = out_cap, .lds_slots = frame_cand_lds_slots(), .slot_bytes = slot_bytes},
                                    ctx->hints);
    if (b.device_plan && !hs.plan.overflow) ctx->stats.darts = ctx->dbg_nd = v.darts;
    ctx->stats.contours_traced = v.contours_traced; ctx->stats.contours_materialised = v.contours_materialised;
    ctx->stats.jump_rounds = v.jump_rounds; ctx->stats.resolve_iterations = v.resolve_iterations;
    if (v.action == Verdict::Fail) return fail(ctx, v.code, v.message);
    if (v.action == Verdict::GrowCands) {
        // Every frame of the batch gets the table of the fullest one: what that costs is known before anything is allocated, and a
        // batch whose tables cannot fit is a limit of this implementation (fewer frames per call cure it), not a HIP failure.
        const size_t had = ctx->cands.cap + ctx->pre_xy.cap + ctx->fin_xy.cap + ctx->work.cap + ctx->cand_big.cap + ctx->outs.cap + ctx->proj.cap;
        // (several windows: a plane's slot is a CandRec, a frame's merged tables hold what merged_cand_capacity makes of the planes')
        const size_t want = b.K > 1 ? (size_t)b.planes * v.next_cand * sizeof(CandRec) +
                                          (size_t)n * merged_cand_capacity(b.K, v.next_cand) * (v.slot_bytes - sizeof(CandRec))
                                    : (size_t)n * v.next_cand * v.slot_bytes;
        size_t free_b = 0, total_b = 0;
        if (want > had && hipMemGetInfo(&free_b, &total_b) == hipSuccess && want - had > free_b)
            return fail(ctx, A3_ERR_LIMIT, "candidate tables of this batch do not fit the device (every frame gets the fullest frame's table): fewer frames per call");
        ctx->hints.max_cand = v.next_cand;
    }
    if (v.action != Verdict::Deliver) return 1;   // the caller's loop re-runs the batch
    const uint32_t total = v.total, n_work = v.n_work, n_pre = v.n_pre;
    const uint32_t* hpf = reinterpret_cast<const uint32_t*>(hc + n_chunks);
    if (per_frame_count) memcpy(per_frame_count, hpf, (size_t)n * 4);
    uint32_t max_per_frame = 0;   // (read now: the staging buffer may be re-allocated below)
    for (uint32_t f = 0; f < n; f++) max_per_frame = std::max(max_per_frame, hpf[f]);
    for (int k = 0; k < kSideKinds; k++)   // the per-frame kinds (read now: the staging buffer may be re-allocated below)
        if (b.has(k) && kSides[k].per_frame) ctx->side_h[k].assign(at<uint8_t>(hp, rb.side[k]), at<uint8_t>(hp, rb.side[k]) + rb.side[k].bytes);
    if (b.charuco) {   // (read now, as the per-frame kinds)
        uint32_t charuco_total = 0;
        memcpy(&charuco_total, at<uint8_t>(hp, rb.charuco_total), 4);
        ctx->h_charuco.resize(charuco_total);
        const size_t staged = std::min<uint32_t>(charuco_total, b.charuco_guess);
        if (staged) memcpy(ctx->h_charuco.data(), at<uint8_t>(hp, rb.charuco), staged * sizeof(a3_charuco_corner));
        if (charuco_total > staged) {   // the guess was short: the rest of the records, straight from the device
            A3_HIP(hipMemcpyAsync(ctx->h_charuco.data() + staged, ctx->charuco_buf.as<a3_charuco_corner>() + staged,
                                  (charuco_total - staged) * sizeof(a3_charuco_corner), hipMemcpyDeviceToHost, st));
            A3_HIP(hipStreamSynchronize(ctx->stream));
        }
        ctx->last_charuco_total = charuco_total;
    }
    if (total > guess) {   // the guess was short: the staging area grows (the head has been consumed) and the whole list is fetched
        rb = refetch_layout(readback_shape(b, 0), total);
        if (int rc = ensure_pinned(ctx, pinned_bytes(rb))) return rc;
        hp = (uint8_t*)ctx->pinned;
        auto fetch = [&](const Span& to, const void* from) { return hipMemcpyAsync(at<uint8_t>(hp, to), from, to.bytes, hipMemcpyDeviceToHost, st); };
        A3_HIP(fetch(rb.markers, ctx->markers_ptr));
        for (int k = 0; k < kSideKinds; k++)
            if (b.has(k) && !kSides[k].per_frame) A3_HIP(fetch(rb.side[k], ctx->side_dev[k]));
        if (b.flags) A3_HIP(fetch(rb.flags, ctx->flags_buf.p));
        A3_HIP(hipStreamSynchronize(ctx->stream));
    }
    if (total) {
        memcpy(out, at<a3_marker>(hp, rb.markers), (size_t)total * sizeof(a3_marker));
        if (b.want_pose && poses) memcpy(poses, at<a3_pose>(hp, rb.side[kSidePoses]), (size_t)total * 2 * sizeof(a3_pose));
    }
    for (int k = 0; k < kSideKinds; k++) {   // the per-marker kinds: `total` records each; from here on the getters answer for this batch
        const uint8_t* const h = at<uint8_t>(hp, rb.side[k]);
        if (b.has(k) && !kSides[k].per_frame && kSides[k].kept) ctx->side_h[k].assign(h, h + (size_t)total * kSides[k].rec);
        ctx->side_valid[k] = b.has(k);
    }
    if (b.flags) ctx->flags_h.assign(at<uint32_t>(hp, rb.flags), at<uint32_t>(hp, rb.flags) + total);
    ctx->flags_valid = b.flags;
    ctx->charuco_valid = b.charuco;
    if (b.taps) {
        const uint32_t* hc32 = reinterpret_cast<const uint32_t*>(ctx->pinned_counts);
        ctx->h_cand_pre.assign(hc32, hc32 + n);
        ctx->h_cand_fin.assign(hc32 + n, hc32 + 2 * (size_t)n);
        for (auto& v : ctx->h_cand_pre) v = std::min(v, b.max_cand);
        ctx->counts_valid = true;
    }
    ctx->last_marker_total = total;
    *out_n = total;
    ctx->stats.markers = total;
    ctx->stats.candidates = n_work;      // work items = quads that survived discard_too_near
    ctx->stats.candidates_pre = n_pre;   // quads after contours_to_candidates (k_compact_markers sums the per-frame counts)
    ctx->markers_valid = true; ctx->last_n = n; ctx->last_max_per_frame = max_per_frame;
    ctx->contours_valid = b.taps && n_chunks == 1;
    if (ctx->contours_valid) { ctx->tap_contours = v.tap_contours; ctx->tap_points = v.tap_points; }
    if (b.prof >= 1) {   // the level in force when the batch was enqueued
        float ms;
        A3_HIP(hipEventElapsedTime(&ms, ctx->ev[0], ctx->ev[1])); ctx->prof_ms[A3_STAGE_THRESHOLD] += ms; ctx->prof_n[A3_STAGE_THRESHOLD]++;
        if (b.prof >= 2) {
            A3_HIP(hipEventElapsedTime(&ms, ctx->ev[1], ctx->ev[2])); ctx->prof_ms[A3_STAGE_CONTOUR] += ms; ctx->prof_n[A3_STAGE_CONTOUR]++;
            A3_HIP(hipEventElapsedTime(&ms, ctx->ev[2], ctx->ev[3])); ctx->prof_ms[A3_STAGE_DECODE] += ms; ctx->prof_n[A3_STAGE_DECODE]++;
        }
    }
    return A3_OK;
}

int run_batch(a3_ctx* ctx, a3_marker* out, a3_pose* poses, size_t out_cap, uint32_t* per_frame_count, size_t* out_n) {
    if (int rc = enqueue_batch(ctx)) return rc;
    return finish_batch(ctx, out, poses, out_cap, per_frame_count, out_n);
}

// The getters of the last collected batch's results, their pointers checked: the records (`rec` bytes each) of the host copy that
// finish_batch kept, refused with `without` when that batch ran without the feature and with `small` when dst holds fewer.
int get_last(a3_ctx* ctx, bool valid, const void* kept, size_t bytes, size_t rec, void* dst, size_t cap, size_t* n, const char* without, const char* small) {
    if (!valid) return fail(ctx, A3_ERR_INVALID, without);
    *n = bytes / rec;
    if (*n > cap) return fail(ctx, A3_ERR_CAPACITY, small);
    if (*n) memcpy(dst, kept, bytes);
    return A3_OK;
}
int get_side(a3_ctx* ctx, SideKind k, void* dst, size_t cap, size_t* n, const char* without, const char* small) {
    return get_last(ctx, ctx->side_valid[k], ctx->side_h[k].data(), ctx->side_h[k].size(), kSides[k].rec, dst, cap, n, without, small);
}

// a3_calibrate_cameras and a3_calibrate_fisheye_cameras: the same checks and staging.  The fisheye model keeps the start's compacted
// points behind the per-view scratch.
int calibrate_impl(a3_ctx* ctx, bool fisheye, const a3_calib_camera* cams, size_t n_cams, const uint32_t* view_offsets, size_t n_views,
                   const float* object_xy, const float* image_xy, a3_calib_result* results, a3_calib_view* views) {
    if (!ctx) return A3_ERR_INVALID;
    size_t n_pts = 0;
    if (const char* m = check_cameras(fisheye, ctx->busy(), cams, n_cams, view_offsets, n_views, object_xy, image_xy, results, n_pts))
        return fail(ctx, A3_ERR_INVALID, m);
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    Layout in{ctx->solve_in, ctx->stream}, scr{ctx->solve_scratch, ctx->stream}, out{ctx->solve_out, ctx->stream};
    const auto s_cams = in.add<a3_calib_camera>(n_cams);
    const auto s_off = in.add<uint32_t>(n_views + 1);
    const auto s_obj = in.add<float>(2 * n_pts), s_img = in.add<float>(2 * n_pts);
    const auto s_blocks = scr.add<double>(n_views, fisheye ? fisheye_calib_view_bytes() : calib_view_bytes());
    const auto s_start_obj = scr.add<float>(fisheye ? 2 * n_pts : 0), s_start_img = scr.add<float>(fisheye ? 2 * n_pts : 0);
    const auto s_res = out.add<a3_calib_result>(n_cams);
    const auto s_views = out.add<a3_calib_view>(n_views);
    A3_HIP(in.ensure()); A3_HIP(scr.ensure()); A3_HIP(out.ensure());
    A3_HIP(in.upload(s_cams, cams, n_cams));
    A3_HIP(in.upload(s_off, view_offsets, n_views + 1));
    A3_HIP(in.upload(s_obj, object_xy, 2 * n_pts)); A3_HIP(in.upload(s_img, image_xy, 2 * n_pts));
    // a view no camera owns is not written by the kernel: it comes back zero, not as what an earlier call left in the buffer
    A3_HIP(out.zero_from(s_views));
    const CalibLaunch cal{.cams = in.at(s_cams), .n_cams = (uint32_t)n_cams, .view_off = in.at(s_off), .obj = in.at(s_obj), .img = in.at(s_img),
                          .scratch = scr.at(s_blocks), .start_obj = scr.at(s_start_obj), .start_img = scr.at(s_start_img), .res = out.at(s_res),
                          .views = out.at(s_views)};
    A3_HIP(fisheye ? launch_calibrate_fisheye(ctx->stream, cal) : launch_calibrate(ctx->stream, cal));
    A3_HIP(out.download(s_res, results));
    A3_HIP(out.download(s_views, views));
    A3_HIP(hipStreamSynchronize(ctx->stream));
    return A3_OK;
}

}  // namespace

// =========================================================================================
// C ABI
// =========================================================================================
extern "C" {

int a3_abi_version(void) { return A3_ABI_VERSION; }

void a3_default_config(a3_config* cfg) {  // src/aruco.rs:32-43
    if (!cfg) return;
    cfg->threshold_window = 7;
    cfg->contour_simplification_epsilon = 0.05;
    cfg->min_side_length_factor = 0.2f;
    cfg->min_corner_separation_factor = 0.1f;
    cfg->homography_sample_size = 49;
    cfg->filter_high_bit_errors = 1;
}

const char* a3_last_error(const a3_ctx* ctx) { return ctx ? ctx->err.c_str() : g_create_error.c_str(); }

int a3_calculate_tau(int device, const uint64_t* codes, size_t n_codes, uint8_t* tau) {
    a3_ctx* ctx = nullptr;
    if (!codes || !tau) return fail(ctx, A3_ERR_INVALID, "a3_calculate_tau: null argument");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(ctx, A3_ERR_NO_DEVICE, "no HIP device");
    A3_HIP(hipSetDevice(device));
    uint64_t* d = nullptr; unsigned int* dt = nullptr;
    unsigned int init = 255, res = 255;
    hipError_t e = hipMalloc(&d, std::max<size_t>(n_codes, 1) * 8);
    if (e == hipSuccess) e = hipMalloc(&dt, 4);
    if (e == hipSuccess && n_codes) e = hipMemcpy(d, codes, n_codes * 8, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(dt, &init, 4, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = launch_calc_tau(nullptr, d, (uint32_t)n_codes, dt);
    if (e == hipSuccess) e = hipMemcpy(&res, dt, 4, hipMemcpyDeviceToHost);
    if (d) (void)hipFree(d);     // on every path
    if (dt) (void)hipFree(dt);
    if (e != hipSuccess) return fail(ctx, A3_ERR_HIP, "a3_calculate_tau", e);
    *tau = (uint8_t)res;
    return A3_OK;
}

int a3_create(int device, const a3_config* cfg, const uint64_t* codes, size_t n_codes, uint8_t num_bits, uint8_t tau, a3_ctx** out) {
    a3_ctx* ctx = nullptr;
    if (!cfg || !out || (!codes && n_codes)) return fail(ctx, A3_ERR_INVALID, "a3_create: null argument");
    if (cfg->threshold_window == 0) return fail(ctx, A3_ERR_INVALID, "threshold_window must be > 0 (imageproc asserts block_radius > 0)");
    if (cfg->threshold_window > 0x7FFFFFFFu)
        return fail(ctx, A3_ERR_INVALID, "threshold_window must be at most 2^31 - 1 (the threshold kernels take the radius as a signed 32-bit int)");
    if (!(cfg->contour_simplification_epsilon > 0.0)) return fail(ctx, A3_ERR_INVALID, "contour_simplification_epsilon must be > 0");
    if (cfg->homography_sample_size == 0 || cfg->homography_sample_size > 200)
        return fail(ctx, A3_ERR_INVALID, "homography_sample_size must be in 1..200");
    if (num_bits == 0 || num_bits > 64) return fail(ctx, A3_ERR_INVALID, "num_bits must be in 1..64");
    if (n_codes > 0xFFFFFFFFull) return fail(ctx, A3_ERR_INVALID, "dictionary too large");
    int count = 0;
    if (hipGetDeviceCount(&count) != hipSuccess || count <= 0) return fail(ctx, A3_ERR_NO_DEVICE, "no HIP device: this library has no CPU path");
    if (device < 0 || device >= count) return fail(ctx, A3_ERR_INVALID, "device index out of range");
    A3_HIP(hipSetDevice(device));
    a3_ctx* c = new a3_ctx();
    c->device = device;
    c->cfg = *cfg;
    c->num_bits = num_bits;
    c->n_codes = (uint32_t)n_codes;
    c->mark_size = mark_size_of(num_bits);
    ctx = c;
    hipError_t e = hipEventCreateWithFlags(&c->ev_in, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_contours, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_k1, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_gate, hipEventDisableTiming);
    if (e == hipSuccess) e = hipEventCreateWithFlags(&c->ev_k1_done, hipEventDisableTiming);
    if (e != hipSuccess) { a3_destroy(c); ctx = nullptr; return fail(ctx, A3_ERR_HIP, "hipEventCreate", e); }
    for (auto& ev : c->ev) {
        e = hipEventCreate(&ev);
        if (e != hipSuccess) { a3_destroy(c); ctx = nullptr; return fail(ctx, A3_ERR_HIP, "hipEventCreate", e); }
    }
    e = c->dict.ensure(std::max<size_t>(n_codes, 1) * 8);
    if (e == hipSuccess && n_codes) e = hipMemcpy(c->dict.p, codes, n_codes * 8, hipMemcpyHostToDevice);
    if (e != hipSuccess) { a3_destroy(c); ctx = nullptr; return fail(ctx, A3_ERR_HIP, "dictionary upload", e); }
    e = c->wtab.ensure(weight_table_bytes());
    // (on the legacy default stream: a stream of the context's own is only created if the caller never passes one)
    if (e == hipSuccess) e = launch_weight_table(nullptr, cfg->homography_sample_size, c->mark_size, cfg->homography_sample_size, c->wtab.as<float>());
    if (e == hipSuccess) e = hipStreamSynchronize(nullptr);
    if (e != hipSuccess) { a3_destroy(c); ctx = nullptr; return fail(ctx, A3_ERR_HIP, "resize weight table", e); }
    if (tau == 0) {  // src/dictionaries.rs:124
        uint8_t t = 255;
        int rc = a3_calculate_tau(device, codes, n_codes, &t);
        if (rc) { a3_destroy(c); return rc; }
        tau = t;
    }
    c->tau = tau;
    { std::lock_guard<std::mutex> lk(g_streams_mu); g_contexts.push_back(c); }
    *out = c;
    return A3_OK;
}

void a3_destroy(a3_ctx* ctx) {
    if (!ctx) return;
    (void)hipSetDevice(ctx->device);
    {
        std::lock_guard<std::mutex> lk(g_streams_mu);
        for (size_t i = 0; i < g_contexts.size(); i++)
            if (g_contexts[i] == ctx) { g_contexts.erase(g_contexts.begin() + (long)i); break; }
    }
    {   // a submitted batch that was never collected: its deferred half is dropped
        std::lock_guard<std::mutex> lk(g_defer_mu);
        for (size_t i = 0; i < g_deferred.size(); i++)
            if (g_deferred[i] == ctx) { g_deferred.erase(g_deferred.begin() + (long)i); break; }
        ctx->back_deferred = false;
        for (size_t i = 0; i < g_held.size(); i++)
            if (g_held[i] == ctx) { g_held.erase(g_held.begin() + (long)i); break; }
        ctx->rest_held = false;
    }
    if (ctx->stream && ctx->stream != ctx->own_stream) (void)hipStreamSynchronize(ctx->stream);
    {   // the device's shared streams may still hold work of this context: handles copied under the mutex, waited for outside it
        DeviceStreams ds;   // (a destroy must not stall every other thread's first use of a stream for the length of the queued work)
        { std::lock_guard<std::mutex> lk(g_streams_mu); ds = g_dev_streams[ctx->device & 63]; }
        if (ds.decode) (void)hipStreamSynchronize(ds.decode);
        if (ds.copy) (void)hipStreamSynchronize(ds.copy);
    }
    if (ctx->own_stream) (void)hipStreamSynchronize(ctx->own_stream);
    DevBuf* bufs[] = {&ctx->dict, &ctx->in, &ctx->grey, &ctx->bin, &ctx->frame_darts, &ctx->frame_darts_dev, &ctx->frame_base, &ctx->pix_base,
                      &ctx->tile_darts, &ctx->d_xy, &ctx->d_succ, &ctx->fin, &ctx->t_cur, &ctx->t_next,
                      &ctx->leader_list, &ctx->leader_keep, &ctx->entry_list, &ctx->es_a, &ctx->es_b,
                      &ctx->contours, &ctx->cyc_start_off, &ctx->points, &ctx->zero_blk, &ctx->cands,
                      &ctx->pre_xy, &ctx->fin_xy, &ctx->fin_count, &ctx->work, &ctx->outs, &ctx->proj, &ctx->patches, &ctx->cand_big,
                      &ctx->tmp_a, &ctx->tmp_b, &ctx->tmp_c, &ctx->tmp_d, &ctx->hsum, &ctx->pose_buf, &ctx->wtab, &ctx->refined_buf,
                      &ctx->board_slot_of, &ctx->board_slot_rec, &ctx->board_buf, &ctx->undist_buf, &ctx->charuco_tab, &ctx->charuco_tmp,
                      &ctx->charuco_buf, &ctx->charuco_und, &ctx->charuco_pose_buf, &ctx->solve_in,
                      &ctx->solve_scratch, &ctx->solve_big, &ctx->solve_out, &ctx->rect_in, &ctx->rect_out, &ctx->plane, &ctx->merged_count, &ctx->flags_buf};
    for (DevBuf* b : bufs) b->release();
    if (ctx->pinned) (void)hipHostFree(ctx->pinned);
    if (ctx->pinned_counts) (void)hipHostFree(ctx->pinned_counts);
    for (auto& ev : ctx->ev) if (ev) (void)hipEventDestroy(ev);
    if (ctx->ev_in) (void)hipEventDestroy(ctx->ev_in);
    if (ctx->ev_contours) (void)hipEventDestroy(ctx->ev_contours);
    if (ctx->ev_k1) (void)hipEventDestroy(ctx->ev_k1);
    if (ctx->ev_gate) (void)hipEventDestroy(ctx->ev_gate);
    if (ctx->ev_k1_done) (void)hipEventDestroy(ctx->ev_k1_done);
    if (ctx->own_stream) (void)hipStreamDestroy(ctx->own_stream);
    delete ctx;
}

int a3_set_stream(a3_ctx* ctx, void* hip_stream) {
    if (!ctx) return A3_ERR_INVALID;
    {   // a chain held back for a burst belongs on the stream its threshold kernel went to: it goes out before the stream changes
        std::lock_guard<std::mutex> lk(g_defer_mu);
        if (ctx->rest_held) (void)flush_held_locked(ctx, nullptr);
    }
    {   // (batch_mode_of reads every live context's stream under this lock, possibly from another thread's submit)
        std::lock_guard<std::mutex> lk(g_streams_mu);
        ctx->stream = hip_stream ? reinterpret_cast<hipStream_t>(hip_stream) : ctx->own_stream;   // (may be null until first needed)
    }
    return A3_OK;
}

// pinned host memory for frames: from it the H2D copy of a3_detect_batch(_submit) is asynchronous and runs at the link's rate
int a3_host_alloc(size_t bytes, void** out) {
    if (!out || bytes == 0) return A3_ERR_INVALID;
    *out = nullptr;
    const hipError_t e = hipHostMalloc(out, bytes, hipHostMallocDefault);
    if (e != hipSuccess) return fail(nullptr, A3_ERR_HIP, "hipHostMalloc", e);
    return A3_OK;
}
int a3_host_free(void* p) {
    if (!p) return A3_OK;
    const hipError_t e = hipHostFree(p);
    return e == hipSuccess ? A3_OK : fail(nullptr, A3_ERR_HIP, "hipHostFree", e);
}
int a3_host_register(void* p, size_t bytes) {
    if (!p || bytes == 0) return A3_ERR_INVALID;
    const hipError_t e = hipHostRegister(p, bytes, hipHostRegisterDefault);
    return e == hipSuccess ? A3_OK : fail(nullptr, A3_ERR_HIP, "hipHostRegister", e);
}
int a3_host_unregister(void* p) {
    if (!p) return A3_ERR_INVALID;
    const hipError_t e = hipHostUnregister(p);
    return e == hipSuccess ? A3_OK : fail(nullptr, A3_ERR_HIP, "hipHostUnregister", e);
}

// The next batch submitted on `ctx` starts on the device only after everything enqueued so far on `other` (its batch in flight
// included) has finished.  A scheduling hint for callers that keep several contexts in flight (include/aruco3_hip.h, "bursts"):
// results do not depend on it.
int a3_order_after(a3_ctx* ctx, a3_ctx* other) {
    if (!ctx || !other) return A3_ERR_INVALID;
    if (ctx == other || ctx->device != other->device) return A3_OK;   // (a context's own batches are in order anyway; other devices do not share a chip)
    A3_HIP(hipSetDevice(ctx->device));
    if (int rc = need_stream(ctx)) return rc;
    if (!other->stream) return A3_OK;   // never used: nothing in flight
    {   // a decode stage still held back would not be covered by an event on the owner's stream: it goes out now
        std::lock_guard<std::mutex> lk(g_defer_mu);
        if (other->back_deferred) { a3_ctx* o = other; if (int rc = flush_deferred_locked(o, nullptr)) { ctx->err = o->err; return rc; } }
        if (other->rest_held) (void)flush_held_locked(other, nullptr);   // (likewise a held chain; its verdict is its owner's)
    }
    if (other->stream == ctx->stream) return A3_OK;   // one stream: already ordered
    A3_HIP(hipEventRecord(other->ev_gate, other->stream));
    A3_HIP(hipStreamWaitEvent(ctx->stream, other->ev_gate, 0));
    ctx->gates_declared = true;
    return A3_OK;
}

int a3_get_stream(const a3_ctx* ctx, void** hip_stream) {
    if (!ctx || !hip_stream) return A3_ERR_INVALID;
    if (int rc = need_stream(const_cast<a3_ctx*>(ctx))) return rc;
    *hip_stream = reinterpret_cast<void*>(ctx->stream);
    return A3_OK;
}

int a3_set_pool_limits(a3_ctx* ctx, uint64_t max_darts, uint64_t max_points) {
    if (!ctx) return A3_ERR_INVALID;
    if (max_darts) ctx->max_darts = std::min<uint64_t>(max_darts, kHardMaxDarts);
    if (max_points) ctx->hints.max_points = std::min<uint64_t>(max_points, kHardMaxPoints);
    return A3_OK;
}

int a3_set_debug_taps(a3_ctx* ctx, int enabled) {
    if (!ctx) return A3_ERR_INVALID;
    ctx->debug_taps = enabled != 0;
    return A3_OK;
}

int a3_get_tau(const a3_ctx* ctx, uint8_t* tau) {
    if (!ctx || !tau) return A3_ERR_INVALID;
    *tau = ctx->tau;
    return A3_OK;
}

// argument checks + H2D staging shared by the synchronous and the split entry points.  -> A3_OK, an error, or
// kNothingToDo (no frames / empty images: the answer is "no markers").
static constexpr int kNothingToDo = 2;
static int stage_input(a3_ctx* ctx, const void* pixels, int memory, int fmt, uint32_t width, uint32_t height, size_t* row_stride,
                       size_t* frame_stride, uint32_t n_frames, const uint8_t** d_pixels) {
    if (n_frames == 0) return kNothingToDo;
    if (!pixels) return fail(ctx, A3_ERR_INVALID, "a3_detect_batch: null pixels");
    if (!format_valid(fmt)) return fail(ctx, A3_ERR_INVALID, "unknown pixel format");
    if (width == 0 || height == 0) return kNothingToDo;   // an empty image has no contours
    if (n_frames > 65535) return fail(ctx, A3_ERR_INVALID, "more than 65535 frames in one call (split the batch)");
    if (width > 65535 || height > 65535 || (uint64_t)width * height >= (1ull << 30))
        return fail(ctx, A3_ERR_INVALID, "image dimensions above 65535 (or 2^30 pixels) are not supported");
    if (const char* m = format_width_error(fmt, width)) return fail(ctx, A3_ERR_INVALID, m);
    if (*row_stride == 0) *row_stride = format_min_row_bytes(fmt, width);
    if (*row_stride < format_min_row_bytes(fmt, width)) return fail(ctx, A3_ERR_INVALID, "row_stride smaller than a row");
    if (*frame_stride == 0) *frame_stride = *row_stride * height;
    if (*frame_stride < format_min_frame_bytes(fmt, width, height, *row_stride)) return fail(ctx, A3_ERR_INVALID, "frame_stride smaller than a frame");
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    *d_pixels = reinterpret_cast<const uint8_t*>(pixels);
    if (memory == A3_MEM_HOST) {
        const size_t bytes = *frame_stride * (n_frames - 1) + format_min_frame_bytes(fmt, width, height, *row_stride);
        A3_HIP(ctx->in.ensure(bytes));
        // On the copy stream, not the compute stream: the kernels of another context's batch (submit / collect with two
        // contexts) keep running while these frames cross the link.  Pageable memory is staged by the runtime and the call
        // returns when the caller's buffer has been read; pinned memory (a3_host_alloc / a3_host_register) makes the copy
        // asynchronous and the buffer must then stay untouched until the batch is collected.
        hipStream_t cs = nullptr;
        A3_HIP(device_stream(ctx->device, kStreamCopy, &cs));
        A3_HIP(hipMemcpyAsync(ctx->in.p, pixels, bytes, hipMemcpyHostToDevice, cs));
        A3_HIP(hipEventRecord(ctx->ev_in, cs));
        A3_HIP(hipStreamWaitEvent(ctx->stream, ctx->ev_in, 0));
        *d_pixels = ctx->in.as<uint8_t>();
    } else if (memory != A3_MEM_DEVICE) return fail(ctx, A3_ERR_INVALID, "memory must be A3_MEM_HOST or A3_MEM_DEVICE");
    return A3_OK;
}

// the board's device tables (id -> slot, slot records) for the board set now, when they are not current: at submit (no batch of this
// context in flight), on the context's stream ahead of the batch
static int upload_board(a3_ctx* ctx) {
    if (ctx->board_dev_version == ctx->board_version) return A3_OK;
    ctx->board_slot_up.assign(std::max<size_t>(ctx->n_codes, 1), 0xFFFF);
    for (size_t i = 0; i < ctx->board_ids.size(); i++) ctx->board_slot_up[ctx->board_ids[i]] = (uint16_t)i;
    ctx->board_slots_up = ctx->board_slots;
    ctx->board_kind_up = ctx->board_kind;
    A3_HIP(ctx->board_slot_of.ensure(ctx->board_slot_up.size() * 2));
    A3_HIP(ctx->board_slot_rec.ensure(ctx->board_slots_up.size()));
    A3_HIP(hipMemcpyAsync(ctx->board_slot_of.p, ctx->board_slot_up.data(), ctx->board_slot_up.size() * 2, hipMemcpyHostToDevice, ctx->stream));
    A3_HIP(hipMemcpyAsync(ctx->board_slot_rec.p, ctx->board_slots_up.data(), ctx->board_slots_up.size(), hipMemcpyHostToDevice, ctx->stream));
    ctx->board_dev_version = ctx->board_version;
    return A3_OK;
}

// the board's ids in slot order, for the recovery stage, when they are not current (as upload_board)
static int upload_recover_ids(a3_ctx* ctx) {
    if (ctx->recover_ids_version == ctx->board_version) return A3_OK;
    ctx->recover_ids_up = ctx->board_ids;
    A3_HIP(ctx->recover_ids.ensure(std::max<size_t>(ctx->recover_ids_up.size(), 1) * 4));
    A3_HIP(hipMemcpyAsync(ctx->recover_ids.p, ctx->recover_ids_up.data(), ctx->recover_ids_up.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    ctx->recover_ids_version = ctx->board_version;
    return A3_OK;
}

// the chessboard's device table for the ChArUco setting in force, when it is not current (as upload_board)
static int upload_charuco(a3_ctx* ctx) {
    if (ctx->charuco_dev_version == ctx->charuco_version) return A3_OK;
    ctx->charuco_tab_up = ctx->charuco_tab_h;
    A3_HIP(ctx->charuco_tab.ensure(ctx->charuco_tab_up.size() * 4));
    A3_HIP(hipMemcpyAsync(ctx->charuco_tab.p, ctx->charuco_tab_up.data(), ctx->charuco_tab_up.size() * 4, hipMemcpyHostToDevice, ctx->stream));
    ctx->charuco_dev_version = ctx->charuco_version;
    return A3_OK;
}

// Starts a batch: its record (a3_ctx::batch) takes the call and every setting in force now, the frames are staged on the device, and
// the board's tables are brought up to date (no batch of this context is in flight).  -> A3_OK, an error, or kNothingToDo.
static int begin_batch(a3_ctx* ctx, const void* pixels, int memory, int fmt, uint32_t width, uint32_t height, size_t row_stride,
                       size_t frame_stride, uint32_t n_frames, size_t out_cap, bool want_pose, float size_mm, const a3_intrinsics* intr) {
    Batch& b = ctx->batch;
    b = Batch{};
    if (ctx->rect_on && (width != ctx->rect.src.image_width || height != ctx->rect.src.image_height))
        return fail(ctx, A3_ERR_INVALID, "a3_detect_batch: with a rectification set the frames must have the size of its src (a3_set_rectification)");
    if (ctx->reduction.factor && n_frames != 0 && pixels && width != 0 && height != 0)
        if (const char* m = check_reduced_size(true, width, height, ctx->reduction.factor)) return fail(ctx, A3_ERR_INVALID, m);
    b.fmt = fmt; b.W = width; b.H = height; b.n = n_frames; b.out_cap = out_cap;
    b.want_pose = want_pose; b.pose_size_mm = size_mm; b.pose_has_intr = intr != nullptr;
    if (intr) b.pose_intr = *intr;
    b.refine = ctx->refine;
    b.refined = b.refine.method != A3_REFINE_NONE;
    b.board = want_pose && !ctx->board_ids.empty();
    if (want_pose && ctx->dist.model != A3_DIST_NONE) {
        if (!intr) return fail(ctx, A3_ERR_INVALID, "a pose batch with lens distortion set needs intrinsics (the coefficients are in focal units)");
        b.dist = ctx->dist;
        b.undist = true;
    }
    b.charuco = ctx->charuco_nc != 0;
    if (b.charuco) {
        b.charuco_cfg = ctx->charuco_cfg;
        b.charuco_nc = ctx->charuco_nc;
        b.charuco_guess = (uint32_t)std::min<uint64_t>((uint64_t)n_frames * b.charuco_nc,
                                                       (uint64_t)ctx->last_charuco_total + ctx->last_charuco_total / 4 + 64);
    }
    b.recover = ctx->recover.mode != 0 && !ctx->board_ids.empty();
    if (b.recover) { b.recover_cfg = ctx->recover; b.recover_slots = (uint32_t)ctx->board_ids.size(); }
    b.K = ctx->n_windows > 1 ? ctx->n_windows : 1;
    b.radius = ctx->n_windows == 1 ? ctx->windows[0] : ctx->cfg.threshold_window;
    for (uint32_t k = 0; k < b.K && b.K > 1; k++) b.win[k] = ctx->windows[k];
    if (const char* m = check_window_planes(n_frames, b.K)) return fail(ctx, A3_ERR_INVALID, m);
    b.planes = n_frames * b.K;
    b.taps = ctx->debug_taps;
    b.sample_frames = ctx->debug_sample_frames;
    b.profiling = ctx->profiling; b.profile_every = ctx->profile_every;
    b.flags = ctx->polarity == A3_POLARITY_BOTH;
    ctx->flags_valid = false;   // (as the kinds that begin_clears: a3_get_marker_flags is refused until this batch is collected)
    b.sides = sides_on(readback_shape(b, 0));
    for (int k = 0; k < kSideKinds; k++)
        if (kSides[k].begin_clears) ctx->side_valid[k] = false;
    ctx->charuco_valid = false;
    b.row_stride = row_stride; b.frame_stride = frame_stride;
    const int rc = stage_input(ctx, pixels, memory, fmt, width, height, &b.row_stride, &b.frame_stride, n_frames, &b.pixels);
    if (rc != A3_OK) return rc;
    b.frames = PixelSrc{b.pixels, b.row_stride, b.frame_stride, fmt}; b.frames_W = width; b.frames_H = height;
    b.plane = ctx->rect_on ? Batch::Plane::Rectified : ctx->reduction.factor ? Batch::Plane::Reduced : Batch::Plane::None;
    if (b.plane != Batch::Plane::None) {   // from here on the (front half's) batch is an A3_FMT_L8 device batch of the plane's size whose frames are the plane
        size_t w, h;
        if (b.plane == Batch::Plane::Rectified) { b.rect_r = ctx->rect; w = b.rect_r.dst.image_width; h = b.rect_r.dst.image_height; }
        else { b.reduce_f = ctx->reduction.factor; w = width / b.reduce_f; h = height / b.reduce_f; }
        A3_HIP(ctx->plane.ensure(w * h * n_frames));
        b.pixels = ctx->plane.as<uint8_t>(); b.fmt = A3_FMT_L8; b.W = (uint32_t)w; b.H = (uint32_t)h;
        b.row_stride = w; b.frame_stride = w * h;
    }
    if (b.board || b.charuco || b.recover) { if (int urc = upload_board(ctx)) return urc; }
    if (b.recover) { if (int urc = upload_recover_ids(ctx)) return urc; }
    if (b.charuco) { if (int urc = upload_charuco(ctx)) return urc; }
    ctx->hints.force_host_plan = false;
    ctx->reruns = 0; ctx->released_others = 0;
    return A3_OK;
}

// what a batch without frames (or with empty images) returns: no markers
static void finish_trivial(a3_ctx* ctx, uint32_t* per_frame_count) {
    const Batch& b = ctx->batch;
    if (per_frame_count && b.n) memset(per_frame_count, 0, (size_t)b.n * 4);
    for (int k = 0; k < kSideKinds; k++) {   // a zero record per frame, no record per marker (the poses' flag is the enqueued batch's)
        if (!kSides[k].kept) continue;
        ctx->side_h[k].assign(b.has(k) && kSides[k].per_frame ? b.n * kSides[k].rec : 0, 0);
        ctx->side_valid[k] = b.has(k);
    }
    ctx->h_charuco.clear(); ctx->charuco_valid = b.charuco;
    ctx->flags_h.clear(); ctx->flags_valid = b.flags;
}

static int run_batch_with_retries(a3_ctx* ctx, a3_marker* out, a3_pose* poses, size_t out_cap, uint32_t* per_frame_count, size_t* out_n) {
    for (int attempt = 0; attempt < 8; attempt++) {
        const int rc = run_batch(ctx, out, poses, out_cap, per_frame_count, out_n);
        if (rc != 1) return rc;
        ctx->reruns++;
    }
    return fail(ctx, A3_ERR_CAPACITY, "contour pools kept overflowing");
}

static int detect_common(a3_ctx* ctx, const void* pixels, int memory, int fmt, uint32_t width, uint32_t height, size_t row_stride,
                         size_t frame_stride, uint32_t n_frames, bool want_pose, float size_mm, const a3_intrinsics* intr, a3_marker* out,
                         a3_pose* poses, size_t out_cap, uint32_t* per_frame_count, size_t* out_n) {
    if (!out_n || (!out && out_cap)) return fail(ctx, A3_ERR_INVALID, "a3_detect_batch: null output");
    *out_n = 0;
    if (ctx->batch.active || ctx->pending_trivial) return fail(ctx, A3_ERR_INVALID, "a submitted batch has not been collected");
    const int rc = begin_batch(ctx, pixels, memory, fmt, width, height, row_stride, frame_stride, n_frames, out_cap, want_pose, size_mm, intr);
    if (rc == kNothingToDo) { finish_trivial(ctx, per_frame_count); return A3_OK; }
    if (rc != A3_OK) return rc;
    return run_batch_with_retries(ctx, out, poses, out_cap, per_frame_count, out_n);
}

int a3_detect_batch(a3_ctx* ctx, const void* pixels, int memory, int fmt, uint32_t width, uint32_t height, size_t row_stride,
                    size_t frame_stride, uint32_t n_frames, a3_marker* out, size_t out_cap, uint32_t* per_frame_count, size_t* out_n) {
    if (!ctx) return A3_ERR_INVALID;
    return detect_common(ctx, pixels, memory, fmt, width, height, row_stride, frame_stride, n_frames, false, 0.0f, nullptr, out, nullptr,
                         out_cap, per_frame_count, out_n);
}

static int submit_common(a3_ctx* ctx, const void* pixels, int memory, int fmt, uint32_t width, uint32_t height, size_t row_stride,
                         size_t frame_stride, uint32_t n_frames, size_t out_cap, bool want_pose, float size_mm, const a3_intrinsics* intr) {
    if (ctx->batch.active || ctx->pending_trivial) return fail(ctx, A3_ERR_INVALID, "a submitted batch has not been collected");
    const int rc = begin_batch(ctx, pixels, memory, fmt, width, height, row_stride, frame_stride, n_frames, out_cap, want_pose, size_mm, intr);
    if (rc == kNothingToDo) { ctx->pending_trivial = true; return A3_OK; }
    if (rc != A3_OK) return rc;
    Batch& b = ctx->batch;
    // Bursts: a context that declared gates (a3_order_after) since its last submit holds its chain back behind its threshold
    // kernel; a submit without gates is the last member of its burst and releases every held chain of the device behind ITS
    // threshold kernel.  This is the library's behaviour behind the public header -- no switch selects it.  Exceptions, all of
    // them "enqueue the whole batch now": every stage is being timed (the stage times are those of stages that run alone); the
    // batch needs a host-side plan (first batch of a shape, or a graph that outgrew the previous plan: the plan waits for the
    // device, and a chain enqueued later by another thread must not); the context SHARES its stream with another context
    // (batch_mode_of != 0: they are in order there anyway, a3_order_after is a no-op, the decode stage is deferred instead);
    // a forced mode 1 / 2 (a3_debug_set_overlap: round 4's default, for A/B).  A context alone on a caller's stream IS held like
    // one on a stream of its own: its chain then lands on that stream behind whatever the caller queued after the submit
    // (stated in the header).
    const bool gated = ctx->gates_declared;
    ctx->gates_declared = false;
    ctx->batch_mode = batch_mode_of(ctx);
    const bool bursts = ctx->batch_mode == 0 && g_overlap_force.load(std::memory_order_relaxed) <= 0 && g_hold_rests && b.profiling < 2;
    // (the plan is the BATCH's: with a rectification set its frames have the view's size b.W x b.H, not the call's width x height)
    if (bursts && gated && device_plan_capacity(ctx->hints, ctx->max_darts, b.planes, b.W, b.H) != 0) {
        if (int erc = enqueue_front(ctx, b, true)) return erc;
        (void)hipStreamQuery(ctx->stream);
        std::lock_guard<std::mutex> lk(g_defer_mu);
        b.active = true;
        ctx->rest_held = true; ctx->held_rc = 0;
        ctx->stepping = A3_STEP_HELD;   // (until the chain goes out: flush_held_locked says how)
        g_held.push_back(ctx);
        return A3_OK;
    }
    bool any_held = false;
    if (bursts) {
        std::lock_guard<std::mutex> lk(g_defer_mu);
        for (a3_ctx* o : g_held) any_held |= (o != ctx && o->device == ctx->device);
    }
    if (any_held) {   // the last member: threshold kernel, then the held chains of the others behind it, then this batch's own
        // A last member that needs a host-side plan cannot be split (enqueue_front refuses to hold it): the others are then released
        // ungated, ahead of its whole batch.
        const bool planned = device_plan_capacity(ctx->hints, ctx->max_darts, b.planes, b.W, b.H) != 0;
        if (planned) { if (int erc = enqueue_front(ctx, b, true)) return erc; }
        uint32_t released = 0;
        {
            std::lock_guard<std::mutex> lk(g_defer_mu);
            const std::vector<a3_ctx*> list = g_held;   // (flush edits g_held)
            for (a3_ctx* o : list)
                if (o != ctx && o->device == ctx->device) { (void)flush_held_locked(o, planned ? ctx->ev_k1_done : nullptr, true); released++; }   // (a failure is o's: its collect reports it)
        }
        const int erc = planned ? enqueue_chain(ctx, b, false) : enqueue_batch(ctx);
        ctx->stepping = A3_STEP_BURST_LAST; ctx->released_others = released;
        return erc;
    }
    ctx->allow_defer = true;    // (a synchronous call, or a re-run, enqueues both halves at once)
    const int erc = enqueue_batch(ctx);
    ctx->allow_defer = false;
    return erc;
}

static int collect_common(a3_ctx* ctx, a3_marker* out, a3_pose* poses, size_t out_cap, uint32_t* per_frame_count, size_t* out_n) {
    *out_n = 0;
    if (ctx->pending_trivial) {
        ctx->pending_trivial = false;
        finish_trivial(ctx, per_frame_count);
        return A3_OK;
    }
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    int rc = finish_batch(ctx, out, poses, out_cap, per_frame_count, out_n);
    const uint32_t stepping = ctx->stepping;   // how the SUBMITTED batch was stepped (a re-run below is a synchronous call of its own)
    // the device asked for a re-run (pool growth, more passes, host-side plan): do it synchronously, into the collect's buffers
    if (rc == 1) { ctx->reruns++; ctx->batch.out_cap = out_cap; rc = run_batch_with_retries(ctx, out, poses, out_cap, per_frame_count, out_n); }
    ctx->stepping = stepping;
    return rc;
}

int a3_detect_batch_submit(a3_ctx* ctx, const void* pixels, int memory, int fmt, uint32_t width, uint32_t height, size_t row_stride,
                           size_t frame_stride, uint32_t n_frames, size_t out_cap) {
    if (!ctx) return A3_ERR_INVALID;
    return submit_common(ctx, pixels, memory, fmt, width, height, row_stride, frame_stride, n_frames, out_cap, false, 0.0f, nullptr);
}

int a3_detect_batch_collect(a3_ctx* ctx, a3_marker* out, size_t out_cap, uint32_t* per_frame_count, size_t* out_n) {
    if (!ctx) return A3_ERR_INVALID;
    if (!out_n || (!out && out_cap)) return fail(ctx, A3_ERR_INVALID, "a3_detect_batch_collect: null output");
    return collect_common(ctx, out, nullptr, out_cap, per_frame_count, out_n);
}

// detect + pose in two halves (BASELINE config 5 pipelined like config 2): the pose request travels with the submitted batch
int a3_detect_batch_pose_submit(a3_ctx* ctx, const void* pixels, int memory, int fmt, uint32_t width, uint32_t height, size_t row_stride,
                                size_t frame_stride, uint32_t n_frames, float marker_size_mm, const a3_intrinsics* intr, size_t out_cap) {
    if (!ctx) return A3_ERR_INVALID;
    return submit_common(ctx, pixels, memory, fmt, width, height, row_stride, frame_stride, n_frames, out_cap, true, marker_size_mm, intr);
}

int a3_detect_batch_pose_collect(a3_ctx* ctx, a3_marker* out, a3_pose* poses, size_t out_cap, uint32_t* per_frame_count, size_t* out_n) {
    if (!ctx) return A3_ERR_INVALID;
    if (!out_n || (!out && out_cap) || (!poses && out_cap)) return fail(ctx, A3_ERR_INVALID, "a3_detect_batch_pose_collect: null output");
    if (!ctx->pending_trivial && ctx->batch.active && !ctx->batch.want_pose)
        return fail(ctx, A3_ERR_INVALID, "a3_detect_batch_pose_collect: the submitted batch was not an a3_detect_batch_pose_submit call");
    return collect_common(ctx, out, poses, out_cap, per_frame_count, out_n);
}

int a3_detect_batch_pose(a3_ctx* ctx, const void* pixels, int memory, int fmt, uint32_t width, uint32_t height, size_t row_stride,
                         size_t frame_stride, uint32_t n_frames, float marker_size_mm, const a3_intrinsics* intr, a3_marker* out,
                         a3_pose* poses, size_t out_cap, uint32_t* per_frame_count, size_t* out_n) {
    if (!ctx || !poses) return A3_ERR_INVALID;
    return detect_common(ctx, pixels, memory, fmt, width, height, row_stride, frame_stride, n_frames, true, marker_size_mm, intr, out, poses,
                         out_cap, per_frame_count, out_n);
}

// Re-runs one contour kernel on the buffers of the last batch (single-chunk batches only) and returns its average device
// time; dbg selects a truncated variant (see the kernels).  The contour graph buffers hold garbage afterwards, which the
// next a3_detect_batch overwrites; nothing reads them in between.
int a3_debug_kernel_time(a3_ctx* ctx, int kernel, int dbg, int reps, float* avg_ms) {
    if (!ctx || !avg_ms || reps <= 0) return A3_ERR_INVALID;
    if (ctx->dbg_chunks != 1 || ctx->dbg_nd == 0) return fail(ctx, A3_ERR_INVALID, "needs a preceding single-chunk batch");
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    hipStream_t st = ctx->stream;
    // the events are owned by a guard: every early return below (A3_HIP) destroys them
    struct EventPair {
        hipEvent_t e0 = nullptr, e1 = nullptr;
        ~EventPair() { if (e0) (void)hipEventDestroy(e0); if (e1) (void)hipEventDestroy(e1); }
    } evp;
    A3_HIP(hipEventCreate(&evp.e0)); A3_HIP(hipEventCreate(&evp.e1));
    const hipEvent_t e0 = evp.e0, e1 = evp.e1;
    double total = 0.0;
    // the product path's launches (contour_chunk, decode_stage) on the whole last batch as one chunk; only what the probe sets differs
    ContourChunk cc = contour_chunk(ctx);
    cc.n_frames = ctx->dbg_frames; cc.n_darts = ctx->dbg_nd; cc.frame_base = ctx->frame_base.as<uint32_t>(); cc.ctr = ctx->counters;
    for (int r = 0; r < reps; r++) {
        A3_HIP(hipMemsetAsync(cc.leader_count, 0, sizeof(BatchScratch::leader_count) + sizeof(BatchScratch::entry_count), st));
        A3_HIP(hipEventRecord(e0, st));
        if (kernel == 0) {
            A3_HIP(hipMemsetAsync(ctx->frame_darts.p, 0, (size_t)ctx->frames * 8, st));
            A3_HIP(launch_dart_count(st, {.bits = cc.bits, .W = cc.W, .H = cc.H, .n_frames = ctx->frames, .frame_darts = ctx->frame_darts.as<unsigned long long>(),
                                          .tile_darts = ctx->tile_darts.as<uint32_t>()}));
        } else if (kernel == 1) {
            cc.dbg = dbg ? dbg : 5;
            A3_HIP(launch_dart_build(st, cc));
        } else if (kernel == 2) {
            cc.dbg = dbg ? dbg : 11;
            A3_HIP(launch_rank_cycles(st, cc));
        } else if (kernel == 3 || kernel == 4) {
            if (kernel == 4) {   // COLD frames, as the pipeline meets them (1.6 GB went through the threshold kernel, the contour stage's buffers since):
                                 // half a gigabyte of the pixel-base plane is overwritten first (garbage after a batch anyway), outside the timed span
                const size_t sweep = std::min<size_t>(ctx->pix_base.cap & ~(size_t)15, (size_t)512 << 20);
                if (sweep) A3_HIP(launch_zero(st, ctx->pix_base.p, sweep));
                A3_HIP(hipEventRecord(e0, st));
            }
            // dbg >= 0: k_projection + k_decode, dbg < 0: k_decode alone; |dbg| 1..5 selects the truncated variant (5 and 0: the whole kernel)
            DecodeStage dec = decode_stage(ctx);
            dec.src = ctx->dbg_src; dec.W = cc.W; dec.H = cc.H; dec.max_cand = ctx->cand_stride; dec.few = ctx->frames_merged <= 64u; dec.grid_blocks = 4096;
            dec.per_frame = nullptr;
            dec.projection = dbg >= 0; dec.variant = dbg < 0 ? -dbg : dbg;
            A3_HIP(launch_decode(st, dec));
        } else if (kernel == 6) {   // the refinement kernel of method dbg (A3_REFINE_SUBPIX / A3_REFINE_EDGES) over the last batch's marker list
            const Batch& b = ctx->batch;
            if (!b.refined || b.plane == Batch::Plane::Reduced || (dbg != A3_REFINE_SUBPIX && dbg != A3_REFINE_EDGES))
                return fail(ctx, A3_ERR_INVALID, "kernel 6: needs a preceding unreduced batch with corner refinement, and dbg = the method to time");
            a3_refine_config rc = b.refine;
            rc.method = (uint32_t)dbg;
            const RefineLaunch rl{.src = ctx->dbg_src, .W = (uint32_t)cc.W, .H = (uint32_t)cc.H, .markers = ctx->markers_ptr, .n_dev = &ctx->head->marker_total,
                                  .n = b.marker_cap, .params = refine_params_for(ctx, rc), .out = ctx->refined_buf.as<float>()};
            A3_HIP(dbg == A3_REFINE_EDGES ? launch_refine_edges(st, rl) : launch_refine_corners(st, rl));
        } else return fail(ctx, A3_ERR_INVALID, "kernel: 0 dart_count, 1 dart_assign, 2 local_contract, 3 decode, 4 decode on cold frames, 6 corner refinement");
        A3_HIP(hipEventRecord(e1, st));
        A3_HIP(hipStreamSynchronize(ctx->stream));
        float ms = 0;
        A3_HIP(hipEventElapsedTime(&ms, e0, e1));
        total += ms;
    }
    *avg_ms = (float)(total / reps);
    return A3_OK;
}

// internal (a3_internal.h): where a submitted batch's decode stage is released (0 not deferred, 1 behind the next batch's
// threshold kernel, 2 behind its k_local_contract); process-wide, for A/B measurements
int a3_debug_set_overlap(int mode) {   // -1: the library decides per batch (default); 0, 1, 2: forced mode
    if (mode < -1 || mode > 2) return A3_ERR_INVALID;
    std::lock_guard<std::mutex> lk(g_defer_mu);
    if (!g_held.empty() || !g_deferred.empty()) return A3_ERR_INVALID;   // batches in flight were submitted under the old mode: collect them first
    g_overlap_force.store(mode, std::memory_order_relaxed);
    return A3_OK;
}

// a kernel of `workgroups` x `threads` that stays resident for `usec` microseconds on `hip_stream` (stand-in for a collective's
// channel kernels while only one GPU is at hand); returns at once
int a3_debug_spin(void* hip_stream, int workgroups, int threads, int usec) {
    if (workgroups < 1 || workgroups > 1024 || threads < 64 || threads > 512 || threads % 64 || usec < 1 || usec > 100000) return A3_ERR_INVALID;
    static uint32_t* sink = nullptr;
    static std::mutex mu;
    {
        std::lock_guard<std::mutex> lk(mu);
        if (!sink) {
            if (hipMalloc(&sink, 4096 * 4) != hipSuccess) return A3_ERR_HIP;
            if (hipMemset(sink, 0, 4096 * 4) != hipSuccess) return A3_ERR_HIP;
        }
    }
    return launch_spin(reinterpret_cast<hipStream_t>(hip_stream), workgroups, threads, usec, sink) == hipSuccess ? A3_OK : A3_ERR_HIP;
}

// always 0: the library has a single build (see a3_internal.h)
int a3_debug_build_flags(void) { return 0; }

// the threshold kernel alone on the context's stream, asynchronously (buffers of a preceding batch of the same shape are re-used)
int a3_debug_launch_threshold(a3_ctx* ctx, const void* pixels_device, int fmt, uint32_t width, uint32_t height, uint32_t n_frames) {
    if (!ctx || !pixels_device || n_frames == 0) return A3_ERR_INVALID;
    A3_HIP(hipSetDevice(ctx->device));
    if (int rc = need_stream(ctx)) return rc;
    if (!format_valid(fmt) || format_width_error(fmt, width)) return A3_ERR_INVALID;
    const size_t bpp = format_bpp(fmt);
    if (threshold_writes_grey_plane(ctx->cfg.threshold_window))
        return fail(ctx, A3_ERR_INVALID, "a3_debug_launch_threshold: this threshold_window / frame layout takes the separable path, which needs a grey plane");
    A3_HIP(ctx->bin.ensure((size_t)words_per_row(width) * 8 * height * n_frames));
    A3_HIP(launch_grey_threshold(ctx->stream, {.pixels = reinterpret_cast<const uint8_t*>(pixels_device), .fmt = fmt, .row_stride = (size_t)width * bpp,
                                               .frame_stride = (size_t)width * bpp * height, .W = (int)width, .H = (int)height, .n = n_frames,
                                               .radius = ctx->cfg.threshold_window, .bits = ctx->bin.as<uint64_t>()}));
    return A3_OK;
}

int a3_debug_set_hold(int on) {
    std::lock_guard<std::mutex> lk(g_defer_mu);
    if (!g_held.empty()) return A3_ERR_INVALID;   // (chains held under the old setting: collect them first)
    g_hold_rests = on != 0;
    return A3_OK;
}

int a3_debug_set_jump_rounds(int rounds) {
    if (rounds < 0 || rounds > 32) return A3_ERR_INVALID;
    g_jump_rounds_cap.store(rounds, std::memory_order_relaxed);
    return A3_OK;
}

int a3_synth_render(int device, void* hip_stream, const a3_synth_frame* frames, uint32_t n_frames, const a3_synth_marker* markers,
                    uint32_t n_markers, uint32_t width, uint32_t height, int paper, float black, float white, int supersample,
                    void* out_rgb_device, size_t row_stride, size_t frame_stride) {
    if (!frames || !out_rgb_device || (n_markers && !markers) || supersample < 1 || supersample > 8) return A3_ERR_INVALID;
    if (n_frames == 0 || width == 0 || height == 0) return A3_OK;
    if (row_stride == 0) row_stride = (size_t)width * 3;
    if (frame_stride == 0) frame_stride = row_stride * height;
    if (row_stride < (size_t)width * 3 || frame_stride < row_stride * (height - 1) + (size_t)width * 3 || height > 65535 || n_frames > 65535)
        return A3_ERR_INVALID;
    for (uint32_t f = 0; f < n_frames; f++)
        if ((uint64_t)frames[f].first_marker + frames[f].n_markers > n_markers) return A3_ERR_INVALID;
    for (uint32_t m = 0; m < n_markers; m++)
        if (markers[m].n == 0 || markers[m].n > 11) return A3_ERR_INVALID;   // 121 cells in two words (CHILITAGS: 10 x 10)
    if (hipSetDevice(device) != hipSuccess) return A3_ERR_NO_DEVICE;
    hipStream_t st = reinterpret_cast<hipStream_t>(hip_stream);
    a3_synth_frame* d_frames = nullptr; a3_synth_marker* d_markers = nullptr;
    hipError_t e = hipMalloc(&d_frames, sizeof(a3_synth_frame) * n_frames);
    if (e == hipSuccess && n_markers) e = hipMalloc(&d_markers, sizeof(a3_synth_marker) * n_markers);
    if (e == hipSuccess) e = hipMemcpyAsync(d_frames, frames, sizeof(a3_synth_frame) * n_frames, hipMemcpyHostToDevice, st);
    if (e == hipSuccess && n_markers) e = hipMemcpyAsync(d_markers, markers, sizeof(a3_synth_marker) * n_markers, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = launch_synth_render(st, {.frames = d_frames, .n_frames = n_frames, .markers = d_markers, .W = width, .H = height, .paper = paper,
                                                      .black = black, .white = white, .supersample = supersample,
                                                      .out = reinterpret_cast<uint8_t*>(out_rgb_device), .row_stride = row_stride, .frame_stride = frame_stride});
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (d_frames) (void)hipFree(d_frames);
    if (d_markers) (void)hipFree(d_markers);
    return e == hipSuccess ? A3_OK : A3_ERR_HIP;
}

int a3_get_stats(const a3_ctx* ctx, a3_stats* stats) {
    if (!ctx || !stats) return A3_ERR_INVALID;
    *stats = ctx->stats;
    stats->stepping = ctx->stepping | (std::min(ctx->released_others, 255u) << 8) | (std::min(ctx->reruns, 255u) << 16);
    return A3_OK;
}

static int download_plane(a3_ctx* ctx, const DevBuf& buf, uint32_t frame, uint8_t* dst) {
    if (!ctx || !dst) return A3_ERR_INVALID;
    if (frame >= ctx->frames_merged) return fail(ctx, A3_ERR_INVALID, "frame index outside the last batch");
    const size_t npx = (size_t)ctx->W * ctx->H;
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    A3_HIP(hipMemcpy(dst, buf.as<uint8_t>() + npx * frame, npx, hipMemcpyDeviceToHost));
    return A3_OK;
}

int a3_download_grey(a3_ctx* ctx, uint32_t frame, uint8_t* dst) {
    if (!ctx) return A3_ERR_INVALID;
    if (!ctx->grey_valid) return fail(ctx, A3_ERR_INVALID, "the grey plane is only kept when debug taps are enabled before the batch");
    return download_plane(ctx, ctx->grey, frame, dst);
}
int a3_download_thresholded(a3_ctx* ctx, uint32_t frame, uint8_t* dst) {
    if (!ctx || !dst) return A3_ERR_INVALID;
    if (frame >= ctx->frames) return fail(ctx, A3_ERR_INVALID, "frame index outside the last batch");
    const size_t npx = (size_t)ctx->W * ctx->H, wpf = (size_t)words_per_row(ctx->W) * ctx->H;
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    A3_HIP(ctx->tmp_a.ensure(npx));
    A3_HIP(launch_unpack_bits(ctx->stream, ctx->bin.as<uint64_t>() + wpf * frame, (int)ctx->W, (int)ctx->H, ctx->tmp_a.as<uint8_t>()));
    A3_HIP(hipStreamSynchronize(ctx->stream));
    A3_HIP(hipMemcpy(dst, ctx->tmp_a.p, npx, hipMemcpyDeviceToHost));
    return A3_OK;
}

int a3_candidate_count(a3_ctx* ctx, uint32_t frame, uint32_t* n_pre, uint32_t* n_final) {
    if (!ctx) return A3_ERR_INVALID;
    if (frame >= ctx->frames_merged) return fail(ctx, A3_ERR_INVALID, "frame index outside the last batch");
    if (ctx->counts_valid && frame < ctx->h_cand_fin.size()) {   // the tapped batch brought them along
        if (n_pre) *n_pre = ctx->h_cand_pre[frame];
        if (n_final) *n_final = ctx->h_cand_fin[frame];
        return A3_OK;
    }
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    uint32_t a = 0, b = 0;
    A3_HIP(hipMemcpy(&a, ctx->pre_count + frame, 4, hipMemcpyDeviceToHost));
    A3_HIP(hipMemcpy(&b, ctx->fin_count.as<uint32_t>() + frame, 4, hipMemcpyDeviceToHost));
    if (n_pre) *n_pre = std::min(a, ctx->cand_stride);
    if (n_final) *n_final = b;
    return A3_OK;
}

int a3_download_candidates(a3_ctx* ctx, uint32_t frame, int before_discard, uint32_t* dst_xy, size_t cap_quads) {
    if (!ctx || !dst_xy) return A3_ERR_INVALID;
    uint32_t a = 0, b = 0;
    if (int rc = a3_candidate_count(ctx, frame, &a, &b)) return rc;
    const uint32_t cnt = before_discard ? a : b;
    if (cnt > cap_quads) return fail(ctx, A3_ERR_CAPACITY, "cap_quads too small");
    std::vector<uint16_t> tmp((size_t)cnt * 8);
    const DevBuf& src = before_discard ? ctx->pre_xy : ctx->fin_xy;
    if (cnt) A3_HIP(hipMemcpy(tmp.data(), src.as<uint16_t>() + (size_t)frame * ctx->cand_stride * 8, tmp.size() * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < tmp.size(); i++) dst_xy[i] = tmp[i];
    return A3_OK;
}

struct DecodeOutHost { uint64_t code; uint64_t codes[4]; uint32_t id; uint8_t valid, rotation, hamming, hom_ok; int32_t decode_ok; uint32_t patch; };

int a3_download_homographies(a3_ctx* ctx, uint32_t frame, uint8_t* dst, uint8_t* ok, uint64_t* codes4, int32_t* decode_ok, size_t cap) {
    if (!ctx) return A3_ERR_INVALID;
    uint32_t b = 0;
    if (int rc = a3_candidate_count(ctx, frame, nullptr, &b)) return rc;
    if (b > cap) return fail(ctx, A3_ERR_CAPACITY, "cap too small");
    if (sizeof(DecodeOutHost) != decode_out_bytes()) return fail(ctx, A3_ERR_INTERNAL, "DecodeOut layout mismatch");
    if (dst && !ctx->debug_taps) return fail(ctx, A3_ERR_INVALID, "patches are only kept after a3_set_debug_taps(ctx, 1)");
    if (ctx->batch.active) return fail(ctx, A3_ERR_INVALID, "a submitted batch has not been collected");   // (its staging buffer is in use)
    if (b == 0) return A3_OK;
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    const uint32_t S = ctx->cfg.homography_sample_size;
    const size_t S2 = (size_t)S * S, rec_bytes = (size_t)b * sizeof(DecodeOutHost);
    const uint8_t* d_outs = (const uint8_t*)ctx->outs.p + (size_t)frame * ctx->cand_stride * sizeof(DecodeOutHost);
    // One trip: the frame's decode records, and its patches gathered by a kernel into one dense array, land in pinned memory
    // through two copies on the stream and one wait (it was a blocking copy per candidate).
    const size_t flag_off = (rec_bytes + 15) & ~(size_t)15, patch_off = flag_off + 16;
    const size_t total = patch_off + (dst ? (size_t)b * S2 : 0);
    A3_HIP(ctx->tmp_a.ensure(total));
    uint8_t* d_tmp = ctx->tmp_a.as<uint8_t>();
    unsigned int* d_missing = reinterpret_cast<unsigned int*>(d_tmp + flag_off);
    hipStream_t st = ctx->stream;
    if (dst) {
        A3_HIP(hipMemsetAsync(d_missing, 0, 4, st));
        A3_HIP(launch_gather_patches(st, d_outs, b, ctx->patches.as<uint8_t>(), ctx->patch_cap, (uint32_t)S2, d_tmp + patch_off, d_missing));
    }
    if (int rc = ensure_pinned(ctx, total + (1 << 16))) return rc;
    uint8_t* hp = (uint8_t*)ctx->pinned;
    A3_HIP(hipMemcpyAsync(hp, d_outs, rec_bytes, hipMemcpyDeviceToHost, st));
    if (dst) A3_HIP(hipMemcpyAsync(hp + flag_off, d_tmp + flag_off, 16 + (size_t)b * S2, hipMemcpyDeviceToHost, st));
    A3_HIP(wait_stream(st));
    const DecodeOutHost* o = reinterpret_cast<const DecodeOutHost*>(hp);
    for (uint32_t k = 0; k < b; k++) {
        if (ok) ok[k] = o[k].hom_ok;
        if (decode_ok) decode_ok[k] = o[k].decode_ok;
        if (codes4) for (int r = 0; r < 4; r++) codes4[4 * k + r] = o[k].codes[r];
    }
    if (dst) {
        memcpy(dst, hp + patch_off, (size_t)b * S2);
        if (*reinterpret_cast<const unsigned int*>(hp + flag_off))
            return fail(ctx, A3_ERR_CAPACITY, "the patch tap was full: a candidate's patch was not kept (split the batch: at most 1024 frames per tapped call)");
    }
    return A3_OK;
}

// ---- Detection gather records on the device (multi-GPU) ----
size_t a3_detection_record_bytes(uint32_t max_markers_per_frame, int with_poses) {
    return 8 + (size_t)max_markers_per_frame * (sizeof(a3_marker) + (with_poses ? 2 * sizeof(a3_pose) : 0));
}

int a3_pack_detections(a3_ctx* ctx, uint32_t first_frame_global, uint32_t max_markers_per_frame, int with_poses, void* dst_device, size_t dst_bytes) {
    if (!ctx || !dst_device) return A3_ERR_INVALID;
    if (!ctx->markers_valid) return fail(ctx, A3_ERR_INVALID, "a3_pack_detections: no finished batch on this context");
    if (with_poses && !ctx->side_valid[kSidePoses]) return fail(ctx, A3_ERR_INVALID, "a3_pack_detections: the last batch was not an a3_detect_batch_pose call");
    if (max_markers_per_frame == 0) return fail(ctx, A3_ERR_INVALID, "a3_pack_detections: max_markers_per_frame must be > 0");
    const size_t need = a3_detection_record_bytes(max_markers_per_frame, with_poses) * ctx->last_n;
    if (dst_bytes < need) return fail(ctx, A3_ERR_CAPACITY, "a3_pack_detections: dst_bytes smaller than frames x record size");
    if (reinterpret_cast<uintptr_t>(dst_device) % 4 != 0) return fail(ctx, A3_ERR_INVALID, "a3_pack_detections: dst must be 4-byte aligned");
    // the host already knows the per-frame counts of that batch: refuse before anything is clipped
    if (ctx->last_max_per_frame > max_markers_per_frame) {
        char msg[160];
        snprintf(msg, sizeof msg, "a3_pack_detections: a frame holds %u markers, the record only %u", ctx->last_max_per_frame, max_markers_per_frame);
        return fail(ctx, A3_ERR_CAPACITY, msg);
    }
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    // pack_overflow is the kernel's overflow flag (cannot fire after the host check; kept as the device-side guard)
    A3_HIP(launch_pack_detections(ctx->stream, ctx->markers_ptr, with_poses ? ctx->pose_buf.as<a3_pose>() : nullptr, ctx->per_frame, ctx->last_n,
                                  first_frame_global, max_markers_per_frame, dst_device, &ctx->head->pack_overflow));
    return A3_OK;
}

// ---- find_contours output of the last batch (debug taps; src/aruco.rs:64) ----
namespace {
int fetch_contours(a3_ctx* ctx, uint32_t frame, std::vector<ContourRec>* recs) {
    if (!ctx->contours_valid) return fail(ctx, A3_ERR_INVALID, "contours are only kept for a single-chunk batch run after a3_set_debug_taps(ctx, 1)");
    if (frame >= ctx->frames) return fail(ctx, A3_ERR_INVALID, "frame index outside the last batch");
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    std::vector<ContourRec> all(ctx->tap_contours);
    if (!all.empty()) A3_HIP(hipMemcpy(all.data(), ctx->contours.p, all.size() * sizeof(ContourRec), hipMemcpyDeviceToHost));
    recs->clear();
    for (const ContourRec& r : all) if (r.frame == frame) recs->push_back(r);
    // the reference's discovery order = ascending start key (2 * raster index of the start pixel, +1 for a hole border)
    std::sort(recs->begin(), recs->end(), [](const ContourRec& a, const ContourRec& b) { return a.start_key < b.start_key; });
    return A3_OK;
}
}  // namespace

int a3_contour_count(a3_ctx* ctx, uint32_t frame, uint32_t* n_contours, uint64_t* n_points) {
    if (!ctx) return A3_ERR_INVALID;
    std::vector<ContourRec> recs;
    if (int rc = fetch_contours(ctx, frame, &recs)) return rc;
    uint64_t pts = 0;
    for (const ContourRec& r : recs) pts += r.n;
    if (n_contours) *n_contours = (uint32_t)recs.size();
    if (n_points) *n_points = pts;
    return A3_OK;
}

int a3_download_contours(a3_ctx* ctx, uint32_t frame, uint32_t* start_keys, uint32_t* lengths, uint32_t* points_xy, size_t cap_contours,
                         size_t cap_points) {
    if (!ctx || !start_keys || !lengths || !points_xy) return A3_ERR_INVALID;
    std::vector<ContourRec> recs;
    if (int rc = fetch_contours(ctx, frame, &recs)) return rc;
    uint64_t pts = 0;
    for (const ContourRec& r : recs) pts += r.n;
    if (recs.size() > cap_contours || pts > cap_points) return fail(ctx, A3_ERR_CAPACITY, "a3_download_contours: caps too small");
    std::vector<uint32_t> pool(ctx->tap_points);
    if (!pool.empty()) A3_HIP(hipMemcpy(pool.data(), ctx->points.p, pool.size() * 4, hipMemcpyDeviceToHost));
    size_t o = 0;
    for (size_t i = 0; i < recs.size(); i++) {
        start_keys[i] = recs[i].start_key;
        lengths[i] = recs[i].n;
        for (uint32_t k = 0; k < recs[i].n; k++) {
            const uint32_t p = pool[(size_t)recs[i].point_base + k];
            points_xy[2 * o] = p & 0xFFFFu; points_xy[2 * o + 1] = p >> 16;
            o++;
        }
    }
    return A3_OK;
}

// ---- internal (a3_internal.h): the small helpers of src/aruco.rs run on their own, for the reference's vectors ----
int a3_debug_clockwise(a3_ctx* ctx, const int32_t* quads_xy, size_t n, int32_t* out_xy) {
    if (!ctx || !quads_xy || !out_xy) return A3_ERR_INVALID;
    if (n == 0) return A3_OK;
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    A3_HIP(ctx->tmp_a.ensure(n * 32)); A3_HIP(ctx->tmp_c.ensure(n * 32));
    A3_HIP(hipMemcpyAsync(ctx->tmp_a.p, quads_xy, n * 32, hipMemcpyHostToDevice, ctx->stream));
    A3_HIP(launch_debug_clockwise(ctx->stream, ctx->tmp_a.as<int32_t>(), (uint32_t)n, ctx->tmp_c.as<int32_t>()));
    A3_HIP(hipMemcpyAsync(out_xy, ctx->tmp_c.p, n * 32, hipMemcpyDeviceToHost, ctx->stream));
    A3_HIP(hipStreamSynchronize(ctx->stream));
    return A3_OK;
}

int a3_debug_rotate_bits(a3_ctx* ctx, const uint8_t* bits, uint32_t n, uint32_t times, uint8_t* out) {
    if (!ctx || !bits || !out || n == 0 || n > 16) return A3_ERR_INVALID;
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    A3_HIP(ctx->tmp_a.ensure(256)); A3_HIP(ctx->tmp_c.ensure(256));
    A3_HIP(hipMemcpyAsync(ctx->tmp_a.p, bits, (size_t)n * n, hipMemcpyHostToDevice, ctx->stream));
    A3_HIP(launch_debug_rotate_bits(ctx->stream, ctx->tmp_a.as<uint8_t>(), n, times & 3u, ctx->tmp_c.as<uint8_t>()));
    A3_HIP(hipMemcpyAsync(out, ctx->tmp_c.p, (size_t)n * n, hipMemcpyDeviceToHost, ctx->stream));
    A3_HIP(hipStreamSynchronize(ctx->stream));
    return A3_OK;
}

// quads in the order given (= the reference's candidate order) through k_frame_candidates' discard_too_near
int a3_debug_discard_too_near(a3_ctx* ctx, const uint32_t* quads_xy, size_t n, float min_distance, uint32_t* out_xy, size_t* n_out) {
    if (!ctx || !quads_xy || !out_xy || !n_out) return A3_ERR_INVALID;
    *n_out = 0;
    if (n == 0) return A3_OK;
    constexpr uint32_t kMaxCand = kMaxCandDefault;
    if (n > kMaxCand) return fail(ctx, A3_ERR_CAPACITY, "a3_debug_discard_too_near: at most 1024 quads");
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    std::vector<CandRec> h(n);
    for (size_t i = 0; i < n; i++) {
        h[i].start_key = (uint32_t)i;   // the given order
        for (int k = 0; k < 8; k++) {
            if (quads_xy[8 * i + k] > 65535u) return fail(ctx, A3_ERR_INVALID, "coordinates above 65535");
            h[i].xy[k] = (uint16_t)quads_xy[8 * i + k];
        }
    }
    A3_HIP(ctx->tmp_a.ensure(kMaxCand * sizeof(CandRec)));
    A3_HIP(ctx->tmp_b.ensure(kMaxCand * 16 * 2));          // pre_xy | fin_xy
    A3_HIP(ctx->tmp_c.ensure(kMaxCand * 4 + 64));          // work list | cand_count, fin_count, work_count
    uint32_t* small = ctx->tmp_c.as<uint32_t>() + kMaxCand;
    const uint32_t init[3] = {(uint32_t)n, 0u, 0u};
    A3_HIP(hipMemcpyAsync(ctx->tmp_a.p, h.data(), n * sizeof(CandRec), hipMemcpyHostToDevice, ctx->stream));
    A3_HIP(hipMemcpyAsync(small, init, sizeof init, hipMemcpyHostToDevice, ctx->stream));
    uint16_t* pre = ctx->tmp_b.as<uint16_t>(); uint16_t* fin = pre + kMaxCand * 8;
    A3_HIP(launch_frame_candidates(ctx->stream, {.n_frames = 1, .max_cand = kMaxCand, .cands = ctx->tmp_a.as<CandRec>(), .cand_count = small,
                                                 .min_distance = min_distance, .pre_xy = pre, .fin_xy = fin, .fin_count = small + 1,
                                                 .work = ctx->tmp_c.as<uint32_t>(), .work_count = small + 2}));
    uint32_t cnt = 0;
    A3_HIP(hipMemcpyAsync(&cnt, small + 1, 4, hipMemcpyDeviceToHost, ctx->stream));
    A3_HIP(hipStreamSynchronize(ctx->stream));
    std::vector<uint16_t> o((size_t)cnt * 8);
    if (cnt) A3_HIP(hipMemcpy(o.data(), fin, o.size() * 2, hipMemcpyDeviceToHost));
    for (size_t i = 0; i < o.size(); i++) out_xy[i] = o[i];
    *n_out = cnt;
    return A3_OK;
}

// The host path of a3_debug_frame_candidates (K == 1: `plane` is "frame", no merged_count, no err_flags) and a3_debug_merge_candidates
// (K = 2..4): one call of launch_frame_candidates or launch_merge_candidates, as the pipeline makes it, on hand-made tables of plane_cand
// slots per plane -- any frame count, any table size, keys as given -- on buffers of its own (freed on return: nothing of the context's
// changes size, so a batch afterwards runs what it would have run).  Every device buffer is filled with 0xFF first, so what the kernel
// left alone comes back as 0xFF.  The callers have checked their arguments; `who` names the caller in what is refused here.
static int debug_candidates(a3_ctx* ctx, const char* who, const char* plane, uint32_t n_frames, uint32_t K, uint32_t plane_cand,
                            const uint32_t* cand_count, const a3_debug_cand* records, float min_distance, uint32_t S, uint16_t* pre_xy,
                            uint16_t* fin_xy, uint32_t* fin_count, uint32_t* work, uint32_t* work_count, void* proj,
                            uint32_t* merged_count /*nullable*/, uint32_t* err_flags /*nullable*/) {
    static_assert(sizeof(a3_debug_cand) == sizeof(CandRec) && sizeof(CandRec) == 20, "a3_debug_cand is a CandRec");
    const size_t planes = (size_t)n_frames * K, plane_slots = planes * plane_cand;
    const uint32_t merged = merged_cand_capacity(K, plane_cand);   // (K == 1: plane_cand)
    const size_t slots = (size_t)n_frames * merged;
    std::vector<CandRec> h(plane_slots);
    memset(h.data(), 0xFF, plane_slots * sizeof(CandRec));
    size_t given = 0;
    std::vector<uint32_t> keys;
    for (size_t p = 0; p < planes; p++) {
        const uint32_t c = std::min(cand_count[p], plane_cand);
        if (c && !records) return fail(ctx, A3_ERR_INVALID, (std::string(who) + ": a NULL argument").c_str());
        keys.resize(c);
        for (uint32_t i = 0; i < c; i++) {
            memcpy(&h[p * plane_cand + i], &records[given + i], sizeof(CandRec));
            keys[i] = records[given + i].start_key;
        }
        std::sort(keys.begin(), keys.end());
        if (std::adjacent_find(keys.begin(), keys.end()) != keys.end())
            return fail(ctx, A3_ERR_INVALID, (std::string(who) + ": a " + plane + "'s start keys must be unique").c_str());
        given += c;
    }
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    struct Own : DevBuf { ~Own() { release(); } } d_cands, d_cnt, d_pre, d_fin, d_work, d_proj, d_big;
    const bool big = merged > frame_cand_lds_slots();
    const size_t proj_bytes = S ? slots * proj_rec_bytes() : 0;
    A3_HIP(d_cands.ensure(plane_slots * sizeof(CandRec)));
    A3_HIP(d_cnt.ensure((planes + (size_t)2 * n_frames + 2) * 4));   // cand_count | fin_count | merged_count | work_count | err_flags
    A3_HIP(d_pre.ensure(slots * 16)); A3_HIP(d_fin.ensure(slots * 16)); A3_HIP(d_work.ensure(slots * 4));
    if (S) A3_HIP(d_proj.ensure(proj_bytes));
    if (big) A3_HIP(d_big.ensure(slots * 4));
    uint32_t* cnt = d_cnt.as<uint32_t>();
    uint32_t* d_fin_count = cnt + planes, * d_merged = d_fin_count + n_frames, * d_work_count = d_merged + n_frames, * d_err = d_work_count + 1;
    hipStream_t st = ctx->stream;
    A3_HIP(hipMemcpyAsync(d_cands.p, h.data(), plane_slots * sizeof(CandRec), hipMemcpyHostToDevice, st));
    A3_HIP(hipMemcpyAsync(cnt, cand_count, planes * 4, hipMemcpyHostToDevice, st));
    A3_HIP(hipMemsetAsync(d_fin_count, 0xFF, (size_t)2 * n_frames * 4, st));
    A3_HIP(hipMemsetAsync(d_work_count, 0, 8, st));
    A3_HIP(hipMemsetAsync(d_pre.p, 0xFF, slots * 16, st)); A3_HIP(hipMemsetAsync(d_fin.p, 0xFF, slots * 16, st));
    A3_HIP(hipMemsetAsync(d_work.p, 0xFF, slots * 4, st));
    if (S) A3_HIP(hipMemsetAsync(d_proj.p, 0xFF, proj_bytes, st));
    if (big) A3_HIP(hipMemsetAsync(d_big.p, 0xFF, slots * 4, st));
    DecodeStage dec;
    dec.n_frames = n_frames; dec.max_cand = merged; dec.cands = d_cands.as<CandRec>(); dec.cand_count = cnt; dec.min_distance = min_distance;
    dec.pre_xy = d_pre.as<uint16_t>(); dec.fin_xy = d_fin.as<uint16_t>(); dec.fin_count = d_fin_count; dec.work = d_work.as<uint32_t>();
    dec.work_count = d_work_count; dec.S = S; dec.proj = S ? d_proj.p : nullptr; dec.big_scratch = big ? d_big.as<float>() : nullptr;
    if (K > 1) {
        dec.windows = K; dec.plane_cand = plane_cand; dec.merged_count = d_merged; dec.err_flags = d_err;
        A3_HIP(launch_merge_candidates(st, dec));
    } else {
        A3_HIP(launch_frame_candidates(st, dec));
    }
    A3_HIP(hipMemcpyAsync(pre_xy, d_pre.p, slots * 16, hipMemcpyDeviceToHost, st));
    A3_HIP(hipMemcpyAsync(fin_xy, d_fin.p, slots * 16, hipMemcpyDeviceToHost, st));
    A3_HIP(hipMemcpyAsync(fin_count, d_fin_count, (size_t)n_frames * 4, hipMemcpyDeviceToHost, st));
    if (merged_count) A3_HIP(hipMemcpyAsync(merged_count, d_merged, (size_t)n_frames * 4, hipMemcpyDeviceToHost, st));
    A3_HIP(hipMemcpyAsync(work, d_work.p, slots * 4, hipMemcpyDeviceToHost, st));
    A3_HIP(hipMemcpyAsync(work_count, d_work_count, 4, hipMemcpyDeviceToHost, st));
    if (err_flags) A3_HIP(hipMemcpyAsync(err_flags, d_err, 4, hipMemcpyDeviceToHost, st));
    if (S) A3_HIP(hipMemcpyAsync(proj, d_proj.p, proj_bytes, hipMemcpyDeviceToHost, st));
    A3_HIP(hipStreamSynchronize(ctx->stream));
    return A3_OK;
}

// k_frame_candidates as the pipeline launches it: one call of launch_frame_candidates.
int a3_debug_frame_candidates(a3_ctx* ctx, uint32_t n_frames, uint32_t max_cand, const uint32_t* cand_count, const a3_debug_cand* records,
                              float min_distance, uint32_t S, uint16_t* pre_xy, uint16_t* fin_xy, uint32_t* fin_count, uint32_t* work,
                              uint32_t* work_count, void* proj) {
    if (!ctx) return A3_ERR_INVALID;
    if (n_frames == 0) return fail(ctx, A3_ERR_INVALID, "a3_debug_frame_candidates: n_frames must be at least 1");
    if (max_cand == 0 || max_cand > kMaxCandLimit) return fail(ctx, A3_ERR_INVALID, "a3_debug_frame_candidates: max_cand must be in 1..65536");
    if (!cand_count || !pre_xy || !fin_xy || !fin_count || !work || !work_count || (S && !proj))
        return fail(ctx, A3_ERR_INVALID, "a3_debug_frame_candidates: a NULL argument");
    if (proj_rec_bytes() != A3_DEBUG_PROJ_BYTES) return fail(ctx, A3_ERR_INVALID, "a3_debug_frame_candidates: ProjRec is not A3_DEBUG_PROJ_BYTES long");
    if ((size_t)n_frames * max_cand > ((size_t)1 << 26)) return fail(ctx, A3_ERR_LIMIT, "a3_debug_frame_candidates: more than 2^26 slots");
    return debug_candidates(ctx, "a3_debug_frame_candidates", "frame", n_frames, 1, max_cand, cand_count, records, min_distance, S, pre_xy, fin_xy,
                            fin_count, work, work_count, proj, nullptr, nullptr);
}

// k_merge_candidates as the pipeline launches it (a3_set_threshold_windows): one call of launch_merge_candidates on per-plane tables.
int a3_debug_merge_candidates(a3_ctx* ctx, uint32_t n_frames, uint32_t n_windows, uint32_t plane_cand, const uint32_t* cand_count,
                              const a3_debug_cand* records, float min_distance, uint32_t S, uint16_t* pre_xy, uint16_t* fin_xy,
                              uint32_t* fin_count, uint32_t* work, uint32_t* work_count, void* proj, uint32_t* merged_count, uint32_t* err_flags) {
    if (!ctx) return A3_ERR_INVALID;
    if (n_frames == 0 || n_windows < 2 || n_windows > A3_MAX_THRESHOLD_WINDOWS) return fail(ctx, A3_ERR_INVALID, "a3_debug_merge_candidates: n_frames >= 1 and 2..4 windows");
    if (plane_cand == 0 || plane_cand > kMaxCandLimit) return fail(ctx, A3_ERR_INVALID, "a3_debug_merge_candidates: plane_cand must be in 1..65536");
    if (!cand_count || !pre_xy || !fin_xy || !fin_count || !work || !work_count || !merged_count || !err_flags || (S && !proj))
        return fail(ctx, A3_ERR_INVALID, "a3_debug_merge_candidates: a NULL argument");
    if ((size_t)n_frames * n_windows * plane_cand > ((size_t)1 << 26)) return fail(ctx, A3_ERR_LIMIT, "a3_debug_merge_candidates: more than 2^26 slots");
    return debug_candidates(ctx, "a3_debug_merge_candidates", "plane", n_frames, n_windows, plane_cand, cand_count, records, min_distance, S, pre_xy,
                            fin_xy, fin_count, work, work_count, proj, merged_count, err_flags);
}

// k_contour_quads as the pipeline launches it -- ONE call of launch_contour_quads with a ContourChunk filled from the arguments -- on a
// hand-made contour table and point pool, on buffers of its own (freed on return: nothing of the context's changes).  Whatever the
// pipeline could never hand the kernel is refused here, because the kernel trusts its tables: it checks no index.
int a3_debug_contour_quads(a3_ctx* ctx, uint32_t width, uint32_t height, uint32_t n_darts, double eps_factor, uint32_t min_edge_length,
                           uint32_t first_frame, uint32_t n_frames, uint32_t max_cand, uint32_t max_contours, uint32_t ctr_contours,
                           uint32_t ctr_err_flags, const a3_debug_contour* records, uint32_t n_records, const uint32_t* points, size_t n_points,
                           uint32_t* cand_count, a3_debug_cand* cands, uint32_t* err_flags) {
    static_assert(sizeof(a3_debug_contour) == sizeof(ContourRec) && sizeof(ContourRec) == 16, "a3_debug_contour is a ContourRec");
    static_assert(sizeof(a3_debug_cand) == sizeof(CandRec), "a3_debug_cand is a CandRec");
    if (!ctx) return A3_ERR_INVALID;
    if (!cand_count || !cands || !err_flags || (n_records && (!records || !points)))
        return fail(ctx, A3_ERR_INVALID, "a3_debug_contour_quads: a NULL argument");
    if (width == 0 || width > 65536u || height == 0 || height > 65536u)
        return fail(ctx, A3_ERR_INVALID, "a3_debug_contour_quads: width and height must be in 1..65536");
    if (n_frames == 0 || n_frames > kMaxChunkFrames || first_frame > kMaxChunkFrames)
        return fail(ctx, A3_ERR_INVALID, "a3_debug_contour_quads: n_frames must be in 1..65536 and first_frame at most 65536");
    if (max_cand == 0 || max_cand > kMaxCandLimit) return fail(ctx, A3_ERR_INVALID, "a3_debug_contour_quads: max_cand must be in 1..65536");
    if (!std::isfinite(eps_factor) || eps_factor < 0.0) return fail(ctx, A3_ERR_INVALID, "a3_debug_contour_quads: eps_factor must be finite and >= 0");
    const size_t frames = (size_t)first_frame + n_frames, slots = frames * max_cand;
    if (slots > ((size_t)1 << 24)) return fail(ctx, A3_ERR_LIMIT, "a3_debug_contour_quads: more than 2^24 slots");
    if (n_points >= ((size_t)1 << 30)) return fail(ctx, A3_ERR_LIMIT, "a3_debug_contour_quads: the point pool must hold fewer than 2^30 points");
    // every record the kernel may read exists -- unless the counters carry the flags on which it reads none
    const bool stale = (ctr_err_flags & (kErrPointPool | kErrContourTable)) != 0;
    if (!stale && std::min(ctr_contours, max_contours) > n_records)
        return fail(ctx, A3_ERR_INVALID, "a3_debug_contour_quads: min(ctr_contours, max_contours) records must be given");
    std::vector<uint64_t> keys(n_records);
    for (uint32_t i = 0; i < n_records; i++) {
        const a3_debug_contour& r = records[i];
        if (r.n == 0) return fail(ctx, A3_ERR_INVALID, "a3_debug_contour_quads: a record with n == 0");
        if ((uint64_t)r.point_base + r.n > n_points) return fail(ctx, A3_ERR_INVALID, "a3_debug_contour_quads: a record's points lie beyond the pool");
        if (r.frame < first_frame || r.frame - first_frame >= n_frames)
            return fail(ctx, A3_ERR_INVALID, "a3_debug_contour_quads: a record's frame lies outside [first_frame, first_frame + n_frames)");
        keys[i] = ((uint64_t)r.frame << 32) | r.start_key;
    }
    std::sort(keys.begin(), keys.end());
    if (std::adjacent_find(keys.begin(), keys.end()) != keys.end())
        return fail(ctx, A3_ERR_INVALID, "a3_debug_contour_quads: a frame's start keys must be unique");
    for (size_t i = 0; i < n_points; i++)
        if ((points[i] & 0xFFFFu) >= width || (points[i] >> 16) >= height)
            return fail(ctx, A3_ERR_INVALID, "a3_debug_contour_quads: a coordinate lies outside width x height");
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    struct Own : DevBuf { ~Own() { release(); } } d_rec, d_pts, d_ctr, d_cands, d_cnt;
    A3_HIP(d_rec.ensure(std::max<size_t>(n_records, 1) * sizeof(ContourRec)));
    A3_HIP(d_pts.ensure(std::max<size_t>(n_points, 1) * 4));
    A3_HIP(d_ctr.ensure(sizeof(DeviceCounters)));
    A3_HIP(d_cands.ensure(slots * sizeof(CandRec)));
    A3_HIP(d_cnt.ensure((frames + 1) * 4));   // cand_count | err_flags
    DeviceCounters hc;
    memset(&hc, 0, sizeof hc);
    hc.contours = ctr_contours; hc.err_flags = ctr_err_flags;
    uint32_t* cnt = d_cnt.as<uint32_t>();
    hipStream_t st = ctx->stream;
    if (n_records) A3_HIP(hipMemcpyAsync(d_rec.p, records, (size_t)n_records * sizeof(ContourRec), hipMemcpyHostToDevice, st));
    if (n_points) A3_HIP(hipMemcpyAsync(d_pts.p, points, n_points * 4, hipMemcpyHostToDevice, st));
    A3_HIP(hipMemcpyAsync(d_ctr.p, &hc, sizeof hc, hipMemcpyHostToDevice, st));
    A3_HIP(hipMemsetAsync(d_cands.p, 0xFF, slots * sizeof(CandRec), st));
    if (first_frame) A3_HIP(hipMemsetAsync(cnt, 0xFF, (size_t)first_frame * 4, st));
    A3_HIP(hipMemsetAsync(cnt + first_frame, 0, ((size_t)n_frames + 1) * 4, st));   // the chunk's counts arrive zeroed, and so does the flag word
    ContourChunk cc;
    cc.first_frame = first_frame; cc.n_frames = n_frames; cc.n_darts = n_darts; cc.ctr = d_ctr.as<DeviceCounters>();
    cc.W = (int)width; cc.H = (int)height; cc.batch_frames = (uint32_t)frames;
    cc.min_edge_length = min_edge_length; cc.eps_factor = eps_factor; cc.contours = d_rec.as<ContourRec>(); cc.points = d_pts.as<uint32_t>();
    cc.max_contours = max_contours; cc.max_points = n_points;
    cc.cands = d_cands.as<CandRec>(); cc.cand_count = cnt; cc.max_cand = max_cand; cc.err_flags = cnt + frames;
    A3_HIP(launch_contour_quads(st, cc));
    A3_HIP(hipMemcpyAsync(cand_count, cnt, frames * 4, hipMemcpyDeviceToHost, st));
    A3_HIP(hipMemcpyAsync(err_flags, cnt + frames, 4, hipMemcpyDeviceToHost, st));
    A3_HIP(hipMemcpyAsync(cands, d_cands.p, slots * sizeof(CandRec), hipMemcpyDeviceToHost, st));
    A3_HIP(hipStreamSynchronize(ctx->stream));
    return A3_OK;
}

int a3_debug_inject_candidates(a3_ctx* ctx, const uint32_t* quads_xy, size_t n) {
    if (!ctx || (!quads_xy && n)) return A3_ERR_INVALID;
    if (ctx->batch.active || ctx->pending_trivial) return fail(ctx, A3_ERR_INVALID, "a3_debug_inject_candidates: a submitted batch has not been collected");
    if (n > kMaxCandDefault) return fail(ctx, A3_ERR_CAPACITY, "a3_debug_inject_candidates: at most 1024 quads");
    ctx->inject.resize(n);
    for (size_t i = 0; i < n; i++) {
        ctx->inject[i].start_key = (uint32_t)i;   // the given order
        for (int k = 0; k < 8; k++) {
            if (quads_xy[8 * i + k] > 65535u) return fail(ctx, A3_ERR_INVALID, "coordinates above 65535");
            ctx->inject[i].xy[k] = (uint16_t)quads_xy[8 * i + k];
        }
    }
    ctx->inject_armed = true;
    return A3_OK;
}

int a3_debug_sample_frames(a3_ctx* ctx, int enabled) {
    if (!ctx) return A3_ERR_INVALID;
    ctx->debug_sample_frames = enabled != 0;
    return A3_OK;
}

// ---- sub-pixel corner refinement (an extension beyond the reference; contract in include/aruco3_hip.h) ----
void a3_default_refine_config(a3_refine_config* cfg) {
    if (!cfg) return;
    cfg->method = A3_REFINE_SUBPIX; cfg->win_half = 5; cfg->relative_win = 0.4f; cfg->max_iterations = 30; cfg->min_shift = 0.01f;
}

static int check_refine_config(a3_ctx* ctx, const a3_refine_config& c) {
    if (c.method != A3_REFINE_NONE && c.method != A3_REFINE_SUBPIX && c.method != A3_REFINE_EDGES) return fail(ctx, A3_ERR_INVALID, "a3_refine_config.method: unknown method");
    if (c.method == A3_REFINE_NONE) return A3_OK;
    if (c.win_half < 1 || c.win_half > 10) return fail(ctx, A3_ERR_INVALID, "a3_refine_config.win_half must be in 1..10");
    if (!(c.relative_win >= 0.0f) || !std::isfinite(c.relative_win)) return fail(ctx, A3_ERR_INVALID, "a3_refine_config.relative_win must be finite and >= 0");
    if (c.max_iterations > 100) return fail(ctx, A3_ERR_INVALID, "a3_refine_config.max_iterations must be at most 100");
    if (!(c.min_shift >= 0.0f) || !std::isfinite(c.min_shift)) return fail(ctx, A3_ERR_INVALID, "a3_refine_config.min_shift must be finite and >= 0");
    return A3_OK;
}

int a3_set_corner_refinement(a3_ctx* ctx, const a3_refine_config* cfg) {
    if (!ctx) return A3_ERR_INVALID;
    a3_refine_config c{};   // NULL: off
    if (cfg) c = *cfg;
    if (int rc = check_refine_config(ctx, c)) return rc;
    if (c.method == A3_REFINE_NONE) c = a3_refine_config{};
    ctx->refine = c;
    return A3_OK;
}

int a3_get_refined_corners(a3_ctx* ctx, float* dst_xy, size_t cap_markers, size_t* n) {
    if (!ctx || !n || (!dst_xy && cap_markers)) return A3_ERR_INVALID;
    *n = 0;
    return get_side(ctx, kSideRefined, dst_xy, cap_markers, n, "a3_get_refined_corners: the last collected batch ran without corner refinement",
                    "a3_get_refined_corners: cap_markers is smaller than the number of markers");
}

int a3_refine_corners(a3_ctx* ctx, const void* pixels, int memory, int fmt, uint32_t width, uint32_t height, size_t row_stride, float* corners_xy,
                      const float* cell_px, size_t n) {
    if (!ctx) return A3_ERR_INVALID;
    if (!corners_xy && n) return fail(ctx, A3_ERR_INVALID, "a3_refine_corners: null corners");
    if (ctx->batch.active || ctx->pending_trivial) return fail(ctx, A3_ERR_INVALID, "a3_refine_corners: a submitted batch has not been collected");
    if (n == 0) return A3_OK;
    if (width == 0 || height == 0) return fail(ctx, A3_ERR_INVALID, "a3_refine_corners: empty image");
    if (n > (1u << 30)) return fail(ctx, A3_ERR_INVALID, "a3_refine_corners: more than 2^30 corners in one call");
    for (size_t k = 0; k < n; k++) {   // (the kernel's tile origin is an int near the corner)
        const float x = corners_xy[2 * k], y = corners_xy[2 * k + 1];
        if (!(x >= -64.0f && x <= (float)width + 64.0f && y >= -64.0f && y <= (float)height + 64.0f))
            return fail(ctx, A3_ERR_INVALID, "a3_refine_corners: a corner is not finite or lies more than 64 px outside the frame");
    }
    a3_refine_config cfg = ctx->refine;
    if (cfg.method == A3_REFINE_NONE) a3_default_refine_config(&cfg);
    const bool edges = cfg.method == A3_REFINE_EDGES;   // quads: four consecutive corners each, cell_px read at the first
    if (edges && n % 4 != 0) return fail(ctx, A3_ERR_INVALID, "a3_refine_corners: method A3_REFINE_EDGES takes quads, n must be a multiple of 4");
    size_t frame_stride = 0;
    const uint8_t* d_pixels = nullptr;
    const int rc = stage_input(ctx, pixels, memory, fmt, width, height, &row_stride, &frame_stride, 1, &d_pixels);
    if (rc != A3_OK) return rc == kNothingToDo ? A3_OK : rc;
    Layout in{ctx->tmp_a, ctx->stream}, out{ctx->tmp_b, ctx->stream};
    const auto s_pts = in.add<float>(2 * n), s_cell = in.add<float>(cell_px ? n : 0), s_out = out.add<float>(2 * n);
    A3_HIP(in.ensure()); A3_HIP(out.ensure());
    A3_HIP(in.upload(s_pts, corners_xy, 2 * n));
    if (cell_px) A3_HIP(in.upload(s_cell, cell_px, n));
    const RefineLaunch rl{.src = {d_pixels, row_stride, frame_stride, fmt}, .W = width, .H = height, .pts = in.at(s_pts),
                          .cell_px = cell_px ? in.at(s_cell) : nullptr, .n = (uint32_t)n, .params = refine_params_for(ctx, cfg), .out = out.at(s_out)};
    A3_HIP(edges ? launch_refine_edges(ctx->stream, rl) : launch_refine_corners(ctx->stream, rl));
    A3_HIP(out.download(s_out, corners_xy));
    A3_HIP(hipStreamSynchronize(ctx->stream));
    return A3_OK;
}

// ---- board pose (an extension beyond the reference; contract in include/aruco3_hip.h) ----
// What the two board setters share, behind their call checks: every id in the dictionary and named once, every marker checked and
// turned into its slot record by marker(its floats, slot) (-> the refusal's message, or nullptr), then the tables swapped in.  A ChArUco
// setting names ids of the board it was checked against, so it goes; recovery needs a (planar) board, so it goes unless keep_recovery.
static int set_board_tables(a3_ctx* ctx, const uint32_t* ids, const float* corners, size_t floats, size_t n, size_t slot_bytes, uint32_t kind,
                            bool keep_recovery, const char* unknown_id, const char* repeated_id, const char* (*marker)(const float*, void*)) {
    std::vector<uint8_t> seen(ctx->n_codes, 0);
    std::vector<uint8_t> slots(n * slot_bytes);
    for (size_t i = 0; i < n; i++) {
        if (ids[i] >= ctx->n_codes) return fail(ctx, A3_ERR_INVALID, unknown_id);
        if (seen[ids[i]]++) return fail(ctx, A3_ERR_INVALID, repeated_id);
        if (const char* m = marker(corners + floats * i, slots.data() + i * slot_bytes)) return fail(ctx, A3_ERR_INVALID, m);
    }
    ctx->board_ids.assign(ids, ids + n);
    ctx->board_slots.swap(slots);
    ctx->board_kind = kind;
    ctx->board_version++;
    if (!keep_recovery) ctx->recover = a3_recover_config{};
    ctx->charuco_nc = 0;
    ctx->charuco_tab_h.clear();
    ctx->charuco_version++;
    return A3_OK;
}

int a3_set_board(a3_ctx* ctx, const uint32_t* ids, const float* corners_xy, size_t n) {
    if (!ctx) return A3_ERR_INVALID;
    if (const char* m = check_board_call(ids, corners_xy, n)) return fail(ctx, A3_ERR_INVALID, m);
    return set_board_tables(ctx, ids, corners_xy, 8, n, board_slot_bytes(), kBoardSlotsPlanar /* (replaces a 3-D board too) */, n != 0,
                            "a3_set_board: an id is not in the dictionary", "a3_set_board: an id appears twice on the board",
                            [](const float* c, void* slot) {
                                const char* m = check_board_marker(c);
                                if (!m) board_slot_from(c, slot);
                                return m;
                            });
}

// the 3-D form: the same tables with Board3Slot records; the settings that need a plane go (a3_board3d_check.h refuses them from here on)
int a3_set_board3d(a3_ctx* ctx, const uint32_t* ids, const float* corners_xyz, size_t n) {
    if (!ctx) return A3_ERR_INVALID;
    if (const char* m = check_board3d_call(ctx->busy(), ids, corners_xyz, n)) return fail(ctx, A3_ERR_INVALID, m);
    return set_board_tables(ctx, ids, corners_xyz, 12, n, board3d_slot_bytes(), n ? kBoardSlots3D : kBoardSlotsPlanar, false,
                            "a3_set_board3d: an id is not in the dictionary", "a3_set_board3d: an id appears twice on the board",
                            [](const float* c, void* slot) {
                                const char* m = check_board3d_marker(c);
                                if (!m) board3d_slot_from(c, slot);
                                return m;
                            });
}

int a3_get_board_poses(a3_ctx* ctx, a3_board_pose* dst, size_t cap_frames, size_t* n) {
    if (!ctx || !n || (!dst && cap_frames)) return A3_ERR_INVALID;
    *n = 0;
    return get_side(ctx, kSideBoard, dst, cap_frames, n, "a3_get_board_poses: the last collected batch was not a pose batch with a board set",
                    "a3_get_board_poses: cap_frames is smaller than the number of frames");
}

int a3_estimate_board_pose(a3_ctx* ctx, const uint32_t* ids, const float* corners_xy, size_t n_markers, const a3_intrinsics* intr,
                           uint32_t image_width, uint32_t image_height, a3_board_pose* out) {
    if (!ctx) return A3_ERR_INVALID;
    if (!out || (n_markers && (!ids || !corners_xy))) return fail(ctx, A3_ERR_INVALID, "a3_estimate_board_pose: null argument");
    if (ctx->batch.active || ctx->pending_trivial) return fail(ctx, A3_ERR_INVALID, "a3_estimate_board_pose: a submitted batch has not been collected");
    if (ctx->board_ids.empty()) return fail(ctx, A3_ERR_INVALID, "a3_estimate_board_pose: no board is set (a3_set_board, a3_set_board3d)");
    if (!intr && (image_width == 0 || image_height == 0)) return fail(ctx, A3_ERR_INVALID, "a3_estimate_board_pose: empty image");
    if (n_markers > (1u << 20)) return fail(ctx, A3_ERR_INVALID, "a3_estimate_board_pose: more than 2^20 markers in one call");
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    if (int urc = upload_board(ctx)) return urc;
    Layout in{ctx->tmp_a, ctx->stream}, res{ctx->tmp_b, ctx->stream}, und{ctx->tmp_c, ctx->stream};
    const auto s_ids = in.add<uint32_t>(std::max<size_t>(n_markers, 1));   // (never an empty buffer)
    const auto s_pts = in.add<float>(8 * n_markers);
    const auto s_out = res.add<a3_board_pose>(1);
    A3_HIP(in.ensure()); A3_HIP(res.ensure());
    A3_HIP(in.upload(s_ids, ids, n_markers)); A3_HIP(in.upload(s_pts, corners_xy, 8 * n_markers));
    float* d_pts = in.at(s_pts);
    if (intr && ctx->dist.model != A3_DIST_NONE && n_markers) {   // undistorted pixel corners, as a pose batch solves from
        const auto s_und = und.add<float>(8 * n_markers), s_und_res = und.add<float>(4 * n_markers);
        A3_HIP(und.ensure());
        A3_HIP(launch_undistort_corners(ctx->stream, nullptr, d_pts, nullptr, (uint32_t)(n_markers * 4), *intr, ctx->dist, und.at(s_und), und.at(s_und_res)));
        d_pts = und.at(s_und);
    }
    const BoardPoseLaunch bp{.m = {.ids = in.at(s_ids), .pts = d_pts, .n = (uint32_t)n_markers, .n_frames = 1u}, .board = board_tables(ctx, 0),
                             .intr = intr, .W = image_width, .H = image_height, .out = res.at(s_out)};
    A3_HIP(bp.board.slot_kind == kBoardSlots3D ? launch_board3d_pose(ctx->stream, bp) : launch_board_pose(ctx->stream, bp));
    A3_HIP(res.download(s_out, out));
    A3_HIP(hipStreamSynchronize(ctx->stream));
    return A3_OK;
}

// ---- board-aided recovery (an extension beyond the reference; contract in include/aruco3_hip.h) ----
// the largest h with sum over k <= h of C(bits, k) * 1000 < 2^bits, in integers; 0 when no h does
static uint8_t recover_default_hamming(uint32_t bits) {
    if (bits == 0 || bits > 64) return 0;
    const unsigned __int128 space = (unsigned __int128)1 << bits;
    unsigned __int128 sum = 0, term = 1;   // C(bits, k)
    uint8_t h = 0;
    for (uint32_t k = 0; k <= bits; k++) {
        sum += term;
        if (sum * 1000 >= space) break;
        h = (uint8_t)k;
        term = term * (bits - k) / (k + 1);
    }
    return h;
}

int a3_default_recover_config(const a3_ctx* ctx, a3_recover_config* cfg) {
    if (!ctx || !cfg) return A3_ERR_INVALID;
    *cfg = a3_recover_config{};
    cfg->mode = 1; cfg->min_markers = 2; cfg->max_distance_px = 10.0f;
    cfg->max_hamming = recover_default_hamming(ctx->num_bits);
    return A3_OK;
}

static int check_recover_config(a3_ctx* ctx, const a3_recover_config& c, const char* who) {
    const char* what = nullptr;
    if (c.mode > 1) what = "mode must be 0 or 1";
    else if (c.min_markers == 0) what = "min_markers must be at least 1";
    else if (!std::isfinite(c.max_distance_px) || !(c.max_distance_px > 0.0f)) what = "max_distance_px must be finite and > 0";
    else if (c.reserved[0] || c.reserved[1] || c.reserved[2]) what = "reserved bytes must be 0";
    if (!what) return A3_OK;
    return fail(ctx, A3_ERR_INVALID, (std::string(who) + ": a3_recover_config." + what).c_str());
}

int a3_set_board_recovery(a3_ctx* ctx, const a3_recover_config* cfg) {
    if (!ctx) return A3_ERR_INVALID;
    if (ctx->busy()) return fail(ctx, A3_ERR_INVALID, "a3_set_board_recovery: a submitted batch has not been collected");
    if (!cfg || cfg->mode == 0) { ctx->recover = a3_recover_config{}; return A3_OK; }
    if (ctx->board_ids.empty()) return fail(ctx, A3_ERR_INVALID, "a3_set_board_recovery: no board is set (a3_set_board)");
    if (const char* m = check_recovery_board_kind(ctx->board_kind == kBoardSlots3D, cfg->mode)) return fail(ctx, A3_ERR_INVALID, m);
    if (int rc = check_recover_config(ctx, *cfg, "a3_set_board_recovery")) return rc;
    ctx->recover = *cfg;
    return A3_OK;
}

int a3_get_board_recovery(const a3_ctx* ctx, a3_recover_config* cfg) {
    if (!ctx || !cfg) return A3_ERR_INVALID;
    *cfg = ctx->recover;
    return A3_OK;
}

int a3_get_recovered_counts(a3_ctx* ctx, uint32_t* per_frame_recovered, size_t n_frames) {
    if (!ctx || (!per_frame_recovered && n_frames)) return A3_ERR_INVALID;
    size_t n = 0;
    return get_side(ctx, kSideRecovered, per_frame_recovered, n_frames, &n,
                    "a3_get_recovered_counts: the last collected batch ran without board recovery",
                    "a3_get_recovered_counts: n_frames is smaller than the number of frames");
}

int a3_recover_markers(a3_ctx* ctx, const uint32_t* detected_ids, const uint32_t* detected_corners_xy, size_t n_detected,
                       const uint32_t* candidate_corners_xy, const uint64_t* codes4, const uint8_t* has_codes, size_t n_candidates,
                       const a3_recover_config* cfg, a3_marker* out, size_t out_cap, size_t* out_n) {
    if (!ctx) return A3_ERR_INVALID;
    if (!cfg || !out_n || (!out && out_cap) || (n_detected && (!detected_ids || !detected_corners_xy)) ||
        (n_candidates && (!candidate_corners_xy || !codes4 || !has_codes)))
        return fail(ctx, A3_ERR_INVALID, "a3_recover_markers: null argument");
    *out_n = 0;
    if (ctx->busy()) return fail(ctx, A3_ERR_INVALID, "a3_recover_markers: a submitted batch has not been collected");
    if (ctx->board_ids.empty()) return fail(ctx, A3_ERR_INVALID, "a3_recover_markers: no board is set (a3_set_board)");
    if (const char* m = check_recover_markers_board_kind(ctx->board_kind == kBoardSlots3D)) return fail(ctx, A3_ERR_INVALID, m);
    if (cfg->mode != 1) return fail(ctx, A3_ERR_INVALID, "a3_recover_markers: a3_recover_config.mode must be 1");
    if (int rc = check_recover_config(ctx, *cfg, "a3_recover_markers")) return rc;
    if (n_detected > (1u << 20)) return fail(ctx, A3_ERR_INVALID, "a3_recover_markers: more than 2^20 detected markers in one call");
    if (n_candidates > kMaxCandLimit) return fail(ctx, A3_ERR_INVALID, "a3_recover_markers: more than A3_MAX_CANDIDATES_PER_FRAME candidates");
    for (size_t i = 0; i < 8 * n_candidates; i++)
        if (candidate_corners_xy[i] > 0xFFFFu) return fail(ctx, A3_ERR_INVALID, "a3_recover_markers: a candidate corner is above 65535");
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    if (int urc = upload_board(ctx)) return urc;
    if (int urc = upload_recover_ids(ctx)) return urc;
    const uint32_t slots = (uint32_t)ctx->board_ids.size(), rec_cap = (uint32_t)std::min<size_t>(slots, std::max<size_t>(n_candidates, 1));
    Layout in{ctx->tmp_a, ctx->stream}, res{ctx->tmp_b, ctx->stream};
    const auto s_ids = in.add<uint32_t>(std::max<size_t>(n_detected, 1));   // (never an empty buffer)
    const auto s_det = in.add<uint32_t>(8 * n_detected), s_cand = in.add<uint32_t>(8 * n_candidates);
    const auto s_codes = in.add<uint64_t>(4 * n_candidates);
    const auto s_has = in.add<uint8_t>(n_candidates);
    const auto s_count = res.add<uint32_t>(1);
    const auto s_rec = res.add<a3_marker>(rec_cap);
    A3_HIP(in.ensure()); A3_HIP(res.ensure());
    A3_HIP(in.upload(s_ids, detected_ids, n_detected)); A3_HIP(in.upload(s_det, detected_corners_xy, 8 * n_detected));
    A3_HIP(in.upload(s_cand, candidate_corners_xy, 8 * n_candidates)); A3_HIP(in.upload(s_codes, codes4, 4 * n_candidates));
    A3_HIP(in.upload(s_has, has_codes, n_candidates));
    A3_HIP(launch_recover_frames(ctx->stream, {.ids = in.at(s_ids), .corners = in.at(s_det), .n = (uint32_t)n_detected, .n_frames = 1u,
                                               .cand_xy = in.at(s_cand), .codes4 = in.at(s_codes), .has_codes = in.at(s_has), .n_cand = (uint32_t)n_candidates,
                                               .board = board_tables(ctx, 0), .slot_ids = ctx->recover_ids.as<uint32_t>(), .n_slots = slots,
                                               .dict = ctx->dict.as<uint64_t>(), .cfg = *cfg, .rec = res.at(s_rec), .rec_cap = rec_cap, .rec_count = res.at(s_count)}));
    uint32_t count = 0;
    A3_HIP(res.download(s_count, &count));
    A3_HIP(hipStreamSynchronize(ctx->stream));
    *out_n = count;
    if (count > out_cap) return fail(ctx, A3_ERR_CAPACITY, "a3_recover_markers: out_cap is smaller than the number of recovered markers");
    if (count) {
        A3_HIP(hipMemcpyAsync(out, res.at(s_rec), (size_t)count * sizeof(a3_marker), hipMemcpyDeviceToHost, ctx->stream));
        A3_HIP(hipStreamSynchronize(ctx->stream));
    }
    return A3_OK;
}

// ---- ChArUco boards (an extension beyond the reference; contract in include/aruco3_hip.h) ----
void a3_default_charuco_config(a3_charuco_config* cfg) {
    if (!cfg) return;
    *cfg = a3_charuco_config{2, 1, 5, 0.5f, 30, 0.01f};
}

static int check_charuco_config(a3_ctx* ctx, const a3_charuco_config& c) {
    if (c.min_markers < 1 || c.min_markers > 4) return fail(ctx, A3_ERR_INVALID, "a3_charuco_config.min_markers must be in 1..4");
    if (c.refine > 1) return fail(ctx, A3_ERR_INVALID, "a3_charuco_config.refine must be 0 or 1");
    if (c.win_half < 1 || c.win_half > 10) return fail(ctx, A3_ERR_INVALID, "a3_charuco_config.win_half must be in 1..10");
    if (!(c.relative_win >= 0.0f) || !std::isfinite(c.relative_win)) return fail(ctx, A3_ERR_INVALID, "a3_charuco_config.relative_win must be finite and >= 0");
    if (c.max_iterations > 100) return fail(ctx, A3_ERR_INVALID, "a3_charuco_config.max_iterations must be at most 100");
    if (!(c.min_shift >= 0.0f) || !std::isfinite(c.min_shift)) return fail(ctx, A3_ERR_INVALID, "a3_charuco_config.min_shift must be finite and >= 0");
    return A3_OK;
}

int a3_set_charuco(a3_ctx* ctx, const float* corners_xy, const uint32_t* adjacent_ids, size_t n_corners, const a3_charuco_config* cfg) {
    if (!ctx) return A3_ERR_INVALID;
    if (n_corners == 0) {
        ctx->charuco_nc = 0; ctx->charuco_tab_h.clear(); ctx->charuco_version++;
        return A3_OK;
    }
    if (n_corners > A3_CHARUCO_MAX_CORNERS) return fail(ctx, A3_ERR_INVALID, "a3_set_charuco: more than A3_CHARUCO_MAX_CORNERS corners");
    if (!corners_xy || !adjacent_ids) return fail(ctx, A3_ERR_INVALID, "a3_set_charuco: null corners or adjacent ids");
    if (ctx->board_ids.empty()) return fail(ctx, A3_ERR_INVALID, "a3_set_charuco: no board is set (a3_set_board)");
    if (const char* m = check_charuco_board_kind(ctx->board_kind == kBoardSlots3D, n_corners)) return fail(ctx, A3_ERR_INVALID, m);
    a3_charuco_config c;
    a3_default_charuco_config(&c);
    if (cfg) c = *cfg;
    if (int rc = check_charuco_config(ctx, c)) return rc;
    std::vector<uint8_t> on_board(ctx->n_codes, 0);
    for (uint32_t id : ctx->board_ids) on_board[id] = 1;
    std::vector<uint32_t> tab(6 * n_corners);
    for (size_t k = 0; k < n_corners; k++) {
        if (!std::isfinite(corners_xy[2 * k]) || !std::isfinite(corners_xy[2 * k + 1]))
            return fail(ctx, A3_ERR_INVALID, "a3_set_charuco: a corner is not finite");
        for (int j = 0; j < 4; j++) {
            const uint32_t id = adjacent_ids[4 * k + j];
            if (id != 0xFFFFFFFFu && (id >= ctx->n_codes || !on_board[id]))
                return fail(ctx, A3_ERR_INVALID, "a3_set_charuco: an adjacent id is not on the board (a3_set_board)");
        }
    }
    memcpy(tab.data(), corners_xy, n_corners * 2 * sizeof(float));
    memcpy(tab.data() + 2 * n_corners, adjacent_ids, n_corners * 4 * sizeof(uint32_t));
    ctx->charuco_tab_h.swap(tab);
    ctx->charuco_nc = (uint32_t)n_corners;
    ctx->charuco_cfg = c;
    ctx->charuco_version++;
    return A3_OK;
}

int a3_get_charuco_corners(a3_ctx* ctx, a3_charuco_corner* dst, size_t cap, size_t* n) {
    if (!ctx || !n || (!dst && cap)) return A3_ERR_INVALID;
    *n = 0;
    return get_last(ctx, ctx->charuco_valid, ctx->h_charuco.data(), ctx->h_charuco.size() * sizeof(a3_charuco_corner), sizeof(a3_charuco_corner), dst, cap, n,
                    "a3_get_charuco_corners: the last collected batch ran without ChArUco",
                    "a3_get_charuco_corners: cap is smaller than the number of corners");
}

int a3_get_charuco_poses(a3_ctx* ctx, a3_charuco_pose* dst, size_t cap_frames, size_t* n) {
    if (!ctx || !n || (!dst && cap_frames)) return A3_ERR_INVALID;
    *n = 0;
    return get_side(ctx, kSideCharucoPoses, dst, cap_frames, n,
                    "a3_get_charuco_poses: the last collected batch was not a pose batch with ChArUco set", "a3_get_charuco_poses: cap_frames is smaller than the number of frames");
}

int a3_interpolate_charuco(a3_ctx* ctx, const void* pixels, int memory, int fmt, uint32_t width, uint32_t height, size_t row_stride,
                           const uint32_t* ids, const float* corners_xy, size_t n_markers, a3_charuco_corner* dst, size_t cap, size_t* n) {
    if (!ctx) return A3_ERR_INVALID;
    if (!n || (!dst && cap) || (n_markers && (!ids || !corners_xy))) return fail(ctx, A3_ERR_INVALID, "a3_interpolate_charuco: null argument");
    *n = 0;
    if (ctx->batch.active || ctx->pending_trivial) return fail(ctx, A3_ERR_INVALID, "a3_interpolate_charuco: a submitted batch has not been collected");
    if (ctx->charuco_nc == 0) return fail(ctx, A3_ERR_INVALID, "a3_interpolate_charuco: ChArUco is not set (a3_set_charuco)");
    if (width == 0 || height == 0) return fail(ctx, A3_ERR_INVALID, "a3_interpolate_charuco: empty image");
    if (n_markers > (1u << 20)) return fail(ctx, A3_ERR_INVALID, "a3_interpolate_charuco: more than 2^20 markers in one call");
    for (size_t k = 0; k < n_markers * 8; k++)
        if (!std::isfinite(corners_xy[k])) return fail(ctx, A3_ERR_INVALID, "a3_interpolate_charuco: a marker corner is not finite");
    size_t frame_stride = 0;
    const uint8_t* d_pixels = nullptr;
    const int src = stage_input(ctx, pixels, memory, fmt, width, height, &row_stride, &frame_stride, 1, &d_pixels);
    if (src != A3_OK) return src;
    if (int urc = upload_board(ctx)) return urc;
    if (int urc = upload_charuco(ctx)) return urc;
    const uint32_t nc = ctx->charuco_nc;
    Layout in{ctx->tmp_a, ctx->stream}, res{ctx->tmp_c, ctx->stream};
    const auto s_ids = in.add<uint32_t>(std::max<size_t>(n_markers, 1));   // (never an empty buffer)
    const auto s_pts = in.add<float>(8 * n_markers);
    // the frame's slot records, its two counts (the second: the total), the records in id order
    const auto s_slots = res.add<a3_charuco_corner>(nc); const auto s_counts = res.add<uint32_t>(2); const auto s_out = res.add<a3_charuco_corner>(nc);
    A3_HIP(in.ensure()); A3_HIP(res.ensure());
    A3_HIP(in.upload(s_ids, ids, n_markers)); A3_HIP(in.upload(s_pts, corners_xy, 8 * n_markers));
    A3_HIP(launch_charuco_corners(ctx->stream, {.src = {d_pixels, row_stride, frame_stride, fmt}, .W = width, .H = height,
                                                .m = {.ids = in.at(s_ids), .pts = in.at(s_pts), .n = (uint32_t)n_markers, .n_frames = 1u},
                                                .board = board_tables(ctx, nc), .min_markers = ctx->charuco_cfg.min_markers, .refine = ctx->charuco_cfg.refine,
                                                .params = charuco_params_for(ctx, ctx->charuco_cfg), .slots_tmp = res.at(s_slots), .counts = res.at(s_counts),
                                                .out = res.at(s_out)}));
    uint32_t total = 0;
    A3_HIP(hipMemcpyAsync(&total, res.at(s_counts) + 1, 4, hipMemcpyDeviceToHost, ctx->stream));
    A3_HIP(hipStreamSynchronize(ctx->stream));
    *n = total;
    if (total > cap) return fail(ctx, A3_ERR_CAPACITY, "a3_interpolate_charuco: cap is smaller than the number of corners");
    if (total) {
        A3_HIP(hipMemcpyAsync(dst, res.at(s_out), (size_t)total * sizeof(a3_charuco_corner), hipMemcpyDeviceToHost, ctx->stream));
        A3_HIP(hipStreamSynchronize(ctx->stream));
    }
    return A3_OK;
}

// ---- lens distortion (an extension beyond the reference; contract in include/aruco3_hip.h) ----
void a3_default_distortion(a3_distortion* d) {
    if (!d) return;
    *d = a3_distortion{};
    d->model = A3_DIST_RATIONAL;
    d->iterations = 20;
    d->max_residual_px = 0.1f;
}

// the coefficients of a model that has some: all finite, and with the fisheye model (which reads k1 k2 k3 k4) the other four exactly 0
static int check_distortion_coefficients(a3_ctx* ctx, const a3_distortion& d, const char* not_finite, const char* not_fisheye) {
    const float k[8] = {d.k1, d.k2, d.p1, d.p2, d.k3, d.k4, d.k5, d.k6};
    for (float v : k)
        if (!std::isfinite(v)) return fail(ctx, A3_ERR_INVALID, not_finite);
    if (d.model == A3_DIST_FISHEYE && (d.p1 != 0.0f || d.p2 != 0.0f || d.k5 != 0.0f || d.k6 != 0.0f)) return fail(ctx, A3_ERR_INVALID, not_fisheye);
    return A3_OK;
}

static int check_distortion(a3_ctx* ctx, const a3_distortion& d) {
    if (d.model != A3_DIST_NONE && d.model != A3_DIST_RATIONAL && d.model != A3_DIST_FISHEYE)
        return fail(ctx, A3_ERR_INVALID, "a3_distortion.model: unknown model");
    if (d.model == A3_DIST_NONE) return A3_OK;
    if (d.iterations < 1 || d.iterations > 100) return fail(ctx, A3_ERR_INVALID, "a3_distortion.iterations must be in 1..100");
    if (int rc = check_distortion_coefficients(ctx, d, "a3_distortion: a coefficient is not finite",
                                               "a3_distortion: model A3_DIST_FISHEYE reads k1 k2 k3 k4; p1 p2 k5 k6 must be 0"))
        return rc;
    if (!(d.max_residual_px >= 0.0f) || !std::isfinite(d.max_residual_px))
        return fail(ctx, A3_ERR_INVALID, "a3_distortion.max_residual_px must be finite and >= 0");
    return A3_OK;
}

int a3_set_distortion(a3_ctx* ctx, const a3_distortion* d) {
    if (!ctx) return A3_ERR_INVALID;
    a3_distortion c{};   // NULL: off
    if (d) c = *d;
    if (int rc = check_distortion(ctx, c)) return rc;
    if (c.model == A3_DIST_NONE) c = a3_distortion{};
    ctx->dist = c;
    return A3_OK;
}

int a3_get_undistorted_corners(a3_ctx* ctx, float* dst_xy, float* residual_px, size_t cap_markers, size_t* n) {
    if (!ctx) return A3_ERR_INVALID;
    if (!n || (!dst_xy && cap_markers)) return fail(ctx, A3_ERR_INVALID, "a3_get_undistorted_corners: null argument");
    const int rc = get_side(ctx, kSideUndist, dst_xy, cap_markers, n, "a3_get_undistorted_corners: the last collected batch ran without lens distortion",
                            "a3_get_undistorted_corners: cap_markers is smaller than the number of markers");   // (*n: untouched by the first refusal)
    if (rc == A3_OK && *n && residual_px) memcpy(residual_px, ctx->side_h[kSideUndistRes].data(), *n * kSides[kSideUndistRes].rec);
    return rc;
}

int a3_undistort_points(a3_ctx* ctx, const float* xy, size_t n, const a3_intrinsics* intr, const a3_distortion* d, float* out_xy,
                        float* residual_px) {
    if (!ctx) return A3_ERR_INVALID;
    if (!intr || !d || (n && (!xy || !out_xy))) return fail(ctx, A3_ERR_INVALID, "a3_undistort_points: null argument");
    if (int rc = check_distortion(ctx, *d)) return rc;
    if (d->model == A3_DIST_NONE) return fail(ctx, A3_ERR_INVALID, "a3_undistort_points: no distortion model (A3_DIST_NONE)");
    if (ctx->batch.active || ctx->pending_trivial) return fail(ctx, A3_ERR_INVALID, "a3_undistort_points: a submitted batch has not been collected");
    if (n > (1u << 30)) return fail(ctx, A3_ERR_INVALID, "a3_undistort_points: more than 2^30 points in one call");
    if (n == 0) return A3_OK;
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    Layout in{ctx->tmp_a, ctx->stream}, out{ctx->tmp_b, ctx->stream};
    const auto s_xy = in.add<float>(2 * n), s_out = out.add<float>(2 * n), s_res = out.add<float>(n);
    A3_HIP(in.ensure()); A3_HIP(out.ensure());
    A3_HIP(in.upload(s_xy, xy, 2 * n));
    A3_HIP(launch_undistort_corners(ctx->stream, nullptr, in.at(s_xy), nullptr, (uint32_t)n, *intr, *d, out.at(s_out), out.at(s_res)));
    A3_HIP(out.download(s_out, out_xy)); A3_HIP(out.download(s_res, residual_px));
    A3_HIP(hipStreamSynchronize(ctx->stream));
    return A3_OK;
}

int a3_calibrate_cameras(a3_ctx* ctx, const a3_calib_camera* cams, size_t n_cams, const uint32_t* view_offsets, size_t n_views,
                         const float* object_xy, const float* image_xy, a3_calib_result* results, a3_calib_view* views) {
    return calibrate_impl(ctx, false, cams, n_cams, view_offsets, n_views, object_xy, image_xy, results, views);
}

int a3_calibrate_fisheye_cameras(a3_ctx* ctx, const a3_calib_camera* cams, size_t n_cams, const uint32_t* view_offsets, size_t n_views,
                                 const float* object_xy, const float* image_xy, a3_calib_result* results, a3_calib_view* views) {
    return calibrate_impl(ctx, true, cams, n_cams, view_offsets, n_views, object_xy, image_xy, results, views);
}

int a3_calibrate_rigs(a3_ctx* ctx, const a3_rig* rigs, size_t n_rigs, const a3_rig_camera* cameras, size_t n_cameras, const a3_rig_observation* obs,
                      size_t n_obs, const float* object_xy, const float* image_xy, a3_rig_result* results, a3_rig_camera_result* camera_results,
                      a3_rig_frame* frames, a3_rig_observation_result* obs_results) {
    if (!ctx) return A3_ERR_INVALID;
    size_t n_frames = 0, n_pts = 0;
    if (const char* m = check_rigs(ctx->busy(), rigs, n_rigs, cameras, n_cameras, obs, n_obs, object_xy, image_xy, results, camera_results, n_frames, n_pts))
        return fail(ctx, A3_ERR_INVALID, m);
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    Layout in{ctx->solve_in, ctx->stream}, scr{ctx->solve_scratch, ctx->stream}, out{ctx->solve_out, ctx->stream};
    const auto s_rigs = in.add<a3_rig>(n_rigs);
    const auto s_cams = in.add<a3_rig_camera>(n_cameras);
    const auto s_obs = in.add<a3_rig_observation>(n_obs);
    const auto s_obj = in.add<float>(2 * std::max<size_t>(n_pts, 1)), s_img = in.add<float>(2 * std::max<size_t>(n_pts, 1));
    const auto s_tab = scr.add<uint32_t>(n_frames, rig_table_bytes());
    const auto s_oscr = scr.add<double>(n_obs, rig_obs_bytes()), s_fscr = scr.add<double>(n_frames, rig_frame_bytes());
    const auto s_res = out.add<a3_rig_result>(n_rigs);
    const auto s_cres = out.add<a3_rig_camera_result>(n_cameras);
    const auto s_frames = out.add<a3_rig_frame>(n_frames);
    const auto s_ores = out.add<a3_rig_observation_result>(n_obs);
    A3_HIP(in.ensure()); A3_HIP(scr.ensure()); A3_HIP(out.ensure());
    A3_HIP(in.upload(s_rigs, rigs, n_rigs));
    A3_HIP(in.upload(s_cams, cameras, n_cameras));
    A3_HIP(in.upload(s_obs, obs, n_obs));
    A3_HIP(in.upload(s_obj, object_xy, 2 * n_pts)); A3_HIP(in.upload(s_img, image_xy, 2 * n_pts));
    // a camera, frame or observation that no rig owns is not written by the kernel: it comes back zero
    A3_HIP(out.zero_from(s_cres));
    A3_HIP(launch_rig(ctx->stream, {.rigs = in.at(s_rigs), .n_rigs = (uint32_t)n_rigs, .cams = in.at(s_cams), .obs = in.at(s_obs), .obj = in.at(s_obj),
                                    .img = in.at(s_img), .tab = scr.at(s_tab), .oscr = scr.at(s_oscr), .fscr = scr.at(s_fscr), .res = out.at(s_res),
                                    .cres = out.at(s_cres), .frames = out.at(s_frames), .ores = out.at(s_ores)}));
    A3_HIP(out.download(s_res, results));
    A3_HIP(out.download(s_cres, camera_results));
    A3_HIP(out.download(s_frames, frames));
    A3_HIP(out.download(s_ores, obs_results));
    A3_HIP(hipStreamSynchronize(ctx->stream));
    return A3_OK;
}

int a3_calibrate_hand_eyes(a3_ctx* ctx, const a3_handeye_problem* problems, size_t n_problems, const a3_handeye_frame* frames, size_t n_frames,
                           const float* object_xy, const float* image_xy, a3_handeye_result* results, a3_handeye_frame_result* frame_results) {
    if (!ctx) return A3_ERR_INVALID;
    size_t n_pts = 0;
    if (const char* m = check_hand_eyes(ctx->busy(), problems, n_problems, frames, n_frames, object_xy, image_xy, results, n_pts))
        return fail(ctx, A3_ERR_INVALID, m);
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    Layout in{ctx->solve_in, ctx->stream}, scr{ctx->solve_scratch, ctx->stream}, out{ctx->solve_out, ctx->stream};
    const auto s_probs = in.add<a3_handeye_problem>(n_problems);
    const auto s_frames = in.add<a3_handeye_frame>(n_frames);
    const auto s_obj = in.add<float>(2 * std::max<size_t>(n_pts, 1)), s_img = in.add<float>(2 * std::max<size_t>(n_pts, 1));
    const auto s_fscr = scr.add<double>(n_frames, handeye_frame_bytes());
    const auto s_res = out.add<a3_handeye_result>(n_problems);
    const auto s_fres = out.add<a3_handeye_frame_result>(n_frames);
    A3_HIP(in.ensure()); A3_HIP(scr.ensure()); A3_HIP(out.ensure());
    A3_HIP(in.upload(s_probs, problems, n_problems));
    A3_HIP(in.upload(s_frames, frames, n_frames));
    A3_HIP(in.upload(s_obj, object_xy, 2 * n_pts)); A3_HIP(in.upload(s_img, image_xy, 2 * n_pts));
    // a frame that no problem owns is not written by the kernel: it comes back zero
    A3_HIP(out.zero_from(s_fres));
    A3_HIP(launch_handeye(ctx->stream, in.at(s_probs), (uint32_t)n_problems, in.at(s_frames), in.at(s_obj), in.at(s_img), scr.at(s_fscr), out.at(s_res),
                          out.at(s_fres)));
    A3_HIP(out.download(s_res, results));
    A3_HIP(out.download(s_fres, frame_results));
    A3_HIP(hipStreamSynchronize(ctx->stream));
    return A3_OK;
}

int a3_build_marker_maps(a3_ctx* ctx, const a3_map* maps, size_t n_maps, const a3_map_marker* markers, size_t n_markers, const a3_map_observation* obs,
                         size_t n_obs, const float* image_xy, a3_map_result* results, a3_map_marker_result* marker_results, a3_map_frame* frames,
                         a3_map_observation_result* obs_results) {
    if (!ctx) return A3_ERR_INVALID;
    size_t n_frames = 0;
    std::vector<uint64_t> big_off;
    uint64_t big_doubles = 0;
    if (const char* m = check_marker_maps(ctx->busy(), maps, n_maps, markers, n_markers, obs, n_obs, image_xy, results, marker_results, n_frames, big_off,
                                          big_doubles))
        return fail(ctx, A3_ERR_INVALID, m);
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    Layout in{ctx->solve_in, ctx->stream}, scr{ctx->solve_scratch, ctx->stream}, out{ctx->solve_out, ctx->stream};
    const auto s_maps = in.add<a3_map>(n_maps);
    const auto s_mk = in.add<a3_map_marker>(n_markers);
    const auto s_obs = in.add<a3_map_observation>(n_obs);
    const auto s_img = in.add<float>(8 * n_obs);
    const auto s_off = in.add<uint64_t>(n_maps);
    const auto s_fo = scr.add<uint32_t>(n_frames), s_ml = scr.add<uint32_t>(n_obs);
    const auto s_oscr = scr.add<double>(n_obs, map_obs_bytes()), s_fscr = scr.add<double>(n_frames, map_frame_bytes());
    const auto s_mscr = scr.add<double>(n_markers, map_marker_bytes());
    const auto s_res = out.add<a3_map_result>(n_maps);
    const auto s_mres = out.add<a3_map_marker_result>(n_markers);
    const auto s_frames = out.add<a3_map_frame>(n_frames);
    const auto s_ores = out.add<a3_map_observation_result>(n_obs);
    A3_HIP(in.ensure()); A3_HIP(scr.ensure()); A3_HIP(out.ensure());
    A3_HIP(ctx->solve_big.ensure(std::max<size_t>(big_doubles, 1) * sizeof(double)));
    A3_HIP(in.upload(s_maps, maps, n_maps));
    A3_HIP(in.upload(s_mk, markers, n_markers));
    A3_HIP(in.upload(s_obs, obs, n_obs));
    A3_HIP(in.upload(s_img, image_xy, 8 * n_obs));
    A3_HIP(in.upload(s_off, big_off.data(), n_maps));
    // a marker, frame or observation that no map owns is not written by the kernel: it comes back zero
    A3_HIP(out.zero_from(s_mres));
    A3_HIP(launch_map(ctx->stream, {.maps = in.at(s_maps), .n_maps = (uint32_t)n_maps, .markers = in.at(s_mk), .obs = in.at(s_obs), .img = in.at(s_img),
                                    .big_off = in.at(s_off), .fo = scr.at(s_fo), .ml = scr.at(s_ml), .oscr = scr.at(s_oscr), .fscr = scr.at(s_fscr),
                                    .mscr = scr.at(s_mscr), .big = ctx->solve_big.as<double>(), .res = out.at(s_res), .mres = out.at(s_mres),
                                    .frames = out.at(s_frames), .ores = out.at(s_ores)}));
    A3_HIP(out.download(s_res, results));
    A3_HIP(out.download(s_mres, marker_results));
    A3_HIP(out.download(s_frames, frames));
    A3_HIP(out.download(s_ores, obs_results));
    A3_HIP(hipStreamSynchronize(ctx->stream));
    return A3_OK;
}

// ---- frame rectification (an extension beyond the reference; contract in include/aruco3_hip.h) ----
void a3_default_rectify(a3_rectify* r, const a3_intrinsics* src, const a3_distortion* d) {
    if (!r) return;
    *r = a3_rectify{};
    if (src) r->src = r->dst = *src;
    if (d) r->distortion = *d;
    r->rotation[0] = r->rotation[4] = r->rotation[8] = 1.0f;
}

// a3_rectify_frames and a3_reduce_frames, both synchronous.  A host-side source: the caller's span (`bytes`, padding included) goes to
// rect_in in one copy.
static int stage_frames_in(a3_ctx* ctx, const void* src, int memory, size_t bytes, const uint8_t** d_src) {
    *d_src = reinterpret_cast<const uint8_t*>(src);
    if (memory != A3_MEM_HOST) return A3_OK;
    A3_HIP(ctx->rect_in.ensure(bytes));
    A3_HIP(hipMemcpyAsync(ctx->rect_in.p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
    *d_src = ctx->rect_in.as<uint8_t>();
    return A3_OK;
}
// Where the kernel writes n_frames frames of `rows` rows of row_bytes: the caller's device frames, or for a host-side destination packed
// rows in rect_out, which finish copies back -- the rows' pixels only -- before it waits for the stream.
struct FramesOut {
    uint8_t* d_dst = nullptr; size_t d_row = 0, d_frame = 0;
    void* host = nullptr; size_t row_stride = 0, frame_stride = 0, rows = 0; uint32_t n_frames = 0;
    int begin(a3_ctx* ctx, void* dst, int memory, size_t row_stride_, size_t frame_stride_, size_t row_bytes, size_t rows_, uint32_t n) {
        d_dst = reinterpret_cast<uint8_t*>(dst); d_row = row_stride = row_stride_; d_frame = frame_stride = frame_stride_; rows = rows_; n_frames = n;
        if (memory != A3_MEM_HOST) return A3_OK;
        host = dst; d_row = row_bytes; d_frame = d_row * rows;
        A3_HIP(ctx->rect_out.ensure(d_frame * n_frames));
        d_dst = ctx->rect_out.as<uint8_t>();
        return A3_OK;
    }
    int finish(a3_ctx* ctx) const {
        if (host && frame_stride == row_stride * rows) {
            A3_HIP(hipMemcpy2DAsync(host, row_stride, d_dst, d_row, d_row, rows * n_frames, hipMemcpyDeviceToHost, ctx->stream));
        } else if (host) {
            for (uint32_t f = 0; f < n_frames; f++)
                A3_HIP(hipMemcpy2DAsync(reinterpret_cast<uint8_t*>(host) + f * frame_stride, row_stride, d_dst + f * d_frame, d_row, d_row, rows,
                                        hipMemcpyDeviceToHost, ctx->stream));
        }
        A3_HIP(hipStreamSynchronize(ctx->stream));
        return A3_OK;
    }
};

int a3_rectify_frames(a3_ctx* ctx, const void* src, int src_memory, int fmt, size_t src_row_stride, size_t src_frame_stride, uint32_t n_frames,
                      const a3_rectify* r, void* dst, int dst_memory, size_t dst_row_stride, size_t dst_frame_stride, a3_rectify_info* info) {
    if (!ctx) return A3_ERR_INVALID;
    if (!src || !r || !dst) return fail(ctx, A3_ERR_INVALID, "a3_rectify_frames: null argument");
    if (ctx->batch.active || ctx->pending_trivial) return fail(ctx, A3_ERR_INVALID, "a3_rectify_frames: a submitted batch has not been collected");
    if (n_frames == 0 || n_frames > 65535) return fail(ctx, A3_ERR_INVALID, "a3_rectify_frames: n_frames must be in 1..65535");
    if (!format_valid(fmt)) return fail(ctx, A3_ERR_INVALID, "a3_rectify_frames: unknown pixel format");
    if ((src_memory != A3_MEM_HOST && src_memory != A3_MEM_DEVICE) || (dst_memory != A3_MEM_HOST && dst_memory != A3_MEM_DEVICE))
        return fail(ctx, A3_ERR_INVALID, "a3_rectify_frames: memory must be A3_MEM_HOST or A3_MEM_DEVICE");
    // bpp: of the source; obpp: of what is written -- the same, but for a packed 4:2:2 source, whose rectified frames are the luma view
    const size_t bpp = format_bpp(fmt), obpp = format_rectified_bpp(fmt);
    if (const char* m = check_rectify_frames_fmt(*r, fmt, src_row_stride, src_frame_stride, dst_row_stride, dst_frame_stride)) return fail(ctx, A3_ERR_INVALID, m);
    const a3_distortion& d = r->distortion;

    const uint32_t sw = r->src.image_width, sh = r->src.image_height, dw = r->dst.image_width, dh = r->dst.image_height;
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    const uint8_t* d_src = nullptr;
    if (int rc = stage_frames_in(ctx, src, src_memory, src_frame_stride * (n_frames - 1) + src_row_stride * (sh - 1) + (size_t)sw * bpp, &d_src)) return rc;
    FramesOut o;
    if (int rc = o.begin(ctx, dst, dst_memory, dst_row_stride, dst_frame_stride, (size_t)dw * obpp, dh, n_frames)) return rc;
    if (format_is_422(fmt))   // the grey form: the luma byte alone, one byte per pixel out
        A3_HIP(launch_rectify_grey(ctx->stream, {.src = d_src, .src_row = src_row_stride, .src_frame = src_frame_stride, .n_frames = n_frames, .fmt = fmt,
                                                 .r = r, .grey = o.d_dst, .dst_row = o.d_row, .dst_frame = o.d_frame}));
    else
        A3_HIP(launch_rectify(ctx->stream, {.src = d_src, .src_row = src_row_stride, .src_frame = src_frame_stride, .n_frames = n_frames, .bpp = (int)bpp, .r = r,
                                            .dst = o.d_dst, .dst_row = o.d_row, .dst_frame = o.d_frame}));
    if (int rc = o.finish(ctx)) return rc;
    if (info) {
        *info = a3_rectify_info{};
        uint32_t tx, ty, tz;
        rectify_grid(dw, dh, n_frames, &tx, &ty, &tz);
        info->tiles = tx * ty;
        info->path_tiles[d.model == A3_DIST_FISHEYE ? 1 : 0] = info->tiles;   // path 0: the rational map (and no lens), path 1: the fisheye map
    }
    return A3_OK;
}

int a3_set_rectification(a3_ctx* ctx, const a3_rectify* r) {
    if (!ctx) return A3_ERR_INVALID;
    if (ctx->busy()) return fail(ctx, A3_ERR_INVALID, "a3_set_rectification: a submitted batch has not been collected");
    if (!r) { ctx->rect_on = false; ctx->rect = a3_rectify{}; return A3_OK; }   // NULL: off
    if (ctx->reduction.factor) return fail(ctx, A3_ERR_INVALID, "a3_set_rectification: a reduction is set (a3_set_reduction): set one or the other");
    const size_t sw = r->src.image_width, sh = r->src.image_height, dw = r->dst.image_width, dh = r->dst.image_height;
    if (const char* m = check_rectify(true, *r, 1, sw, sw * sh, dw, dw * dh)) return fail(ctx, A3_ERR_INVALID, m);
    ctx->rect = *r;
    ctx->rect_on = true;
    return A3_OK;
}

int a3_get_rectification(const a3_ctx* ctx, a3_rectify* r, int* enabled) {
    if (!ctx || !r || !enabled) return A3_ERR_INVALID;
    *r = ctx->rect;
    *enabled = ctx->rect_on ? 1 : 0;
    return A3_OK;
}

// ---- detection on reduced frames (an extension beyond the reference; contract in include/aruco3_hip.h) ----
int a3_reduce_frames(a3_ctx* ctx, const void* src, int src_memory, int fmt, uint32_t width, uint32_t height, size_t src_row_stride,
                     size_t src_frame_stride, uint32_t n_frames, uint32_t factor, void* dst, int dst_memory, size_t dst_row_stride,
                     size_t dst_frame_stride) {
    if (!ctx) return A3_ERR_INVALID;
    if (!src || !dst) return fail(ctx, A3_ERR_INVALID, "a3_reduce_frames: null argument");
    if (ctx->busy()) return fail(ctx, A3_ERR_INVALID, "a3_reduce_frames: a submitted batch has not been collected");
    if (const char* m = check_reduce_frames(src, src_memory, fmt, width, height, src_row_stride, src_frame_stride, n_frames, factor, dst, dst_memory,
                                            dst_row_stride, dst_frame_stride))
        return fail(ctx, A3_ERR_INVALID, m);
    const size_t bpp = reduce_bpp(fmt), w = width / factor, h = height / factor;
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    const uint8_t* d_src = nullptr;
    if (int rc = stage_frames_in(ctx, src, src_memory, src_frame_stride * (n_frames - 1) + src_row_stride * (height - 1) + (size_t)width * bpp, &d_src)) return rc;
    FramesOut o;
    if (int rc = o.begin(ctx, dst, dst_memory, dst_row_stride, dst_frame_stride, w, h, n_frames)) return rc;
    A3_HIP(launch_reduce_frames(ctx->stream, {.src = d_src, .src_row = src_row_stride, .src_frame = src_frame_stride, .n_frames = n_frames, .fmt = fmt,
                                              .W = width, .H = height, .factor = factor, .dst = o.d_dst, .dst_row = o.d_row, .dst_frame = o.d_frame}));
    return o.finish(ctx);
}

int a3_set_reduction(a3_ctx* ctx, const a3_reduction* r) {
    if (!ctx) return A3_ERR_INVALID;
    if (ctx->busy()) return fail(ctx, A3_ERR_INVALID, "a3_set_reduction: a submitted batch has not been collected");
    if (!r) { ctx->reduction = a3_reduction{}; return A3_OK; }   // NULL: off
    if (const char* m = check_reduction(*r)) return fail(ctx, A3_ERR_INVALID, m);
    if (ctx->rect_on) return fail(ctx, A3_ERR_INVALID, "a3_set_reduction: a rectification is set (a3_set_rectification): set one or the other");
    ctx->reduction = *r;
    return A3_OK;
}

int a3_set_threshold_windows(a3_ctx* ctx, const uint32_t* radii, size_t n) {
    if (!ctx) return A3_ERR_INVALID;
    if (const char* m = check_threshold_windows(ctx->busy(), radii, n)) return fail(ctx, A3_ERR_INVALID, m);
    ctx->n_windows = radii ? (uint32_t)n : 0;
    for (uint32_t k = 0; k < A3_MAX_THRESHOLD_WINDOWS; k++) ctx->windows[k] = k < ctx->n_windows ? radii[k] : 0;
    return A3_OK;
}

int a3_get_threshold_windows(const a3_ctx* ctx, uint32_t* radii, size_t cap, size_t* n) {
    if (!ctx || !n || (!radii && cap)) return A3_ERR_INVALID;
    *n = ctx->n_windows;
    if (ctx->n_windows > cap) return fail(const_cast<a3_ctx*>(ctx), A3_ERR_CAPACITY, "a3_get_threshold_windows: cap is smaller than the number of windows set");
    for (uint32_t k = 0; k < ctx->n_windows; k++) radii[k] = ctx->windows[k];
    return A3_OK;
}

// ---- inverted markers (an extension beyond the reference; contract in include/aruco3_hip.h) ----
int a3_set_marker_polarity(a3_ctx* ctx, int mode) {
    if (!ctx) return A3_ERR_INVALID;
    if (mode != A3_POLARITY_DARK && mode != A3_POLARITY_BOTH) return fail(ctx, A3_ERR_INVALID, "a3_set_marker_polarity: unknown mode");
    ctx->polarity = mode;
    return A3_OK;
}

int a3_get_marker_polarity(const a3_ctx* ctx, int* mode) {
    if (!ctx || !mode) return A3_ERR_INVALID;
    *mode = ctx->polarity;
    return A3_OK;
}

int a3_get_marker_flags(a3_ctx* ctx, uint32_t* dst, size_t cap_markers, size_t* n) {
    if (!ctx || !n || (!dst && cap_markers)) return A3_ERR_INVALID;
    *n = 0;
    return get_last(ctx, ctx->flags_valid, ctx->flags_h.data(), ctx->flags_h.size() * kFlagsRec, kFlagsRec, dst, cap_markers, n,
                    "a3_get_marker_flags: the last collected batch did not run in mode A3_POLARITY_BOTH",
                    "a3_get_marker_flags: cap_markers is smaller than the number of markers");
}

int a3_get_reduction(const a3_ctx* ctx, a3_reduction* r, int* enabled) {
    if (!ctx || !r || !enabled) return A3_ERR_INVALID;
    *r = ctx->reduction;
    *enabled = ctx->reduction.factor ? 1 : 0;
    return A3_OK;
}

static int pose_common(a3_ctx* ctx, const uint32_t* corners, const float* norm, size_t n, int mode, float size_mm, const a3_intrinsics* intr,
                       uint32_t iw, uint32_t ih, a3_pose* out) {
    if (!ctx || !out || (!corners && !norm)) return A3_ERR_INVALID;
    if (n == 0) return A3_OK;
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    const size_t in_bytes = n * 8 * 4;
    A3_HIP(ctx->tmp_a.ensure(in_bytes));
    A3_HIP(ctx->tmp_b.ensure(n * 2 * sizeof(a3_pose)));
    A3_HIP(hipMemcpyAsync(ctx->tmp_a.p, corners ? (const void*)corners : (const void*)norm, in_bytes, hipMemcpyHostToDevice, ctx->stream));
    float fx = 1, fy = 1, cx = 0, cy = 0;
    if (intr) { fx = intr->focal_x; fy = intr->focal_y; cx = intr->principal_x; cy = intr->principal_y; }
    A3_HIP(launch_pose(ctx->stream, {.corners = corners ? ctx->tmp_a.as<uint32_t>() : nullptr, .corner_stride = 8u, .norm_pts = norm ? ctx->tmp_a.as<float>() : nullptr,
                                     .n = (uint32_t)n, .mode = mode, .marker_size_mm = size_mm, .iw = (float)iw, .ih = (float)ih, .fx = fx, .fy = fy, .cx = cx,
                                     .cy = cy, .out = ctx->tmp_b.as<a3_pose>()}));
    A3_HIP(hipMemcpyAsync(out, ctx->tmp_b.p, n * 2 * sizeof(a3_pose), hipMemcpyDeviceToHost, ctx->stream));
    A3_HIP(hipStreamSynchronize(ctx->stream));
    return A3_OK;
}

int a3_estimate_pose(a3_ctx* ctx, const uint32_t* corners_xy, size_t n, float marker_size_mm, const a3_intrinsics* intr, uint32_t image_width,
                     uint32_t image_height, a3_pose* out) {
    if (!corners_xy) return A3_ERR_INVALID;
    return pose_common(ctx, corners_xy, nullptr, n, intr ? 1 : 0, marker_size_mm, intr, image_width, image_height, out);
}

int a3_estimate_pose_normalized(a3_ctx* ctx, const float* points_xy, size_t n, float marker_size_mm, a3_pose* out) {
    if (!points_xy) return A3_ERR_INVALID;
    return pose_common(ctx, nullptr, points_xy, n, 2, marker_size_mm, nullptr, 1, 1, out);
}

int a3_find_nearest(a3_ctx* ctx, const uint64_t* bits, size_t n, uint32_t* idx, uint8_t* dist) {
    if (!ctx || !bits || !idx || !dist) return A3_ERR_INVALID;
    if (n == 0) return A3_OK;
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    A3_HIP(ctx->tmp_a.ensure(n * 8));
    A3_HIP(ctx->tmp_c.ensure(n * 4));
    A3_HIP(ctx->tmp_d.ensure(n));
    A3_HIP(hipMemcpyAsync(ctx->tmp_a.p, bits, n * 8, hipMemcpyHostToDevice, ctx->stream));
    A3_HIP(launch_find_nearest(ctx->stream, ctx->dict.as<uint64_t>(), ctx->n_codes, ctx->tmp_a.as<uint64_t>(), (uint32_t)n, ctx->tmp_c.as<uint32_t>(),
                               ctx->tmp_d.as<uint8_t>()));
    A3_HIP(hipMemcpyAsync(idx, ctx->tmp_c.p, n * 4, hipMemcpyDeviceToHost, ctx->stream));
    A3_HIP(hipMemcpyAsync(dist, ctx->tmp_d.p, n, hipMemcpyDeviceToHost, ctx->stream));
    A3_HIP(hipStreamSynchronize(ctx->stream));
    return A3_OK;
}

int a3_set_profiling(a3_ctx* ctx, int enabled) {
    if (!ctx) return A3_ERR_INVALID;
    ctx->profiling = enabled == A3_PROFILE_STAGES ? 2 : ((enabled == A3_PROFILE_THRESHOLD_ONLY || enabled == A3_PROFILE_THRESHOLD_SAMPLED) ? 1 : 0);
    ctx->profile_every = enabled == A3_PROFILE_THRESHOLD_SAMPLED ? 4 : 1;
    return A3_OK;
}

int a3_get_profile(a3_ctx* ctx, int stage, double* total_ms, uint64_t* launches, int reset) {
    if (!ctx || stage < 0 || stage >= A3_STAGE_COUNT) return A3_ERR_INVALID;
    if (total_ms) *total_ms = ctx->prof_ms[stage];
    if (launches) *launches = ctx->prof_n[stage];
    if (reset) { ctx->prof_ms[stage] = 0; ctx->prof_n[stage] = 0; }
    return A3_OK;
}

int a3_selftest_ieee(a3_ctx* ctx, const double* a, const double* b, size_t n, double* sqrt_a, double* a_div_b, float* sqrtf_a, float* a_divf_b) {
    if (!ctx || !a || !b || !sqrt_a || !a_div_b || !sqrtf_a || !a_divf_b) return A3_ERR_INVALID;
    if (n == 0) return A3_OK;
    A3_HIP(hipSetDevice(ctx->device));
    if (int rcs_ = need_stream(ctx)) return rcs_;
    A3_HIP(ctx->tmp_a.ensure(n * 8)); A3_HIP(ctx->tmp_b.ensure(n * 8)); A3_HIP(ctx->tmp_c.ensure(n * 16)); A3_HIP(ctx->tmp_d.ensure(n * 8));
    A3_HIP(hipMemcpy(ctx->tmp_a.p, a, n * 8, hipMemcpyHostToDevice));
    A3_HIP(hipMemcpy(ctx->tmp_b.p, b, n * 8, hipMemcpyHostToDevice));
    double* sq = ctx->tmp_c.as<double>(); double* dv = sq + n;
    float* sqf = ctx->tmp_d.as<float>(); float* dvf = sqf + n;
    A3_HIP(launch_selftest(ctx->stream, ctx->tmp_a.as<double>(), ctx->tmp_b.as<double>(), (uint32_t)n, sq, dv, sqf, dvf));
    A3_HIP(hipStreamSynchronize(ctx->stream));
    A3_HIP(hipMemcpy(sqrt_a, sq, n * 8, hipMemcpyDeviceToHost));
    A3_HIP(hipMemcpy(a_div_b, dv, n * 8, hipMemcpyDeviceToHost));
    A3_HIP(hipMemcpy(sqrtf_a, sqf, n * 4, hipMemcpyDeviceToHost));
    A3_HIP(hipMemcpy(a_divf_b, dvf, n * 4, hipMemcpyDeviceToHost));
    return A3_OK;
}

}  // extern "C"
