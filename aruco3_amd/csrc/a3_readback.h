// A batch's fixed-size side results, and where its results lie in the pinned staging buffer they are read back through -- the one
// definition of both: ensure_back_buffers sizes the buffer by it, enqueue_back copies to its spans, finish_batch reads from them, the
// getters hand the kept copies out (a3_api.hip).  Host arithmetic on the public header's records only -- no HIP, no context -- so a plain
// C++ program checks every case (tests/readback_layout.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/aruco3_hip.h"

namespace a3 {

// what the batch record knows: frames, markers and ChArUco records read back speculatively, the bytes of the head, what is switched on
// (recover: the batch ran board-aided recovery; flags: it ran in mode A3_POLARITY_BOTH and carries a flag word per marker)
struct ReadbackShape { uint32_t n, guess, charuco_guess; size_t head_bytes; bool pose, refine, undist, board, charuco; bool recover = false; bool flags = false; };

// The side results: arrays of fixed-size records that travel with a batch's marker list, in the order they lie in the staging buffer.
// (The ChArUco corner records are not among them: a variable number, with a guess, a total and a tail fetch of their own.  Nor are the
// marker flags of a3_get_marker_flags, one uint32_t per marker: the table's kinds are written out once more, by number, in
// tests/readback_layout.cpp, so the flags have a span of their own behind everything else -- Readback::flags, kFlagsRec bytes a marker --
// and every layout without them is byte for byte what it was.)
enum SideKind { kSidePoses, kSideRefined, kSideBoard, kSideUndist, kSideUndistRes, kSideCharucoPoses, kSideRecovered, kSideKinds };
struct SideDesc {
    size_t rec;                          // the bytes of one record
    bool per_frame;                      // one record per frame; else one per marker, in marker order
    bool (*on)(const ReadbackShape&);    // the batch's switches that turn it on
    bool kept;                           // finish_batch keeps a host copy for the kind's getter (poses go to the caller's buffer at once)
    bool begin_clears;                   // begin_batch invalidates the kept copy
};
// begin_clears: a getter called between submit and collect is refused for these kinds, but for refined corners and poses it still
// answers for the previous batch (the poses' flag falls when the batch is enqueued, the refined corners' stays until collect).  That is
// how the library has behaved since each kind was added; making it uniform would change behaviour.
inline constexpr SideDesc kSides[kSideKinds] = {
    /* poses */ {2 * sizeof(a3_pose), false, [](const ReadbackShape& s) { return s.pose; }, false, false},
    /* refined */ {8 * sizeof(float), false, [](const ReadbackShape& s) { return s.refine; }, true, false},
    /* board */ {sizeof(a3_board_pose), true, [](const ReadbackShape& s) { return s.board; }, true, true},
    /* undist */ {8 * sizeof(float), false, [](const ReadbackShape& s) { return s.undist; }, true, true},
    /* undist_res */ {4 * sizeof(float), false, [](const ReadbackShape& s) { return s.undist; }, true, true},   // (residuals: with the corners)
    /* charuco_poses */ {sizeof(a3_charuco_pose), true, [](const ReadbackShape& s) { return s.charuco && s.pose; }, true, true},
    /* recovered */ {sizeof(uint32_t), true, [](const ReadbackShape& s) { return s.recover; }, true, true},
};
// the kinds a batch of these switches produces, one bit per kind
inline uint32_t sides_on(const ReadbackShape& s) {
    uint32_t m = 0;
    for (int k = 0; k < kSideKinds; k++) m |= (uint32_t)kSides[k].on(s) << k;
    return m;
}

struct Span { size_t off = 0, bytes = 0; };
constexpr size_t kFlagsRec = sizeof(uint32_t);
struct Readback { Span head, markers, charuco_total, charuco, side[kSideKinds], flags; size_t end = 0; };
template <typename T> inline T* at(void* base, const Span& s) { return reinterpret_cast<T*>(static_cast<uint8_t*>(base) + s.off); }

// The spans follow each other without padding: head, markers, then the side results in the table's order, the ChArUco records directly
// ahead of their poses, the marker flags last; the span of a feature that is off is empty.  `refetch`: the layout of refetch_layout below.
inline Readback readback_layout(const ReadbackShape& s, bool refetch = false) {
    Readback r;
    auto put = [&r](Span& sp, bool on, size_t count, size_t elem) { sp = {r.end, on ? count * elem : 0}; r.end += sp.bytes; };
    put(r.head, !refetch, 1, s.head_bytes);   // [scratch 256 B | counters | per-frame counts], a multiple of 8
    put(r.markers, true, s.guess, sizeof(a3_marker));   // (directly behind the head, as on the device: one copy brings both)
    for (int k = 0; k < kSideKinds; k++) {
        if (k == kSideCharucoPoses) {
            put(r.charuco_total, s.charuco && !refetch, 1, 16);   // the record count in the first 4 bytes of a 16-byte slot
            put(r.charuco, s.charuco && !refetch, s.charuco_guess, sizeof(a3_charuco_corner));
        }
        const SideDesc& d = kSides[k];
        put(r.side[k], d.on(s) && !(refetch && d.per_frame), d.per_frame ? s.n : s.guess, d.rec);
    }
    put(r.flags, s.flags, s.guess, kFlagsRec);   // per marker: staged with the guess, fetched again with the whole list
    return r;
}
// The marker guess was short: the head, the per-frame kinds and the ChArUco records have been consumed, and the whole list of `total`
// markers is fetched to the start of the buffer with its per-marker kinds behind it.
inline Readback refetch_layout(ReadbackShape s, uint32_t total) {
    s.guess = total;
    return readback_layout(s, true);
}
// what is asked of the pinned allocation for a layout: 64 KB of slack behind its end
inline size_t pinned_bytes(const Readback& r) { return r.end + (1 << 16); }

}  // namespace a3
