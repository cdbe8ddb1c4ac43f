// Where a batch's results lie in the pinned staging buffer they are read back through -- the one definition: ensure_back_buffers sizes
// the buffer by it, enqueue_back copies to its spans, finish_batch reads from them (a3_api.hip).  Host arithmetic on the public header's
// records only -- no HIP, no context -- so a plain C++ program checks every case (tests/readback_layout.cpp).
#pragma once
#include <cstddef>
#include <cstdint>

#include "../../include/aruco3_hip.h"

namespace a3 {

// what the batch record knows: frames, markers and ChArUco records read back speculatively, the bytes of the head, what is switched on
// (recover: the batch ran board-aided recovery -- one count per frame travels behind everything else)
struct ReadbackShape { uint32_t n, guess, charuco_guess; size_t head_bytes; bool pose, refine, undist, board, charuco; bool recover = false; };
struct Span { size_t off = 0, bytes = 0; };
struct Readback { Span head, markers, poses, refined, board, undist, undist_res, charuco_total, charuco, charuco_poses; size_t end = 0; Span recovered; };
template <typename T> inline T* at(void* base, const Span& s) { return reinterpret_cast<T*>(static_cast<uint8_t*>(base) + s.off); }

// The spans follow each other in this order without padding; the span of a feature that is off is empty.
inline Readback readback_layout(const ReadbackShape& s) {
    Readback r;
    auto put = [&r](Span& sp, bool on, size_t count, size_t elem) { sp = {r.end, on ? count * elem : 0}; r.end += sp.bytes; };
    put(r.head, true, 1, s.head_bytes);   // [scratch 256 B | counters | per-frame counts], a multiple of 8
    put(r.markers, true, s.guess, sizeof(a3_marker));   // (directly behind the head, as on the device: one copy brings both)
    put(r.poses, s.pose, s.guess, 2 * sizeof(a3_pose));
    put(r.refined, s.refine, s.guess, 8 * sizeof(float));
    put(r.board, s.board, s.n, sizeof(a3_board_pose));   // one per frame, whatever the marker count
    put(r.undist, s.undist, s.guess, 8 * sizeof(float));
    put(r.undist_res, s.undist, s.guess, 4 * sizeof(float));
    put(r.charuco_total, s.charuco, 1, 16);   // the record count in the first 4 bytes of a 16-byte slot
    put(r.charuco, s.charuco, s.charuco_guess, sizeof(a3_charuco_corner));
    put(r.charuco_poses, s.charuco && s.pose, s.n, sizeof(a3_charuco_pose));   // one per frame
    put(r.recovered, s.recover, s.n, sizeof(uint32_t));   // recovered markers per frame (last: every span before it lies where it lay)
    return r;
}
// The marker guess was short: head, board poses, ChArUco results and recovered counts have been consumed, and the whole list of `total` markers is
// fetched to the start of the buffer: markers, poses, refined corners, undistorted corners, residuals.
inline Readback refetch_layout(ReadbackShape s, uint32_t total) {
    s.head_bytes = 0; s.guess = total; s.board = s.charuco = s.recover = false;
    return readback_layout(s);
}
// what is asked of the pinned allocation for a layout: 64 KB of slack behind its end
inline size_t pinned_bytes(const Readback& r) { return r.end + (1 << 16); }

}  // namespace a3
