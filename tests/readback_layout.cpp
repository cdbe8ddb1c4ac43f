// The staging layout of a batch's read-back (aruco3_amd/csrc/a3_readback.h) against the byte-offset sums a3_api.hip wrote out by hand
// before the header existed, on every feature combination (the 64 of pose / refine / undist / board / charuco / recover, the ones the
// library never produces included) crossed with frame counts, marker guesses, ChArUco guesses and head sizes.  A stand-alone program, built
// with the address and undefined-behaviour sanitizers by tests/test_readback_layout.py: the simulated round trip copies through a heap
// buffer of exactly the layout's end, so a span that runs past it stops the program.  The table of side results (kSides) is tied to the layout: a
// kind's span holds its record bytes times the guess, the total or the frame count when its switches are on, nothing otherwise.  Prints one
// summary line; exit status 1 and the failed expression on the first mismatch.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../aruco3_amd/csrc/a3_readback.h"

using namespace a3;

namespace {

// the parent's Batch fields that served as offset arithmetic (begin_batch)
struct Parent {
    size_t head_bytes, guess, n, charuco_guess, pose_bytes, refine_bytes, undist_bytes, board_bytes, recover_bytes;
    bool want_pose, charuco;
    explicit Parent(const ReadbackShape& s)
        : head_bytes(s.head_bytes), guess(s.guess), n(s.n), charuco_guess(s.charuco_guess), pose_bytes(s.pose ? 2 * sizeof(a3_pose) : 0),
          refine_bytes(s.refine ? 8 * sizeof(float) : 0), undist_bytes(s.undist ? 12 * sizeof(float) : 0),
          board_bytes(s.board ? (size_t)s.n * sizeof(a3_board_pose) : 0), recover_bytes(s.recover ? (size_t)s.n * 4 : 0), want_pose(s.pose), charuco(s.charuco) {}
    // charuco_stage_off / charuco_stage_bytes
    size_t charuco_stage_off() const { return head_bytes + guess * (sizeof(a3_marker) + pose_bytes + refine_bytes + undist_bytes) + board_bytes; }
    size_t charuco_stage_bytes() const {
        return charuco ? 16 + charuco_guess * sizeof(a3_charuco_corner) + (want_pose ? n * sizeof(a3_charuco_pose) : 0) : 0;
    }
    // ensure_back_buffers: the argument of ensure_pinned (the recovered counts came later, behind everything else)
    size_t pinned() const {
        return head_bytes + guess * (sizeof(a3_marker) + 2 * sizeof(a3_pose) + refine_bytes + undist_bytes) + board_bytes + charuco_stage_bytes() + recover_bytes + (1 << 16);
    }
};

long g_checks = 0;
#define CHECK(cond)                                                                                              \
    do {                                                                                                         \
        g_checks++;                                                                                              \
        if (!(cond)) {                                                                                           \
            printf("FAILED %s (line %d): n %u guess %u charuco_guess %u head %zu pose %d refine %d undist %d board %d charuco %d recover %d total %u\n", #cond, \
                   __LINE__, s.n, s.guess, s.charuco_guess, s.head_bytes, s.pose, s.refine, s.undist, s.board, s.charuco, s.recover, total); \
            exit(1);                                                                                             \
        }                                                                                                        \
    } while (0)

struct Named { const Span* sp; size_t align; };

// disjoint, in the stated order, inside [0, end]; every non-empty span aligned for its record type
void check_order(const ReadbackShape& s, uint32_t total, const Readback& r) {
    const Named spans[] = {{&r.head, alignof(uint64_t)}, {&r.markers, alignof(a3_marker)}, {&r.side[kSidePoses], alignof(a3_pose)},
                           {&r.side[kSideRefined], alignof(float)}, {&r.side[kSideBoard], alignof(a3_board_pose)}, {&r.side[kSideUndist], alignof(float)},
                           {&r.side[kSideUndistRes], alignof(float)}, {&r.charuco_total, alignof(uint32_t)}, {&r.charuco, alignof(a3_charuco_corner)},
                           {&r.side[kSideCharucoPoses], alignof(a3_charuco_pose)}, {&r.side[kSideRecovered], alignof(uint32_t)}};
    size_t at_least = 0;
    for (const Named& x : spans) {
        CHECK(x.sp->off >= at_least);
        CHECK(x.sp->off + x.sp->bytes <= r.end);
        if (x.sp->bytes) CHECK(x.sp->off % x.align == 0);
        at_least = x.sp->off + x.sp->bytes;
    }
}

// One source array per span, each with its own byte pattern: span i's array starts 4099 * i bytes into one table without a short period.
std::vector<uint8_t> g_pattern;
const uint8_t* pattern(unsigned seg, size_t bytes) {
    if (g_pattern.empty()) {
        g_pattern.resize((size_t)5 << 20);
        uint8_t* d = g_pattern.data();
        for (size_t k = 0; k < g_pattern.size(); k++) d[k] = (uint8_t)(((uint32_t)k * 2654435761u) >> 24);
    }
    if (seg * 4099u + bytes > g_pattern.size()) { printf("FAILED: a span of %zu bytes outgrows the pattern table\n", bytes); exit(1); }
    return g_pattern.data() + seg * 4099u;
}
struct Copy { size_t off, bytes; };
// the writer's copies into a heap buffer of exactly `bytes`, then the reader's offsets must give every array back
void round_trip(const ReadbackShape& s, uint32_t total, size_t bytes, const std::vector<Copy>& writes, const std::vector<Copy>& reads) {
    uint8_t* buf = static_cast<uint8_t*>(malloc(bytes ? bytes : 1));
    CHECK(writes.size() == reads.size());
    for (unsigned i = 0; i < writes.size(); i++)
        if (writes[i].bytes) memcpy(buf + writes[i].off, pattern(i, writes[i].bytes), writes[i].bytes);
    for (unsigned i = 0; i < reads.size(); i++)   // (what the reader takes for span i: the writer's count of bytes, from its own offset)
        if (writes[i].bytes) CHECK(memcmp(buf + reads[i].off, pattern(i, writes[i].bytes), writes[i].bytes) == 0);
    free(buf);
}

// the table against a layout: a kind's span holds `markers` (per-marker kinds) or `frames` (per-frame kinds) records when its switches
// are on -- written out here once more, from the issue's table -- and nothing when they are off
void check_table(const ReadbackShape& s, uint32_t total, const Readback& r, size_t markers, size_t frames) {
    const bool on[kSideKinds] = {s.pose, s.refine, s.board, s.undist, s.undist, s.charuco && s.pose, s.recover};
    const size_t rec[kSideKinds] = {2 * sizeof(a3_pose), 32, sizeof(a3_board_pose), 32, 16, sizeof(a3_charuco_pose), 4};
    const bool per_frame[kSideKinds] = {false, false, true, false, false, true, true};
    for (int k = 0; k < kSideKinds; k++) {
        CHECK(kSides[k].rec == rec[k] && kSides[k].per_frame == per_frame[k] && kSides[k].on(s) == on[k]);
        CHECK((sides_on(s) >> k & 1u) == (on[k] ? 1u : 0u));
        CHECK(r.side[k].bytes == (on[k] ? rec[k] * (per_frame[k] ? frames : markers) : 0));
    }
}

void check_staged(const ReadbackShape& s) {
    const uint32_t total = 0;
    const Readback r = readback_layout(s);
    check_table(s, total, r, s.guess, s.n);
    const Parent p(s);
    const size_t g = p.guess, m = sizeof(a3_marker);
    // enqueue_back: the destinations and sizes of its copies
    CHECK(r.head.off == 0 && r.head.bytes == p.head_bytes);
    CHECK(r.markers.off == p.head_bytes && r.head.bytes + r.markers.bytes == p.head_bytes + g * m);   // (head and markers: one copy)
    const size_t h_poses = p.head_bytes + g * m;
    CHECK(r.side[kSidePoses].off == h_poses && r.side[kSidePoses].bytes == g * p.pose_bytes);
    CHECK(r.side[kSideRefined].off == h_poses + g * p.pose_bytes && r.side[kSideRefined].bytes == g * p.refine_bytes);
    CHECK(r.side[kSideBoard].off == h_poses + g * (p.pose_bytes + p.refine_bytes) && r.side[kSideBoard].bytes == p.board_bytes);
    const size_t hu = h_poses + g * (p.pose_bytes + p.refine_bytes) + p.board_bytes;
    CHECK(r.side[kSideUndist].off == hu && r.side[kSideUndist].bytes == (p.undist_bytes ? g * 32 : 0));
    CHECK(r.side[kSideUndistRes].off == hu + (p.undist_bytes ? g * 32 : 0) && r.side[kSideUndistRes].bytes == (p.undist_bytes ? g * 16 : 0));
    const size_t hc = p.charuco_stage_off();
    CHECK(r.charuco_total.off == hc && r.charuco_total.bytes == (p.charuco ? 16u : 0u));
    if (p.charuco) {   // (the parent computed these only with ChArUco on)
        CHECK(r.charuco.off == hc + 16 && r.charuco.bytes == p.charuco_guess * sizeof(a3_charuco_corner));
        CHECK(r.side[kSideCharucoPoses].off == hc + 16 + p.charuco_guess * sizeof(a3_charuco_corner));
    }
    CHECK(r.side[kSideCharucoPoses].bytes == (p.charuco && p.want_pose ? p.n * sizeof(a3_charuco_pose) : 0));
    CHECK(r.side[kSideRecovered].off == hc + p.charuco_stage_bytes() && r.side[kSideRecovered].bytes == p.recover_bytes);
    CHECK(r.end == hc + p.charuco_stage_bytes() + p.recover_bytes);
    check_order(s, total, r);
    // ensure_back_buffers
    CHECK(pinned_bytes(r) >= r.end && pinned_bytes(r) <= p.pinned());
    // finish_batch: the sources it read from (its own copy of every sum)
    const size_t f_markers = p.head_bytes, f_poses = p.head_bytes + g * m, f_refined = p.head_bytes + g * (m + p.pose_bytes);
    const size_t f_undist = p.head_bytes + g * (m + p.pose_bytes + p.refine_bytes) + p.board_bytes, f_undist_res = f_undist + g * 8 * sizeof(float);
    const size_t f_board = p.head_bytes + g * (m + p.pose_bytes + p.refine_bytes);
    const size_t f_charuco = hc + 16, f_charuco_poses = hc + 16 + p.charuco_guess * sizeof(a3_charuco_corner);
    const size_t f_recovered = hc + p.charuco_stage_bytes();
    const Span* spans[] = {&r.head, &r.markers, &r.side[kSidePoses], &r.side[kSideRefined], &r.side[kSideBoard], &r.side[kSideUndist], &r.side[kSideUndistRes], &r.charuco_total, &r.charuco, &r.side[kSideCharucoPoses], &r.side[kSideRecovered]};
    std::vector<Copy> writes;
    for (const Span* sp : spans) writes.push_back({sp->off, sp->bytes});
    round_trip(s, total, r.end, writes,
               {{0, 0}, {f_markers, 0}, {f_poses, 0}, {f_refined, 0}, {f_board, 0}, {f_undist, 0}, {f_undist_res, 0}, {hc, 0}, {f_charuco, 0},
                {f_charuco_poses, 0}, {f_recovered, 0}});
}

void check_refetch(const ReadbackShape& s, uint32_t total, bool copy) {
    const Readback r = refetch_layout(s, total);
    check_table(s, total, r, total, 0);
    const Parent p(s);
    const size_t t = total, m = sizeof(a3_marker);
    // finish_batch, `if (total > guess)`: markers at the start of the buffer, poses, refined corners, undistorted corners, residuals
    const size_t f_poses = t * m, f_refined = t * (m + p.pose_bytes), f_undist = t * (m + p.pose_bytes + p.refine_bytes);
    const size_t f_undist_res = f_undist + (p.undist_bytes ? t * 8 * sizeof(float) : 0);   // (h_undist + total * 8, with distortion only)
    CHECK(r.head.bytes == 0 && r.markers.off == 0 && r.markers.bytes == t * m);
    CHECK(r.side[kSidePoses].off == f_poses && r.side[kSidePoses].bytes == t * p.pose_bytes);
    CHECK(r.side[kSideRefined].off == f_refined && r.side[kSideRefined].bytes == t * p.refine_bytes);
    CHECK(r.side[kSideUndist].off == f_undist && r.side[kSideUndist].bytes == (p.undist_bytes ? t * 32 : 0));
    CHECK(r.side[kSideUndistRes].off == f_undist_res && r.side[kSideUndistRes].bytes == (p.undist_bytes ? t * 16 : 0));
    CHECK(r.side[kSideBoard].bytes == 0 && r.charuco_total.bytes == 0 && r.charuco.bytes == 0 && r.side[kSideCharucoPoses].bytes == 0);
    CHECK(r.side[kSideRecovered].bytes == 0);
    CHECK(r.end == t * (m + p.pose_bytes + p.refine_bytes + p.undist_bytes));
    check_order(s, total, r);
    CHECK(pinned_bytes(r) >= r.end && pinned_bytes(r) <= t * (m + 2 * sizeof(a3_pose) + p.refine_bytes + p.undist_bytes) + (1 << 16));
    if (!copy) return;
    const Span* spans[] = {&r.markers, &r.side[kSidePoses], &r.side[kSideRefined], &r.side[kSideUndist], &r.side[kSideUndistRes]};
    std::vector<Copy> writes;
    for (const Span* sp : spans) writes.push_back({sp->off, sp->bytes});
    round_trip(s, total, r.end, writes, {{0, 0}, {f_poses, 0}, {f_refined, 0}, {f_undist, 0}, {f_undist_res, 0}});
}

}  // namespace

int main() {
    long cases = 0, refetches = 0;
    for (unsigned features = 0; features < 64; features++)
        for (uint32_t n : {1u, 3u, 256u})
            for (uint32_t guess : {0u, 1u, 64u, 65u, 4096u})
                for (uint32_t charuco_guess : {0u, 1u, 64u, n * 24u})
                    for (size_t head_bytes : {(size_t)264, (size_t)400, ((size_t)4 * n + 1288 + 7) & ~(size_t)7}) {
                        const ReadbackShape s{n, guess, charuco_guess, head_bytes, (features & 1) != 0, (features & 2) != 0, (features & 4) != 0,
                                              (features & 8) != 0, (features & 16) != 0, (features & 32) != 0};
                        check_staged(s);
                        cases++;
                        // (the re-fetch reads neither the head nor the ChArUco guess: its offsets are checked on every case, the
                        // copies -- up to 10 MB each -- once per feature set, frame count, guess and total)
                        for (uint32_t total : {guess + 1u, 10u * guess + 7u}) { check_refetch(s, total, charuco_guess == 0 && head_bytes == 264); refetches++; }
                    }
    printf("readback layout: %ld staged cases, %ld re-fetch cases, %ld checks\n", cases, refetches, g_checks);
    return 0;
}
