// The batch head, the verdict and the plan arithmetic (aruco3_amd/csrc/a3_batch_head.h) without a GPU.  Three parts:
//   1. designed cases: one input per branch of batch_verdict and per precedence pair, each with the action, code, message, hints and
//      stats written out by hand from finish_batch as it stood before the header existed;
//   2. a seeded random sweep against that finish_batch's decision sequence, transcribed here literally (parent_finish: it reads the
//      scratch words by number, hs[N], and the context's loose fields) -- action, code, message, hints and stats must agree on every
//      head, and every branch must be reached;
//   3. the plan functions against the loops and sums enqueue_chain held, transcribed the same way.
// A stand-alone program, built with the address and undefined-behaviour sanitizers by tests/test_batch_verdict.py.  Prints one summary
// line; exit status 1 and the failed expression on the first mismatch.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../aruco3_amd/csrc/a3_batch_head.h"

using namespace a3;

namespace {

long g_checks = 0;
const char* g_case = "";
#define CHECK(cond)                                                                              \
    do {                                                                                         \
        g_checks++;                                                                              \
        if (!(cond)) { printf("FAILED %s (line %d) in: %s\n", #cond, __LINE__, g_case); exit(1); } \
    } while (0)

// ---- the parent's finish_batch, from the wait to the last check, on a stand-in for the context ------------------------------------------
struct ParentStats { uint64_t darts = 0, contours_traced = 0, contours_materialised = 0; uint32_t jump_rounds = 0, resolve_iterations = 0; };
struct ParentCtx {
    uint64_t max_points; uint32_t max_contours, max_cand;
    int jump_rounds_hint, resolve_iters_hint, resolve_full_ttl, entry_global_ttl;
    bool plan_valid, force_host_plan; uint32_t plan_n, plan_W, plan_H; uint64_t plan_darts;
    ParentStats stats; uint32_t dbg_nd = 0;
    int err_code = 0; const char* err = nullptr;
};
struct ParentBatch { bool device_plan; uint32_t n, W, H; size_t n_chunks; uint64_t chunk0_darts; int rounds_max; };
struct ParentOut { int branch = -1; uint32_t total = 0, n_work = 0, n_pre = 0, tap_contours = 0; uint64_t tap_points = 0; size_t want = 0; };
enum Branch { kPlanOverflow, kEntryOverflow, kJumpShort, kResolveNotRun, kResolveMorePasses, kPoolGrowth, kBrokenEvent, kScatter, kResolveFailed,
              kCandLimit, kSlotLimit, kCandGrowth, kMarkerCapFlag, kOutCap, kDelivered, kBranches };
int fail(ParentCtx* c, int code, const char* what) { c->err_code = code; c->err = what; return code; }
#define AT(k) o.branch = k;

// slot_base: sizeof(CandRec) + 16 + 16 + 4 + decode_out_bytes() + proj_rec_bytes() of the library; the device always has room here
int parent_finish(ParentCtx* ctx, const ParentBatch& b, const unsigned int* hs, const DeviceCounters* hc, size_t out_cap, uint32_t lds_slots_,
                  size_t slot_base, ParentOut& o) {
    const size_t n_chunks = b.n_chunks;
    const uint32_t n = b.n;
    if (b.device_plan) {
        if (hs[9]) { ctx->force_host_plan = true; AT(kPlanOverflow) return 1; }   // the graph outgrew the hint: plan on the host this once
        ctx->stats.darts = hs[8];
        ctx->dbg_nd = hs[8];
        ctx->plan_darts = hs[8];
    } else {
        ctx->plan_valid = n_chunks == 1;
        ctx->plan_n = n; ctx->plan_W = b.W; ctx->plan_H = b.H;
        ctx->plan_darts = n_chunks == 1 ? b.chunk0_darts : 0;
    }
    unsigned int flags = hs[4];
    for (int sh = 0; sh < 16; sh++) ctx->stats.contours_traced += hs[48 + sh];   // borders finished inside k_local_contract (kDead)
    uint64_t need_points = 0; uint32_t need_contours = 0;
    bool jump_short = false, resolve_needed = false, entry_overflow = false;
    for (size_t ci = 0; ci < n_chunks; ci++) {
        flags |= hc[ci].err_flags;
        resolve_needed |= hc[ci].resolve_needed != 0;
        entry_overflow |= hc[ci].entry_overflow != 0;
        need_points = std::max<uint64_t>(need_points, hc[ci].points);
        need_contours = std::max(need_contours, hc[ci].contours);
        ctx->stats.contours_traced += hc[ci].traced;
        ctx->stats.contours_materialised += hc[ci].contours;
        for (int r = 0; r < 32; r++) if (hc[ci].jump_changed[r]) ctx->stats.jump_rounds = std::max<uint32_t>(ctx->stats.jump_rounds, r + 1);
        uint32_t it = hc[ci].resolve_needed ? 1 : 0;
        for (int r = 0; r < 16 - 1; r++) if (hc[ci].resolve_changed[r]) it = r + 2;
        ctx->stats.resolve_iterations = std::max(ctx->stats.resolve_iterations, it);
        if (b.rounds_max > 0 && b.rounds_max < 32 && hc[ci].jump_changed[b.rounds_max - 1] != 0) jump_short = true;
    }
    if (entry_overflow) { ctx->entry_global_ttl = 64; ctx->jump_rounds_hint = std::max(ctx->jump_rounds_hint, 12); AT(kEntryOverflow) return 1; }
    if (ctx->entry_global_ttl > 0) ctx->entry_global_ttl--;
    if (jump_short && ctx->jump_rounds_hint < 32) { ctx->jump_rounds_hint = 32; AT(kJumpShort) return 1; }
    if (resolve_needed) {
        const bool ran = ctx->resolve_full_ttl > 0;
        ctx->resolve_full_ttl = 64;
        if (!ran) { AT(kResolveNotRun) return 1; }
    } else if (ctx->resolve_full_ttl > 0) ctx->resolve_full_ttl--;
    if ((flags & 16u) && ctx->resolve_iters_hint < 16) { ctx->resolve_iters_hint = 16; AT(kResolveMorePasses) return 1; }
    ctx->jump_rounds_hint = std::max(4, std::min(32, (int)ctx->stats.jump_rounds + 2));
    if (flags & (2u | 4u)) {
        if (need_points > ctx->max_points) ctx->max_points = std::min<uint64_t>(3ull << 30, std::max(need_points, ctx->max_points * 2));
        if (need_contours > ctx->max_contours) ctx->max_contours = std::max(need_contours, ctx->max_contours * 2);
        AT(kPoolGrowth) return 1;
    }
    if (flags & 1u) { AT(kBrokenEvent) return fail(ctx, A3_ERR_INTERNAL, "contour graph: a start event lies on an open chain"); }
    if (flags & 64u) { AT(kScatter) return fail(ctx, A3_ERR_INTERNAL, "contour points: a border slot, rank or point index out of range"); }
    if (flags & 16u) { AT(kResolveFailed) return fail(ctx, A3_ERR_INTERNAL, "contour start resolution did not converge"); }
    if (flags & 8u) {
        const uint32_t lds_slots = lds_slots_, need = std::max(hs[5], ctx->max_cand + 1u);
        if (need > 65536u) { AT(kCandLimit) return fail(ctx, A3_ERR_LIMIT, "a frame holds more than 65536 quad candidates (A3_MAX_CANDIDATES_PER_FRAME)"); }
        uint32_t next = ctx->max_cand;
        while (next < need) next = next < lds_slots ? std::min(lds_slots, next * 2) : std::min(65536u, next * 2);
        if ((uint64_t)n * next > 0xFFFFFFFFull) { AT(kSlotLimit) return fail(ctx, A3_ERR_LIMIT, "frames x candidate slots per frame exceeds 2^32: fewer frames per call"); }
        {
            const size_t per_slot = slot_base + (next > lds_slots ? 4 : 0);
            o.want = (size_t)n * next * per_slot;
        }
        ctx->max_cand = next;
        AT(kCandGrowth) return 1;
    }
    if (flags & 32u) { AT(kMarkerCapFlag) return fail(ctx, A3_ERR_CAPACITY, "out_cap is smaller than the number of markers found"); }
    const uint32_t total = hs[1];
    if (total > out_cap) { AT(kOutCap) return fail(ctx, A3_ERR_CAPACITY, "out_cap is smaller than the number of markers found"); }
    o.total = total; o.n_work = hs[0]; o.n_pre = hs[2];
    o.tap_contours = n_chunks ? hc[0].contours : 0u; o.tap_points = n_chunks ? hc[0].points : 0ull;
    AT(kDelivered) return 0;
}

// ---- one input, through both ------------------------------------------------------------------------------------------------------------
constexpr size_t kSlotBase = 100;
struct In {
    unsigned int hs[64] = {};
    DeviceCounters hc[3] = {};
    BatchFacts f{4, 640, 480, false, 1, 1000, 10, 100, 6144, kSlotBase};
    BatchHints h;
};
static_assert(sizeof(BatchScratch) == sizeof(In::hs), "the head is 64 words");
struct Result { int rc; Verdict v; BatchHints h; ParentOut o; };

bool same_text(const char* a, const char* b) { return (a == nullptr) == (b == nullptr) && (!a || strcmp(a, b) == 0); }

// runs the header and the transcript on `in`; they must agree on everything.  -> what the header said, with finish_batch's commit of a
// table growth applied (the device has room)
Result run(const In& in) {
    Result r;
    r.h = in.h;
    BatchScratch head;
    memcpy(&head, in.hs, sizeof head);
    r.v = batch_verdict(head, in.hc, in.f, r.h);
    if (r.v.action == Verdict::GrowCands) r.h.max_cand = r.v.next_cand;
    r.rc = r.v.action == Verdict::Deliver ? 0 : r.v.action == Verdict::Fail ? r.v.code : 1;

    const BatchHints& h0 = in.h;
    ParentCtx c{h0.max_points, h0.max_contours, h0.max_cand, h0.jump_rounds_hint, h0.resolve_iters_hint, h0.resolve_full_ttl, h0.entry_global_ttl,
                h0.plan_valid, h0.force_host_plan, h0.plan_n, h0.plan_W, h0.plan_H, h0.plan_darts, {}, 0, 0, nullptr};
    const ParentBatch b{in.f.device_plan, in.f.n, in.f.W, in.f.H, in.f.n_chunks, in.f.chunk0_darts, in.f.rounds_max};
    const int rc = parent_finish(&c, b, in.hs, in.hc, in.f.out_cap, in.f.lds_slots, kSlotBase, r.o);
    CHECK(rc == r.rc);
    CHECK((rc < 0) == (r.v.action == Verdict::Fail) && (r.o.branch == kCandGrowth) == (r.v.action == Verdict::GrowCands));
    if (rc < 0) CHECK(c.err_code == r.v.code && same_text(c.err, r.v.message));
    else CHECK(r.v.code == A3_OK && r.v.message == nullptr);
    const BatchHints& h = r.h;
    CHECK(h.max_points == c.max_points && h.max_contours == c.max_contours && h.max_cand == c.max_cand);
    CHECK(h.jump_rounds_hint == c.jump_rounds_hint && h.resolve_iters_hint == c.resolve_iters_hint);
    CHECK(h.resolve_full_ttl == c.resolve_full_ttl && h.entry_global_ttl == c.entry_global_ttl);
    CHECK(h.plan_valid == c.plan_valid && h.force_host_plan == c.force_host_plan && h.plan_n == c.plan_n && h.plan_W == c.plan_W && h.plan_H == c.plan_H);
    CHECK(h.plan_darts == c.plan_darts);
    if (in.f.device_plan && r.o.branch != kPlanOverflow) CHECK(r.v.darts == c.stats.darts && r.v.darts == c.dbg_nd);
    CHECK(r.v.contours_traced == c.stats.contours_traced && r.v.contours_materialised == c.stats.contours_materialised);
    CHECK(r.v.jump_rounds == c.stats.jump_rounds && r.v.resolve_iterations == c.stats.resolve_iterations);
    if (r.o.branch == kCandGrowth) CHECK((size_t)in.f.n * r.v.next_cand * r.v.slot_bytes == r.o.want);
    if (rc == 0) {
        CHECK(r.v.total == r.o.total && r.v.n_work == r.o.n_work && r.v.n_pre == r.o.n_pre);
        CHECK(r.v.tap_contours == r.o.tap_contours && r.v.tap_points == r.o.tap_points);
    }
    return r;
}

// ---- 1. designed cases ------------------------------------------------------------------------------------------------------------------
const char* const kMsgBroken = "contour graph: a start event lies on an open chain";
const char* const kMsgScatter = "contour points: a border slot, rank or point index out of range";
const char* const kMsgResolve = "contour start resolution did not converge";
const char* const kMsgCandLimit = "a frame holds more than 65536 quad candidates (A3_MAX_CANDIDATES_PER_FRAME)";
const char* const kMsgSlotLimit = "frames x candidate slots per frame exceeds 2^32: fewer frames per call";
const char* const kMsgOutCap = "out_cap is smaller than the number of markers found";

// a quiet one-chunk host-planned batch of 4 frames: 7 markers from 9 work items of 11 quads, 5 borders of 50 points out of 6 traced in
// the chunk and 1 + 2 finished early (dead shards 0 and 15), three doubling rounds that did work
In quiet() {
    In in;
    in.hs[0] = 9; in.hs[1] = 7; in.hs[2] = 11; in.hs[48] = 1; in.hs[63] = 2;
    in.hc[0].contours = 5; in.hc[0].points = 50; in.hc[0].traced = 6;
    in.hc[0].jump_changed[0] = in.hc[0].jump_changed[1] = in.hc[0].jump_changed[2] = 1;
    return in;
}
bool is(const Result& r, Verdict::Action a, int code = A3_OK, const char* msg = nullptr) {
    return r.v.action == a && r.v.code == code && same_text(r.v.message, msg);
}
long designed_cases() {
    long cases = 0;
#define CASE(name) g_case = name; cases++;
    const BatchHints d;   // a new context's hints
    {   CASE("deliver: host plan, one chunk")
        const Result r = run(quiet());
        CHECK(is(r, Verdict::Deliver) && r.v.total == 7 && r.v.n_work == 9 && r.v.n_pre == 11 && r.v.tap_contours == 5 && r.v.tap_points == 50);
        CHECK(r.v.contours_traced == 9 && r.v.contours_materialised == 5 && r.v.jump_rounds == 3 && r.v.resolve_iterations == 0);
        CHECK(r.h.plan_valid && r.h.plan_n == 4 && r.h.plan_W == 640 && r.h.plan_H == 480 && r.h.plan_darts == 1000 && !r.h.force_host_plan);
        CHECK(r.h.jump_rounds_hint == 5 && r.h.resolve_iters_hint == 4 && r.h.resolve_full_ttl == 0 && r.h.entry_global_ttl == 0);
        CHECK(r.h.max_points == d.max_points && r.h.max_contours == d.max_contours && r.h.max_cand == 1024);
    }
    {   CASE("deliver: host plan, two chunks and none")
        In in = quiet(); in.f.n_chunks = 2; in.hc[1].contours = 8; in.hc[1].points = 70; in.hc[1].traced = 10; in.hc[1].jump_changed[6] = 1;
        in.hc[1].resolve_needed = 0; in.hc[1].resolve_changed[0] = 1; in.h.plan_valid = true; in.h.plan_darts = 5;
        Result r = run(in);
        CHECK(is(r, Verdict::Deliver) && !r.h.plan_valid && r.h.plan_darts == 0 && r.v.contours_traced == 19 && r.v.contours_materialised == 13);
        CHECK(r.v.jump_rounds == 7 && r.h.jump_rounds_hint == 9 && r.v.resolve_iterations == 2 && r.v.tap_contours == 5 && r.v.tap_points == 50);
        in = quiet(); in.f.n_chunks = 0; in.hc[0].err_flags = kErrBrokenEvent;   // (counters the batch does not own are not looked at)
        r = run(in);
        CHECK(is(r, Verdict::Deliver) && r.v.tap_contours == 0 && r.v.tap_points == 0 && r.v.contours_traced == 3 && r.h.jump_rounds_hint == 4 && !r.h.plan_valid);
    }
    {   CASE("deliver: device plan keeps the shape and follows the dart total")
        In in = quiet(); in.f.device_plan = true; in.hs[8] = 4321; in.hs[10] = 2000; in.hs[11] = 4321;
        in.h.plan_valid = true; in.h.plan_n = 4; in.h.plan_W = 640; in.h.plan_H = 480; in.h.plan_darts = 4000;
        const Result r = run(in);
        CHECK(is(r, Verdict::Deliver) && r.v.darts == 4321 && r.h.plan_darts == 4321 && r.h.plan_valid && r.h.plan_n == 4);
    }
    {   CASE("device-plan overflow: before everything, an entry overflow included")
        In in = quiet(); in.f.device_plan = true; in.hs[9] = 1; in.hs[11] = 99999; in.hc[0].entry_overflow = 1; in.hs[4] = kErrBrokenEvent;
        in.h.entry_global_ttl = 3; in.h.plan_darts = 4000;
        const Result r = run(in);
        CHECK(is(r, Verdict::Rerun) && r.h.force_host_plan && r.h.entry_global_ttl == 3 && r.h.jump_rounds_hint == 10 && r.h.plan_darts == 4000);
        CHECK(r.v.contours_traced == 0 && r.v.jump_rounds == 0);
        in.f.device_plan = false;   // the same words on a host-planned batch: nobody wrote the plan, the entry overflow speaks
        CHECK(run(in).o.branch == kEntryOverflow);
    }
    {   CASE("entry overflow: before a short jump launch")
        In in = quiet(); in.hc[0].entry_overflow = 1; in.hc[0].jump_changed[9] = 1; in.h.entry_global_ttl = 5;
        Result r = run(in);
        CHECK(is(r, Verdict::Rerun) && r.h.entry_global_ttl == 64 && r.h.jump_rounds_hint == 12);
        in.h.jump_rounds_hint = 20;
        r = run(in);
        CHECK(is(r, Verdict::Rerun) && r.h.entry_global_ttl == 64 && r.h.jump_rounds_hint == 20);
    }
    {   CASE("short jump launch; with the hint already 32; TTL decay")
        In in = quiet(); in.hc[0].jump_changed[9] = 1; in.h.entry_global_ttl = 5;
        Result r = run(in);
        CHECK(is(r, Verdict::Rerun) && r.h.jump_rounds_hint == 32 && r.h.entry_global_ttl == 4 && r.v.jump_rounds == 10);
        in.h.jump_rounds_hint = 32;   // all rounds were allowed: the last one launched moved something, and that is that
        r = run(in);
        CHECK(is(r, Verdict::Deliver) && r.h.jump_rounds_hint == 12 && r.h.entry_global_ttl == 4);
        in.h.jump_rounds_hint = 10; in.f.rounds_max = 32; in.hc[0].jump_changed[31] = 1;   // a launch of 32 rounds is never short
        r = run(in);
        CHECK(is(r, Verdict::Deliver) && r.v.jump_rounds == 32 && r.h.jump_rounds_hint == 32);
        in = quiet(); in.f.rounds_max = 0; in.h.entry_global_ttl = 1; in.h.resolve_full_ttl = 1;
        r = run(in);
        CHECK(is(r, Verdict::Deliver) && r.h.entry_global_ttl == 0 && r.h.resolve_full_ttl == 0);
        CHECK(run(quiet()).h.entry_global_ttl == 0);
    }
    {   CASE("jump_rounds_hint = clamp(jump_rounds + 2, 4, 32)")
        In in = quiet(); in.f.rounds_max = 0;
        for (int r = 0; r < 32; r++) in.hc[0].jump_changed[r] = 0;
        CHECK(run(in).h.jump_rounds_hint == 4);
        in.hc[0].jump_changed[0] = 1; CHECK(run(in).h.jump_rounds_hint == 4);
        in.hc[0].jump_changed[1] = 1; CHECK(run(in).h.jump_rounds_hint == 4);
        in.hc[0].jump_changed[2] = 1; CHECK(run(in).h.jump_rounds_hint == 5);
        in.hc[0].jump_changed[28] = 1; CHECK(run(in).h.jump_rounds_hint == 31);
        in.hc[0].jump_changed[29] = 1; CHECK(run(in).h.jump_rounds_hint == 32);
        in.hc[0].jump_changed[31] = 1; CHECK(run(in).h.jump_rounds_hint == 32);
    }
    {   CASE("resolve_needed: TTL above zero delivers, at zero re-runs")
        In in = quiet(); in.hc[0].resolve_needed = 1; in.hc[0].resolve_changed[0] = 1; in.hc[0].resolve_changed[1] = 1;
        Result r = run(in);
        CHECK(is(r, Verdict::Rerun) && r.h.resolve_full_ttl == 64 && r.h.jump_rounds_hint == 10 && r.v.resolve_iterations == 3);
        in.h.resolve_full_ttl = 1;
        r = run(in);
        CHECK(is(r, Verdict::Deliver) && r.h.resolve_full_ttl == 64 && r.v.resolve_iterations == 3);
        in.hc[0].resolve_changed[0] = in.hc[0].resolve_changed[1] = 0;
        CHECK(run(in).v.resolve_iterations == 1);
        in.hc[0].resolve_changed[14] = 1; in.hc[0].resolve_changed[15] = 1;   // (the last slot names no pass that could follow)
        CHECK(run(in).v.resolve_iterations == 16);
    }
    {   CASE("kErrResolve: below the maximum a re-run, at the maximum an error")
        In in = quiet(); in.hc[0].err_flags = kErrResolve; in.hs[4] = kErrPointPool;
        Result r = run(in);
        CHECK(is(r, Verdict::Rerun) && r.h.resolve_iters_hint == 16 && r.h.jump_rounds_hint == 10 && r.h.max_points == d.max_points);
        in.h.resolve_iters_hint = 16; in.hs[4] = 0;
        r = run(in);
        CHECK(is(r, Verdict::Fail, A3_ERR_INTERNAL, kMsgResolve) && r.h.jump_rounds_hint == 5);
        in.hs[4] = kErrPointPool;   // a pool that overflowed is grown first
        CHECK(is(run(in), Verdict::Rerun));
    }
    {   CASE("pool growth: need below the pool, above it, points capped")
        In in = quiet(); in.hs[4] = kErrPointPool | kErrContourTable; in.h.max_points = 1000; in.h.max_contours = 100;
        Result r = run(in);   // 50 points, 5 contours: nothing grows, still a re-run
        CHECK(is(r, Verdict::Rerun) && r.h.max_points == 1000 && r.h.max_contours == 100 && r.h.jump_rounds_hint == 5);
        in.hc[0].points = 1500; in.hc[0].contours = 150;   // above: at least double
        r = run(in);
        CHECK(is(r, Verdict::Rerun) && r.h.max_points == 2000 && r.h.max_contours == 200);
        in.hc[0].points = 2500; in.hc[0].contours = 250; in.hc[0].err_flags = kErrPointPool; in.hs[4] = 0;   // the need where it is more than double
        r = run(in);
        CHECK(is(r, Verdict::Rerun) && r.h.max_points == 2500 && r.h.max_contours == 250);
        in.f.n_chunks = 2; in.hc[1].points = 4ull << 30; in.hc[1].contours = 7;   // the largest chunk's need; points end at kHardMaxPoints
        r = run(in);
        CHECK(is(r, Verdict::Rerun) && r.h.max_points == kHardMaxPoints && kHardMaxPoints == 3ull << 30 && r.h.max_contours == 250);
        in.h.max_points = 2ull << 30; in.hc[1].points = (2ull << 30) + 1;
        CHECK(run(in).h.max_points == kHardMaxPoints);
    }
    {   CASE("the three internal errors, in their order")
        In in = quiet(); in.hs[4] = kErrBrokenEvent | kErrScatter | kErrCandTable | kErrMarkerCap; in.h.resolve_iters_hint = 16; in.hc[0].err_flags = kErrResolve;
        CHECK(is(run(in), Verdict::Fail, A3_ERR_INTERNAL, kMsgBroken));
        in.hs[4] &= ~kErrBrokenEvent;
        CHECK(is(run(in), Verdict::Fail, A3_ERR_INTERNAL, kMsgScatter));
        in.hs[4] &= ~kErrScatter;
        CHECK(is(run(in), Verdict::Fail, A3_ERR_INTERNAL, kMsgResolve));
        in.hc[0].err_flags = 0;
        CHECK(is(run(in), Verdict::GrowCands));
        in.hs[4] = kErrMarkerCap;
        CHECK(is(run(in), Verdict::Fail, A3_ERR_CAPACITY, kMsgOutCap));
    }
    {   CASE("candidate tables: the ladder for 6144 LDS slots")
        In in = quiet(); in.hs[4] = kErrCandTable;   // word 5 is 0: one step at a time
        const uint32_t ladder[] = {1024, 2048, 4096, 6144, 12288, 24576, 49152, 65536};
        for (int i = 0; i + 1 < 8; i++) {
            in.h.max_cand = ladder[i];
            const Result r = run(in);
            CHECK(is(r, Verdict::GrowCands) && r.v.next_cand == ladder[i + 1] && r.h.max_cand == ladder[i + 1]);
            CHECK(r.v.slot_bytes == kSlotBase + (ladder[i + 1] > 6144 ? 4 : 0));
        }
        in.h.max_cand = 65536;
        CHECK(is(run(in), Verdict::Fail, A3_ERR_LIMIT, kMsgCandLimit));
    }
    {   CASE("candidate tables: straight to the table that holds word 5; the two limits")
        In in = quiet(); in.hs[4] = kErrCandTable;
        const uint32_t most[] = {1025, 2048, 2049, 4097, 6144, 6145, 12289, 50000, 65536}, next[] = {2048, 2048, 4096, 6144, 6144, 12288, 24576, 65536, 65536};
        for (int i = 0; i < 9; i++) { in.hs[5] = most[i]; CHECK(run(in).v.next_cand == next[i]); }
        in.hs[5] = 100;   // (a count the table holds: the flag still asks for the next table)
        CHECK(run(in).v.next_cand == 2048);
        in.hs[5] = 65537;
        Result r = run(in);
        CHECK(is(r, Verdict::Fail, A3_ERR_LIMIT, kMsgCandLimit) && r.h.max_cand == 1024);
        in.hs[5] = 5000; in.f.n = 699051;   // x 6144 = 2^32 + 2048
        r = run(in);
        CHECK(is(r, Verdict::Fail, A3_ERR_LIMIT, kMsgSlotLimit) && r.h.max_cand == 1024);
        in.f.n = 699050;   // x 6144 = 2^32 - 4096
        CHECK(is(run(in), Verdict::GrowCands));
        in.f.n = 65536; in.hs[5] = 65536; CHECK(is(run(in), Verdict::Fail, A3_ERR_LIMIT, kMsgSlotLimit));   // x 65536 = 2^32: one more than fits
        in.f.n = 65535; CHECK(is(run(in), Verdict::GrowCands));
    }
    {   CASE("kErrMarkerCap and total > out_cap")
        In in = quiet(); in.hc[0].err_flags = kErrMarkerCap;
        CHECK(is(run(in), Verdict::Fail, A3_ERR_CAPACITY, kMsgOutCap));
        in.hc[0].err_flags = 0; in.f.out_cap = 6;
        CHECK(is(run(in), Verdict::Fail, A3_ERR_CAPACITY, kMsgOutCap));
        in.f.out_cap = 7;
        CHECK(is(run(in), Verdict::Deliver));
    }
#undef CASE
    return cases;
}

// ---- 2. the sweep -----------------------------------------------------------------------------------------------------------------------
uint64_t g_rng = 0x9E3779B97F4A7C15ull;
uint32_t rnd() {   // splitmix64
    uint64_t z = (g_rng += 0x9E3779B97F4A7C15ull);
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return (uint32_t)((z ^ (z >> 31)) >> 16);
}
bool one_in(uint32_t k) { return rnd() % k == 0; }
template <typename T, size_t N> T pick(const T (&a)[N]) { return a[rnd() % N]; }

In random_input() {
    In in;
    const uint32_t frames[] = {1, 3, 64, 4096, 65535, 65536, 65537, 699050, 699051, 1u << 20};
    const uint32_t tables[] = {1024, 2048, 4096, 6144, 12288, 24576, 49152, 65536, 1500, 8192};
    const uint32_t counts[] = {0, 1, 1025, 5000, 6144, 6145, 30000, 65536, 65537, 0xFFFFFFFFu};
    const uint64_t pools[] = {1000, 64ull << 20, 2ull << 30, 3ull << 30};
    const uint64_t needs[] = {0, 999, 1001, 1ull << 27, (2ull << 30) + 1, 5ull << 30};
    const int hints[] = {4, 10, 12, 31, 32}, ttls[] = {0, 0, 1, 2, 64};
    BatchFacts& f = in.f;
    f.n = pick(frames); f.W = 1 + rnd() % 4000; f.H = 1 + rnd() % 3000; f.device_plan = one_in(2); f.n_chunks = f.device_plan ? 1 : rnd() % 4;
    f.chunk0_darts = rnd(); f.rounds_max = (int)(rnd() % 34); f.out_cap = one_in(4) ? rnd() % 8 : 1000; f.lds_slots = one_in(8) ? 4096 : 6144;
    BatchHints& h = in.h;
    h.jump_rounds_hint = pick(hints); h.resolve_iters_hint = one_in(2) ? 4 : 16; h.resolve_full_ttl = pick(ttls); h.entry_global_ttl = pick(ttls);
    h.plan_valid = one_in(2); h.force_host_plan = false; h.plan_n = f.n; h.plan_W = rnd(); h.plan_H = rnd(); h.plan_darts = rnd();
    h.max_points = pick(pools); h.max_contours = one_in(2) ? 100 : 1u << 20; h.max_cand = pick(tables);
    for (unsigned int& w : in.hs) w = one_in(4) ? rnd() % 9 : 0;   // (the unused words too: nobody may read them)
    in.hs[1] = rnd() % 12; in.hs[5] = pick(counts); in.hs[9] = one_in(12); in.hs[8] = rnd();
    unsigned int flags = 0;
    for (unsigned bit : {kErrBrokenEvent, kErrPointPool, kErrContourTable, kErrCandTable, kErrResolve, kErrMarkerCap, kErrScatter, 128u}) if (one_in(10)) flags |= bit;
    if (one_in(3)) flags |= kErrCandTable;
    in.hs[4] = one_in(2) ? flags : 0;
    for (DeviceCounters& c : in.hc) {   // (all three, whatever n_chunks says)
        c.darts = rnd(); c.points = pick(needs); c.contours = one_in(3) ? 3u << 20 : rnd() % 200; c.traced = rnd() % 1000;
        c.err_flags = one_in(3) ? flags : 0; c.resolve_needed = one_in(8) ? 1 + rnd() % 2 : 0; c.entry_overflow = one_in(16);
        const uint32_t live = rnd() % 33;
        for (uint32_t r = 0; r < 32; r++) c.jump_changed[r] = r < live && !one_in(8) ? 1 + rnd() % 5 : 0;
        if (one_in(4)) for (uint32_t r = 0; r < 16; r++) c.resolve_changed[r] = one_in(3);
        c.pad[0] = rnd();
    }
    return in;
}

// ---- 3. the plan ------------------------------------------------------------------------------------------------------------------------
// enqueue_chain's chunk loop and base loop as they stood; -> false: refused
bool parent_split(const std::vector<uint64_t>& fd, uint64_t& max_darts, uint32_t max_frames, std::vector<Chunk>& chunks, uint64_t& stats_darts,
                  uint32_t& max_chunk_frames, uint64_t& max_chunk_darts, std::vector<uint32_t>& bases) {
    const uint32_t n = (uint32_t)fd.size();
    uint64_t biggest = 0;
    for (uint64_t v : fd) { biggest = std::max(biggest, v); stats_darts += v; }
    if (biggest > (1ull << 30) - (1ull << 16)) return false;
    if (biggest > max_darts) max_darts = biggest;  // one frame must fit; grow the pool
    Chunk c{0, 0, 0, 0};
    for (uint32_t f = 0; f < n; f++) {
        if (c.count && (c.darts + fd[f] > max_darts || c.count >= max_frames)) { chunks.push_back(c); c = Chunk{f, 0, 0, 0}; }
        c.count++; c.darts += fd[f]; c.max_frame_darts = (uint32_t)std::max<uint64_t>(c.max_frame_darts, fd[f]);
    }
    if (c.count) chunks.push_back(c);
    max_chunk_frames = 0; max_chunk_darts = 0;
    for (auto& c : chunks) { max_chunk_frames = std::max(max_chunk_frames, c.count); max_chunk_darts = std::max(max_chunk_darts, c.darts); }
    for (auto& c : chunks) {
        uint32_t acc = 0;
        for (uint32_t i = 0; i < max_chunk_frames + 1; i++) {
            bases.push_back(acc);
            if (i < c.count) acc += (uint32_t)fd[c.first + i];
        }
    }
    return true;
}
void check_split(const std::vector<uint64_t>& fd, uint64_t max_darts, uint32_t max_frames) {
    const uint32_t n = (uint32_t)fd.size();
    std::vector<Chunk> want, got(n);
    std::vector<uint32_t> want_bases;
    uint64_t want_max = max_darts, want_total = 0, want_chunk_darts = 0; uint32_t want_frames = 0;
    const bool ok = parent_split(fd, want_max, max_frames, want, want_total, want_frames, want_chunk_darts, want_bases);
    const ChunkSplit s = split_chunks(fd.data(), n, max_darts, max_frames, got.data());
    CHECK(s.refused == !ok && s.total_darts == want_total);
    if (!ok) { CHECK(s.max_darts == max_darts && s.n_chunks == 0); return; }
    CHECK(s.max_darts == want_max && s.n_chunks == want.size() && s.max_chunk_frames == want_frames && s.max_chunk_darts == want_chunk_darts);
    const size_t stride = (size_t)s.max_chunk_frames + 1;
    uint32_t* bases = static_cast<uint32_t*>(malloc(std::max<size_t>(stride * s.n_chunks, 1) * 4));   // exactly what enqueue_chain stages
    uint32_t next_frame = 0;
    for (uint32_t i = 0; i < s.n_chunks; i++) {
        const Chunk& a = got[i], & b = want[i];
        CHECK(a.first == b.first && a.count == b.count && a.darts == b.darts && a.max_frame_darts == b.max_frame_darts);
        CHECK(a.first == next_frame && a.count >= 1 && a.count <= max_frames && a.darts <= s.max_darts);
        next_frame += a.count;
        chunk_frame_bases(fd.data(), a, (uint32_t)stride, bases + i * stride);
    }
    CHECK(next_frame == n && want_bases.size() == stride * s.n_chunks);
    CHECK(want_bases.empty() || memcmp(bases, want_bases.data(), want_bases.size() * 4) == 0);
    free(bases);
}
long plan_cases() {
    long cases = 0;
    g_case = "chunk split and frame bases";
    const uint64_t hard = (1ull << 30) - (1ull << 16);
    CHECK(kHardMaxDarts == hard && kMaxChunkFrames == 65536);
    check_split({}, 1000, 8); cases++;
    check_split({0, 0, 0}, 1000, 8); cases++;                      // empty frames: one chunk of nothing
    check_split({0, 5, 0, 0, 7, 0}, 10, 8); cases++;
    check_split({3, 5000, 4}, 1000, 8); cases++;                   // one frame larger than max_darts: the pool grows to it
    check_split({5000}, 1000, 8); cases++;
    check_split({3, hard, 4}, 1000, 8); cases++;                   // the largest frame that is not refused
    check_split({3, hard + 1, 4}, 1000, 8); cases++;               // refused
    check_split({1ull << 40}, 48ull << 20, kMaxChunkFrames); cases++;
    check_split({600, 400, 1, 999, 1000, 1}, 1000, 8); cases++;    // a chunk filled exactly
    check_split(std::vector<uint64_t>(kMaxChunkFrames, 2), 48ull << 20, kMaxChunkFrames); cases++;       // exactly one chunk's frames
    check_split(std::vector<uint64_t>(kMaxChunkFrames + 1, 2), 48ull << 20, kMaxChunkFrames); cases++;   // ... and one more
    check_split(std::vector<uint64_t>(kMaxChunkFrames + 1, 0), 48ull << 20, kMaxChunkFrames); cases++;
    for (int k = 0; k < 3000; k++) {   // random mixes
        std::vector<uint64_t> fd(rnd() % 40);
        const uint64_t scales[] = {1, 10, 1000, 1u << 20};
        const uint64_t scale = pick(scales);
        for (uint64_t& v : fd) v = one_in(4) ? 0 : one_in(50) ? hard + rnd() % 3 - 1 : rnd() % (scale * 30);
        check_split(fd, scale * (1 + rnd() % 40), 1 + rnd() % 9);
        cases++;
    }
    g_case = "doubling rounds";
    for (uint64_t d = 0; d <= 0xFFFFFFFFull; d = d < 70 ? d + 1 : d * 2 - 1 + rnd() % 3)
        for (int hint : {4, 10, 12, 31, 32})
            for (int cap : {0, 1, 5, 40}) {
                int rounds = 1;   // enqueue_chain's lines
                while ((1ull << rounds) < (uint64_t)(uint32_t)d && rounds < 31) rounds++;
                rounds += 1;  // the round that observes "nothing moved"
                rounds = std::min(rounds, hint);
                if (cap > 0 && hint < 32) rounds = std::min(rounds, cap);
                CHECK(chunk_rounds((uint32_t)d, hint, cap) == rounds);
                cases++;
            }
    CHECK(chunk_rounds(0, 32, 0) == 2 && chunk_rounds(2, 32, 0) == 2 && chunk_rounds(3, 32, 0) == 3 && chunk_rounds(1024, 32, 0) == 11 && chunk_rounds(1025, 32, 0) == 12);
    CHECK(chunk_rounds(0xFFFFFFFFu, 32, 0) == 32 && chunk_rounds(0xFFFFFFFFu, 32, 3) == 32 && chunk_rounds(0xFFFFFFFFu, 31, 3) == 3 && chunk_rounds(1024, 10, 0) == 10);
    g_case = "zero_layout";
    CHECK(sizeof(DeviceCounters) == 232 && sizeof(a3_marker) == 56);
    for (size_t n_chunks : {1, 2, 7})
        for (uint32_t chunk_frames : {1u, 3u, 64u, 1000u})
            for (uint32_t n : {1u, 3u, 64u, 1001u, 65537u})
                for (uint32_t marker_cap : {1u, 1024u, 100000u}) {
                    const ZeroLayout z = zero_layout(n_chunks, chunk_frames, n, marker_cap);
                    const size_t head = (256 + 232 * n_chunks + 4 * (size_t)n + 7) / 8 * 8;
                    const size_t counts = (4 * (size_t)chunk_frames + 4 * (size_t)n + 15) / 16 * 16;   // frame_cursor | cand_count
                    CHECK(z.ctr_bytes == 232 * n_chunks && z.head_bytes == head && z.head_off == (counts + 255) / 256 * 256);
                    CHECK(z.total == z.head_off + head + 56 * (size_t)marker_cap && z.head_off >= 4 * ((size_t)chunk_frames + n));
                    cases++;
                }
    g_case = "marker_cap_of, marker_guess_of";
    CHECK(marker_cap_of(1024, 4, 100) == 100 && marker_cap_of(1024, 4, 0) == 1 && marker_cap_of(1024, 4, 5000) == 4096 && marker_cap_of(65536, 65535, ~(size_t)0) == 0xFFFF0000u);
    CHECK(marker_guess_of(0, 1000) == 64 && marker_guess_of(100, 1000) == 189 && marker_guess_of(100, 150) == 150 && marker_guess_of(0xFFFFFFFFu, 0xFFFFFFFFu) == 0xFFFFFFFFu);
    cases += 8;
    g_case = "pool_darts_of";
    const uint64_t K = 1ull << 17;
    CHECK(pool_darts_of(0, 0, 2) == 1 && pool_darts_of(0, 12345, 2) == 12345 && pool_darts_of(1ull << 40, 12345, 0) == 12345);   // several chunks: as asked
    CHECK(pool_darts_of(0, 0, 1) == K && pool_darts_of(0, 1, 1) == K && pool_darts_of(0, K, 1) == K && pool_darts_of(0, K + 1, 1) == 2 * K);
    CHECK(pool_darts_of(0, 16 * K, 1) == 16 * K && pool_darts_of(0, 16 * K + 1, 1) == 16 * K + 2 * K);      // the step doubles above 16 steps
    CHECK(pool_darts_of(0, 32 * K, 1) == 32 * K && pool_darts_of(0, 32 * K + 1, 1) == 32 * K + 4 * K);
    CHECK(pool_darts_of(0, 30 * K + 1, 1) == 32 * K && pool_darts_of(0, 28 * K, 1) == 28 * K);
    CHECK(pool_darts_of(48ull << 20, 1000, 1) == 2 * K);                            // 1000 * 1.5 + 128 k = 132 572, below the limit
    CHECK(pool_darts_of(48ull << 20, 40ull << 20, 1) == 48ull << 20);               // the limit, where 1.5 x would pass it
    CHECK(pool_darts_of(48ull << 20, 50ull << 20, 1) == 52ull << 20);               // a chunk above the limit: itself, in steps of 4 M
    CHECK(pool_darts_of(0, hard - 5, 1) == hard && pool_darts_of(0, hard, 1) == hard && pool_darts_of(0, hard + 1, 1) == hard + 1);   // never past the hard limit by rounding
    cases += 20;
    for (int k = 0; k < 20000; k++) {   // an eighth of an octave: 16 to 32 steps in the pool, less than a step added
        const uint64_t want = ((uint64_t)rnd() << (rnd() % 8)) % hard + 1, got = pool_darts_of(0, want, 1);
        uint64_t step = K;
        while (step * 16 < want) step <<= 1;
        CHECK(got >= want && got - want < step && (got % step == 0 || got == hard) && (want <= 16 * K || (step * 8 < want && want <= step * 16)));
        cases++;
    }
    g_case = "device_plan_capacity";
    BatchHints h;
    h.plan_valid = true; h.plan_n = 8; h.plan_W = 640; h.plan_H = 480; h.plan_darts = 1000;
    const uint64_t md = 48ull << 20;
    CHECK(device_plan_capacity(h, md, 8, 640, 480) == 1000 + 250 + 65536);
    { BatchHints x = h; x.plan_valid = false; CHECK(device_plan_capacity(x, md, 8, 640, 480) == 0); }
    { BatchHints x = h; x.force_host_plan = true; CHECK(device_plan_capacity(x, md, 8, 640, 480) == 0); }
    CHECK(device_plan_capacity(h, md, 9, 640, 480) == 0 && device_plan_capacity(h, md, 8, 641, 480) == 0 && device_plan_capacity(h, md, 8, 640, 479) == 0);
    { BatchHints x = h; x.plan_n = 65537; CHECK(device_plan_capacity(x, md, 65537, 640, 480) == 0); x.plan_n = 65536; CHECK(device_plan_capacity(x, md, 65536, 640, 480) == 66786); }
    CHECK(device_plan_capacity(h, 66786, 8, 640, 480) == 66786 && device_plan_capacity(h, 66785, 8, 640, 480) == 0);
    { BatchHints x = h; x.plan_darts = 0; CHECK(device_plan_capacity(x, md, 8, 640, 480) == 65536); x.plan_darts = 7; CHECK(device_plan_capacity(x, md, 8, 640, 480) == 65544); }
    cases += 13;
    return cases;
}

}  // namespace

int main() {
    const long designed = designed_cases();
    g_case = "the sweep";
    long per_branch[kBranches] = {};
    const long heads = 200000;
    for (long i = 0; i < heads; i++) per_branch[run(random_input()).o.branch]++;
    for (int k = 0; k < kBranches; k++)
        if (per_branch[k] == 0) { printf("FAILED: the sweep never reached branch %d\n", k); return 1; }
    const long plans = plan_cases();
    printf("batch verdict: %ld designed cases, %ld random heads over %d branches (fewest %ld), %ld plan cases, %ld checks\n", designed, heads, (int)kBranches,
           *std::min_element(per_branch, per_branch + kBranches), plans, g_checks);
    return 0;
}
