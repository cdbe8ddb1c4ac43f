// a3_board.h -- the board-pose pieces of include/aruco3_hip.h (a3_set_board, a3_set_board3d, a3_set_charuco): board slots, the frame's run of
// the marker list, the duplicate bitmap, the start marker and its IPPE, the per-corner residual / Jacobian sums, the LDL^T step, the Cayley
// update, the Levenberg-Marquardt loop, and board_pose_body<Model>, the one body of the three pose kernels.  A Model is a small struct that
// says where a correspondence comes from, how it is summed, how the start marker's pose is carried into the board frame, what is counted
// and when a solve is attempted: PlanarMarkers (k_board_pose, below), Board3Markers (k_board3d_pose, a3_board3d.h) and CharucoRecords
// (k_charuco_pose, k_charuco.hip).  k_charuco_interp and k_recover_frames take the frame run and the duplicate bitmap from here too.
// Built with -ffp-contract=off: the same inputs give the same bits in every kernel.
#pragma once
#include <cmath>

#include "a3_common.h"
#include "a3_ippe.h"
#include "a3_launch.h"

namespace a3 {

constexpr uint16_t kNoSlot = 0xFFFF;
constexpr int kBoardCache = 4;   // corners per lane held in registers (lane l: l, l + 64, l + 128, l + 192)

struct BoardSlot {   // per board marker, built by a3_set_board (host, float)
    float x[4], y[4];
    float side, cs, sn, cx, cy, pad[3];
};
static_assert(sizeof(BoardSlot) == 64, "BoardSlot is 64 bytes");

struct BoardArgs {
    const a3_marker* markers;     // batch: the compacted marker list; nullptr: stand-alone (ids / pts)
    const uint32_t* ids;          // stand-alone: n ids
    const float* pts;             // stand-alone: 8 float corners per marker, pixels
    const float* refined;         // batch with refinement: 8 floats per marker (nullable)
    const unsigned int* n_dev;    // batch: markers produced
    const uint32_t* per_frame;    // batch: markers per frame
    uint32_t n, n_frames;         // batch: marker capacity; stand-alone: marker count (one frame)
    const uint16_t* slot_of;      // n_codes entries, kNoSlot: not on the board
    uint32_t n_codes;
    const BoardSlot* slots;
    int has_intr;
    float iw, ih, fx, fy, cx, cy;
    a3_board_pose* out;
};

// the kernels' view of a marker source and the board's tables (a3_launch.h); intr == nullptr: normalised by the image size
inline BoardArgs board_args(const MarkerSrc& m, const BoardTables& t, const a3_intrinsics* intr, uint32_t W, uint32_t H) {
    BoardArgs a{};
    a.markers = m.markers; a.ids = m.ids; a.pts = m.pts; a.refined = m.corners; a.n_dev = m.n_dev; a.per_frame = m.per_frame;
    a.n = m.n; a.n_frames = m.n_frames; a.slot_of = t.slot_of; a.n_codes = t.n_codes; a.slots = reinterpret_cast<const BoardSlot*>(t.slots);
    a.has_intr = intr ? 1 : 0; a.iw = (float)W; a.ih = (float)H;
    if (intr) { a.fx = intr->focal_x; a.fy = intr->focal_y; a.cx = intr->principal_x; a.cy = intr->principal_y; }
    return a;
}

struct BoardAcc {
    float h[21], g[6], cost, pix;
};

__device__ __forceinline__ uint32_t board_slot(const BoardArgs& a, uint32_t m) {
    const uint32_t id = a.markers ? a.markers[m].id : a.ids[m];
    return id < a.n_codes ? (uint32_t)a.slot_of[id] : (uint32_t)kNoSlot;
}

// image corner k of marker m in pixels (refined, integer, or the caller's floats)
__device__ __forceinline__ void board_image_px(const BoardArgs& a, uint32_t m, int k, float* x, float* y) {
    if (a.refined) { *x = a.refined[8 * (size_t)m + 2 * k]; *y = a.refined[8 * (size_t)m + 2 * k + 1]; }
    else if (a.markers) { *x = (float)a.markers[m].corners[2 * k]; *y = (float)a.markers[m].corners[2 * k + 1]; }
    else { *x = a.pts[8 * (size_t)m + 2 * k]; *y = a.pts[8 * (size_t)m + 2 * k + 1]; }
}

// as k_pose normalises (modes 0 / 1, 3 / 4)
__device__ __forceinline__ void board_normalise(const BoardArgs& a, float x, float y, float* u, float* v) {
    if (a.has_intr) { *u = (x - a.cx) / a.fx; *v = (y - a.cy) / a.fy; }
    else { *u = x / a.iw; *v = y / a.ih; }
}

__device__ __forceinline__ bool board_dup(const uint32_t* s_dup, uint32_t slot) { return (s_dup[slot >> 5] >> (slot & 31)) & 1u; }

// corner c of the frame (marker first + c / 4, corner c % 4): board point and normalised image point; false when not used
__device__ __forceinline__ bool board_corner(const BoardArgs& a, const uint32_t* s_dup, uint32_t first, uint32_t c, float* bx, float* by,
                                             float* mx, float* my) {
    const uint32_t m = first + (c >> 2);
    const int k = (int)(c & 3u);
    const uint32_t slot = board_slot(a, m);
    if (slot == kNoSlot || board_dup(s_dup, slot)) return false;
    *bx = a.slots[slot].x[k]; *by = a.slots[slot].y[k];
    float x, y;
    board_image_px(a, m, k, &x, &y);
    board_normalise(a, x, y, mx, my);
    return true;
}

__device__ __forceinline__ void board_accum(BoardAcc& s, const float R[9], const float t[3], float bx, float by, float mx, float my,
                                            float sx, float sy) {
    const float qx = R[0] * bx + R[1] * by, qy = R[3] * bx + R[4] * by, qz = R[6] * bx + R[7] * by;
    const float px = qx + t[0], py = qy + t[1], pz = qz + t[2];
    const float zz = pz > 1e-5f ? pz : 1e-5f;
    const float u = px / zz, v = py / zz;
    const float a = 1.0f / zz, a2 = 2.0f * a;
    const float ru = u - mx, rv = v - my;
    const float ju[6] = {-(a2 * u) * qy, a2 * (qz + u * qx), -a2 * qy, a, 0.0f, -(a * u)};
    const float jv[6] = {-a2 * (qz + v * qy), (a2 * v) * qx, a2 * qx, 0.0f, a, -(a * v)};
    int idx = 0;
    for (int r = 0; r < 6; r++) {
        for (int c = r; c < 6; c++) { s.h[idx] += ju[r] * ju[c] + jv[r] * jv[c]; idx++; }
        s.g[r] += ju[r] * ru + jv[r] * rv;
    }
    s.cost += ru * ru + rv * rv;
    const float eu = ru * sx, ev = rv * sy;
    s.pix += eu * eu + ev * ev;
}

__device__ __forceinline__ float wave_sum_f(float v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ uint32_t wave_sum_u(uint32_t v) {
    for (int o = 32; o >= 1; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// (J^T J + lambda diag(J^T J)) d = -J^T r by LDL^T; false when a pivot is not positive and finite
__device__ __forceinline__ bool board_solve(const float h[21], const float g[6], float lambda, float d[6]) {
    float A[6][6];
    int idx = 0;
    for (int r = 0; r < 6; r++)
        for (int c = r; c < 6; c++) { A[r][c] = h[idx]; A[c][r] = h[idx]; idx++; }
    for (int r = 0; r < 6; r++) A[r][r] = A[r][r] + lambda * A[r][r];
    float L[6][6], D[6];
    for (int j = 0; j < 6; j++) {
        for (int i = j; i < 6; i++) {
            float s = A[i][j];
            for (int k = 0; k < j; k++) s = s - L[i][k] * L[j][k] * D[k];
            if (i == j) {
                if (!(s > 0.0f) || !isfinite(s)) return false;
                D[j] = s;
                L[j][j] = 1.0f;
            } else L[i][j] = s / D[j];
        }
    }
    float y[6];
    for (int i = 0; i < 6; i++) {
        float s = -g[i];
        for (int k = 0; k < i; k++) s = s - L[i][k] * y[k];
        y[i] = s;
    }
    for (int i = 5; i >= 0; i--) {
        float s = y[i] / D[i];
        for (int k = i + 1; k < 6; k++) s = s - L[k][i] * d[k];
        d[i] = s;
    }
    return true;
}

// R <- cay(w) R
__device__ __forceinline__ void board_cayley(const float w[3], const float R[9], float Rn[9]) {
    const float n2 = (w[0] * w[0] + w[1] * w[1]) + w[2] * w[2];
    const float k = 2.0f / (1.0f + n2);
    const float W[9] = {0.0f, -w[2], w[1], w[2], 0.0f, -w[0], -w[1], w[0], 0.0f};
    float C[9];
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) {
            const float w2 = w[r] * w[c] - (r == c ? n2 : 0.0f);
            C[3 * r + c] = (r == c ? 1.0f : 0.0f) + k * (W[3 * r + c] + w2);
        }
    for (int r = 0; r < 3; r++)
        for (int c = 0; c < 3; c++) Rn[3 * r + c] = (C[3 * r] * R[c] + C[3 * r + 1] * R[3 + c]) + C[3 * r + 2] * R[6 + c];
}

__device__ __forceinline__ bool pose_finite(const a3_pose& p) {
    bool ok = true;
    for (int q = 0; q < 9; q++) ok = ok && isfinite(p.rotation[q]);
    for (int q = 0; q < 3; q++) ok = ok && isfinite(p.translation[q]);
    return ok;
}

// IPPE of marker m of the frame (normalised as the per-marker poses), with that marker's board side
__device__ __forceinline__ void board_ippe(const BoardArgs& a, uint32_t m, float side, a3_pose* p0, a3_pose* p1) {
    float pts[8];
    for (int k = 0; k < 4; k++) {
        float x, y;
        board_image_px(a, m, k, &x, &y);
        board_normalise(a, x, y, &pts[2 * k], &pts[2 * k + 1]);
    }
    solve_normalized(pts, side, p0, p1);
}

// Levenberg-Marquardt from (R, t) as the contract states it; evaluate(R, t, acc) sums one state over the caller's correspondences
// (wave-uniform result).  -> evaluations; `s` holds the final state's sums.
template <typename Eval>
__device__ __forceinline__ uint32_t board_lm(Eval&& evaluate, float R[9], float t[3], BoardAcc& s) {
    evaluate(R, t, s);
    uint32_t evals = 1;
    float lambda = 1e-3f;
    while (evals < A3_BOARD_MAX_EVALS && s.cost > 0.0f) {
        float d[6];
        if (!board_solve(s.h, s.g, lambda, d)) { lambda = lambda * 10.0f; evals++; continue; }
        float Rn[9], tn[3];
        board_cayley(d, R, Rn);
        for (int r = 0; r < 3; r++) tn[r] = t[r] + d[3 + r];
        BoardAcc s2;
        evaluate(Rn, tn, s2);
        evals++;
        if (s2.cost < s.cost) {
            const float rel = (s.cost - s2.cost) / s.cost;
            for (int q = 0; q < 9; q++) R[q] = Rn[q];
            for (int q = 0; q < 3; q++) t[q] = tn[q];
            s = s2;
            lambda = lambda / 10.0f;
            if (rel < A3_BOARD_REL_TOL) break;
        } else lambda = lambda * 10.0f;
    }
    return evals;
}

// The frame's run of the marker list: first index and count (every lane of every wave gets the same).  batch: frame f's run starts at
// the sum of per_frame before it and ends at the list's end, min(n, *n_dev), at the latest; stand-alone: the n caller markers, one frame.
__device__ __forceinline__ void board_frame_run(bool batch, const uint32_t* per_frame, uint32_t n, const unsigned int* n_dev, uint32_t f, int lane,
                                                uint32_t* first, uint32_t* cnt) {
    *first = 0; *cnt = n;
    if (batch) {
        uint32_t before = 0;
        for (uint32_t g = (uint32_t)lane; g < f; g += 64) before += per_frame[g];
        *first = wave_sum_u(before);
        const uint32_t limit = min(n, *n_dev);
        *cnt = *first >= limit ? 0u : min(per_frame[f], limit - *first);
    }
}

// The duplicate rule on two LDS bitmaps over the board slots (A3_BOARD_MAX_MARKERS / 32 words each): s_seen gets the slots of the run's
// cnt markers, s_dup those met more than once.  Called by the whole workgroup (two barriers); the threads with `takes_part` walk the run
// from `t` in steps of `stride`.  slot_of(i): the slot of the run's marker i, kNoSlot for one that does not count.
template <typename SlotOf>
__device__ __forceinline__ void board_mark_duplicates(uint32_t* s_seen, uint32_t* s_dup, uint32_t cnt, bool takes_part, uint32_t t, uint32_t stride,
                                                      SlotOf&& slot_of) {
    if (threadIdx.x < A3_BOARD_MAX_MARKERS / 32) { s_seen[threadIdx.x] = 0; s_dup[threadIdx.x] = 0; }
    __syncthreads();
    if (takes_part)
        for (uint32_t i = t; i < cnt; i += stride) {
            const uint32_t slot = slot_of(i);
            if (slot == kNoSlot) continue;
            const uint32_t bit = 1u << (slot & 31);
            if (atomicOr(&s_seen[slot >> 5], bit) & bit) atomicOr(&s_dup[slot >> 5], bit);
        }
    __syncthreads();
}

struct BoardStart {
    uint32_t used, rejected;              // the run's board markers: not duplicated / duplicated (wave sums)
    uint32_t best_i;                      // this lane's best marker of the run ...
    unsigned long long best_key, top;     // ... its key, and the wave's largest key (0: no marker has finite IPPE poses)
};

// The counts and the start marker: the largest image quad whose IPPE poses are finite, then the lowest slot.  Slot: BoardSlot or
// Board3Slot (.side is read).  Behind a test of .top, the owner lane's best_i names the marker and the key's low half the slot.
template <typename Slot>
__device__ __forceinline__ BoardStart board_start_marker(const BoardArgs& a, const Slot* slots, const uint32_t* s_dup, uint32_t first, uint32_t cnt,
                                                         int lane) {
    BoardStart b{};
    for (uint32_t i = (uint32_t)lane; i < cnt; i += 64) {
        const uint32_t slot = board_slot(a, first + i);
        if (slot == kNoSlot) continue;
        if (board_dup(s_dup, slot)) { b.rejected++; continue; }
        b.used++;
        float x[4], y[4];
        for (int k = 0; k < 4; k++) board_image_px(a, first + i, k, &x[k], &y[k]);
        float s = 0.0f;
        for (int k = 0; k < 4; k++) { const int k1 = (k + 1) & 3; s = s + (x[k] * y[k1] - x[k1] * y[k]); }
        const float area = 0.5f * fabsf(s);
        const unsigned long long key = ((unsigned long long)__float_as_uint(area) << 32) | (unsigned long long)(0xFFFFu - slot);
        if (key > b.best_key) {
            a3_pose q0, q1;
            board_ippe(a, first + i, slots[slot].side, &q0, &q1);
            if (pose_finite(q0) && pose_finite(q1)) { b.best_key = key; b.best_i = i; }
        }
    }
    b.used = wave_sum_u(b.used);
    b.rejected = wave_sum_u(b.rejected);
    b.top = b.best_key;
    for (int o = 32; o >= 1; o >>= 1) { const unsigned long long v = __shfl_xor(b.top, o); b.top = v > b.top ? v : b.top; }
    return b;
}

// the start marker's IPPE pose carried into the board frame by the marker's in-plane rotation and centre
__device__ __forceinline__ void board_planar_start(const BoardSlot& bs, const a3_pose& pm, float R[9], float t[3]) {
    const float* Rm = pm.rotation;
    for (int r = 0; r < 3; r++) {
        R[3 * r] = Rm[3 * r] * bs.cs - Rm[3 * r + 1] * bs.sn;
        R[3 * r + 1] = Rm[3 * r] * bs.sn + Rm[3 * r + 1] * bs.cs;
        R[3 * r + 2] = Rm[3 * r + 2];
    }
    for (int r = 0; r < 3; r++) t[r] = pm.translation[r] - (R[3 * r] * bs.cx + R[3 * r + 1] * bs.cy);
}

// The pose kernels' body: one workgroup of two waves per frame, one wave per IPPE start, so the two solves, each a serial chain of small
// reductions and a 6x6 solve, overlap.  The frame's markers are a contiguous run of the marker list; duplicate board ids are found on
// the LDS bitmaps by the first wave.  Correspondences are not kept in LDS: a lane caches the first kBoardCache it owns in registers and
// re-reads the rest from L2 on every evaluation, so a frame with many costs bandwidth, not occupancy.  Every sum ends in an xor
// butterfly, which leaves the same bits in every lane: the solve state and the control flow are wave-uniform.  A Model gives
//   Slot, Record, Corr           the slot record, the output record (a3_board_pose's pose fields), one correspondence
//   slots(a)                     the board's slot records
//   bind(a, f, lane, first, cnt, s_dup)   the frame, before the duplicates are marked
//   count(), corner(a, c, o)     the correspondences 0 .. count(): o <- correspondence c, false when it is not used
//   accum(s, R, t, o, sx, sy)    one correspondence's terms of the sums
//   start(bs, pm, R, t)          the start marker's IPPE pose pm carried into the board frame
//   solves(top), denominator(b), counts(rec, b)   whether a solve is attempted, what rms_px divides by, the record's counts
template <typename Model>
__device__ __forceinline__ void board_pose_body(const BoardArgs& a, Model m, typename Model::Record* out) {
    __shared__ uint32_t s_seen[A3_BOARD_MAX_MARKERS / 32], s_dup[A3_BOARD_MAX_MARKERS / 32];
    __shared__ float s_res[2][16];   // per start: R (9), t (3), cost, pixel cost, evaluations (as bits)
    const uint32_t f = blockIdx.x;
    const int wave = threadIdx.x >> 6, lane = threadIdx.x & 63;
    const typename Model::Slot* const slots = Model::slots(a);
    uint32_t first, cnt;
    board_frame_run(a.markers != nullptr, a.per_frame, a.n, a.n_dev, f, lane, &first, &cnt);
    m.bind(a, f, lane, first, cnt, s_dup);
    board_mark_duplicates(s_seen, s_dup, cnt, wave == 0, (uint32_t)lane, 64u, [&](uint32_t i) { return board_slot(a, first + i); });
    const BoardStart b = board_start_marker(a, slots, s_dup, first, cnt, lane);
    const bool solve = m.solves(b.top != 0);   // (uniform over the workgroup)
    if (solve) {
        const unsigned long long owners = __ballot(b.best_key == b.top);
        const uint32_t mi = first + (uint32_t)__shfl((int)b.best_i, (int)__builtin_ctzll(owners));
        const typename Model::Slot& bs = slots[0xFFFFu - (uint32_t)(b.top & 0xFFFFu)];
        a3_pose p[2];
        board_ippe(a, mi, bs.side, &p[0], &p[1]);
        const a3_pose& pm = wave ? p[1] : p[0];
        const float sx = a.has_intr ? a.fx : a.iw, sy = a.has_intr ? a.fy : a.ih;
        const uint32_t nc = m.count();
        // ---- the lane's cached correspondences ----
        typename Model::Corr cached[kBoardCache];
        bool cok[kBoardCache];
        for (int j = 0; j < kBoardCache; j++) {
            const uint32_t c = (uint32_t)lane + 64u * (uint32_t)j;
            cok[j] = c < nc && m.corner(a, c, cached[j]);
        }
        auto evaluate = [&](const float R[9], const float t[3], BoardAcc& s) {
            for (int q = 0; q < 21; q++) s.h[q] = 0.0f;
            for (int q = 0; q < 6; q++) s.g[q] = 0.0f;
            s.cost = 0.0f; s.pix = 0.0f;
            for (int j = 0; j < kBoardCache; j++)
                if (cok[j]) Model::accum(s, R, t, cached[j], sx, sy);
            for (uint32_t c = (uint32_t)lane + 64u * kBoardCache; c < nc; c += 64) {
                typename Model::Corr o;
                if (m.corner(a, c, o)) Model::accum(s, R, t, o, sx, sy);
            }
            for (int q = 0; q < 21; q++) s.h[q] = wave_sum_f(s.h[q]);
            for (int q = 0; q < 6; q++) s.g[q] = wave_sum_f(s.g[q]);
            s.cost = wave_sum_f(s.cost);
            s.pix = wave_sum_f(s.pix);
        };
        // ---- this wave's start, carried into the board frame, then Levenberg-Marquardt ----
        float R[9], t[3];
        Model::start(bs, pm, R, t);
        BoardAcc s;
        const uint32_t evals = board_lm(evaluate, R, t, s);
        if (lane == 0) {
            for (int q = 0; q < 9; q++) s_res[wave][q] = R[q];
            for (int q = 0; q < 3; q++) s_res[wave][9 + q] = t[q];
            s_res[wave][12] = s.cost; s_res[wave][13] = s.pix; s_res[wave][14] = __uint_as_float(evals);
        }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
        typename Model::Record rec{};
        m.counts(rec, b);
        if (solve) {
            const int k = s_res[1][12] < s_res[0][12] ? 1 : 0;   // (ties: the first IPPE pose)
            const float den = m.denominator(b);
            rec.status = A3_BOARD_OK;
            rec.iterations = __float_as_uint(s_res[k][14]);
            rec.rms_px = sqrtf(s_res[k][13] / den);
            rec.alt_rms_px = sqrtf(s_res[1 - k][13] / den);
            for (int q = 0; q < 9; q++) rec.rotation[q] = s_res[k][q];
            for (int q = 0; q < 3; q++) rec.translation[q] = s_res[k][9 + q];
        }
        out[f] = rec;
    }
}

// What the planar and the 3-D marker models share: the correspondences are the four corners of the run's markers, every board marker not
// duplicated is counted, and any start marker is enough to solve.
struct BoardMarkerRun {
    using Record = a3_board_pose;
    uint32_t first = 0, cnt = 0;
    const uint32_t* s_dup = nullptr;
    __device__ void bind(const BoardArgs&, uint32_t, int, uint32_t first_, uint32_t cnt_, const uint32_t* s_dup_) { first = first_; cnt = cnt_; s_dup = s_dup_; }
    __device__ uint32_t count() const { return 4 * cnt; }
    __device__ bool solves(bool top) const { return top; }
    __device__ float denominator(const BoardStart& b) const { return (float)(4u * b.used); }
    __device__ void counts(a3_board_pose& rec, const BoardStart& b) const { rec.markers_used = b.used; rec.markers_rejected = b.rejected; }
};

struct BoardCorr {   // a planar correspondence: board point, normalised image point
    float bx, by, mx, my;
};

struct PlanarMarkers : BoardMarkerRun {   // a3_set_board: k_board_pose
    using Slot = BoardSlot;
    using Corr = BoardCorr;
    __device__ static const BoardSlot* slots(const BoardArgs& a) { return a.slots; }
    __device__ bool corner(const BoardArgs& a, uint32_t c, BoardCorr& o) const { return board_corner(a, s_dup, first, c, &o.bx, &o.by, &o.mx, &o.my); }
    __device__ static void accum(BoardAcc& s, const float R[9], const float t[3], const BoardCorr& o, float sx, float sy) {
        board_accum(s, R, t, o.bx, o.by, o.mx, o.my, sx, sy);
    }
    __device__ static void start(const BoardSlot& bs, const a3_pose& pm, float R[9], float t[3]) { board_planar_start(bs, pm, R, t); }
};

}  // namespace a3
