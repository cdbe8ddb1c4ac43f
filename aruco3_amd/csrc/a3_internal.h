/*
 * a3_internal.h -- entry points of libaruco3_hip.so that are NOT part of the binding surface (include/aruco3_hip.h):
 * tuning probes and single-stage hooks used by this repository's tests and tools only.  A Rust/C binding of the detector
 * has no business calling them; they may change without an ABI version bump.
 */
#ifndef ARUCO3_HIP_INTERNAL_H
#define ARUCO3_HIP_INTERNAL_H

#include "../../include/aruco3_hip.h"

#ifdef __cplusplus
extern "C" {
#endif

/* kernel-level timing for tuning (tools/kernel_probe.py): re-runs one kernel (0 dart_count, 1 dart_assign, 2 local_contract,
 * 3 decode, 4 decode with the frames evicted from the caches before every run: bench.py's roofline_warp) on the buffers of the last single-chunk batch, optionally truncated (dbg), and returns the average device time.
 * The internal contour buffers hold garbage afterwards; results already returned are unaffected. */
int  a3_debug_kernel_time(a3_ctx *ctx, int kernel, int dbg, int reps, float *avg_ms);

/* Where the decode stage of a SUBMITTED batch is released when another context submits behind it (see a3_api.hip,
 * "deferred decode"): 0 = never deferred (both halves of a batch enqueued at once, as a3_detect_batch always does), 1 = behind
 * the next batch's threshold kernel, 2 = behind its k_local_contract (the default); -1 = the library decides per batch (its default).
 * Process-wide; results are identical in every mode -- tools/ use it for A/B timing inside one process, since two boxes of the pool
 * differ by more than the effect. */
int  a3_debug_set_overlap(int mode);

/* A stand-in for a collective's channel kernels, for a box with one GPU: `workgroups` workgroups of `threads` threads stay
 * resident on `hip_stream` for `usec` microseconds (48 live registers per lane, a read and a short sleep per turn).
 * tools/spin_probe.py measures what such company does to the threshold kernel and to a step. */
int  a3_debug_spin(void *hip_stream, int workgroups, int threads, int usec);

/* 0: contexts that declared burst gates (a3_order_after) enqueue their whole batch at submit, as round 3's library did; 1 (default):
 * they hold the chain behind their threshold kernel until the burst's last member has enqueued its own (a3_api.hip, submit_common).
 * Process-wide, for A/B timing; results are identical. */
int  a3_debug_set_hold(int on);

/* At most `rounds` global pointer-doubling rounds per chunk (the dense-graph path of the contour stage; 0 = no cap, the default).
 * Process-wide.  Fewer rounds than a graph needs leave its entry states unconverged: the library sees it and re-runs the batch with
 * all rounds, so results are identical -- tests/ use it to walk that path on purpose. */
int  a3_debug_set_jump_rounds(int rounds);

/* the threshold kernel alone, asynchronously, on the context's stream (tools/k1_concurrency.py: how several launches in flight
 * at once share the chip) */
int  a3_debug_launch_threshold(a3_ctx *ctx, const void *pixels_device, int fmt, uint32_t width, uint32_t height, uint32_t n_frames);

/* which build this is: always 0 now that the library has no tuning build and no kernel build options (bit 0 was a build that read
 * tuning knobs from the environment, bit 1 a non-default kernel build option).  Kept because bench.py and the GPU tests report it
 * for whichever library A3_HIP_LIB names. */
int  a3_debug_build_flags(void);

/* numerics self-check used by the GPU tests: evaluates the IEEE operations the kernels rely on (f64 sqrt/div, f32 sqrt/div)
 * for n inputs so that the host can compare them bit for bit */
int  a3_selftest_ieee(a3_ctx *ctx, const double *a, const double *b, size_t n, double *sqrt_a, double *a_div_b,
                      float *sqrtf_a, float *a_divf_b);

/* The reference's own vectors for its small helpers (src/aruco.rs:400-459), fed through the device code that implements
 * them inside the pipeline kernels:
 *   enforce_clockwise_corners (src/aruco.rs:168-185)  -> the winding fix of k_contour_quads, n quads of 4 (x, y) i32 pairs
 *   rotate_bit_matrix         (src/aruco.rs:315-326)  -> k_decode's rotation mapping applied `times` times to an n x n matrix
 *   discard_too_near          (src/aruco.rs:187-232)  -> k_frame_candidates on one frame whose candidates are `quads_xy` in order */
int  a3_debug_clockwise(a3_ctx *ctx, const int32_t *quads_xy, size_t n, int32_t *out_xy);
int  a3_debug_rotate_bits(a3_ctx *ctx, const uint8_t *bits, uint32_t n, uint32_t times, uint8_t *out);
/* Quirk Q4 (src/aruco.rs:255-257: a failed projection -> 1 x 1 black patch -> code 0 looked up): the quads given here REPLACE the
 * candidate list of frame 0 of the NEXT batch of this context (a synchronous a3_detect_batch of one frame), in the given order,
 * between the contour stage and k_frame_candidates -- the place of the list enforce_clockwise_corners leaves behind
 * (src/aruco.rs:68).  A convex hull never yields the collinear / repeated-corner quad that makes the 8 x 8 solve fail; this is
 * the only way to lead one through discard_too_near, the solve, k_decode's 1 x 1 stand-in and the accept test on the device.
 * One shot: the batch after that runs unchanged. */
int  a3_debug_inject_candidates(a3_ctx *ctx, const uint32_t *quads_xy, size_t n);
/* Debug taps switch the decode stage's source to the packed grey plane, so a tapped batch's patches say nothing about the sampler
 * an untapped batch runs on the caller's pixel format, strides and alignment.  While this is set, a tapped batch still gets its
 * grey plane (for the grey tap) but its decode stage samples what an untapped batch would: the caller's frames, or the grey plane
 * only where the threshold window itself needs it.  A host-side selection; applies to batches started afterwards. */
int  a3_debug_sample_frames(a3_ctx *ctx, int enabled);
int  a3_debug_discard_too_near(a3_ctx *ctx, const uint32_t *quads_xy, size_t n, float min_distance, uint32_t *out_xy, size_t *n_out);

/* k_frame_candidates (candidate order by start key, discard_too_near, compaction, the work list, the projections) launched exactly
 * as the pipeline launches it -- ONE call of launch_frame_candidates, so the table size picks the kernel's form: all in LDS up to
 * 6144 slots per frame, through memory above -- on hand-made candidate tables.  The product never calls it; tests/ do, because the
 * contour stage cannot be made to produce a chosen candidate list and the two hooks above stop at one frame of 1024 quads whose
 * keys are 0..n-1.
 *   n_frames >= 1, max_cand in 1..65536 (slots per frame), cand_count[n_frames] (may exceed max_cand: an overflowed frame),
 *   records: frame after frame, min(cand_count[f], max_cand) records each, in the order of the frame's table (keys unique per frame),
 *   S: homography_sample_size, 0 = no projections (proj may then be NULL).
 * Out, each for n_frames * max_cand slots and filled with 0xFF bytes wherever the kernel did not write: pre_xy and fin_xy (8 x u16 per
 * slot), work (u32 per slot), proj (A3_DEBUG_PROJ_BYTES per slot, indexed like work: 9 x f32 inverse, i32 ok); fin_count[n_frames];
 * *work_count.  Runs on buffers of its own and frees them: the context's buffers and settings are what they were. */
typedef struct { uint32_t start_key; uint16_t xy[8]; } a3_debug_cand;
#define A3_DEBUG_PROJ_BYTES 40
int  a3_debug_frame_candidates(a3_ctx *ctx, uint32_t n_frames, uint32_t max_cand, const uint32_t *cand_count, const a3_debug_cand *records,
                               float min_distance, uint32_t S, uint16_t *pre_xy, uint16_t *fin_xy, uint32_t *fin_count, uint32_t *work,
                               uint32_t *work_count, void *proj);

/* k_merge_candidates (a3_set_threshold_windows: the K planes' candidates of every frame ranked by (window, start key), the discard with
 * the rotation across windows, compaction, the work list, the projections) launched exactly as the pipeline launches it -- ONE call of
 * launch_merge_candidates, so the merged capacity M = min(n_windows * plane_cand, 65536) picks the kernel's form: all in LDS up to 6144
 * merged slots per frame, through memory above -- on hand-made per-plane tables.  The product never calls it; tests/ do.
 *   n_frames >= 1, n_windows in 2..4, plane_cand in 1..65536 (slots per plane), cand_count[n_windows * n_frames] at plane index
 *   k * n_frames + f (may exceed plane_cand: an overflowed plane), records: plane after plane in that index order, min(cand_count[p],
 *   plane_cand) records each (keys unique per plane), S: homography_sample_size, 0 = no projections (proj may then be NULL).
 * Out, each for n_frames * M slots and filled with 0xFF bytes wherever the kernel did not write: pre_xy and fin_xy (8 x u16 per slot),
 * work (u32 per slot), proj (A3_DEBUG_PROJ_BYTES per slot, indexed like work); fin_count[n_frames]; merged_count[n_frames]; *work_count;
 * *err_flags (the kErr* word, zeroed first: kErrCandTable = 8 for a frame whose planes sum beyond M).  Runs on buffers of its own. */
int  a3_debug_merge_candidates(a3_ctx *ctx, uint32_t n_frames, uint32_t n_windows, uint32_t plane_cand, const uint32_t *cand_count,
                               const a3_debug_cand *records, float min_distance, uint32_t S, uint16_t *pre_xy, uint16_t *fin_xy,
                               uint32_t *fin_count, uint32_t *work, uint32_t *work_count, void *proj, uint32_t *merged_count,
                               uint32_t *err_flags);

/* k_contour_quads (per traced border: Douglas-Peucker with the arg-max over a group's lanes, the hull of the four kept points, the
 * squared-edge filter of quirk Q1, the winding fix) launched exactly as the pipeline launches it -- ONE call of launch_contour_quads with
 * a ContourChunk filled from the arguments, so width and height pick the 24-bit or the 64-bit numerators and n_darts sizes the grid (160
 * wave groups and 1024 16-lane groups at the least, 10240 and 65536 from 2^23 darts on) -- on a hand-made contour table and point pool.
 * The product never calls it; tests/ do, because whole images cannot be made to hand the kernel a chosen border.
 *   width, height in 1..65536; first_frame + n_frames frames of max_cand (1..65536) slots, at most 2^24 slots in all;
 *   records[n_records]: {frame, start_key, point_base, n} in the table's order; points[n_points]: x | y << 16;
 *   max_contours: the table's capacity as the kernel is told it; ctr_contours, ctr_err_flags: DeviceCounters::contours and ::err_flags
 *   as the kernel finds them.  The kernel reads the first min(ctr_contours, max_contours) records; that many must be given, unless
 *   ctr_err_flags carries kErrPointPool (2) or kErrContourTable (4), on which it reads none.
 * Refused with A3_ERR_INVALID, because the kernel checks none of it and the pipeline never produces it: a record with n == 0 or with
 * points beyond the pool, a frame outside [first_frame, first_frame + n_frames), a coordinate >= width or height, two records of one
 * frame with the same start key, NULL arguments.
 * Out: cand_count[first_frame + n_frames], cands[(first_frame + n_frames) * max_cand] and *err_flags (the kErr* word the kernel raises
 * kErrCandTable = 8 in).  The tables are filled with 0xFF bytes first and the chunk's counts and the flag word zeroed, as the pipeline has
 * them: a slot the kernel did not write, and every count and slot of a frame below first_frame, comes back as 0xFF.  Slot order within a
 * frame is the order of an atomic and not part of the contract.  Runs on buffers of its own and frees them: the context's buffers and
 * settings are what they were. */
typedef struct { uint32_t frame, start_key, point_base, n; } a3_debug_contour;
int  a3_debug_contour_quads(a3_ctx *ctx, uint32_t width, uint32_t height, uint32_t n_darts, double eps_factor, uint32_t min_edge_length,
                            uint32_t first_frame, uint32_t n_frames, uint32_t max_cand, uint32_t max_contours, uint32_t ctr_contours,
                            uint32_t ctr_err_flags, const a3_debug_contour *records, uint32_t n_records, const uint32_t *points, size_t n_points,
                            uint32_t *cand_count, a3_debug_cand *cands, uint32_t *err_flags);

#ifdef __cplusplus
}
#endif
#endif
