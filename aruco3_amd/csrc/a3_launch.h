// a3_launch.h -- every function one translation unit of the library defines and another calls: the kernel files' launchers and
// size accessors, declared once, with the contract of each (what may be null, how capacities relate to counts, which buffers arrive
// zeroed).  A launcher with more than eight parameters besides the stream takes (hipStream_t, const X&): X is a plain aggregate
// whose members all default to null / 0, built at the call site with designated initialisers, so an optional input is a member the
// caller leaves out.  Groups that travel together to several launchers are one struct, built once and passed on (ContourChunk,
// DecodeStage, MarkerSrc, BoardTables).  The records the kernels keep to themselves (EntryState, FinState, ProjRec, DecodeOut, BoardSlot,
// Board3Slot, RefineParams, the solvers' scratch) stay opaque here: the host sees their sizes and void pointers.  Ahead of the
// declarations: the two helpers with which a launcher turns a run-time format or radius into its kernel's template argument.
#pragma once

#include <type_traits>

#include "a3_common.h"
#include "a3_format.h"
#include "a3_threshold_plan.h"   // threshold_path, threshold_writes_grey_plane

namespace a3 {

// ---- a launcher's run-time argument as a template argument of its kernel -------------------------------------------------------------
// f(std::integral_constant<int, A3_FMT_*>{}) for the format fmt names, and what f returns; hipErrorInvalidValue for a value that names
// none (every public entry has refused such a value -- format_valid -- before a launcher runs).  The one place that lists the formats
// for the kernels that are templates on them.
template <class F>
hipError_t with_format(int fmt, F&& f) {
    switch (fmt) {
        case A3_FMT_RGB8: return f(std::integral_constant<int, A3_FMT_RGB8>{});
        case A3_FMT_RGBA8: return f(std::integral_constant<int, A3_FMT_RGBA8>{});
        case A3_FMT_L8: return f(std::integral_constant<int, A3_FMT_L8>{});
        case A3_FMT_BGRA8: return f(std::integral_constant<int, A3_FMT_BGRA8>{});
        case A3_FMT_YUYV8: return f(std::integral_constant<int, A3_FMT_YUYV8>{});
        case A3_FMT_UYVY8: return f(std::integral_constant<int, A3_FMT_UYVY8>{});
        default: return hipErrorInvalidValue;
    }
}
// f(std::integral_constant<int, R>{}) for the R in LO..HI that radius equals; hipErrorInvalidValue outside.  Instantiates f for every R
// of the range and for no other.
template <int LO, int HI, class F>
hipError_t with_radius(uint32_t radius, F&& f) {
    if constexpr (LO > HI) return hipErrorInvalidValue;
    else return radius == (uint32_t)LO ? f(std::integral_constant<int, LO>{}) : with_radius<LO + 1, HI>(radius, f);
}

// ---- k_threshold.hip (+ _r1, _r2, _big): grey + adaptive threshold ----------------------------------------------------------
// n frames of W x H pixels -> the packed image `bits`.  grey (nullable): the grey plane is written too; the separable and the
// brute-force path (a3_threshold_plan.h: threshold_writes_grey_plane) need it, the separable one hsum_tmp (one u16 per pixel) as well,
// the fused kernels need neither.  fmt: any A3_FMT_*; for A3_FMT_YUYV8 / A3_FMT_UYVY8 (2 bytes per pixel, W even) the grey level is the
// luma byte as it stands (a3_format.h).
struct ThresholdLaunch {
    const uint8_t* pixels = nullptr; int fmt = 0; size_t row_stride = 0, frame_stride = 0; int W = 0, H = 0; uint32_t n = 0, radius = 0;
    uint8_t* grey = nullptr; uint64_t* bits = nullptr; uint16_t* hsum_tmp = nullptr;
};
hipError_t launch_grey_threshold(hipStream_t st, const ThresholdLaunch& t);
hipError_t launch_k1_r1(hipStream_t st, const ThresholdLaunch& t);   // radii 1..3
hipError_t launch_k1_r2(hipStream_t st, const ThresholdLaunch& t);   // radii 4..6
hipError_t launch_ring_threshold(hipStream_t st, const ThresholdLaunch& t);   // radii 8..31, any frame layout

// ---- k_contours.hip: the contour stage ----------------------------------------------------------------------------------------
// the tile tables of a batch: tile_darts[frames * tiles] | tile_off[frames * tiles] | second-half counts of k_dart_count[frames *
// tiles], followed (8-byte aligned) by the word masks; launch_dart_count writes them, launch_dart_build reads them
size_t tile_darts_bytes(uint32_t W, uint32_t H, uint32_t n_frames);
// The darts of every frame and tile.  plan != nullptr: the launch of k_tile_scan also plans the batch on the device
// (frame_base[0..n_frames], *plan -- BatchScratch::plan -- against plan_cap) and zeroes [zero_p, zero_p + zero_bytes), the counter block, a multiple of
// 16 bytes; frame_darts arrives zeroed.
struct DartCountLaunch {
    const uint64_t* bits = nullptr; int W = 0, H = 0; uint32_t first_frame = 0, n_frames = 0; unsigned long long* frame_darts = nullptr;
    uint32_t* tile_darts = nullptr; uint64_t plan_cap = 0; uint32_t* frame_base = nullptr; PlanWords* plan = nullptr; void* zero_p = nullptr;
    size_t zero_bytes = 0;
};
hipError_t launch_dart_count(hipStream_t st, const DartCountLaunch& d);
hipError_t launch_zero(hipStream_t st, void* p, size_t bytes);   // bytes: a multiple of 16, p 16-byte aligned

size_t entry_state_bytes();
size_t fin_state_bytes();
size_t entry_slots(uint32_t n_darts);
size_t leader_list_bytes(uint32_t n_darts);

// One chunk of a batch's contour graph, as launch_dart_build, launch_rank_cycles, launch_resolve, launch_select_scatter and
// launch_contour_quads take it, in that order: the buffers and settings are the batch's, the first block below is the chunk's.
struct ContourChunk {
    // the chunk: frames [first_frame, first_frame + n_frames) of the batch, n_darts darts, frame_base[0..n_frames] into them
    uint32_t first_frame = 0, n_frames = 0, n_darts = 0; const uint32_t* frame_base = nullptr; DeviceCounters* ctr = nullptr;
    int max_rounds = 0;                  // doubling rounds of the global form (frame_entries == nullptr)
    uint32_t* frame_entries = nullptr;   // per-frame entry counts, zeroed; nullptr: the global rounds
    unsigned int* dead_count = nullptr;  // BatchScratch::dead_count; nullptr: no border is dropped early (debug taps, sparse graphs)
    // the batch
    int W = 0, H = 0;
    uint32_t batch_frames = 0;           // the frames launch_dart_count laid the tile tables out for
    const uint64_t* bits = nullptr; const uint32_t* tile_darts = nullptr;
    const uint32_t* n_live = nullptr;    // the dart total on the device (a device-planned batch: n_darts is its capacity); nullable
    uint32_t* pix_base = nullptr; uint64_t* d_rec = nullptr; uint32_t* d_succ = nullptr; uint32_t* entry_list = nullptr;
    unsigned int* entry_count = nullptr, * leader_count = nullptr;   // BatchScratch's, zeroed per chunk
    void* es_a = nullptr, * es_b = nullptr;   // EntryState[entry_slots(n_darts)]
    void* fin = nullptr;                      // FinState[n_darts]
    uint32_t* leader_list = nullptr, * leader_keep = nullptr; uint64_t* t_cur = nullptr, * t_next = nullptr;
    int resolve_iters = 0;               // fixpoint passes of launch_resolve; 0: none, k_cycle_select checks the natural starts inline
    int inline_resolve_W = 0;            // ... against this row width (W); 0 with fixpoint passes
    uint32_t min_edge_length = 0; double eps_factor = 0.0; ContourRec* contours = nullptr; uint32_t* cyc_start_off = nullptr;
    uint32_t* points = nullptr; uint32_t max_contours = 0; uint64_t max_points = 0;
    bool keep_all = false;               // debug taps: every border is kept
    CandRec* cands = nullptr;            // batch_frames x max_cand, and cand_count[batch_frames]: the launcher moves to first_frame
    uint32_t* cand_count = nullptr; uint32_t max_cand = 0; unsigned int* err_flags = nullptr;
    // a3_debug_kernel_time only (0 in the product path).  phase: 0 everything, 1 k_local_contract only, 2 what follows it.  dbg:
    // launch_dart_build 1..4 stop k_dart_assign early and leave d_succ alone, 5 = everything; launch_rank_cycles n > 0 runs n doubling
    // rounds of k_local_contract instead of 11, -1 none, and nothing behind it
    int phase = 0, dbg = 0;
};
hipError_t launch_dart_build(hipStream_t st, const ContourChunk& c);
// leaders + ranks for every dart of the chunk
hipError_t launch_rank_cycles(hipStream_t st, const ContourChunk& c);
hipError_t launch_resolve(hipStream_t st, const ContourChunk& c);
hipError_t launch_select_scatter(hipStream_t st, const ContourChunk& c);
hipError_t launch_contour_quads(hipStream_t st, const ContourChunk& c);
hipError_t launch_debug_clockwise(hipStream_t st, const int32_t* in, uint32_t n, int32_t* out);
hipError_t launch_unpack_bits(hipStream_t st, const uint64_t* bits, int W, int H, uint8_t* out);

// ---- k_decode.hip: candidates -> markers -> poses -------------------------------------------------------------------------------
size_t decode_out_bytes();
size_t proj_rec_bytes();
size_t weight_table_bytes();
uint32_t frame_cand_lds_slots();
// The decode stage of n_frames frames with max_cand candidate slots each, as launch_frame_candidates, launch_decode and
// launch_compact_markers take it, in that order; a caller of one of them fills what that one reads.
struct DecodeStage {
    uint32_t n_frames = 0, first_frame = 0, max_cand = 0;
    // launch_frame_candidates.  Per frame: the quads in start-key order (pre_xy), discard_too_near's survivors (fin_xy, fin_count), their
    // work items and, with S > 0, their projections (proj).  work_count arrives zeroed; big_scratch: n_frames x max_cand floats, needed
    // when max_cand > frame_cand_lds_slots().
    const CandRec* cands = nullptr; const uint32_t* cand_count = nullptr; float min_distance = 0.0f;
    uint16_t* pre_xy = nullptr, * fin_xy = nullptr; uint32_t* fin_count = nullptr, * work = nullptr; unsigned int* work_count = nullptr;
    uint32_t S = 0; void* proj = nullptr; float* big_scratch = nullptr;
    // launch_merge_candidates (a3_set_threshold_windows, windows = 2..4) in launch_frame_candidates' place: cands and cand_count are the
    // n_frames x windows PLANES' (plane (k, f) at k * n_frames + f, plane_cand slots each), every other table is the frames' with
    // max_cand = merged_cand_capacity(windows, plane_cand) slots; merged_count[n_frames]: the concatenated lists' lengths, which the
    // caller then hands to launch_compact_markers as its cand_count.  big_scratch: needed when max_cand > frame_cand_lds_slots().
    uint32_t windows = 0, plane_cand = 0; uint32_t* merged_count = nullptr;
    // launch_decode: k_decode over the work list.  n: cells per side; patches (nullable, debug taps): patch_cap warped patches are kept;
    // per_frame: nullable; few (at most 64 frames): all four waves of a workgroup run the stages behind the sampling.  inverted
    // (a3_set_marker_polarity, A3_POLARITY_BOTH): k_decode's instantiations that read a bit matrix with an all-lit perimeter complemented
    // and give it decode_ok 2; false: the instantiations without any of that.
    PixelSrc src{}; int W = 0, H = 0; uint32_t n = 0, max_taps = 0; const uint64_t* dict = nullptr; uint32_t n_codes = 0, tau = 0; int filter = 0;
    const float* wtab = nullptr; void* outs = nullptr; uint8_t* patches = nullptr; uint32_t patch_cap = 0; uint32_t* per_frame = nullptr;
    int grid_blocks = 0; bool few = false, inverted = false;
    // ... a3_debug_kernel_time only: k_projection runs first (the product's projections come from k_frame_candidates); k_decode stops
    // early: 1 = no sampling, 2 / 3 / 4 = after sampling / Otsu / bits, 0 and 5 = the whole kernel
    bool projection = false; int variant = 0;
    // launch_compact_markers: the marker list (capacity marker_cap), its total and the sum of cand_count (cand_pre_total: BatchScratch's, with
    // cand_most kCandMostFromPre words behind it)
    a3_marker* markers = nullptr; uint32_t marker_cap = 0; unsigned int* marker_total = nullptr, * err_flags = nullptr, * cand_pre_total = nullptr;
};
hipError_t launch_frame_candidates(hipStream_t st, const DecodeStage& d);
hipError_t launch_merge_candidates(hipStream_t st, const DecodeStage& d);
hipError_t launch_decode(hipStream_t st, const DecodeStage& d);
hipError_t launch_compact_markers(hipStream_t st, const DecodeStage& d);
// The flag words of a batch's final marker list (a3_get_marker_flags), one lane per marker: flags[i] = A3_MARKER_INVERTED when the
// DecodeOut record at slot markers[i].frame * max_cand + markers[i].candidate_index has decode_ok == 2, else 0 (also for a marker whose
// frame or index lies outside n_frames x max_cand).  markers: the list (capacity n, count *n_dev) as launch_compact_markers or
// launch_recover_merge left it, frames batch-relative; outs: the DecodeOut records launch_decode wrote; flags: n words.  Runs ahead of
// launch_scale_markers and the refinement, which reads the flags.
struct MarkerFlagsLaunch {
    const a3_marker* markers = nullptr; const unsigned int* n_dev = nullptr; uint32_t n = 0; const void* outs = nullptr;
    uint32_t n_frames = 0, max_cand = 0; uint32_t* flags = nullptr;
};
hipError_t launch_marker_flags(hipStream_t st, const MarkerFlagsLaunch& m);
hipError_t launch_weight_table(hipStream_t st, uint32_t S, uint32_t n, uint32_t max_taps, float* wtab);
hipError_t launch_pack_detections(hipStream_t st, const a3_marker* markers, const a3_pose* poses, const uint32_t* per_frame, uint32_t n_frames,
                                  uint32_t first_frame_global, uint32_t maxm, void* dst, unsigned int* overflow);
hipError_t launch_debug_rotate_bits(hipStream_t st, const uint8_t* in, uint32_t n, uint32_t r, uint8_t* out);
hipError_t launch_gather_patches(hipStream_t st, const void* outs_frame, uint32_t n_cand, const uint8_t* patches, uint32_t patch_cap, uint32_t S2,
                                 uint8_t* dst, unsigned int* missing);
// IPPE, one lane per marker.  mode 0: pts = corners / (iw, ih); 1: unprojected through the intrinsics; 2: norm_pts are normalised
// already; 3 / 4: as 0 / 1 from the float corners in norm_pts (8 per marker).  corner_stride: u32 words between the corner lists of
// consecutive markers (8 for a packed list, 14 inside a3_marker[]); n_dev (nullable): the marker count on the device, n its capacity.
struct PoseLaunch {
    const uint32_t* corners = nullptr; uint32_t corner_stride = 0; const float* norm_pts = nullptr; uint32_t n = 0;
    const unsigned int* n_dev = nullptr; int mode = 0; float marker_size_mm = 0.0f, iw = 0.0f, ih = 0.0f, fx = 0.0f, fy = 0.0f, cx = 0.0f, cy = 0.0f;
    a3_pose* out = nullptr;
};
hipError_t launch_pose(hipStream_t st, const PoseLaunch& p);
hipError_t launch_find_nearest(hipStream_t st, const uint64_t* dict, uint32_t n_codes, const uint64_t* bits, uint32_t n, uint32_t* idx, uint8_t* dist);
hipError_t launch_calc_tau(hipStream_t st, const uint64_t* dict, uint32_t n_codes, unsigned int* tau);
hipError_t launch_selftest(hipStream_t st, const double* a, const double* b, uint32_t n, double* sq, double* dv, float* sqf, float* dvf);

// ---- markers as the board, ChArUco, refinement and undistortion kernels take them ---------------------------------------------------
// Either a batch's marker list on the device -- markers (capacity n), their count n_dev, per_frame[n_frames], optionally their float
// corners (8 per marker: undistorted or refined) -- or one frame (n_frames = 1) of n caller markers: ids and pts (8 floats each).
// markers != nullptr selects the first form.
struct MarkerSrc {
    const a3_marker* markers = nullptr; const unsigned int* n_dev = nullptr; const uint32_t* per_frame = nullptr; const float* corners = nullptr;
    const uint32_t* ids = nullptr; const float* pts = nullptr; uint32_t n = 0, n_frames = 0;
};
// the board's device tables (a3_set_board: id -> slot, n_codes entries; BoardSlot records) and the ChArUco table (a3_set_charuco: nc
// chessboard corners cxy, their adjacent ids adj), nc = 0 without one.  slot_kind says which records `slots` holds: kBoardSlotsPlanar
// (a3_set_board: BoardSlot, what every launcher but launch_board3d_pose reads) or kBoardSlots3D (a3_set_board3d: Board3Slot)
constexpr uint32_t kBoardSlotsPlanar = 0, kBoardSlots3D = 1;
struct BoardTables {
    const uint16_t* slot_of = nullptr; uint32_t n_codes = 0; const void* slots = nullptr; const float* cxy = nullptr; const uint32_t* adj = nullptr;
    uint32_t nc = 0, slot_kind = kBoardSlotsPlanar;
};

// ---- k_refine.hip -------------------------------------------------------------------------------------------------------------------
size_t refine_params_bytes();
void refine_params(void* out, const a3_refine_config& cfg, uint32_t cells);
// markers != nullptr: the corners of a batch's marker list (capacity n, count n_dev) -> 8 floats per marker; else n stand-alone corners
// pts (2 floats each) with their cell sizes cell_px (nullable).  (One workgroup per marker up to 1024, then a workgroup-stride loop.)
struct RefineLaunch {
    PixelSrc src{}; uint32_t W = 0, H = 0; const a3_marker* markers = nullptr; const unsigned int* n_dev = nullptr;
    const float* pts = nullptr, * cell_px = nullptr; uint32_t n = 0;
    const void* params = nullptr;   // refine_params()
    float* out = nullptr;
    // launch_refine_edges with markers only (nullable): the list's flag words (launch_marker_flags); a marker flagged A3_MARKER_INVERTED
    // is bright inside and its gradients are taken with the opposite sign.  nullptr, a zero word, stand-alone quads: dark inside.
    const uint32_t* flags = nullptr;
};
hipError_t launch_refine_corners(hipStream_t st, const RefineLaunch& r);

// ---- k_edge_refine.hip --------------------------------------------------------------------------------------------------------------
// method A3_REFINE_EDGES of the same launch: markers != nullptr as above; else the n / 4 stand-alone quads of pts (n corners, a multiple
// of 4), cell_px (nullable) read at each quad's first corner.  params: refine_params() (the weight tables are not read).  (One wave
// per marker, four per workgroup, up to 1024 workgroups, then a workgroup-stride loop.)
hipError_t launch_refine_edges(hipStream_t st, const RefineLaunch& r);

// ---- k_undistort.hip ----------------------------------------------------------------------------------------------------------------
// markers / pts: the corners' source (pts wins when both are given); n_dev: the device-side marker count of a batch (n = its marker
// capacity), or nullptr for n stand-alone points.  out_xy: 2 floats per corner, out_res: 1.
hipError_t launch_undistort_corners(hipStream_t st, const a3_marker* markers, const float* pts, const unsigned int* n_dev, uint32_t n,
                                    const a3_intrinsics& in, const a3_distortion& d, float* out_xy, float* out_res);

// ---- k_board.hip --------------------------------------------------------------------------------------------------------------------
size_t board_slot_bytes();
void board_slot_from(const float xy[8], void* out);   // one slot record from a checked marker's corners
// one a3_board_pose per frame of m.  intr == nullptr: normalised by the image size (W, H).
struct BoardPoseLaunch {
    MarkerSrc m; BoardTables board; const a3_intrinsics* intr = nullptr; uint32_t W = 0, H = 0; a3_board_pose* out = nullptr;
};
hipError_t launch_board_pose(hipStream_t st, const BoardPoseLaunch& b);

// ---- k_board3d.hip ------------------------------------------------------------------------------------------------------------------
size_t board3d_slot_bytes();
void board3d_slot_from(const float xyz[12], void* out);   // one Board3Slot record from a checked marker's corners (a3_board3d_check.h)
// one a3_board_pose per frame of b.m from a 3-D board: b.board.slots holds Board3Slot records and b.board.slot_kind says so
// (kBoardSlots3D; anything else: hipErrorInvalidValue, nothing is launched).  Every other member as launch_board_pose takes it.
hipError_t launch_board3d_pose(hipStream_t st, const BoardPoseLaunch& b);

// ---- k_recover.hip ------------------------------------------------------------------------------------------------------------------
// Board-aided recovery (a3_set_board_recovery).  Stage 1, one workgroup per frame: the board markers no marker of the frame carries,
// matched to the frame's rejected candidates; frame f's records go to rec[f * rec_cap ...] in candidate order, their number to
// rec_count[f].  Detected markers: a batch's list (markers != nullptr: capacity n, count n_dev, per_frame[n_frames]) or one frame of n
// caller markers (ids, corners: 8 u32 each).  Candidates: a batch's (outs != nullptr: DecodeOut and fin_xy records, max_cand slots per
// frame, fin_count[n_frames]; those with valid == 0 are eligible) or one frame of n_cand caller quads (cand_xy: 8 u32 each, codes4: 4 each,
// has_codes: 1 each; all eligible).  slot_ids: the board's ids in slot order (n_slots <= A3_BOARD_MAX_MARKERS); rec_cap >= min(n_slots,
// candidates per frame).
struct RecoverLaunch {
    const a3_marker* markers = nullptr; const unsigned int* n_dev = nullptr; const uint32_t* per_frame = nullptr; const uint32_t* ids = nullptr;
    const uint32_t* corners = nullptr; uint32_t n = 0, n_frames = 0;
    const void* outs = nullptr; const uint16_t* fin_xy = nullptr; const uint32_t* fin_count = nullptr; uint32_t max_cand = 0;
    const uint32_t* cand_xy = nullptr; const uint64_t* codes4 = nullptr; const uint8_t* has_codes = nullptr; uint32_t n_cand = 0;
    BoardTables board; const uint32_t* slot_ids = nullptr; uint32_t n_slots = 0; const uint64_t* dict = nullptr;
    a3_recover_config cfg{};
    a3_marker* rec = nullptr; uint32_t rec_cap = 0; uint32_t* rec_count = nullptr;
};
hipError_t launch_recover_frames(hipStream_t st, const RecoverLaunch& r);
// Stage 2, one workgroup per frame: the merged list -- per frame the detected markers (det: capacity det_cap, det_per_frame[n_frames]) in
// their order, then stage 1's records -- into out (capacity out_cap), its counts into per_frame and its total into *marker_total;
// a total above out_cap raises kErrMarkerCap in *err_flags and nothing is stored past the capacity.
struct RecoverMergeLaunch {
    const a3_marker* det = nullptr; uint32_t det_cap = 0; const uint32_t* det_per_frame = nullptr; const a3_marker* rec = nullptr; uint32_t rec_cap = 0;
    const uint32_t* rec_count = nullptr; uint32_t n_frames = 0; a3_marker* out = nullptr; uint32_t out_cap = 0; uint32_t* per_frame = nullptr;
    unsigned int* marker_total = nullptr, * err_flags = nullptr;
};
hipError_t launch_recover_merge(hipStream_t st, const RecoverMergeLaunch& m);

// ---- k_charuco.hip ------------------------------------------------------------------------------------------------------------------
// The corner stage of m's frames (m.corners: the batch's refined corners or nullptr).  slots_tmp: n_frames x nc records; counts:
// n_frames + 1; out: n_frames x nc records; und (nullable, with intr and dist): 2 floats per record.
struct CharucoCornersLaunch {
    PixelSrc src{}; uint32_t W = 0, H = 0; MarkerSrc m; BoardTables board; uint32_t min_markers = 0, refine = 0;
    const void* params = nullptr;   // refine_params()
    const a3_intrinsics* intr = nullptr; const a3_distortion* dist = nullptr; a3_charuco_corner* slots_tmp = nullptr; uint32_t* counts = nullptr;
    a3_charuco_corner* out = nullptr; float* und = nullptr;
};
hipError_t launch_charuco_corners(hipStream_t st, const CharucoCornersLaunch& c);
// one a3_charuco_pose per frame of a batch from the records launch_charuco_corners wrote (the same counts / recs / und); m.corners: the
// markers' float corners (undistorted, else refined, else nullptr) as k_board_pose reads them
struct CharucoPoseLaunch {
    MarkerSrc m; BoardTables board; const uint32_t* counts = nullptr; const a3_charuco_corner* recs = nullptr; const float* und = nullptr;
    const a3_intrinsics* intr = nullptr; uint32_t W = 0, H = 0; a3_charuco_pose* out = nullptr;
};
hipError_t launch_charuco_pose(hipStream_t st, const CharucoPoseLaunch& c);

// ---- the solvers (k_calib, k_calib_fisheye, k_rig, k_handeye, k_map): one workgroup per problem; the scratch segments hold *_bytes()
// per record; every pointer is device memory the caller has checked and staged (a3_solve_check.h) ------------------------------------
size_t calib_view_bytes();
size_t fisheye_calib_view_bytes();
// start_obj, start_img: the fisheye model only (2 floats per point each)
struct CalibLaunch {
    const a3_calib_camera* cams = nullptr; uint32_t n_cams = 0; const uint32_t* view_off = nullptr; const float* obj = nullptr, * img = nullptr;
    double* scratch = nullptr; float* start_obj = nullptr, * start_img = nullptr; a3_calib_result* res = nullptr; a3_calib_view* views = nullptr;
};
hipError_t launch_calibrate(hipStream_t st, const CalibLaunch& c);
hipError_t launch_calibrate_fisheye(hipStream_t st, const CalibLaunch& c);
size_t rig_obs_bytes();
size_t rig_frame_bytes();
size_t rig_table_bytes();
struct RigLaunch {
    const a3_rig* rigs = nullptr; uint32_t n_rigs = 0; const a3_rig_camera* cams = nullptr; const a3_rig_observation* obs = nullptr;
    const float* obj = nullptr, * img = nullptr; uint32_t* tab = nullptr; double* oscr = nullptr, * fscr = nullptr; a3_rig_result* res = nullptr;
    a3_rig_camera_result* cres = nullptr; a3_rig_frame* frames = nullptr; a3_rig_observation_result* ores = nullptr;
};
hipError_t launch_rig(hipStream_t st, const RigLaunch& r);
size_t handeye_frame_bytes();
hipError_t launch_handeye(hipStream_t st, const a3_handeye_problem* probs, uint32_t n_probs, const a3_handeye_frame* frames, const float* obj,
                          const float* img, double* fscr, a3_handeye_result* res, a3_handeye_frame_result* fres);
size_t map_obs_bytes();
size_t map_frame_bytes();
size_t map_marker_bytes();
struct MapLaunch {
    const a3_map* maps = nullptr; uint32_t n_maps = 0; const a3_map_marker* markers = nullptr; const a3_map_observation* obs = nullptr;
    const float* img = nullptr; const uint64_t* big_off = nullptr; uint32_t* fo = nullptr, * ml = nullptr;
    double* oscr = nullptr, * fscr = nullptr, * mscr = nullptr, * big = nullptr; a3_map_result* res = nullptr; a3_map_marker_result* mres = nullptr;
    a3_map_frame* frames = nullptr; a3_map_observation_result* ores = nullptr;
};
hipError_t launch_map(hipStream_t st, const MapLaunch& m);

// ---- k_rectify.hip, k_synth.hip ---------------------------------------------------------------------------------------------------------
void rectify_grid(uint32_t dw, uint32_t dh, uint32_t n_frames, uint32_t* tiles_x, uint32_t* tiles_y, uint32_t* chunks);
// src / dst: device memory; bpp 1, 3 or 4.  The caller has checked every size and stride (a3_rectify_frames).
struct RectifyLaunch {
    const uint8_t* src = nullptr; size_t src_row = 0, src_frame = 0; uint32_t n_frames = 0; int bpp = 0; const a3_rectify* r = nullptr;
    uint8_t* dst = nullptr; size_t dst_row = 0, dst_frame = 0;
};
hipError_t launch_rectify(hipStream_t st, const RectifyLaunch& r);
// The grey form (a3_set_rectification): the same map, taps and blend, then one byte per pixel -- luma_of the rectified pixel's rounded
// bytes in fmt's channel order (A3_FMT_L8: the byte), which is what every sampler of the tree makes of the rectified colour frame.
// src: device memory, n_frames frames of r->src's size in format fmt (an A3_FMT_*); grey: device memory, n_frames planes of r->dst's
// size, tightly packed (row stride = r->dst.image_width), every byte of which is written and nothing else.  The caller has checked
// r (a3_rectify_check.h) and every size and stride.
// fmt A3_FMT_YUYV8 / A3_FMT_UYVY8 (packed 4:2:2, 2 bytes per pixel in src's strides): the luma byte alone is blended and is the output
// byte -- what fmt A3_FMT_L8 gives on a plane of those luma bytes.  These two formats have the grey form only, so a3_rectify_frames
// comes here for them, with its caller's strides in dst_row / dst_frame (bytes; dst_row 0: tightly packed, as above).
struct RectifyGreyLaunch {
    const uint8_t* src = nullptr; size_t src_row = 0, src_frame = 0; uint32_t n_frames = 0; int fmt = 0; const a3_rectify* r = nullptr;
    uint8_t* grey = nullptr; size_t dst_row = 0, dst_frame = 0;
};
hipError_t launch_rectify_grey(hipStream_t st, const RectifyGreyLaunch& r);
// ---- k_reduce.hip ---------------------------------------------------------------------------------------------------------------------
// The reduced grey plane (a3_reduce_frames, a3_set_reduction): n_frames frames of W x H pixels in format fmt (an A3_FMT_*) -> planes of
// (W / factor) x (H / factor) bytes, byte (j, i) = (sum of luma_of over the factor x factor block at (factor j, factor i) + factor^2 / 2)
// / factor^2 (A3_FMT_YUYV8 / A3_FMT_UYVY8: the luma byte in luma_of's place).  src, dst: device memory; factor 2, 3 or 4.  Nothing past a row's W / factor bytes is written.  The caller has checked
// every size and stride (a3_reduce_check.h).
struct ReduceLaunch {
    const uint8_t* src = nullptr; size_t src_row = 0, src_frame = 0; uint32_t n_frames = 0; int fmt = 0; uint32_t W = 0, H = 0, factor = 0;
    uint8_t* dst = nullptr; size_t dst_row = 0, dst_frame = 0;
};
hipError_t launch_reduce_frames(hipStream_t st, const ReduceLaunch& r);
// corners[8] of every marker of a device-resident list (capacity n, count n_dev) -> factor * c + factor / 2, in place
struct ScaleMarkersLaunch {
    a3_marker* markers = nullptr; const unsigned int* n_dev = nullptr; uint32_t n = 0, factor = 0;
};
hipError_t launch_scale_markers(hipStream_t st, const ScaleMarkersLaunch& s);
struct SynthLaunch {
    const a3_synth_frame* frames = nullptr; uint32_t n_frames = 0; const a3_synth_marker* markers = nullptr; uint32_t W = 0, H = 0; int paper = 0;
    float black = 0.0f, white = 0.0f; int supersample = 0; uint8_t* out = nullptr; size_t row_stride = 0, frame_stride = 0;
};
hipError_t launch_synth_render(hipStream_t st, const SynthLaunch& s);
// `workgroups` x `threads` that stay resident for `usec` microseconds (a3_debug_spin)
hipError_t launch_spin(hipStream_t st, int workgroups, int threads, int usec, uint32_t* sink);

}  // namespace a3
