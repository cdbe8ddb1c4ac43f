"""Detection with several threshold windows on the device (a3_set_threshold_windows): the K threshold launches, the contour stage on
n x K planes and k_merge_candidates, held against the oracle run once per window and the merged discard restated in
tests/multiwindow_util.py.  Integers are compared bit for bit, poses within 1e-4.  GPU only."""
import ctypes as C

import numpy as np
import pytest

from tests import multiwindow_util as mw
from tests.util import marker_tuples

pytestmark = pytest.mark.gpu
LDS_SLOTS = 6144   # k_decode.hip, kFrameCandLds: merged tables above it take the through-memory form


def _args(frames):
    from aruco3_amd import _lib

    a = np.ascontiguousarray(frames)
    if a.ndim == 3:
        a = a[..., None]
    n, h, w, c = a.shape
    return (a.ctypes.data, _lib.MEM_HOST, {1: _lib.FMT_L8, 3: _lib.FMT_RGB8}[c], w, h, w * c, h * w * c, n), a


def _detector(d, windows=None, factor=0.1, min_side=None, window=7, **kw):
    from aruco3_amd.aruco import Detector, DetectorConfig

    cfg = DetectorConfig(threshold_window=window, min_corner_separation_factor=factor)
    if min_side is not None:
        cfg.min_side_length_factor = min_side
    return Detector(cfg, d, threshold_windows=windows, **kw)


def _as_expected(markers):
    """marker_tuples reordered as multiwindow_util.expected_markers has them"""
    return [(f, i, c, xy, hd, rot, ci) for f, i, c, xy, hd, rot, ci in marker_tuples(markers)]


def _isolated(img, c):
    h, w = img.shape
    if len(c) != 1:
        return False
    x, y = (int(v) for v in c[0])
    return not any((dx or dy) and 0 <= x + dx < w and 0 <= y + dy < h and img[y + dy, x + dx] for dy in (-1, 0, 1) for dx in (-1, 0, 1))


def _check_stages(ctx, oracle, exp, frames, windows, contours=False):
    """every stage the taps expose, after a tapped batch of `frames` under `windows`"""
    n, (h, w) = len(frames), frames.shape[1:3]
    for f, e in enumerate(exp):
        assert np.array_equal(ctx.download_grey(f, w, h), e["planes"][0]["grey"]), f
        for k, wk in enumerate(windows):
            thr = ctx.download_grey(k * n + f, w, h, thresholded=True)
            ref = oracle.adaptive_threshold(e["planes"][0]["grey"], wk)
            assert np.array_equal(ref, e["planes"][k]["thresholded"])
            bad = np.argwhere(thr != ref)
            assert bad.size == 0, f"plane ({k}, {f}) differs at {bad[:5].tolist()} ({len(bad)} px)"
            if contours:
                cs, btype, _ = oracle.find_contours(ref)
                keep = [i for i, c in enumerate(cs) if not _isolated(ref, c)]
                keys, pts = ctx.contours(k * n + f)
                assert len(pts) == len(keep), (k, f, len(pts), len(keep))
                for j, i in enumerate(keep):
                    c = cs[i].astype(np.int64)
                    assert int(keys[j]) == 2 * (int(c[0][1]) * w + int(c[0][0])) + int(btype[i]) and np.array_equal(pts[j], c), (k, f, j)
        assert ctx.candidates(f, before_discard=True).tolist() == e["pre"].tolist(), f"frame {f}: the concatenated list differs"
        assert ctx.candidates(f).tolist() == e["fin"].tolist(), f"frame {f}: the final candidates differ"
        if e["final"] is not None:
            _, ok, codes, dec = ctx.homographies(f, with_patches=False)
            assert ok.tolist() == e["final"]["homography_ok"].tolist() and dec.tolist() == e["final"]["decode_ok"].tolist()
            assert codes.tolist() == e["final"]["codes"].tolist()


# ------------------------------------------------------------------------------------------------------------------
# 1. one window: the ordinary path with that radius
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("w", (1, 7, 12, 31))
def test_one_window_is_the_single_window_path(dicts, w):
    d = dicts.new_from_named_dict("ARUCO_DEFAULT")
    args, keep = _args(mw.config1_frames(3))
    ref_m, ref_per = _detector(d, window=w)._context().detect_batch(*args)
    assert len(ref_m) >= 3
    ctx = _detector(d, windows=(w,), window=9)._context()      # (the config's own window is another one: the set radius decides)
    assert ctx.get_threshold_windows() == (w,)
    m, per = ctx.detect_batch(*args)
    assert marker_tuples(m) == marker_tuples(ref_m) and per.tolist() == ref_per.tolist()


def test_unsetting_returns_the_plain_result(dicts):
    d = dicts.new_from_named_dict("ARUCO_DEFAULT")
    args, keep = _args(mw.config1_frames(3))
    ctx = _detector(d)._context()
    plain_m, plain_per = ctx.detect_batch(*args)
    ctx.set_threshold_windows((3, 7, 15))
    m, per = ctx.detect_batch(*args)
    assert ctx.get_threshold_windows() == (3, 7, 15) and marker_tuples(m) != marker_tuples(plain_m)
    for off in (None, ()):
        ctx.set_threshold_windows((7, 15))
        ctx.set_threshold_windows(off)
        assert ctx.get_threshold_windows() == ()
        m, per = ctx.detect_batch(*args)
        assert marker_tuples(m) == marker_tuples(plain_m) and per.tolist() == plain_per.tolist()


# ------------------------------------------------------------------------------------------------------------------
# 2. stage by stage: one batch of three frames, so the plane index matters
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("factor", mw.FACTORS)
@pytest.mark.parametrize("crop", (None, (634, 470)), ids=("640x480", "634x470"))
def test_stage_by_stage(dicts, oracle, crop, factor):
    d = dicts.new_from_named_dict("ARUCO_DEFAULT")
    frames = mw.config1_frames(3, crop)
    exp = mw.expectation(oracle, d, frames, mw.WINDOWS, factor, key=("config1", crop))
    want = mw.expected_markers(exp)
    assert len(want) >= 12 and sum(e["census"]["rotation_only_kills"] for e in exp) >= 1
    args, keep = _args(frames)
    ctx = _detector(d, windows=mw.WINDOWS, factor=factor)._context()
    for taps in (True, False):
        ctx.set_debug_taps(taps)
        m, per = ctx.detect_batch(*args)
        assert _as_expected(m) == want, taps
        assert per.tolist() == [len(e["final"]["markers"]) for e in exp]
        if taps:
            _check_stages(ctx, oracle, exp, frames, mw.WINDOWS, contours=crop is None and factor == 0.1)
            s = ctx.stats()
            assert s["candidates_pre"] == sum(len(e["pre"]) for e in exp) and s["candidates"] == sum(len(e["fin"]) for e in exp)
    # the merge finds what no single window of the set finds alone here
    assert len(want) > max(sum(len(e["planes"][k]["markers"]) for e in exp) for k in (1, 2))


# ------------------------------------------------------------------------------------------------------------------
# 3. designed frames: squares on a flat field
# ------------------------------------------------------------------------------------------------------------------
_DW, _DH, _DWIN, _DFACTOR, _DSIDE = 400, 300, (3, 15), 0.01, 0.5


def _designed():
    blank = mw.squares_frame(_DW, _DH, [])
    # a bright 4 x 4 square on black: radius r paints a ring of side 4 + 2r around it, 10 (too short a side) at 3 and 34 at 15
    lone = mw.squares_frame(_DW, _DH, [(100, 100, 104, 104)], background=0, ink=255)
    forty = mw.squares_frame(_DW, _DH, mw.grid_boxes(8, 5, 14, 30))
    seventy = mw.squares_frame(_DW, _DH, mw.grid_boxes(10, 7, 14, 30))
    return np.stack([forty, blank, lone, seventy])


def test_designed_frames(dicts, oracle):
    d = dicts.new_from_named_dict("ARUCO_DEFAULT")
    frames = _designed()
    exp = mw.expectation(oracle, d, frames[..., None], _DWIN, _DFACTOR, key="designed", min_side=_DSIDE)
    counts = [[len(p["candidates_pre"]) for p in e["planes"]] for e in exp]
    assert counts[1] == [0, 0]                                                     # no candidate in any plane
    assert counts[2][0] == 0 and counts[2][1] >= 1                                 # one plane empty, another not
    assert max(counts[0]) <= 64 < sum(counts[0])                                   # merged beyond 64, each plane within
    assert max(counts[3]) > 64                                                     # a single plane beyond 64
    assert all(len(e["fin"]) < len(e["pre"]) for e in (exp[0], exp[3]))            # the discard has work to do
    args, keep = _args(frames)
    ctx = _detector(d, windows=_DWIN, factor=_DFACTOR, min_side=_DSIDE)._context()
    for taps in (True, False):
        ctx.set_debug_taps(taps)
        m, per = ctx.detect_batch(*args)
        assert _as_expected(m) == mw.expected_markers(exp) and per.tolist() == [0 if e["final"] is None else len(e["final"]["markers"]) for e in exp]
        if taps:
            _check_stages(ctx, oracle, exp, frames, _DWIN)
    # each frame alone: a batch of one (the blank one: a batch without a contour graph)
    for f in (1, 2, 0):
        a1, k1 = _args(frames[f: f + 1])
        ctx.set_debug_taps(True)
        m, per = ctx.detect_batch(*a1)
        assert ctx.candidates(0, before_discard=True).tolist() == exp[f]["pre"].tolist() and ctx.candidates(0).tolist() == exp[f]["fin"].tolist()


# ------------------------------------------------------------------------------------------------------------------
# 4. the through-memory form (and 8: a plane that outgrows its table is re-run, the merged tables growing with it)
# ------------------------------------------------------------------------------------------------------------------
def test_through_memory_form(dicts, oracle):
    """69 x 51 squares of 6 px: 3519 quads in each of two planes -- the per-plane tables grow 1024 -> 4096 in a re-run, the merged
    tables hold 8192 slots (beyond kFrameCandLds) and the merged list 7038"""
    d = dicts.new_from_named_dict("ARUCO_DEFAULT")
    w, h, windows, factor, side = 640, 480, (1, 2), 0.001, 0.05
    img = mw.squares_frame(w, h, mw.grid_boxes((w - 16) // 9, (h - 16) // 9, 6, 9))
    e = mw.expect_frame(oracle, d, img, windows, factor, side)
    assert len(e["pre"]) > LDS_SLOTS and all(2048 < len(p["candidates_pre"]) <= 4096 for p in e["planes"])
    assert 0 < len(e["fin"]) < len(e["pre"])
    args, keep = _args(img[None])
    ctx = _detector(d, windows=windows, factor=factor, min_side=side)._context()
    ctx.set_debug_taps(True)
    m, per = ctx.detect_batch(*args, out_cap=8192)
    assert ctx.stats()["reruns"] >= 1      # the first pass overflowed the planes' tables: re-run
    pre, fin = ctx.candidates(0, before_discard=True), ctx.candidates(0)
    assert np.array_equal(pre, e["pre"]) and np.array_equal(fin, e["fin"])
    assert _as_expected(m) == mw.expected_markers([e])


# ------------------------------------------------------------------------------------------------------------------
# the kernel alone on hand-made tables: rotated copies, ties and late bigger quads across windows, in all three forms
# ------------------------------------------------------------------------------------------------------------------
def _hand_made(n_groups, rng, K):
    """per window a list of quads: groups of up to K near-copies of one quad, one per window, each rotated by a random number of
    corners and jittered by a pixel or two (some exact copies: ties), the bigger one sometimes in a later window"""
    lists = [[] for _ in range(K)]
    for g in range(n_groups):
        cx, cy, s = 100 + 150 * (g % 60), 100 + 150 * (g // 60), int(rng.integers(20, 50))
        base = np.array([(cx - s, cy - s), (cx + s, cy - s), (cx + s, cy + s), (cx - s, cy + s)])
        for k in range(K):
            if rng.integers(0, 4) == 0 and k:
                continue
            grow = int(rng.integers(-2, 3))
            q = base + np.array([(-grow, -grow), (grow, -grow), (grow, grow), (-grow, grow)]) + rng.integers(-1, 2, size=(4, 2)) * int(rng.integers(0, 2))
            lists[k].append(np.roll(q, -int(rng.integers(0, 4)), axis=0))
    return [np.array(q).reshape(-1, 4, 2) for q in lists]


@pytest.mark.parametrize("form,K,plane_cand,groups", (("reg", 3, 1024, 20), ("lds", 3, 1024, 300), ("lds_full", 2, 3072, 700), ("big", 2, 3073, 700),
                                                     ("big4", 4, 2048, 400)))
def test_kernel_on_hand_made_tables(dicts, form, K, plane_cand, groups):
    from aruco3_amd import _lib

    d = dicts.new_from_named_dict("ARUCO_DEFAULT")
    ctx = _detector(d)._context()
    rng = np.random.default_rng(77 + groups + K)
    frames = [_hand_made(groups, rng, K), [np.zeros((0, 4, 2), np.int64)] * K, _hand_made(3, rng, K), _hand_made(max(groups // 2, 2), rng, K)]
    n = len(frames)
    counts = np.zeros(K * n, dtype=np.uint32)
    recs = []
    for k in range(K):
        for f in range(n):
            q = frames[f][k]
            keys = np.sort(rng.choice(1 << 20, size=len(q), replace=False)).astype(np.uint32)      # ascending: the list's order
            r = np.zeros(len(q), dtype=_lib.CAND_DTYPE)
            r["start_key"], r["xy"] = keys, q.reshape(-1, 8)
            recs.append(r[rng.permutation(len(q))])                                                # the table's order is not
            counts[k * n + f] = len(q)
    md = 12.0
    out = ctx.debug_merge_candidates(n, K, plane_cand, counts, np.concatenate(recs), md, S=0)
    m = out["merged_cap"]
    assert (m > LDS_SLOTS) == form.startswith("big") and out["err_flags"] == 0
    total, census = 0, dict(rotation_only_kills=0, cross_equal_perimeter_pairs=0, i_dies=0)
    for f in range(n):
        pre, win, kept, c = mw.merged_model(frames[f], md)
        for key in census:
            census[key] += c[key]
        assert out["merged_count"][f] == len(pre) and out["fin_count"][f] == len(kept), f
        assert (form != "reg" or len(pre) <= 64) and (form == "reg" or f != 0 or len(pre) > 64)
        assert np.array_equal(out["pre_xy"][f, :len(pre)], pre) and np.array_equal(out["fin_xy"][f, :len(kept)], pre[kept]), f
        assert np.all(out["fin_xy"][f, len(kept):] == 0xFFFF)                                      # nothing written past the survivors
        total += len(kept)
    assert out["work_count"] == total and sorted(out["work"][:total].tolist()) == [f * m + i for f in range(n) for i in range(out["fin_count"][f])]
    assert census["rotation_only_kills"] >= 1 and census["cross_equal_perimeter_pairs"] >= 1 and census["i_dies"] >= 1, census


def test_kernel_flags_planes_and_sums_beyond_their_tables(dicts):
    """a plane beyond plane_cand: the frame is left empty and reports the fullest plane (the contour stage has raised the flag); planes
    that sum beyond the merged capacity -- possible only at the format's limit -- raise kErrCandTable and report the sum"""
    from aruco3_amd import _lib

    d = dicts.new_from_named_dict("ARUCO_DEFAULT")
    ctx = _detector(d)._context()
    rng = np.random.default_rng(5)
    q = _hand_made(8, rng, 2)

    def recs(quads):
        r = np.zeros(len(quads), dtype=_lib.CAND_DTYPE)
        r["start_key"], r["xy"] = np.arange(len(quads)), quads.reshape(-1, 8)
        return r
    out = ctx.debug_merge_candidates(2, 2, 4, [4, 3, 9, 2], np.concatenate([recs(q[0][:4]), recs(q[0][:3]), recs(q[1][:4]), recs(q[1][:2])]), 12.0)
    assert out["merged_count"].tolist() == [9, 5] and out["fin_count"][0] == 0 and out["err_flags"] == 0
    pre, _, kept, _ = mw.merged_model([q[0][:3], q[1][:2]], 12.0)
    assert np.array_equal(out["fin_xy"][1, :len(kept)], pre[kept]) and out["work_count"] == len(kept)
    far = np.array([[(10 + 3 * i, 5), (12 + 3 * i, 5), (12 + 3 * i, 7), (10 + 3 * i, 7)] for i in range(16385)])
    cnt = [16385, 16385, 16385, 16385]
    out = ctx.debug_merge_candidates(1, 4, 16385, cnt, np.concatenate([recs(far)] * 4), 0.0)
    assert out["merged_cap"] == 65536 and out["merged_count"].tolist() == [65540] and out["err_flags"] == 8 and out["fin_count"][0] == 0


_ONE_PLANE = (("reg_2_kill_j", 2, 1024), ("reg_2_i_dies", 2, 1024), ("reg_64", 64, 1024), ("lds_65", 65, 1024), ("big_65", 65, 3073))


def _one_plane_quads(name, c):
    """c quads of candidates_util.clusters in walk order.  Two quads make one row, which either kills j or lets i die: both orders of
    one close pair, the bigger quad first (j is killed) and second (i dies)."""
    from tests import candidates_util as cu

    rng = np.random.default_rng(4200 + c)
    if c > 2:
        return cu.clusters(c, rng, n_clusters=4), rng
    q = cu.clusters(2, rng, n_clusters=1)
    per = cu.perimeters(q.reshape(2, 8).astype(np.float32))
    assert per[0] != per[1]
    bigger_first = per[0] > per[1]
    return (q if bigger_first == name.endswith("kill_j") else q[::-1]), rng


@pytest.mark.parametrize("name,c,plane_cand", _ONE_PLANE, ids=[p[0] for p in _ONE_PLANE])
def test_one_filled_plane_is_the_single_table_walk(dicts, oracle, name, c, plane_cand):
    """k_merge_candidates and k_frame_candidates run one body: with K = 2 and every count of plane 1 at zero, every output of the
    merge is what candidates_util.model expects of plane 0's table alone (projections: oracle.from_control_points), and equals
    a3_debug_frame_candidates' on that table slot for slot, the 0xFF remainder included.  One frame of c quads and an empty one:
    c = 2 and 64 take the register walk, 65 the LDS walk, 65 in planes of 3073 (merged capacity 6146, beyond kFrameCandLds) the
    through-memory one."""
    from tests import candidates_util as cu

    md, S, n = 25.0, 49, 2
    quads, rng = _one_plane_quads(name, c)
    fr = cu.frame(name, quads, rng, plane_cand)
    order, kept, census = cu.model(fr.records["xy"].reshape(-1, 4, 2), fr.records["start_key"], md)
    srt = fr.records["xy"][order]
    assert np.array_equal(srt.reshape(-1, 4, 2), quads)
    kills_j = c - len(kept) - census["i_dies"]          # a dead quad was killed as some row's j, or died as a row's i
    if c == 2:
        assert (kills_j, census["i_dies"]) == ((1, 0) if name.endswith("kill_j") else (0, 1)), census
    else:
        assert kills_j >= 1 and census["i_dies"] >= 1 and len(kept) >= 2, census
    ctx = _detector(dicts.new_from_named_dict("ARUCO_DEFAULT"))._context()
    got = ctx.debug_merge_candidates(n, 2, plane_cand, [c, 0, 0, 0], fr.records, md, S=S)
    m, total = got["merged_cap"], len(kept)
    assert m == 2 * plane_cand and (m > LDS_SLOTS) == name.startswith("big") and got["err_flags"] == 0
    assert got["merged_count"].tolist() == [c, 0] and got["fin_count"].tolist() == [total, 0] and got["work_count"] == total
    pre, fin = got["pre_xy"].reshape(n, m, 8), got["fin_xy"].reshape(n, m, 8)
    assert np.array_equal(pre[0, :c], srt) and (pre[0, c:] == 0xFFFF).all() and (pre[1] == 0xFFFF).all()
    assert np.array_equal(fin[0, :total], srt[kept]) and (fin[0, total:] == 0xFFFF).all() and (fin[1] == 0xFFFF).all()
    assert got["work"][:total].tolist() == list(range(total)) and (got["work"][total:] == 0xFFFFFFFF).all()
    proj = got["proj"]
    assert (proj[total:].view(np.uint8) == 0xFF).all()
    to = np.array([0, 0, S, 0, S, S, 0, S], dtype=np.float32)
    solved = 0
    for pos, quad in enumerate(srt[kept]):
        ok, _, inv = oracle.from_control_points(quad.astype(np.float32), to)
        assert int(proj[pos]["ok"]) == int(ok), (pos, quad)
        if ok:
            assert np.array_equal(proj[pos]["inv"].view(np.uint32), inv.view(np.uint32)), (pos, quad)
            solved += 1
    assert solved >= 1
    # the single-table kernel on plane 0's records, in tables of the merged size
    one = ctx.debug_frame_candidates([c, 0], fr.records, m, md, S)
    for key in ("pre_xy", "fin_xy"):
        assert np.array_equal(got[key].reshape(n, m, 8), one[key]), key
    assert np.array_equal(got["fin_count"], one["fin_count"]) and np.array_equal(got["work"], one["work"]) and one["work_count"] == total
    assert np.array_equal(proj["ok"], one["proj"]["ok"])
    solved_at = proj["ok"] == 1                         # (a failed solve leaves no defined inverse behind)
    assert np.array_equal(proj["inv"][solved_at].view(np.uint32), one["proj"]["inv"][solved_at].view(np.uint32))
    assert np.array_equal(proj[total:].view(np.uint8), one["proj"][total:].view(np.uint8))


# ------------------------------------------------------------------------------------------------------------------
# 5. composition
# ------------------------------------------------------------------------------------------------------------------
def test_with_refinement_and_poses(dicts, oracle):
    """everything behind the marker list composes unchanged: the markers are test 2's, the refined corners are the refinement oracle's
    from those markers on frame f, and the poses are a3_estimate_pose's on the corners the batch solved from"""
    from aruco3_amd import _lib
    from aruco3_amd.aruco import CornerRefinement
    from tests import refine_oracle as refo

    d = dicts.new_from_named_dict("ARUCO_DEFAULT")
    frames = mw.config1_frames(3)
    exp = mw.expectation(oracle, d, frames, mw.WINDOWS, 0.1, key=("config1", None))
    args, keep = _args(frames)
    intr = _lib.Intrinsics(640, 480, 600.0, 590.0, 323.5, 237.75)

    def poses_of(rec, n):
        return np.frombuffer(rec, dtype=np.float32).reshape(-1, 2, 13)[:n]
    # without refinement: a3_estimate_pose on the integer corners
    ctx0 = _detector(d, windows=mw.WINDOWS)._context()
    m0, per0, poses0 = ctx0.detect_batch_pose(*args, 50.0, intr)
    assert _as_expected(m0) == mw.expected_markers(exp)
    assert np.allclose(poses0, poses_of(ctx0.estimate_pose(m0["corners"], 50.0, intrinsics=intr), len(m0)), rtol=0, atol=1e-4)
    # with it: the same markers, the oracle's refined corners, a3_estimate_pose_normalized on them
    det = _detector(d, windows=mw.WINDOWS, refinement=CornerRefinement())
    ctx = det._context()
    det._apply_refinement(ctx)
    m, per, poses = ctx.detect_batch_pose(*args, 50.0, intr)
    assert _as_expected(m) == mw.expected_markers(exp) and per.tolist() == per0.tolist()
    refined = ctx.refined_corners()
    cells = int(np.ceil(np.sqrt(d.num_bits))) + 2
    pos = 0
    for f in range(3):
        cnt = int(per[f])
        want = refo.refine_markers(oracle.to_luma8(frames[f]), [mk["corners"] for mk in m[pos: pos + cnt]], cells)
        assert np.array_equal(np.asarray(want, np.float32).view(np.uint32), refined[pos: pos + cnt].view(np.uint32)), f
        pos += cnt
    q = refined.astype(np.float32)
    pts = np.stack([(q[..., 0] - np.float32(intr.principal_x)) / np.float32(intr.focal_x),
                    (q[..., 1] - np.float32(intr.principal_y)) / np.float32(intr.focal_y)], axis=-1).astype(np.float32)
    assert np.allclose(poses, poses_of(ctx.estimate_pose_normalized(pts.reshape(-1, 8), 50.0), len(m)), rtol=0, atol=1e-4)
    assert np.abs(poses - poses0).max() > 0      # (the refined corners do move the poses: not the same comparison twice)


def test_with_reduction(dicts, oracle):
    import aruco3_amd
    from aruco3_amd.aruco import Reduction

    d = dicts.new_from_named_dict("ARUCO_DEFAULT")
    from aruco3_amd import synth

    spec = synth.SynthSpec(960, 720, n_markers=(3, 3), side=(170.0, 230.0), min_center_sep=300.0, rotation_deg=(-20.0, 20.0))
    frames = np.stack([synth.render_frame(spec, d.code_list, d.num_bits, 4100 + i)[0] for i in range(2)])
    small = aruco3_amd.reduce_frames(frames, 2)
    a_small, k1 = _args(small)
    ref_m, ref_per = _detector(d, windows=mw.WINDOWS)._context().detect_batch(*a_small)
    assert len(ref_m) >= 4
    a_full, k2 = _args(frames)
    m, per = _detector(d, windows=mw.WINDOWS, reduction=Reduction(2))._context().detect_batch(*a_full)
    want = [(f, i, c, tuple(2 * v + 1 for v in xy), hd, rot, ci) for f, i, c, xy, hd, rot, ci in marker_tuples(ref_m)]
    assert marker_tuples(m) == want and per.tolist() == ref_per.tolist()


# ------------------------------------------------------------------------------------------------------------------
# 6. in flight
# ------------------------------------------------------------------------------------------------------------------
def test_batch_queue(dicts, oracle):
    from aruco3_amd.aruco import BatchQueue

    d = dicts.new_from_named_dict("ARUCO_DEFAULT")
    frames = mw.config1_frames(3)
    exp = mw.expectation(oracle, d, frames, mw.WINDOWS, 0.1, key=("config1", None))
    det = _detector(d, windows=mw.WINDOWS)
    sync = det.detect_batch(frames)
    want = [[(m.id, m.code, tuple(m.corners), m.hamming_distance) for m in f.markers] for f in sync]
    assert want == [[(m["id"], m["code"], tuple(m["corners"]), m["hamming_distance"]) for m in e["final"]["markers"]] for e in exp]
    for gates in (False, True):
        q = BatchQueue(det, depth=2, gates=gates)
        try:
            for rounds in range(2):
                q.submit(frames)
                q.submit(frames)
                for _ in range(2):
                    got = q.collect()
                    assert [[(m.id, m.code, tuple(m.corners), m.hamming_distance) for m in f.markers] for f in got] == want, (gates, rounds)
        finally:
            q.close()


# ------------------------------------------------------------------------------------------------------------------
# 7. refusals, through the C ABI
# ------------------------------------------------------------------------------------------------------------------
def test_refusals(dicts):
    from aruco3_amd import _lib

    d = dicts.new_from_named_dict("ARUCO_DEFAULT")
    ctx = _detector(d)._context()
    L = _lib.load()
    ctx.set_threshold_windows((3, 7))

    def current():
        arr, n = (C.c_uint32 * 4)(), C.c_size_t(99)
        assert L.a3_get_threshold_windows(ctx.handle, arr, 4, C.byref(n)) == _lib.OK
        return [int(arr[i]) for i in range(n.value)]

    def refused(radii, want):
        arr = (C.c_uint32 * max(len(radii), 1))(*radii)
        rc = L.a3_set_threshold_windows(ctx.handle, arr, len(radii))
        msg = L.a3_last_error(ctx.handle)
        msg = msg.decode() if isinstance(msg, bytes) else C.cast(msg, C.c_char_p).value.decode()
        assert rc == _lib.ERR_INVALID and msg == want, (radii, rc, msg)
        assert current() == [3, 7]

    refused((1, 2, 3, 4, 5), "a3_set_threshold_windows: more than A3_MAX_THRESHOLD_WINDOWS (4) windows")
    refused((0,), "a3_set_threshold_windows: a radius must be > 0 (imageproc asserts block_radius > 0)")
    refused((3, 0), "a3_set_threshold_windows: a radius must be > 0 (imageproc asserts block_radius > 0)")
    refused((0x80000000,), "a3_set_threshold_windows: a radius must be at most 2^31 - 1 (the threshold kernels take it as a signed 32-bit int)")
    refused((7, 32), "a3_set_threshold_windows: in a set of two or more every radius must be in 1..31")
    refused((7, 7), "a3_set_threshold_windows: the radii must be strictly ascending")
    refused((15, 7, 3), "a3_set_threshold_windows: the radii must be strictly ascending")
    # a batch submitted and not yet collected: refused, off included; accepted again after the collect
    args, keep = _args(mw.config1_frames(1))
    ctx.submit(*args)
    refused((3, 7, 15), "a3_set_threshold_windows: a submitted batch has not been collected")
    assert L.a3_set_threshold_windows(ctx.handle, None, 0) == _lib.ERR_INVALID and current() == [3, 7]
    m, per = ctx.collect()
    # the getter's capacity
    n = C.c_size_t(0)
    assert L.a3_get_threshold_windows(ctx.handle, (C.c_uint32 * 1)(), 1, C.byref(n)) == _lib.ERR_CAPACITY and n.value == 2
    ctx.set_threshold_windows((1, 2, 30, 31))
    assert current() == [1, 2, 30, 31]
    ctx.set_threshold_windows((0x7FFFFFFF,))
    assert current() == [0x7FFFFFFF]
    assert L.a3_set_threshold_windows(ctx.handle, None, 3) == _lib.OK and current() == []
    # frames x windows beyond 65535 is the detect call's to refuse (nothing is read: the check comes before the frames are touched)
    ctx.set_threshold_windows((3, 7, 15, 31))
    out, per, nn = np.zeros(1, _lib.MARKER_DTYPE), np.zeros(16384, np.uint32), C.c_size_t()
    px = np.zeros(16, np.uint8)
    rc = L.a3_detect_batch(ctx.handle, C.c_void_p(px.ctypes.data), _lib.MEM_HOST, _lib.FMT_L8, 4, 4, 4, 0, 16384, out.ctypes.data_as(C.c_void_p), 1,
                           per.ctypes.data_as(C.POINTER(C.c_uint32)), C.byref(nn))
    assert rc == _lib.ERR_INVALID
