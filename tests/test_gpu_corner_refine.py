"""Sub-pixel corner refinement on the MI355X (k_refine_corners, a3_set_corner_refinement / a3_get_refined_corners /
a3_refine_corners): bit-equal to the CPU restatement (tests/refine_oracle.c) started from the same integer corners, in every frame format
and layout, through every scheduling path; poses from the refined corners; refinement off leaves every result as it was."""
import numpy as np
import pytest

from tests import refine_oracle as refo
from tests.util import marker_tuples

pytestmark = pytest.mark.gpu


def _torch():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("needs the MI355X")
    return torch


def _dict(name):
    from aruco3_amd import ARDictionary

    return ARDictionary.new_from_named_dict(name)


def _ctx(d, refine=True):
    from aruco3_amd import _lib

    ctx = _lib.Context(_lib.default_config(), d.code_list, d.num_bits, d._tau)
    if refine:
        ctx.set_corner_refinement(_lib.default_refine_config())
    return ctx


def _cells(d):
    return int(np.ceil(np.sqrt(d.num_bits))) + 2


def _expect(oracle, d, frames_host, markers, per, frames_to_check=None):
    """the oracle's refinement of every marker (a3_marker order, window from its quad) -> float32 (n, 4, 2), NaN for unchecked frames"""
    out = np.full((len(markers), 4, 2), np.nan, np.float32)
    pos = 0
    for f in range(len(per)):
        cnt = int(per[f])
        if cnt and (frames_to_check is None or f in frames_to_check):
            grey = oracle.to_luma8(np.ascontiguousarray(frames_host(f) if callable(frames_host) else frames_host[f]))
            out[pos: pos + cnt] = refo.refine_markers(grey, [m["corners"] for m in markers[pos: pos + cnt]], _cells(d))
        pos += cnt
    return out


def _bit_equal(got, want):
    got = np.asarray(got, np.float32)
    want = np.asarray(want, np.float32)
    sel = ~np.isnan(want)
    assert got.shape == want.shape
    bad = np.argwhere(sel & (got.view(np.uint32) != want.view(np.uint32)))
    assert bad.size == 0, (bad[:4].tolist(), got[tuple(bad[0][:1])] if bad.size else None, want[tuple(bad[0][:1])] if bad.size else None)
    return int(sel.sum() // 8)


@pytest.mark.parametrize("config,count", [(1, 4), (4, 3), (5, 2)])
def test_batch_refined_corners_equal_oracle(oracle, config, count):
    from aruco3_amd import _lib, synth

    torch = _torch()
    frames, _ = synth.config_frames(config, count)
    _, name = synth.config_spec(config)
    d = _dict(name)
    h, w = frames.shape[1:3]
    dev = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    plain = _ctx(d, refine=False)
    m0, p0 = plain.detect_batch(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, count)
    ctx = _ctx(d)
    m, p = ctx.detect_batch(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, count)
    assert marker_tuples(m) == marker_tuples(m0) and p.tolist() == p0.tolist()     # refinement adds, it changes nothing
    assert len(m) >= count * 3
    assert _bit_equal(ctx.refined_corners(), _expect(oracle, d, frames, m, p)) == len(m)
    with pytest.raises(_lib.A3Error) as e:   # the plain context's last batch ran without refinement
        plain.refined_corners()
    assert e.value.code == _lib.ERR_INVALID


def test_config2_full_batch_equal_oracle(oracle):
    """BASELINE config 2: one 256-frame 1080p batch rendered on the device; every marker refined, 32 frames checked against the oracle"""
    from aruco3_amd import _lib, synth

    torch = _torch()
    spec, name = synth.config_spec(2)
    d = _dict(name)
    seeds = [synth.frame_seed(2, i) for i in range(256)]
    dev, _ = synth.render_frames_device(spec, d.code_list, d.num_bits, seeds)
    torch.cuda.synchronize()
    w, h = spec.width, spec.height
    ctx = _ctx(d)
    m, p = ctx.detect_batch(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, 256, out_cap=256 * 64)
    ref = ctx.refined_corners()
    assert ref.shape == (len(m), 4, 2) and len(m) >= 256 * 3
    check = set(range(0, 256, 8))
    n = _bit_equal(ref, _expect(oracle, d, lambda f: dev[f].cpu().numpy(), m, p, frames_to_check=check))
    assert n >= 32 * 3


def _layouts(frames, fmt_name):
    """(fmt, host array of frame 0.., row_stride, frame_stride, byte offset) variants: packed, padded rows, padded frames + offset"""
    from aruco3_amd import _lib

    n, h, w, _ = frames.shape
    if fmt_name == "rgb":
        px, fmt = frames, _lib.FMT_RGB8
    elif fmt_name == "rgba":
        px, fmt = np.concatenate([frames, np.full(frames.shape[:3] + (1,), 255, np.uint8)], axis=3), _lib.FMT_RGBA8
    elif fmt_name == "bgra":
        px, fmt = np.concatenate([frames[..., ::-1], np.full(frames.shape[:3] + (1,), 255, np.uint8)], axis=3), _lib.FMT_BGRA8
    else:
        px, fmt = np.stack([_lib_luma(f) for f in frames])[..., None], _lib.FMT_L8
    bpp = px.shape[3]
    out = []
    for pad_row, pad_frame, off in ((0, 0, 0), (40, 0, 0), (24, 1000, 13)):
        rs = w * bpp + pad_row
        fs = rs * h + pad_frame
        buf = np.zeros(off + fs * n + 64, np.uint8)
        for f in range(n):
            for y in range(h):
                buf[off + f * fs + y * rs: off + f * fs + y * rs + w * bpp] = px[f, y].reshape(-1)
        out.append((fmt, buf, off, rs, fs, px))
    return out


def _lib_luma(frame):
    f = frame.astype(np.uint32)
    return ((2126 * f[..., 0] + 7152 * f[..., 1] + 722 * f[..., 2]) // 10000).astype(np.uint8)


@pytest.mark.parametrize("fmt_name", ["rgb", "rgba", "bgra", "l8"])
def test_formats_layouts_memory_and_taps(oracle, fmt_name):
    from aruco3_amd import _lib, synth

    torch = _torch()
    frames, _ = synth.config_frames(1, 2)
    d = _dict("ARUCO_DEFAULT")
    n, h, w, _ = frames.shape
    base = None
    for fmt, buf, off, rs, fs, px in _layouts(frames, fmt_name):
        for memory in (_lib.MEM_HOST, _lib.MEM_DEVICE):
            for taps in (False, True):
                ctx = _ctx(d)
                ctx.set_debug_taps(taps)
                if memory == _lib.MEM_HOST:
                    ptr, keep = buf.ctypes.data + off, buf
                else:
                    keep = torch.from_numpy(buf).cuda()
                    torch.cuda.synchronize()
                    ptr = keep.data_ptr() + off
                m, p = ctx.detect_batch(ptr, memory, fmt, w, h, rs, fs, n)
                got = ctx.refined_corners()
                if base is None:   # (into_luma8 of every format is the luma of the RGB frames)
                    base = (marker_tuples(m), got.copy())
                    assert _bit_equal(got, _expect(oracle, d, frames, m, p)) == len(m) >= 8
                assert marker_tuples(m) == base[0], (fmt_name, off, memory, taps)
                assert np.array_equal(got.view(np.uint32), base[1].view(np.uint32)), (fmt_name, off, memory, taps)
                del keep


def test_standalone_refine_equals_oracle(oracle):
    from aruco3_amd import _lib, synth

    torch = _torch()
    frames, truths = synth.config_frames(2, 1)
    d = _dict("ARUCO")
    h, w = frames.shape[1:3]
    grey = oracle.to_luma8(frames[0])
    rng = np.random.default_rng(5)
    starts = np.concatenate([np.asarray(t.corners) for t in truths[0]]) + rng.uniform(-1.5, 1.5, size=(4 * len(truths[0]), 2))
    starts = np.concatenate([starts, [[0.0, 0.0], [w - 1.0, h - 1.0], [3.25, h - 2.5]]]).astype(np.float32)   # + frame corners
    cell = rng.uniform(5.0, 40.0, size=len(starts)).astype(np.float32)
    ctx = _ctx(d, refine=False)   # (off on the context: a3_refine_corners uses the default settings)
    dev = torch.from_numpy(frames[0]).cuda()
    torch.cuda.synchronize()
    for cp in (None, cell):
        want = refo.refine_corners(grey, starts, refo.RefineConfig.default(), cp)
        got_h = ctx.refine_corners(frames[0].ctypes.data, _lib.MEM_HOST, _lib.FMT_RGB8, w, h, w * 3, starts, cp)
        got_d = ctx.refine_corners(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, starts, cp)
        assert np.array_equal(got_h.view(np.uint32), want.view(np.uint32))
        assert np.array_equal(got_d.view(np.uint32), want.view(np.uint32))
        assert np.abs(want - starts).max() > 0.1
    small = refo.RefineConfig(1, 3, 0.0, 7, 0.05)   # the context's own setting when refinement is on
    ctx.set_corner_refinement(_lib.RefineConfig(1, 3, 0.0, 7, 0.05))
    got = ctx.refine_corners(frames[0].ctypes.data, _lib.MEM_HOST, _lib.FMT_RGB8, w, h, w * 3, starts)
    assert np.array_equal(got.view(np.uint32), refo.refine_corners(grey, starts, small).view(np.uint32))
    with pytest.raises(_lib.A3Error):
        ctx.refine_corners(frames[0].ctypes.data, _lib.MEM_HOST, _lib.FMT_RGB8, w, h, w * 3, np.array([[np.nan, 3.0]], np.float32))
    with pytest.raises(_lib.A3Error):
        ctx.set_corner_refinement(_lib.RefineConfig(1, 11, 0.4, 30, 0.01))


def _pose_arrays(oracle, pts):
    p1, p2 = oracle.solve_with_normalized_points(pts, 100.0)
    return np.array([np.concatenate([[e], r.reshape(9), t]) for e, r, t in (p1, p2)], np.float32)


@pytest.mark.parametrize("use_intr", [False, True])
def test_poses_from_refined_corners(oracle, use_intr):
    from aruco3_amd import _lib, synth

    torch = _torch()
    frames, _ = synth.config_frames(5, 2)
    d = _dict("ARUCO")
    n, h, w, _ = frames.shape
    dev = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    intr = _lib.Intrinsics(w, h, 1400.0, 1390.0, w / 2 + 3.5, h / 2 - 2.25) if use_intr else None
    args = (dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, n, 100.0, intr)
    plain = _ctx(d, refine=False)
    m0, p0, poses0 = plain.detect_batch_pose(*args)
    never = _ctx(d, refine=False)
    ctx = _ctx(d)
    m, p, poses = ctx.detect_batch_pose(*args)
    ref = ctx.refined_corners()
    assert marker_tuples(m) == marker_tuples(m0) and len(m) >= 16
    assert _bit_equal(ref, _expect(oracle, d, frames, m, p)) == len(m)
    for i in range(len(m)):
        q = ref[i].astype(np.float32)
        if use_intr:
            pts = np.stack([(q[:, 0] - np.float32(intr.principal_x)) / np.float32(intr.focal_x),
                            (q[:, 1] - np.float32(intr.principal_y)) / np.float32(intr.focal_y)], axis=1)
        else:
            pts = np.stack([q[:, 0] / np.float32(w), q[:, 1] / np.float32(h)], axis=1)
        want = _pose_arrays(oracle, pts.astype(np.float32).reshape(8))
        assert np.array_equal(poses[i].view(np.uint32), want.view(np.uint32)), i
    # refinement switched off again: the poses are the integer-corner poses, byte for byte those of a context that never had it
    ctx.set_corner_refinement(None)
    m1, p1, poses1 = ctx.detect_batch_pose(*args)
    m2, p2, poses2 = never.detect_batch_pose(*args)
    assert marker_tuples(m1) == marker_tuples(m0) == marker_tuples(m2) and p1.tolist() == p0.tolist() == p2.tolist()
    assert np.array_equal(poses1.view(np.uint32), poses0.view(np.uint32)) and np.array_equal(poses2.view(np.uint32), poses0.view(np.uint32))
    with pytest.raises(_lib.A3Error) as e:
        ctx.refined_corners()
    assert e.value.code == _lib.ERR_INVALID


@pytest.mark.parametrize("gates", [False, True])
def test_batch_queue_rotation_carries_refined_corners(oracle, gates):
    from aruco3_amd import synth
    from aruco3_amd.aruco import BatchQueue, CornerRefinement, Detector, DetectorConfig

    torch = _torch()
    frames, _ = synth.config_frames(1, 16)
    d = _dict("ARUCO_DEFAULT")
    det = Detector(DetectorConfig.default(), d, refinement=CornerRefinement())
    dev = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    q = BatchQueue(det, depth=4, gates=gates)
    got = []
    for b in range(8):   # two rotations of batches of two frames
        if q.full:
            got += q.collect()
        q.submit(dev[2 * b: 2 * b + 2])
    while len(q):
        got += q.collect()
    q.close()
    assert len(got) == 16
    for f, detn in enumerate(got):
        grey = oracle.to_luma8(frames[f])
        want = refo.refine_markers(grey, [np.array(mk.corners).reshape(8) for mk in detn.markers], _cells(d))
        assert len(detn.markers) >= 3
        for mk, wq in zip(detn.markers, want):
            assert np.array_equal(np.array(mk.corners_refined, np.float32).view(np.uint32), wq.view(np.uint32))
    single = det.detect(frames[3])   # the Detector surface
    assert [mk.corners_refined for mk in single.markers] == [mk.corners_refined for mk in got[3].markers]
    plain = Detector(DetectorConfig.default(), d).detect(frames[3])
    assert all(mk.corners_refined is None for mk in plain.markers)
    assert [(mk.id, mk.corners) for mk in plain.markers] == [(mk.id, mk.corners) for mk in single.markers]


def test_more_markers_than_the_staging_guess(oracle):
    """one small batch sizes the speculative read-back (guess = 1.25 x its markers + 64); a 40-frame batch then has more markers,
    which finish_batch fetches after growing the staging area -- refined corners included; submit / collect as well"""
    from aruco3_amd import _lib, synth

    torch = _torch()
    frames, _ = synth.config_frames(1, 40)
    d = _dict("ARUCO_DEFAULT")
    h, w = frames.shape[1:3]
    dev = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    ctx = _ctx(d)
    ctx.detect_batch(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, 1)
    assert ctx.stats()["markers"] <= 8
    m, p = ctx.detect_batch(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, 40)
    assert len(m) > 8 * 1.25 + 64
    want = _expect(oracle, d, frames, m, p)
    assert _bit_equal(ctx.refined_corners(), want) == len(m)
    ctx.detect_batch(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, 1)
    ctx.submit_pose(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, 40, 100.0)
    m2, p2, _ = ctx.collect_pose()
    assert marker_tuples(m2) == marker_tuples(m)
    assert _bit_equal(ctx.refined_corners(), want) == len(m)


def test_synchronous_rerun_recomputes_refined_corners(oracle):
    """a noise frame in a batch shaped like the clean one before it outgrows the device plan: the batch is re-run synchronously
    (a3_stats reruns) and the refined corners come from the re-run -- plain call and submit / collect"""
    from aruco3_amd import _lib, synth

    torch = _torch()
    frames, _ = synth.config_frames(1, 2)
    d = _dict("ARUCO_DEFAULT")
    h, w = frames.shape[1:3]
    mixed = frames.copy()
    mixed[1] = synth.noise_frame(w, h, 11)
    ctx = _ctx(d)
    for use_submit in (False, True):
        clean = torch.from_numpy(frames).cuda()
        mix = torch.from_numpy(mixed).cuda()
        torch.cuda.synchronize()
        ctx.detect_batch(clean.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, 2)
        if use_submit:
            ctx.submit(mix.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, 2)
            m, p = ctx.collect()
        else:
            m, p = ctx.detect_batch(mix.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, 2)
        assert ctx.stats()["reruns"] >= 1, ctx.stats()
        assert int(p[0]) >= 3
        assert _bit_equal(ctx.refined_corners(), _expect(oracle, d, mixed, m, p)) == len(m)
        ctx = _ctx(d)   # (a fresh plan for the second form)


def test_refinement_set_between_submit_and_collect_applies_to_later_batches(oracle):
    from aruco3_amd import _lib, synth

    torch = _torch()
    frames, _ = synth.config_frames(1, 2)
    d = _dict("ARUCO_DEFAULT")
    h, w = frames.shape[1:3]
    dev = torch.from_numpy(frames).cuda()
    torch.cuda.synchronize()
    ctx = _ctx(d, refine=False)
    ctx.submit(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, 2)
    ctx.set_corner_refinement(_lib.default_refine_config())
    ctx.collect()
    with pytest.raises(_lib.A3Error) as e:   # the batch was submitted without refinement
        ctx.refined_corners()
    assert e.value.code == _lib.ERR_INVALID
    m, p = ctx.detect_batch(dev.data_ptr(), _lib.MEM_DEVICE, _lib.FMT_RGB8, w, h, w * 3, w * h * 3, 2)
    assert _bit_equal(ctx.refined_corners(), _expect(oracle, d, frames, m, p)) == len(m)
