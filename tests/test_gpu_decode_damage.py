"""The decode stage's error-correcting lookup on DAMAGED markers, GPU half: k_decode (both instantiations: `<256, 256>` for batches
of up to 64 frames, `<256, 64>` beyond) and compact_frame_wave against the numpy expectation of tests/damage_util.py AND the oracle,
on the frames and quads tests/test_decode_damage.py has shown to deliver the drawn bits.  All equalities are exact.  GPU only."""
import numpy as np
import pytest

from tests import damage_util as du
from tests.util import assert_frame_parity, marker_tuples, markers_of_hip, markers_of_oracle

pytestmark = pytest.mark.gpu


def _args(frames):
    """frames [n, h, w] (L8) or [n, h, w, 3] (RGB8) in host memory -> the arguments of detect_batch / submit"""
    from aruco3_amd import _lib

    assert frames.flags["C_CONTIGUOUS"] and frames.dtype == np.uint8
    n, h, w = frames.shape[:3]
    c = frames.shape[3] if frames.ndim == 4 else 1
    return (frames.ctypes.data, _lib.MEM_HOST, _lib.FMT_RGB8 if c == 3 else _lib.FMT_L8, w, h, w * c, h * w * c, n)


def _context(name, filt, config=None):
    from aruco3_amd.aruco import Detector

    d = du.dictionary(name)
    det = Detector(config or du.detector_config(filt, d.num_bits), d)
    ctx = det._context()
    assert ctx.tau == du.tau_of(name)     # (a table that declares tau 0 has it computed by k_calc_tau: numpy's minimum pairwise distance)
    return det, ctx


def _agree(hip, numpy_, oracle_, what):
    """the three descriptions of one thing; on a failure, which pair disagrees and where"""
    pairs = [label for label, a, b in (("HIP != numpy", hip, numpy_), ("HIP != oracle", hip, oracle_), ("numpy != oracle", numpy_, oracle_))
             if a != b]
    if pairs:
        k = next((i for i, t in enumerate(zip(hip, numpy_, oracle_)) if not t[0] == t[1] == t[2]), min(len(hip), len(numpy_), len(oracle_)))
        at = lambda x: x[k] if k < len(x) else "(missing)"
        raise AssertionError(f"{what}: {', '.join(pairs)}; first at entry {k} of {len(hip)} / {len(numpy_)} / {len(oracle_)}: "
                             f"HIP {at(hip)}, numpy {at(numpy_)}, oracle {at(oracle_)}")


def _split(markers, per):
    out, pos = [], 0
    for c in per.tolist():
        out.append(markers_of_hip(markers[pos: pos + c]))
        pos += c
    assert pos == len(markers)
    return out


# ------------------------------------------------------------------------------------------------------------------
# family a: quads handed in, one-frame batches (k_decode<256, 256>)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", du.ALL)
def test_injected_quads(oracle, name):
    """every pattern's quad from each of its four corners: the tapped codes and decode_ok are numpy's, the marker records numpy's and
    the oracle's, per_frame counts the accepted candidates, taps on and off and submit / collect return the same records; filter on
    and off (off: every pattern that passes the border test is accepted with its true distance, however large), L8 and RGB8"""
    nb, _, codes = du.table(name)
    tau = du.tau_of(name)
    cap = 1024
    seen_distance = 0
    for filt in (True, False):
        det, ctx = _context(name, filt)
        for fi, (img, quads, views, _) in enumerate(du.injected_frames(name)):
            exp = [du.expect_view(v, codes) for v in views]
            want = [m for m in (du.expected_marker(e, q, tau, filt) for e, q in zip(exp, quads)) if m is not None]
            for frame in (img, du.as_rgb(img)):
                frames = np.ascontiguousarray(frame[None])
                args = _args(frames)
                what = f"{name}, filter {filt}, frame {fi}, {'RGB8' if frame.ndim == 3 else 'L8'}"
                ref = oracle.detect(frame, codes, nb, tau, config=du.oracle_config(oracle, filt, nb), quads=quads)
                got = {}
                for taps in (True, False):
                    ctx.set_debug_taps(taps)
                    # the hook is one-shot, disarmed at the first enqueue: a batch the library runs twice (first use of a shape, grown
                    # tables) would decode the frame's own quads the second time -- so the frame goes through once as it is first
                    ctx.detect_batch(*args, out_cap=cap)
                    ctx.debug_inject_candidates(quads)
                    m, per = ctx.detect_batch(*args, out_cap=cap)
                    got[taps] = marker_tuples(m)
                    if taps:
                        assert ctx.candidates(0, before_discard=True).tolist() == quads.tolist(), what
                        assert ctx.candidates(0).tolist() == quads.tolist(), what
                        _, ok, tapped, dec = ctx.homographies(0, with_patches=False)
                        assert ok.all(), what
                        _agree(dec.tolist(), [e.decode_ok for e in exp], ref["decode_ok"].tolist(), what + ": decode_ok")
                        _agree([[int(c) for c in r] for r in tapped], [e.codes for e in exp], [[int(c) for c in r] for r in ref["codes"]],
                               what + ": codes")
                    _agree(markers_of_hip(m), want, markers_of_oracle(ref), f"{what}, taps {taps}: markers")
                    assert [int(r["candidate_index"]) for r in m] == [k for k, e in enumerate(exp) if e.accepted(tau, filt)], what
                    assert per.tolist() == [len(want)], what                      # k_decode's atomicAdd against numpy
                assert got[True] == got[False], what + ": taps on and off differ"
                ctx.debug_inject_candidates(quads)
                ctx.submit(*args, out_cap=cap)
                m, per = ctx.collect()
                assert marker_tuples(m) == got[False] and per.tolist() == [len(want)], what + ": submit / collect differs from detect_batch"
            if not filt:
                assert len(want) == sum(e.decode_ok for e in exp)
                seen_distance = max([seen_distance] + [m[3] for m in want])
        del det
    assert seen_distance == du.summary(name)["max_distance"]
    if name == "CHILITAGS":
        assert 30 <= seen_distance <= 64      # an all-white interior of a 64-bit table: far above any tau, inside a3_marker's uint8_t


# ------------------------------------------------------------------------------------------------------------------
# family b: found quads, more than 64 frames a batch (k_decode<256, 64>), and the same frames in chunks of 64 (k_decode<256, 256>)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", du.ALL)
def test_found_quads(oracle, name):
    nb, _, codes = du.table(name)
    tau = du.tau_of(name)
    grey, _ = du.found_frames(name)
    n = len(grey)
    assert n > 64
    cap = 128 * n
    for filt in (True, False):
        det, ctx = _context(name, filt)
        for frames in (grey, np.stack([du.as_rgb(g) for g in grey])):
            args = _args(frames)
            what = f"{name}, filter {filt}, {'RGB8' if frames.ndim == 4 else 'L8'}"
            ctx.set_debug_taps(False)
            m0, per0 = ctx.detect_batch(*args, out_cap=cap)
            ctx.submit(*args, out_cap=cap)
            ms, pers = ctx.collect()
            assert marker_tuples(ms) == marker_tuples(m0) and pers.tolist() == per0.tolist(), what + ": submit / collect differs"
            # the same data through the other instantiation: chunks of at most 64 frames
            pieces, counts = [], []
            for f0 in range(0, n, 64):
                part = np.ascontiguousarray(frames[f0: f0 + 64])
                mp, pp = ctx.detect_batch(*_args(part), out_cap=cap)
                pieces += [(t[0] + f0,) + t[1:] for t in marker_tuples(mp)]
                counts += pp.tolist()
            assert pieces == marker_tuples(m0) and counts == per0.tolist(), what + ": chunks of 64 frames differ from the whole batch"
            ctx.set_debug_taps(True)
            m1, per1 = ctx.detect_batch(*args, out_cap=cap)
            assert marker_tuples(m1) == marker_tuples(m0) and per1.tolist() == per0.tolist(), what + ": taps on and off differ"
            assert [int(r["frame"]) for r in m1] == [f for f, c in enumerate(per1.tolist()) for _ in range(c)]
            per_frame = _split(m1, per1)
            for f in range(n):
                ref = oracle.detect(frames[f], codes, nb, tau, config=du.oracle_config(oracle, filt, nb))
                cands = ctx.candidates(f)
                assert cands.tolist() == ref["candidates"].tolist(), f"{what}, frame {f}: candidates"
                _, ok, tapped, dec = ctx.homographies(f, with_patches=False)
                assert dec.tolist() == ref["decode_ok"].tolist() and tapped.tolist() == ref["codes"].tolist(), f"{what}, frame {f}: codes"
                want, idx, _ = du.expected_of_candidates({"codes": tapped, "decode_ok": dec, "candidates": cands}, codes, tau, filt)
                _agree(per_frame[f], want, markers_of_oracle(ref), f"{what}, frame {f}: markers")
                assert int(per1[f]) == len(want)
        del det


# ------------------------------------------------------------------------------------------------------------------
# family c: damaged tables through the renderer, every stage
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", du.FAMILY_C)
def test_rendered_damage(oracle, name):
    """nothing injected, nothing axis-aligned: every stage HIP == oracle, the nearest-code rule on the tapped codes, and with sigma 0
    exactly the markers the oracle recovers with their drawn id and distance are recovered on the device"""
    from aruco3_amd.aruco import DetectorConfig

    nb, _, codes = du.table(name)
    tau = du.tau_of(name)
    _, damage = du.damaged_table(name)
    for filt in (True, False):
        det, ctx = _context(name, filt, DetectorConfig(min_corner_separation_factor=du.C_SEPARATION, filter_high_bit_errors=filt))
        ocfg = oracle.Config.default()
        ocfg.filter_high_bit_errors = int(filt)
        ocfg.min_corner_separation_factor = du.C_SEPARATION
        for sigma in (0, 6):
            for paper in (True, False):
                made = du.family_c_frames(name, sigma, paper)
                frames = np.ascontiguousarray(np.stack([img for img, _ in made]))
                ctx.set_debug_taps(True)
                m, per = ctx.detect_batch(*_args(frames), out_cap=128 * len(frames))
                got = _split(m, per)
                for f, (img, truth) in enumerate(made):
                    what = f"{name}, filter {filt}, sigma {sigma}, paper {paper}, frame {f}"
                    ref = oracle.detect(img, codes, nb, tau, config=ocfg)
                    assert_frame_parity(ctx, f, img, ref, du.C_W, du.C_H)
                    _, _, tapped, dec = ctx.homographies(f, with_patches=False)
                    want, _, _ = du.expected_of_candidates({"codes": tapped, "decode_ok": dec, "candidates": ctx.candidates(f)}, codes, tau, filt)
                    _agree(got[f], want, markers_of_oracle(ref), what + ": markers")
                    if sigma == 0:
                        assert du.recovered(got[f], truth, damage, tau) == du.recovered(markers_of_oracle(ref), truth, damage, tau), what
        del det


# ------------------------------------------------------------------------------------------------------------------
# poses of a damaged batch: a wrong corner rotation cannot hide behind a right id
# ------------------------------------------------------------------------------------------------------------------
def _pose_batch(name):
    """a3_detect_batch_pose on the first 16 found-quad frames of `name`, filter off -> (ctx, frames, markers, per, poses)"""
    det, ctx = _context(name, False)
    frames = np.ascontiguousarray(du.found_frames(name)[0][:16])
    ctx.set_debug_taps(True)
    markers, per, poses = ctx.detect_batch_pose(*_args(frames), 40.0, None, out_cap=128 * len(frames))
    assert len(markers) == int(per.sum()) == len(poses) >= 64
    return det, ctx, frames, markers, per, poses


def _pose_bits(error, rotation, translation):
    return np.concatenate([[error], np.asarray(rotation).ravel(), np.asarray(translation).ravel()]).astype(np.float32).tobytes()


@pytest.mark.parametrize("name", ("ARUCO", "APRILTAG_36H10"))
def test_poses_of_a_damaged_batch_belong_to_the_rotated_corners(name):
    """the corners a3_detect_batch_pose returns are numpy's (the candidate's, rotated left by the expected rotation, at rotations 1,
    2 and 3 under an inexact match among them), and each pose pair is bit-equal to a3_estimate_pose on those corners"""
    nb, _, codes = du.table(name)
    tau = du.tau_of(name)
    det, ctx, frames, markers, per, poses = _pose_batch(name)
    pos, rotations = 0, set()
    for f in range(len(frames)):
        _, _, tapped, dec = ctx.homographies(f, with_patches=False)
        want, _, exps = du.expected_of_candidates({"codes": tapped, "decode_ok": dec, "candidates": ctx.candidates(f)}, codes, tau, False)
        assert markers_of_hip(markers[pos: pos + int(per[f])]) == want, (name, f)
        rotations |= {(e.rotation, e.distance > 0) for e in exps if e.decode_ok}
        pos += int(per[f])
    assert rotations >= {(1, True), (2, True), (3, True)}
    h, w = frames.shape[1:3]
    alone = ctx.estimate_pose(np.stack([m["corners"] for m in markers]), 40.0, (w, h))
    for i in range(len(markers)):
        for k in range(2):
            r = alone[2 * i + k]
            assert poses[i, k].tobytes() == _pose_bits(r.error, r.rotation, r.translation), (name, i, k)


@pytest.mark.parametrize("name", ("ARUCO", "APRILTAG_36H10"))
def test_poses_of_a_damaged_batch_equal_the_oracles_solve(oracle, name):
    """each pose pair against the oracle's solve (src/pose.rs:52-81) on numpy's expected, rotated corners, bit for bit"""
    nb, _, codes = du.table(name)
    tau = du.tau_of(name)
    det, ctx, frames, markers, per, poses = _pose_batch(name)
    h, w = frames.shape[1:3]
    pos, worst, differ = 0, 0.0, 0
    for f in range(len(frames)):
        _, _, tapped, dec = ctx.homographies(f, with_patches=False)
        want, _, _ = du.expected_of_candidates({"codes": tapped, "decode_ok": dec, "candidates": ctx.candidates(f)}, codes, tau, False)
        assert len(want) == int(per[f])
        for j, m in enumerate(want):
            ref = oracle.solve_with_undistorted_points(np.array(m[2], dtype=np.uint32), 40.0, (w, h))
            for k in range(2):
                bits = _pose_bits(*ref[k])
                if poses[pos + j, k].tobytes() != bits:
                    differ += 1
                    with np.errstate(invalid="ignore"):
                        worst = max(worst, float(np.nanmax(np.abs(poses[pos + j, k].astype(np.float64) - np.frombuffer(bits, np.float32)))))
        pos += int(per[f])
    print(f"{name}: {differ} of {2 * len(markers)} poses differ from the oracle's in some bit, largest difference {worst:.3g}")
    assert differ == 0


def test_computed_tau_is_numpys():
    """ARTAG declares tau 0: k_calc_tau's value is numpy's minimum pairwise distance (0: the table holds one code twice), and the
    boundary patterns of that table were built from numpy's value, not from `ctx.tau`; the other two tables that declare 0 as well"""
    from aruco3_amd import _lib
    from aruco3_amd.dictionaries import ARDictionary

    det, ctx = _context("ARTAG", True)
    codes = du.table("ARTAG")[2]
    assert ctx.tau == du.numpy_tau(codes) == du.tau_of("ARTAG")
    assert [p for p in du.patterns("ARTAG") if "boundary_reject" in p.tags and p.expect.distance == du.numpy_tau(codes)]
    for other in ("ARTOOLKITPLUS", "ARTOOLKITPLUSBCH"):
        c = ARDictionary.new_from_named_dict(other).code_list
        assert _lib.calculate_tau(c) == du.numpy_tau(c), other
