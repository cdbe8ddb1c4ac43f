"""Inverted (bright-on-dark) markers, a3_set_marker_polarity's A3_POLARITY_BOTH: the rule in plain numpy, frames that carry inverted
markers, and the expectation of a whole frame.  Shared by tests/test_inverted_expectation.py (CPU) and tests/test_gpu_inverted.py.

The rule is written from include/aruco3_hip.h, on the n x n bit matrix as it stands after resize and `> 127`:
  * no perimeter cell lit (this test first): tests/damage_util.py's expect_view, decode_ok 1;
  * every perimeter cell lit: every cell complemented, then the same four codes, lookup, rotation choice and filter; decode_ok 2;
  * anything else: no codes, decode_ok 0.

Frames.  `complemented` is 255 - frame: every marker of the frame is inverted, and so is its quiet zone and the background.  `mixed`
complements the quiet-zone rectangle of some slots of a damage_util drawing and leaves the others: dark and inverted markers side by
side, no marker cut (a slot's rectangle holds the whole marker and its quiet zone, and the rectangles of two slots never touch).

The expectation of a frame takes the oracle's candidates and warped patches (the stages ahead of the bit matrix do not change) and
applies otsu_level, the binary threshold, resize_triangle and `> 127` to each patch with the oracle's own functions, then the rule."""
import numpy as np

from tests import damage_util as du

DICTS = ("ARUCO", "APRILTAG_16H5", "ARUCO_MIP_36H12", "CHILITAGS")
SEPARATION = 0.02     # min_corner_separation_factor: a marker's square and its quiet zone's are two quads a quiet zone's width apart
MIN_SIDE = 0.02       # min_side_length_factor


def expect_view_both(view, codes):
    """what the decode stage in mode BOTH must make of the n x n cell matrix `view` -> (Expect, inverted)"""
    view = (np.asarray(view) != 0).astype(np.uint8)
    rim = np.concatenate([view[0], view[-1], view[:, 0], view[:, -1]])
    if not rim.any():
        return du.expect_view(view, codes), False
    if rim.all():
        e = du.expect_codes(du.rotated_codes((1 - view)[1:-1, 1:-1]), codes)
        e.decode_ok = 2
        return e, True
    return du.Expect(0, [0, 0, 0, 0]), False


def expect_view_dark(view, codes):
    """mode DARK on the same matrix -> (Expect, False)"""
    return du.expect_view((np.asarray(view) != 0).astype(np.uint8), codes), False


def complemented(frames):
    return (255 - np.asarray(frames, dtype=np.uint8)).astype(np.uint8)


def slot_rects(count, num_bits, family="b"):
    """the quiet-zone rectangle (x0, y0, x1, y1) of each of the first `count` slots of du.draw_frame's grid"""
    cell, cols, rows = du.geometry(num_bits, family)
    side = (du.side_cells(num_bits) + 2) * cell
    out = []
    for s in range(count):
        cx, cy = (s % cols * 2 + 1) * du.W // (2 * cols), (s // cols * 2 + 1) * du.H // (2 * rows)
        x0, y0 = cx - side // 2, cy - side // 2
        out.append((x0 - du.QUIET, y0 - du.QUIET, x0 + side + du.QUIET, y0 + side + du.QUIET))
    return out


def mixed(frame, count, num_bits, seed, family="b"):
    """-> (frame with the rectangles of a seeded half of its `count` slots complemented, which slots): at least one of each kind
    when the frame holds two or more"""
    rng = np.random.default_rng(seed)
    inv = rng.random(count) < 0.5
    if count >= 2:
        inv[0], inv[1] = True, False
    out = np.array(frame, dtype=np.uint8, copy=True)
    for on, (x0, y0, x1, y1) in zip(inv.tolist(), slot_rects(count, num_bits, family)):
        if on:
            out[y0:y1, x0:x1] = 255 - out[y0:y1, x0:x1]
    return out, inv


def oracle_config(oracle, filt, num_bits):
    cfg = oracle.Config.default()
    cfg.homography_sample_size = du.sample_size(num_bits)
    cfg.min_side_length_factor = MIN_SIDE
    cfg.min_corner_separation_factor = SEPARATION
    cfg.filter_high_bit_errors = int(filt)
    return cfg


def detector_config(filt, num_bits):
    from aruco3_amd.aruco import DetectorConfig

    return DetectorConfig(min_side_length_factor=MIN_SIDE, min_corner_separation_factor=SEPARATION,
                          homography_sample_size=du.sample_size(num_bits), filter_high_bit_errors=bool(filt))


def bits_of_patch(oracle, patch, ok, n):
    """the n x n bit matrix of one candidate: otsu_level, threshold(Binary), resize(Triangle), `> 127`; a failed projection is the
    reference's 1 x 1 black patch (quirk Q4)"""
    p = np.asarray(patch, dtype=np.uint8) if ok else np.zeros((1, 1), np.uint8)
    level = oracle.otsu_level(p)
    binary = np.where(p > level, 255, 0).astype(np.uint8)
    return (oracle.resize_triangle(binary, n, n) > 127).astype(np.uint8)


def expect_frame(oracle, ref, codes, num_bits, tau, filt, both=True):
    """`ref`: oracle.detect of the frame -> (marker tuples as tests.util.markers_of_* give them, their candidate indices, their
    inverted flags, (Expect, inverted) per candidate)"""
    n = du.side_cells(num_bits) + 2
    rule = expect_view_both if both else expect_view_dark
    markers, idx, flags, per = [], [], [], []
    for k, (patch, ok, quad) in enumerate(zip(ref["homographies"], ref["homography_ok"], ref["candidates"])):
        e, inv = rule(bits_of_patch(oracle, patch, bool(ok), n), codes)
        per.append((e, inv))
        m = du.expected_marker(e, quad, tau, filt)
        if m is not None:
            markers.append(m)
            idx.append(k)
            flags.append(int(inv))
    return markers, idx, flags, per


# ---- a board scene with inverted markers, for the board-aided recovery ---------------------------------------------------------------
RECOVER_DISTANCE_PX = 16.0   # see board_scene


def board_scene():
    """tests/recover_scene.py's three frames with the quiet-zone rectangle of every drawn marker complemented and the board left
    bright: bright-on-dark markers, each in a dark rectangle QUIET px wider than the marker.  (On a wholly dark ground the adaptive
    threshold's halo round a bright marker is a second quad per marker, the same id is then seen twice in a frame, and the recovery
    contract excludes such ids from the board fit.)  At the default min_corner_separation_factor the rectangle's quad, the longer
    perimeter, survives discard_too_near in the marker's place and reads the marker's code at a distance of 1 or 2; its corners lie
    QUIET px outside the board's in x and y, so the recovery runs with max_distance_px RECOVER_DISTANCE_PX (QUIET * sqrt 2 = 11.3
    is more than the default 10).  Frame 1's marker damaged by tau cells is refused by the filter and placed by the board."""
    from tests import recover_scene as rs

    b = rs.board()
    frames = rs.frames().copy()
    spots = rs.place(b)
    for f, slots in enumerate((range(len(b)), range(len(b)), (0,))):
        for s in slots:
            x0, y0 = spots[s]
            r = frames[f, y0 - du.QUIET: y0 + rs.SIDE + du.QUIET, x0 - du.QUIET: x0 + rs.SIDE + du.QUIET]
            r[...] = 255 - r
    return b, np.ascontiguousarray(frames)


def expected_recovery(oracle, imgs, b, dictionary, config, min_markers, max_distance_px, max_hamming):
    """tests/recover_scene.py's `expected` with the rule of this file in the decoder's place: the contract's merged list of a batch in
    mode BOTH -> (marker tuples as tests.util.marker_tuples makes them, per-frame counts, recovered per frame, flags, decode_ok of each
    marker's candidate)"""
    from tests import recover_oracle

    codes, nb, tau = dictionary.code_list, dictionary.num_bits, dictionary._tau
    merged, per, rec, flags, decs = [], [], [], [], []
    for f, img in enumerate(imgs):
        ref = oracle.detect(img, codes, nb, tau, config=config)
        markers, idx, fl, cands = expect_frame(oracle, ref, codes, nb, tau, bool(config.filter_high_bit_errors))
        rejected = np.array([c for c in range(len(ref["candidates"])) if c not in idx], np.int64)
        codes4 = np.array([[int(c) for c in e.codes] for e, _ in cands], np.uint64).reshape(-1, 4)
        has = np.array([int(bool(ok) and e.decode_ok != 0) for (e, _), ok in zip(cands, ref["homography_ok"])], np.uint8)
        got = recover_oracle.recover_markers(b, codes, [m[0] for m in markers], [m[2] for m in markers], ref["candidates"][rejected],
                                             codes4[rejected], has[rejected], min_markers, max_distance_px, max_hamming, frame=f)
        for m, k, x in zip(markers, idx, fl):
            merged.append((f, m[0], m[1], tuple(v for xy in m[2] for v in xy), m[3], m[4], k))
            flags.append(x)
            decs.append(cands[k][0].decode_ok)
        for m in got:
            k = int(rejected[int(m["candidate_index"])])
            merged.append((f, int(m["id"]), int(m["code"]), tuple(int(v) for v in m["corners"]), int(m["hamming_distance"]), int(m["rotation"]), k))
            flags.append(int(cands[k][0].decode_ok == 2))
            decs.append(cands[k][0].decode_ok)
        per.append(len(markers) + len(got))
        rec.append(len(got))
    return merged, per, rec, flags, decs
