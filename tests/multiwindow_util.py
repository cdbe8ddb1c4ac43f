"""Detection with several threshold windows (a3_set_threshold_windows): the merged discard restated and the expectations the tests
share -- tests/test_multiwindow.py (CPU: the inputs exercise the merge) and tests/test_gpu_multiwindow.py (GPU: the library equals them).

`merged_model` is step 3 of the definition in include/aruco3_hip.h written in numpy float32 from that text and from
src/aruco.rs:187-232 -- not from the kernel: the reference's walk over the concatenated list, where a pair from different windows takes
the smallest of the four distances between quad i and quad j rotated left by r.  Beside the survivors it returns a census of what the
walk did with pairs the plain discard would have treated differently."""
import numpy as np

F32 = np.float32
WINDOWS = (3, 7, 15)
FACTORS = (0.1, 0.005)


def _sum4_sqrt(d):
    """((s0+s1)+s2)+s3 of sqrt(dx*dx+dy*dy) over the four (dx, dy) pairs of the last axis, every operation rounded to float32"""
    s = np.sqrt(d[..., 0::2] * d[..., 0::2] + d[..., 1::2] * d[..., 1::2])
    return ((s[..., 0] + s[..., 1]) + s[..., 2]) + s[..., 3]


def perimeters(x):
    return _sum4_sqrt(x - np.roll(x.reshape(-1, 4, 2), -1, axis=1).reshape(-1, 8))


def min_distance_of(w, h, factor):
    """min(W, H) * min_corner_separation_factor as the detector forms it (src/aruco.rs:56): one float32 product"""
    return F32(min(w, h)) * F32(factor)


def merged_model(lists, min_distance):
    """lists: per window, that plane's candidates (n_k, 4, 2) in the reference's order.  -> (concat (n, 4, 2) uint32, window (n,),
    kept: the surviving indices into concat, census)"""
    lists = [np.asarray(q, dtype=np.uint32).reshape(-1, 4, 2) for q in lists]
    concat = np.concatenate(lists) if lists else np.zeros((0, 4, 2), np.uint32)
    win = np.concatenate([np.full(len(q), k, dtype=np.int64) for k, q in enumerate(lists)]) if lists else np.zeros(0, np.int64)
    n = len(concat)
    census = dict(rotation_only_kills=0, cross_equal_perimeter_pairs=0, cross_kills=0, i_dies=0)
    if n == 0:
        return concat, win, np.zeros(0, np.int64), census
    x = concat.reshape(n, 8).astype(F32)
    rot = [np.roll(x.reshape(n, 4, 2), -r, axis=1).reshape(n, 8) for r in range(4)]   # corner p of rot[r][j] = corner (p + r) % 4 of j
    per = perimeters(x)
    md = F32(min_distance)
    dead = np.zeros(n, dtype=bool)
    for i in range(n - 1):
        if dead[i]:
            continue
        cross = win[i + 1:] != win[i]
        d0 = _sum4_sqrt(x[i] - rot[0][i + 1:])
        dist = d0.copy()
        for r in (1, 2, 3):
            dr = _sum4_sqrt(x[i] - rot[r][i + 1:])
            take = cross & (dr < dist)
            dist[take] = dr[take]
        close = (dist / F32(4)) < md
        plain_close = (d0 / F32(4)) < md
        for j in i + 1 + np.nonzero(close)[0]:                 # j ascending; dead ones skipped
            if dead[j]:
                continue
            c = bool(cross[j - i - 1])
            census["cross_equal_perimeter_pairs"] += c and per[i] == per[j]
            census["rotation_only_kills"] += not plain_close[j - i - 1]
            census["cross_kills"] += c
            if per[i] >= per[j]:
                dead[j] = True
            else:
                dead[i] = True
                census["i_dies"] += 1
                break                                          # the rest of i's row is a no-op
    census = {k: int(v) for k, v in census.items()}
    return concat, win, np.nonzero(~dead)[0], census


def oracle_config(oracle, window, factor=0.1, min_side=None):
    cfg = oracle.Config.default()
    cfg.threshold_window = int(window)
    cfg.min_corner_separation_factor = float(factor)
    if min_side is not None:
        cfg.min_side_length_factor = float(min_side)
    return cfg


def expect_frame(oracle, d, img, windows, factor=0.1, min_side=None):
    """one frame under `windows`: dict(planes: the oracle's run per window (thresholded, candidates_pre ...), pre: the concatenated
    list, win, kept, fin: the survivors, census, final: the oracle's decode of the survivors, handed over as its candidate list)"""
    h, w = img.shape[:2]
    planes = [oracle.detect(img, d.code_list, d.num_bits, d.tau, config=oracle_config(oracle, wk, factor, min_side)) for wk in windows]
    pre, win, kept, census = merged_model([p["candidates_pre"] for p in planes], min_distance_of(w, h, factor))
    fin = pre[kept]
    final = oracle.detect(img, d.code_list, d.num_bits, d.tau, config=oracle_config(oracle, windows[0], factor, min_side), quads=fin) if len(fin) else None
    return dict(planes=planes, pre=pre, win=win, kept=kept, fin=fin, census=census, final=final)


_cache = {}


def expectation(oracle, d, frames, windows=WINDOWS, factor=0.1, key=None, min_side=None):
    """expect_frame for every frame of `frames`; with `key` the result is computed once and shared (callers must not modify it)"""
    k = None if key is None else (key, tuple(windows), float(factor), min_side)
    if k is not None and k in _cache:
        return _cache[k]
    out = [expect_frame(oracle, d, img, windows, factor, min_side) for img in frames]
    if k is not None:
        _cache[k] = out
    return out


def expected_markers(exp):
    """(frame, id, code, corners[8], hamming distance, rotation, candidate_index) of every marker of an expectation, in the library's
    order: frame by frame, candidate order within a frame"""
    out = []
    for f, e in enumerate(exp):
        if e["final"] is None:
            continue
        for m in e["final"]["markers"]:
            out.append((f, m["id"], m["code"], tuple(int(v) for xy in m["corners"] for v in xy), m["hamming_distance"], m["rotation"],
                        m["candidate_index"]))
    return out


def config1_frames(n=3, crop=None):
    """BASELINE config 1's first n frames (640 x 480 RGB); crop = (w, h): their top-left corner, as a contiguous batch"""
    from aruco3_amd import synth

    frames, _ = synth.config_frames(1, n)
    frames = np.ascontiguousarray(frames)
    if crop is not None:
        frames = np.ascontiguousarray(frames[:, :crop[1], :crop[0]])
    return frames


def squares_frame(w, h, boxes, background=200, ink=30):
    """a flat grey field with filled axis-aligned rectangles (x0, y0, x1, y1), x1 / y1 exclusive: L8"""
    img = np.full((h, w), background, dtype=np.uint8)
    for x0, y0, x1, y1 in boxes:
        img[y0:y1, x0:x1] = ink
    return img


def grid_boxes(nx, ny, side, pitch, x0=8, y0=8):
    return [(x0 + pitch * i, y0 + pitch * j, x0 + pitch * i + side, y0 + pitch * j + side) for j in range(ny) for i in range(nx)]
