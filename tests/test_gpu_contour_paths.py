"""The contour stage on every path it takes, border for border against the oracle (tests/contour_scenes.py's scenes).

Every case runs twice:
  * taps on: every border of every frame -- count, discovery order, start key + border type, point sequence -- equals
    oracle.find_contours (_compare_contours), and so do the per-frame candidates and the markers;
  * taps off (the product path, which prunes and on dense graphs finishes short borders early): a3_stats.candidates_pre /
    .candidates and the markers equal oracle.detect; .contours_traced equals the oracle's border count without 1-pixel specks;
    .contours_materialised equals the number of those borders the parity-safe bound of k_cycle_select keeps
    (n >= 5, n^2 >= 8 min_edge_length, n * epsilon < image diagonal + 1).
The contours_materialised check restates the implementation's bound (see _taps_off); the others compare with the oracle.
The driver-path cases (long borders, point-pool growth, history after decay, mixed and chunked batches) also assert the a3_stats
evidence of the path they target; the shape sweep, wide frames and fuzz assert only one chunk and the counts above.  GPU only.

`python tests/test_gpu_contour_paths.py <cases> <first_seed>` runs a longer seeded soak of the fuzz case."""
import sys
from pathlib import Path

import numpy as np
import pytest

if __name__ == "__main__":
    sys.path.insert(0, str(Path(__file__).resolve().parent.parent))

from tests import contour_scenes as S
from tests.test_gpu_shard_taps import _compare_contours, _detect_host, _detector, _isolated
from tests.util import marker_tuples

pytestmark = pytest.mark.gpu

EPS = 0.05          # DetectorConfig.contour_simplification_epsilon (default)


def _frames(h, w, names, seed):
    return np.stack([S.SCENES[n](h, w, seed + i) for i, n in enumerate(names)])


def _expected(oracle, d, frames):
    """per frame: oracle.detect, and (traced, kept) border counts of the product path"""
    n, h, w = frames.shape
    mel = S.min_edge_length(h, w)
    diag = float(np.sqrt(float(w) * w + float(h) * h))
    res, traced, kept = [], 0, 0
    for f in range(n):
        r = oracle.detect(frames[f], d.code_list, d.num_bits, d._tau)
        cs, _, _ = oracle.find_contours(r["thresholded"])
        for c in cs:
            if _isolated(r["thresholded"], c):
                continue
            ln = len(c)
            traced += 1
            kept += ln >= 5 and ln * ln >= 8 * mel and ln * EPS < diag + 1.0
        res.append(r)
    return res, traced, kept


def _markers_of(res):
    return [[(m["id"], m["code"], tuple(v for c in m["corners"] for v in c), m["hamming_distance"], m["rotation"]) for m in r["markers"]]
            for r in res]


def _hip_markers(m, per):
    out, k = [], 0
    for c in per.tolist():
        out.append([(int(x["id"]), int(x["code"]), tuple(int(v) for v in x["corners"]), int(x["hamming_distance"]), int(x["rotation"]))
                    for x in m[k:k + c]])
        k += c
    return out


def _taps_on(det, oracle, frames, res):
    """full border parity + candidates + markers; -> a3_stats of the tapped batch"""
    ctx, n_borders = _compare_contours(det, oracle, frames)
    st = ctx.stats()
    for f, r in enumerate(res):
        assert ctx.candidates(f, before_discard=True).tolist() == r["candidates_pre"].tolist(), f
        assert ctx.candidates(f).tolist() == r["candidates"].tolist(), f
    assert st["contours_traced"] == st["contours_materialised"] == n_borders, st          # taps: nothing is pruned
    assert st["chunks"] == 1, st
    return st


def _taps_off(det, frames, res, traced, kept):
    ctx, m, per = _detect_host(det, frames[..., None], taps=False)
    st = ctx.stats()
    assert _hip_markers(m, per) == _markers_of(res)
    assert st["candidates_pre"] == sum(len(r["candidates_pre"]) for r in res), st
    assert st["candidates"] == sum(len(r["candidates"]) for r in res), st
    assert st["markers"] == sum(len(r["markers"]) for r in res), st
    assert st["contours_traced"] == traced, (st, traced)
    # This one pins the IMPLEMENTATION, not the reference: `kept` restates k_cycle_select's parity-safe bound, so a change of that
    # bound fails here even when every output stays the same (a tighter bound that is still parity-safe must update _expected).
    assert st["contours_materialised"] == kept, (st, kept)
    return st, (marker_tuples(m), per.tolist())


def _case(det, oracle, frames, taps=(True, False)):
    """-> {taps: a3_stats}"""
    d = det.dictionary
    res, traced, kept = _expected(oracle, d, frames)
    out = {}
    for t in taps:
        out[t] = _taps_on(det, oracle, frames, res) if t else _taps_off(det, frames, res, traced, kept)[0]
    return out


# ------------------------------------------------------------------------------------------------------------------
# a. shapes that end mid-word, mid-tile, on a tile edge (a tile: 4 words x 64 rows = 256 x 64 px)
# ------------------------------------------------------------------------------------------------------------------
_ALL = ["serpentine", "spiral", "nested_rings", "checker1", "checker2", "checker3", "comb", "edges", "specks", "prune_bound",
        "blobs", "anomaly"]
_SHAPES = [(1, 1, _ALL), (2, 3, _ALL), (3, 2, _ALL), (16, 64, ["prune_bound", "specks", "checker2", "edges"]),
           (19, 48, ["prune_bound", "checker1", "blobs_dense"]), (63, 65, _ALL), (65, 63, _ALL), (64, 256, _ALL), (65, 257, _ALL),
           (127, 255, _ALL), (333, 251, _ALL), (480, 640, ["nested_rings", "checker2", "comb", "edges", "prune_bound", "blobs"]),
           (1080, 1920, ["comb", "edges", "prune_bound", "blobs_sparse"])]


@pytest.mark.parametrize("h,w,names", _SHAPES, ids=[f"{h}x{w}" for h, w, _ in _SHAPES])
def test_shape_sweep(dicts, oracle, h, w, names):
    """structured scenes in one batch per shape.  Evidence: one chunk; the darts were built (a3_stats.darts > 0 unless the frames
    are too small to hold a border); the product path kept no more borders than it traced."""
    det = _detector(dicts, "ARUCO_DEFAULT")
    frames = _frames(h, w, names, 11 * h + w)
    st = _case(det, oracle, frames)
    assert st[False]["chunks"] == 1 and st[False]["contours_materialised"] <= st[False]["contours_traced"]
    assert (st[True]["darts"] > 0) == (st[True]["contours_traced"] > 0), st


# ------------------------------------------------------------------------------------------------------------------
# b. borders of 150 k and 1 M points
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,least", [(480, 640, 150_000), (1080, 1920, 1_000_000)])
def test_long_borders(dicts, oracle, h, w, least):
    """serpentine and spiral: taps on, every point equals the oracle's.  Product path: the long borders fail the diagonal bound
    (n * epsilon >= diagonal + 1) and are pruned -- contours_materialised says so -- and nothing else changes."""
    det = _detector(dicts, "ARUCO_DEFAULT")
    frames = _frames(h, w, ["serpentine", "spiral"], 3)
    st = _case(det, oracle, frames)
    diag = float(np.hypot(w, h))
    assert st[False]["contours_traced"] == 2 and st[False]["contours_materialised"] == 0          # both pruned ...
    assert least * EPS >= diag + 1.0                                                                # ... by the diagonal bound
    assert st[True]["contours_materialised"] == 2, st


@pytest.mark.parametrize("h,w,least", [(480, 640, 150_000), (1080, 1920, 1_000_000)])
def test_point_pool_growth_rerun(dicts, oracle, h, w, least):
    """kErrPointPool: a context whose point pool (a3_set_pool_limits) is a tenth of the serpentine's border.  The pool must grow
    (a3_stats reruns one more than on a fresh context with the default pool) and every point must equal the oracle's.  Regression:
    k_contour_quads used to read the records of the borders that had not fit, which k_cycle_select never writes."""
    frames = _frames(h, w, ["serpentine", "spiral"], 3)
    ctx, n = _compare_contours(_detector(dicts, "ARUCO_DEFAULT"), oracle, frames)
    st = ctx.stats()
    small = _detector(dicts, "ARUCO_DEFAULT")
    small._context().set_pool_limits(max_points=least // 10)
    ctx, n2 = _compare_contours(small, oracle, frames)
    s2 = ctx.stats()
    assert n == n2 == 2 and s2["reruns"] >= st["reruns"] + 1, (st, s2)     # (both contexts fresh: the same re-runs besides the pool's)
    _, pts = ctx.contours(0)
    assert len(pts[0]) >= least


# ------------------------------------------------------------------------------------------------------------------
# c. hints that decayed over many clean batches, then every kind of batch
# ------------------------------------------------------------------------------------------------------------------
# What the driver (a3_api.hip, finish_batch) re-runs a batch for, in the order it checks, and what a3_stats shows of each:
#   plan      the device plan (a batch shaped like the last one) is sized by the last batch's darts, plan_darts * 5/4 + 65536: a
#             graph that outgrows it is planned on the host and re-run.  Predicted from a3_stats.darts of both batches.
#   overflow  a frame has more than 2048 entries for k_entry_frame's LDS: re-run on the global doubling rounds, with
#             entry_global_ttl = 64 and jump_rounds_hint raised to 12.  k_entry_frame reports no rounds, k_entry_jump does: on a
#             context whose entry_global_ttl had decayed, jump_rounds > 0 means the batch overflowed.
#   short     the last global round still moved something (jump_changed[rounds - 1]): re-run with 32 rounds.  After an overflow the
#             launch had min(12, log2 darts + 2) = 12 rounds at these sizes, so jump_rounds >= 12 means it was short.
#   resolve   a natural start did not fire and the fixpoint passes were not in the launch (resolve_full_ttl had decayed): re-run with
#             them, resolve_full_ttl = 64.  resolve_iterations >= 1.
# Point-pool and table growth cannot happen here (default pools, a few hundred thousand points).
_DECAY = 66   # > 64: entry_global_ttl and resolve_full_ttl have reached 0, jump_rounds_hint its floor of 4


def _decayed(dicts, taps):
    """a fresh context after _DECAY clean 640 x 480 batches -> (det, clean frame, a3_stats of the last clean batch).  The clean
    batches ran k_entry_frame (jump_rounds 0) without a fixpoint pass or a re-run."""
    from aruco3_amd import synth
    from oracle import a3oracle

    det = _detector(dicts, "ARUCO_DEFAULT")
    rgb, _ = synth.config_frames(1, 1)
    clean = a3oracle.to_luma8(rgb[0])[None]
    for _ in range(_DECAY):
        ctx, _, _ = _detect_host(det, clean[..., None], taps=taps)
    st = ctx.stats()
    assert (st["reruns"], st["jump_rounds"], st["resolve_iterations"], st["chunks"]) == (0, 0, 0, 1), st
    return det, clean, st


def _causes(st, prev, decayed_entry, decayed_resolve):
    """the re-run causes a3_stats shows for one batch after `prev` (same shape, one chunk) -> dict of bools"""
    return {"plan": st["darts"] > prev["darts"] + prev["darts"] // 4 + 65536,
            "overflow": decayed_entry and st["jump_rounds"] > 0,
            "short": st["jump_rounds"] >= 12,
            "resolve": decayed_resolve and st["resolve_iterations"] >= 1}


def _step(det, oracle, frames, taps, prev, decayed_entry, decayed_resolve):
    st = _case(det, oracle, frames, taps=(taps,))[taps]
    c = _causes(st, prev, decayed_entry, decayed_resolve)
    assert st["reruns"] == sum(c.values()), (st, c)          # every re-run accounted for by its cause
    assert st["resolve_iterations"] <= 4, st                  # (the default four passes converged: no kErrResolve re-run)
    return st, c


@pytest.mark.parametrize("taps", [True, False], ids=["taps_on", "taps_off"])
def test_history_after_decay(dicts, oracle, taps):
    """Each step that needs a decayed context gets a fresh one (_decayed).  Evidence per step (see _causes):
      1. serpentine: overflow AND short launch -- entries beyond k_entry_frame's LDS, then more than the 12 global rounds the
         overflow re-run gave it; no fixpoint pass;
      2. clean, same context: no re-run, and jump_rounds > 0: the overflow of step 1 keeps the context on the global rounds;
      3. noise, fresh context: overflow only (its global rounds fit 12); the clean batch after it runs on the global rounds too;
      4. column-0 anomaly, fresh context: its natural start does not fire, the fixpoint passes had decayed out of the launch: a
         re-run for them (plus an overflow if its entries outgrow LDS, which the accounting allows); then the same frame again
         needs no re-run, the passes now being in the launch (resolve_iterations the same);
      5. clean after it: no re-run, no fixpoint pass needed, the same borders and markers as before the history."""
    h, w = 480, 640
    # 1, 2
    det, clean, st0 = _decayed(dicts, taps)
    st1, c1 = _step(det, oracle, S.serpentine(h, w, 0)[None], taps, st0, True, True)
    assert c1["overflow"] and c1["short"] and not c1["resolve"], (st1, c1)
    st2, c2 = _step(det, oracle, clean, taps, st1, False, False)
    assert st2["reruns"] == 0 and st2["jump_rounds"] > 0 and st2["resolve_iterations"] == 0, st2
    # 3
    det, clean, st0 = _decayed(dicts, taps)
    st3, c3 = _step(det, oracle, S.noise(h, w, 7)[None], taps, st0, True, True)
    assert c3["overflow"] and not c3["short"] and not c3["resolve"], (st3, c3)
    st, _ = _step(det, oracle, clean, taps, st3, False, False)
    assert st["reruns"] == 0 and st["jump_rounds"] > 0, st
    # 4, 5
    det, clean, st0 = _decayed(dicts, taps)
    anomaly = S.anomaly(h, w, 0)[None]
    st4, c4 = _step(det, oracle, anomaly, taps, st0, True, True)
    assert c4["resolve"] and not c4["short"], (st4, c4)
    again, _ = _step(det, oracle, anomaly, taps, st4, False, False)
    assert again["reruns"] == 0 and again["resolve_iterations"] == st4["resolve_iterations"], (st4, again)
    st5, _ = _step(det, oracle, clean, taps, again, False, False)
    assert st5["reruns"] == 0 and st5["resolve_iterations"] == 0, st5


# ------------------------------------------------------------------------------------------------------------------
# d. one batch of mixed frame kinds, whole and chunked
# ------------------------------------------------------------------------------------------------------------------
_MIX = ["clean", "serpentine", "noise", "blank", "anomaly", "specks"]


def _mixed(h, w):
    from aruco3_amd import synth
    from oracle import a3oracle

    rgb, _ = synth.config_frames(1, 1)
    out = [a3oracle.to_luma8(rgb[0]) if n == "clean" else S.SCENES[n](h, w, 5) for n in _MIX]
    return np.stack(out)


def test_mixed_batch_whole_and_chunked(dicts, oracle):
    """[clean markers, serpentine, noise, blank, anomaly, specks] at 480 x 640 in one batch: the noise frame's entries overflow
    k_entry_frame's LDS, so the whole batch goes the global way (reruns >= 1, jump_rounds > 0); full parity.  Then on a context
    whose a3_set_pool_limits max_darts is the largest frame's dart count: a3_stats chunks >= 3, a chunk boundary next to the
    serpentine (predicted from the per-frame dart counts with the library's greedy split), and the same candidates and markers as
    the single-chunk run and the oracle."""
    det = _detector(dicts, "ARUCO_DEFAULT")
    frames = _mixed(480, 640)
    st = _case(det, oracle, frames)
    assert st[True]["reruns"] >= 1 and st[True]["jump_rounds"] > 0, st
    # per-frame dart counts, one frame per batch
    fd = []
    for f in range(len(frames)):
        c, _, _ = _detect_host(_detector(dicts, "ARUCO_DEFAULT"), frames[f:f + 1, ..., None], taps=False)
        fd.append(c.stats()["darts"])
    limit = max(fd)
    split, cur, acc = [], [], 0
    for f, v in enumerate(fd):
        if cur and acc + v > limit:
            split.append(cur); cur, acc = [], 0
        cur.append(f); acc += v
    split.append(cur)
    serp = _MIX.index("serpentine")
    assert len(split) >= 3 and any(serp in (c[0], c[-1]) for c in split), (fd, split)
    res, traced, kept = _expected(oracle, det.dictionary, frames)
    whole = _taps_off(det, frames, res, traced, kept)[1]
    for taps in (False, True):
        chunked = _detector(dicts, "ARUCO_DEFAULT")
        cctx = chunked._context()
        cctx.set_pool_limits(max_darts=limit)
        cctx, m, per = _detect_host(chunked, frames[..., None], taps=taps)
        s = cctx.stats()
        assert s["chunks"] == len(split), (s, split)
        assert (marker_tuples(m), per.tolist()) == whole
        assert s["candidates_pre"] == sum(len(r["candidates_pre"]) for r in res) and s["candidates"] == sum(len(r["candidates"]) for r in res)
        if taps:
            for f, r in enumerate(res):
                assert cctx.candidates(f, before_discard=True).tolist() == r["candidates_pre"].tolist(), f
        else:
            assert s["contours_traced"] == traced and s["contours_materialised"] == kept, (s, traced, kept)


# ------------------------------------------------------------------------------------------------------------------
# e. frames wider or taller than 16 384 (no 14-bit coordinates)
# ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w", [(96, 16448), (16448, 96)])
def test_wide_frames(dicts, oracle, h, w):
    """full border parity past 16 384; evidence: the frame is wider or taller than 16 384 (by construction), and the oracle has
    candidates beyond that coordinate, which the product path must deliver too"""
    det = _detector(dicts, "ARUCO_DEFAULT")
    frames = _frames(h, w, ["prune_bound", "comb", "edges", "blobs_sparse"], 1)
    res, _, _ = _expected(oracle, det.dictionary, frames)
    far = [q for r in res for q in r["candidates_pre"].tolist() if max(max(p) for p in q) >= 16384]
    assert far
    st = _case(det, oracle, frames)
    assert st[False]["candidates_pre"] > len(far) // 2


# ------------------------------------------------------------------------------------------------------------------
# f. seeded fuzz: scene, shape and batch composition
# ------------------------------------------------------------------------------------------------------------------
def _fuzz_one(dicts, oracle, seed):
    rng = np.random.default_rng(seed)
    h = int(rng.choice([1, 2, 5, 17, 63, 64, 65, 100, 127, 128, 129, 200, 257]))
    w = int(rng.choice([1, 3, 6, 31, 65, 100, 255, 256, 257, 300, 513]))
    names = list(rng.choice(sorted(S.SCENES), size=int(rng.integers(1, 6))))
    frames = _frames(h, w, names, int(rng.integers(0, 1 << 20)))
    st = _case(_detector(dicts, "ARUCO_DEFAULT"), oracle, frames)
    return (h, w, names, st[False]["reruns"], st[True]["contours_traced"])


@pytest.mark.parametrize("seed", [1, 2, 3, 4, 5, 6, 7, 8])
def test_seeded_fuzz(dicts, oracle, seed):
    _fuzz_one(dicts, oracle, seed)


if __name__ == "__main__":
    from aruco3_amd.dictionaries import ARDictionary
    from oracle import a3oracle

    cases = int(sys.argv[1]) if len(sys.argv) > 1 else 100
    first = int(sys.argv[2]) if len(sys.argv) > 2 else 1000
    a3oracle.build()
    for s in range(first, first + cases):
        print(s, _fuzz_one(ARDictionary, a3oracle, s), flush=True)
    print(f"soak ok: {cases} seeds from {first}")
