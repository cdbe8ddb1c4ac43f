"""Inputs and a second reference for k_frame_candidates (candidate order by start key, discard_too_near, compaction, work list,
projections), shared by tests/test_candidate_cases.py (CPU: the inputs reach what they are for) and
tests/test_gpu_frame_candidates.py (GPU: the kernel equals the oracle on them).

`model` is discard_too_near written from src/aruco.rs:187-232 in numpy float32 -- not from the kernel and not from the oracle -- and
returns, beside the survivors, a census of what the walk did: which of its order-dependent branches an input reaches.

A launch is one call of the kernel: a table size (`max_cand`, which picks the kernel's form), a `min_distance`, a sample size S and
a list of frames.  A frame's quads are built in the order the walk is to see them; `frame()` gives them random unique u32 keys
(0 and 2^32-1 among them) that sort into that order and shuffles the records, so the rank sort is never the identity."""
from dataclasses import dataclass, field
from functools import lru_cache

import numpy as np

LDS_SLOTS = 6144                      # k_decode.hip, kFrameCandLds: tables above it take the through-memory form
TABLES = (1024, 6144, 6145, 12288)
COUNTS = (0, 1, 2, 3, 63, 64, 65, 66, 127, 128, 129, 1024)      # and max_cand, max_cand + 1, per table
CLUSTER_COUNTS = {1024: (40, 64, 65, 300), 6144: (1500, 6144), 6145: (), 12288: (7000, 12288)}
F32 = np.float32
TINY = float(np.nextafter(F32(0), F32(1)))                     # the smallest positive float32
MIN_DISTANCES = (0.0, TINY,
                 float(np.nextafter(F32(5), F32(0))), 5.0, float(np.nextafter(F32(5), F32(9))),
                 float(np.nextafter(F32(10), F32(0))), 10.0, float(np.nextafter(F32(10), F32(99))),
                 25.0, 1e9)
CENSUS_KEYS = ("i_dies", "i_dies_gap64", "i_dies_gap128", "kills_then_dies", "survivor_behind_bigger", "dead_j_skipped",
               "dead_j_skipped_bigger", "ties", "knife_pairs")
CAND_DTYPE = np.dtype([("start_key", "<u4"), ("xy", "<u2", (8,))])


# ----------------------------------------------------------------------------------------------------------------------
# the second reference
# ----------------------------------------------------------------------------------------------------------------------
def _sum4_sqrt(d):
    """((s0+s1)+s2)+s3 of sqrt(dx*dx+dy*dy) over the four (dx, dy) pairs of the last axis, every operation rounded to float32"""
    s = np.sqrt(d[..., 0::2] * d[..., 0::2] + d[..., 1::2] * d[..., 1::2])
    return ((s[..., 0] + s[..., 1]) + s[..., 2]) + s[..., 3]


def perimeters(x):
    return _sum4_sqrt(x - np.roll(x.reshape(-1, 4, 2), -1, axis=1).reshape(-1, 8))


def model(quads, keys, min_distance):
    """quads (n, 4, 2), keys (n): stable sort by key, then discard_too_near as src/aruco.rs:187-232 walks it.
    Returns (order, kept, census): the sort permutation, the surviving indices INTO THE SORTED list, and the census."""
    q = np.asarray(quads).reshape(-1, 8)
    order = np.argsort(np.asarray(keys, dtype=np.uint32), kind="stable")
    x = q[order].astype(F32)
    n = x.shape[0]
    md = F32(min_distance)
    census = dict.fromkeys(CENSUS_KEYS, 0)
    if n == 0:
        return order, np.zeros(0, dtype=np.int64), census
    per = perimeters(x)
    dead = np.zeros(n, dtype=bool)
    for i in range(n - 1):
        if dead[i]:
            continue
        mean = _sum4_sqrt(x[i] - x[i + 1:]) / F32(4)
        close = mean < md
        js = i + 1 + np.nonzero(close)[0]                     # close pairs of this row, j ascending
        alive = ~dead[js]
        bigger = alive & (per[js] > per[i])                  # a live close j with perimeter_i >= perimeter_j false: i dies there
        stop = int(np.argmax(bigger)) if bigger.any() else len(js)     # from js[stop] on, i is dead and the row a no-op
        head, head_alive = js[:stop], alive[:stop]
        last = int(js[stop]) if stop < len(js) else n                 # the pairs row i compares: live j up to the one that kills i
        census["knife_pairs"] += int(np.count_nonzero((mean == md) & ~dead[i + 1:] & (np.arange(i + 1, n) <= last)))
        census["dead_j_skipped"] += int(np.count_nonzero(~head_alive))
        census["dead_j_skipped_bigger"] += int(np.count_nonzero(~head_alive & (per[head] > per[i])))
        killed = head[head_alive]
        census["ties"] += int(np.count_nonzero(per[killed] == per[i]))
        dead[killed] = True
        if stop < len(js):
            first = int(js[stop])
            dead[i] = True
            census["i_dies"] += 1
            census["i_dies_gap64"] += first - i - 1 >= 64
            census["i_dies_gap128"] += first - i - 1 >= 128
            census["kills_then_dies"] += len(killed) > 0
            census["survivor_behind_bigger"] += bool(alive[stop + 1:].any())
    census = {k: int(v) for k, v in census.items()}
    return order, np.nonzero(~dead)[0], census


# ----------------------------------------------------------------------------------------------------------------------
# frames and launches
# ----------------------------------------------------------------------------------------------------------------------
@dataclass
class Frame:
    name: str
    count: int                      # cand_count[f]; above the table: an overflowed frame (records past the table are not supplied)
    records: np.ndarray             # CAND_DTYPE, min(count, max_cand), in table order


@dataclass
class Launch:
    name: str
    max_cand: int
    min_distance: float
    S: int
    frames: list = field(default_factory=list)

    def form_of(self, fr):
        """which of the kernel's three walks a frame takes (None: no walk -- fewer than two quads, or overflowed)"""
        if fr.count > self.max_cand or fr.count < 2:
            return None
        return "reg" if fr.count <= 64 else ("lds" if self.max_cand <= LDS_SLOTS else "big")


def unique_keys(n, rng):
    """n unique u32 keys, ascending, 0 and 2^32-1 among them when there is room"""
    keys = set()
    if n >= 1:
        keys.add(0 if rng.integers(0, 2) or n >= 2 else 0xFFFFFFFF)
    if n >= 2:
        keys.add(0xFFFFFFFF)
    while len(keys) < n:
        keys.update(int(k) for k in rng.integers(0, 1 << 32, size=n - len(keys), dtype=np.uint64))
    keys = np.array(sorted(keys), dtype=np.uint32)
    assert len(keys) == n and (n < 2 or not np.array_equal(keys, np.arange(n)))
    return keys


def frame(name, quads, rng, max_cand, count=None):
    """quads in the order the walk is to see them -> shuffled records with keys that sort back into it.  count > len(quads)
    declares an overflowed frame: the table is full (len(quads) == max_cand) and the rest was never stored."""
    q = np.asarray(quads, dtype=np.int64).reshape(-1, 8)
    assert q.size == 0 or (q.min() >= 0 and q.max() <= 65535)
    n = q.shape[0]
    assert n <= max_cand and (count is None or (count > max_cand and n == max_cand))
    rec = np.zeros(n, dtype=CAND_DTYPE)
    rec["start_key"] = unique_keys(n, rng)
    rec["xy"] = q
    perm = rng.permutation(n)
    while n >= 2 and np.array_equal(perm, np.arange(n)):          # never the order the keys sort into
        perm = rng.permutation(n)
    rec = rec[perm]
    return Frame(name, n if count is None else count, rec)


def square(cx, cy, s):
    return [(cx - s, cy - s), (cx + s, cy - s), (cx + s, cy + s), (cx - s, cy + s)]


# ---- builders: each returns quads (n, 4, 2) in walk order --------------------------------------------------------------
def far_apart(n, rng, x0=100, y0=30000):
    """squares on a 200-pixel grid: no pair closer than 200 on average"""
    k = np.arange(n)
    return np.array([square(x0 + 200 * int(i % 100), y0 + 200 * int(i // 100), int(s)) for i, s in zip(k, rng.integers(20, 60, size=n))],
                    dtype=np.int64).reshape(n, 4, 2)


def clusters(n, rng, n_clusters=None, jitter=6, side=(20, 60), extent=None):
    """the recipe of test_reference_helper_vectors_on_device, scaled up: squares of random half side around a few centres, every
    corner jittered -- about one cluster per 20 quads, so most rows die early"""
    if n == 0:
        return np.zeros((0, 4, 2), dtype=np.int64)
    n_clusters = n_clusters or max(1, n // 20)
    extent = extent or int(min(60000, 900 + 250 * np.sqrt(n_clusters)))
    centres = rng.integers(70, extent, size=(n_clusters, 2))
    c = centres[rng.integers(0, n_clusters, size=n)]
    s = rng.integers(side[0], side[1], size=n)
    unit = np.array([(-1, -1), (1, -1), (1, 1), (-1, 1)])
    q = c[:, None, :] + s[:, None, None] * unit[None] + rng.integers(-jitter, jitter + 1, size=(n, 4, 2))
    return np.clip(q, 0, 65535)


def ties(n, rng):
    """translated copies of one quad: equal perimeters bit for bit, so of a close pair the earlier one wins"""
    base = np.array([(300, 300), (371, 290), (390, 377), (295, 360)])
    return base[None] + rng.integers(0, 9, size=(n, 1, 2)) + 400 * rng.integers(0, 3, size=(n, 1, 2))


_LEN5 = np.array([(3, 4), (4, 3), (-3, 4), (-4, 3), (3, -4), (4, -3), (-3, -4), (-4, -3), (5, 0), (-5, 0), (0, 5), (0, -5)])


def knife(n, rng):
    """pairs 300 pixels apart: a quad and a copy whose every corner is moved by an integer vector of length exactly 5 or exactly 10,
    so the pair's mean corner distance is exactly 5.0 or 10.0 and the strict `<` alone decides it at those values.  Whole-quad shifts
    (by (3, 4), (6, 8) ...) keep the perimeter (a tie on top), per-corner ones change it either way."""
    base = np.array([(0, 0), (60, -2), (63, 61), (-1, 57)])
    out = []
    for g in range((n + 1) // 2):
        at = base + (500 + 300 * (g % 50), 500 + 300 * (g // 50))
        v = _LEN5[rng.integers(0, len(_LEN5), size=4)] * int(rng.integers(1, 3))
        pair = [at, at + (v if rng.integers(0, 2) else v[0])]
        out += pair[::-1] if rng.integers(0, 2) else pair
    return np.array(out)[:n]


def duplicates(n, rng):
    """identical quads: mean distance 0 -- not < 0.0 (all kept), < the smallest positive float (the first kept)"""
    return np.repeat(np.array([square(700, 700, 33)]), n, axis=0)


def late_bigger(first_gap, rng, lead=2, behind=5, second_bigger=True):
    """a small quad at index i = lead, close smaller ones at i+1 .. i+first_gap, the first bigger one at i+first_gap+1, close smaller
    ones behind it (they survive row i: i is dead by then), then a second bigger one.  Row i kills first_gap quads and dies;
    first_gap = 63 + k puts the first bigger one k lanes into the LDS walk's second 64-quad trip, 127 + k into its third."""
    cx, cy, s = 4000, 4000, 60
    q = [square(200 + 300 * k, 200, 30) for k in range(lead)]                              # far from everything
    q.append(square(cx, cy, s))                                                               # i
    q += [np.array(square(cx, cy, s - int(d))) + rng.integers(-1, 2, size=(4, 2)) for d in rng.integers(3, 12, size=first_gap)]
    q.append(square(cx, cy, s + 4))                                                           # the first bigger one
    q += [np.array(square(cx, cy, s - int(d))) + rng.integers(-1, 2, size=(4, 2)) for d in rng.integers(3, 12, size=behind)]
    if second_bigger:
        q.append(square(cx, cy, s + 9))
    return np.array([np.asarray(a) for a in q])


def masked(gap, rng):
    """a (index 0) is close to j and not to i; j is close to i and bigger than i; a is at least as big as j.  Row a kills j, so row
    i (index 1) meets a dead j = 2 + gap that would otherwise have killed it, and survives.  gap far-apart quads in between move j
    into a later trip; a small close quad behind j is there for i to kill."""
    a, i, j = square(1000, 1000, 50), square(1040, 1000, 40), square(1020, 1000, 45)
    q = [a, i] + list(far_apart(gap, rng)) + [j, square(1042, 1000, 36)]
    return np.array([np.asarray(v) for v in q])


def corners(rng):
    """coordinates 0 and 65535: the whole plane, its corners' unit squares, degenerate quads (no projection: ok = 0) and the
    longest distances the format allows (dx*dx = 4.3e9 in float32)"""
    m = 65535
    q = [square(1, 1, 1), [(0, 0), (m, 0), (m, m), (0, m)], square(m - 1, m - 1, 1), [(0, 0)] * 4, [(m, m)] * 4, [(0, 0), (m, m), (0, 0), (m, m)],
         square(m - 1, 1, 1), square(1, m - 1, 1), [(0, 0), (2, 0), (2, 2), (0, 2)], [(m - 3, m - 3), (m, m - 3), (m, m), (m - 3, m)],
         [(0, 0), (m, 0), (m, 1), (0, 1)], [(0, 0), (m, 1), (m, m), (0, m - 1)]]
    return np.array(q)[rng.permutation(len(q))]


def padded(quads, total, rng):
    """far-apart fillers mixed in at random places (the quads keep their relative order) until the frame has `total` quads"""
    quads = np.asarray(quads)
    extra = total - len(quads)
    if extra <= 0:
        return quads
    fill = far_apart(extra, rng, x0=30000, y0=100)
    slot = np.sort(rng.permutation(total)[: len(quads)])
    out = np.empty((total, 4, 2), dtype=np.int64)
    mask = np.zeros(total, dtype=bool)
    mask[slot] = True
    out[mask], out[~mask] = quads, fill
    return out


REFERENCE_VECTOR = np.array([                  # test_drop_too_near, src/aruco.rs:446-459: min_distance 10.0 leaves one
    [(0, 0), (10, 0), (10, 10), (0, 10)],
    [(1, 0), (10, 0), (10, 10), (0, 10)],
    [(0, 0), (10, 2), (10, 10), (0, 10)],
    [(0, 0), (10, 0), (10, 10), (3, 10)]])


def builder_frames(form, rng, max_cand):
    """every builder once (some twice), in the given form: `reg` keeps every frame at 2..64 quads (`total` is ignored), the other two
    pad every frame past 64"""
    big = form != "reg"
    lo = 65 if big else 2

    def fr(name, quads, total=None):
        q = padded(quads, max(lo, total or 0), rng) if big else np.asarray(quads)
        assert lo <= len(q) and (big or len(q) <= 64), (name, len(q))
        return frame(name, q, rng, max_cand)

    out = [fr("far_apart", far_apart(130 if big else 40, rng)),
           fr("clusters", clusters(200 if big else 50, rng, n_clusters=4)),
           fr("ties", ties(150 if big else 40, rng)),
           fr("knife", knife(150 if big else 50, rng)),
           fr("knife_padded", knife(40, rng), total=200),
           fr("duplicates", duplicates(140 if big else 30, rng)),
           fr("duplicates_padded", duplicates(70 if big else 20, rng), total=210),
           fr("corners", corners(rng), total=100),
           fr("reference_vector", REFERENCE_VECTOR, total=70)]
    if big:
        for trip in (0, 1):
            for k in (0, 1, 63):
                out.append(frame(f"late_bigger_{trip}_{k}", late_bigger(63 + 64 * trip + k, rng), rng, max_cand))
        out += [frame(f"masked_{g}", masked(g, rng), rng, max_cand) for g in (63, 64, 130)]
    else:
        out += [frame(f"late_bigger_{k}", late_bigger(k, rng, behind=4), rng, max_cand) for k in (0, 1, 30, 54)]
        out += [frame(f"masked_{g}", masked(g, rng), rng, max_cand) for g in (0, 1, 30, 60)]
    return out


def _sweep_frames(max_cand, rng, counts):
    out = []
    for c in counts:
        if c <= max_cand:
            out.append(frame(f"c{c}", clusters(c, rng), rng, max_cand))
        elif c == max_cand + 1:
            out.append(frame(f"c{c}_overflow", clusters(max_cand, rng), rng, max_cand, count=c))
    return out


@lru_cache(maxsize=None)
def launches():
    """every launch the GPU test makes, seeded: name -> Launch"""
    out = []
    for t, table in enumerate(TABLES):                                   # counts and cluster sizes per table
        rng = np.random.default_rng(1000 + t)
        counts = sorted(set(COUNTS + CLUSTER_COUNTS[table] + (table, table + 1)))
        out.append(Launch(f"sweep_{table}", table, 25.0, 49 if table in (1024, 6145) else 0, _sweep_frames(table, rng, counts)))
    for f, (form, table) in enumerate((("reg", 1024), ("lds", 1024), ("big", 6145))):     # every builder at every min_distance
        frames = builder_frames(form, np.random.default_rng(2000 + f), table)
        for m, md in enumerate(MIN_DISTANCES):
            out.append(Launch(f"builders_{form}_md{m}", table, md, 49, frames))
            if form == "lds" and md == 25.0:                                              # the same frames without projections
                out.append(Launch("builders_lds_md%d_no_projections" % m, table, md, 0, frames))
    out.append(Launch("builders_lds_6144", 6144, 25.0, 49, builder_frames("lds", np.random.default_rng(2100), 6144)))
    for t, table in enumerate((1024, 6145)):                              # 70 frames: more workgroups than one wave's worth in flight
        rng = np.random.default_rng(3000 + t)
        pool = [c for c in COUNTS if c <= table] + [table]
        counts = [pool[k % len(pool)] for k in range(68)]
        counts[5], counts[40] = 0, 0
        counts = [int(c) for c in rng.permutation(counts)]
        counts.insert(17, table + 1)
        counts.insert(60, table + 300)
        frames = []
        for k, c in enumerate(counts):
            if c <= table:
                frames.append(frame(f"f{k}_c{c}", clusters(c, rng), rng, table))
            else:
                frames.append(frame(f"f{k}_c{c}_overflow", clusters(table, rng), rng, table, count=c))
        assert len(frames) == 70
        out.append(Launch(f"many_frames_{table}", table, 25.0, 49, frames))
    names = [l.name for l in out]
    assert len(set(names)) == len(names)
    return {l.name: l for l in out}


# ----------------------------------------------------------------------------------------------------------------------
# expected results, computed once per launch and shared
# ----------------------------------------------------------------------------------------------------------------------
_expected = {}


def expected(name, oracle):
    """per frame of launch `name`: None for an overflowed frame, else dict(sorted=(c, 4, 2) u16 quads by key, kept=the oracle's
    surviving indices into it, fin=the oracle's surviving quads, model_kept, census).  Cached; callers must not modify it."""
    if name in _expected:
        return _expected[name]
    L = launches()[name]
    key = (id(L.frames), L.min_distance)
    out = _by_frames.get(key)
    if out is None:
        out = []
        for fr in L.frames:
            if fr.count > L.max_cand:
                out.append(None)
                continue
            quads = fr.records["xy"].reshape(-1, 4, 2)
            order, model_kept, census = model(quads, fr.records["start_key"], L.min_distance)
            srt = quads[order]
            if len(srt):
                fin, kept = oracle.discard_too_near(srt.astype(np.uint32), L.min_distance)
            else:
                fin, kept = np.zeros((0, 4, 2), dtype=np.uint32), np.zeros(0, dtype=np.uint32)
            for a in (srt, fin, kept, model_kept):
                a.setflags(write=False)
            out.append(dict(sorted=srt, kept=kept, fin=fin.astype(np.uint16), model_kept=model_kept, census=census))
        _by_frames[key] = out
    _expected[name] = out
    return out


_by_frames = {}


def census_by_form(oracle):
    """the census summed over every frame of every launch, per kernel form"""
    total = {form: dict.fromkeys(CENSUS_KEYS, 0) for form in ("reg", "lds", "big")}
    for name, L in launches().items():
        for fr, e in zip(L.frames, expected(name, oracle)):
            form = L.form_of(fr)
            if form:
                for k in CENSUS_KEYS:
                    total[form][k] += e["census"][k]
    return total
