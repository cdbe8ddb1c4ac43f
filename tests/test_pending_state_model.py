"""The 8-byte per-dart states of the contour stage (csrc/k_contours.hip, FinState), restated in Python and checked against plain
list ranking -- no GPU.

k_local_contract contracts windows inside tiles of 1024 or 2048 consecutive darts.  A dart whose window wraps its cycle inside the
tile gets its final state at once (leader = the cycle's smallest key, hops to it).  A dart whose window reaches a dart outside the
tile gets a PENDING state {entry slot, window length, hops to the window's minimum, low 11 bits of that minimum}.  The entry
stage starts every entry's window from its own dart's state (entry_start) and resolves the reduced list; k_jump_finalize then
turns every pending state into the final one (resolve_pending).  Here each of those steps is restated -- the bit packing
included -- and the result must equal what walking every cycle gives: for every dart, the dart of smallest
(event key << 32 | dart) on its cycle, and the hops forward to it."""
import numpy as np
import pytest

NO_KEY = 0xFFFFFFFF
PEND = 0x80000000
PEND_SLOT = 0x3FFFFFFF
FIN_HOPS = 0x3FFFFFFF
FIN_EVENT = 0x80000000


# ---- the packing of a pending FinState (pend_pack / pend_* in k_contours.hip) ----
def pend_pack(slot, dist, off, min_dart):
    m = min_dart & 0x7FF
    return (PEND | ((m >> 10) << 30) | (slot & PEND_SLOT), ((dist - 1) | (off << 11) | ((m & 0x3FF) << 22)) & 0xFFFFFFFF)


def is_pending(s):
    return bool(s[0] & PEND)


def pend_slot(s):
    return s[0] & PEND_SLOT


def pend_dist(s):
    return (s[1] & 0x7FF) + 1


def pend_off(s):
    return (s[1] >> 11) & 0x7FF


def pend_min(s, d):
    return (d & ~0x7FF) | (((s[0] >> 30) & 1) << 10) | (s[1] >> 22)


def resolve_pending(s, d, g_key, g_off):
    leader = g_key & 0xFFFFFFFF
    hops = pend_off(s) if leader == pend_min(s, d) else (pend_dist(s) + g_off) & FIN_HOPS
    return leader, hops | (FIN_EVENT if (g_key >> 32) != NO_KEY else 0)


# ---- the stages ----
def local_states(succ, ev, lt, rng):
    """k_local_contract's output: per dart a final or pending state; entry slots handed out in an arbitrary order (the kernel's
    atomics), entry_list[slot] = entry dart"""
    n = len(succ)
    key = [(int(ev[d]) << 32) | d for d in range(n)]
    entries = sorted({int(succ[d]) for d in range(n) if succ[d] // lt != d // lt})
    slots = rng.permutation(len(entries)) + int(rng.integers(0, 5))   # slots need not start at 0 or be dense
    slot_of = {e: int(s) for e, s in zip(entries, slots)}
    entry_list = {int(s): e for e, s in zip(entries, slots)}
    fin = []
    for d in range(n):
        lo = d // lt * lt
        best, off, j, dist = key[d], 0, d, 0
        while True:          # the window [d, j): grows until it leaves the tile or wraps (a cycle inside a tile is < lt long)
            dist += 1
            j = int(succ[j])
            if not lo <= j < lo + lt:
                fin.append(pend_pack(slot_of[j], dist, off, best & 0xFFFFFFFF))
                break
            if j == d:
                fin.append((best & 0xFFFFFFFF, off | (FIN_EVENT if (best >> 32) != NO_KEY else 0)))
                break
            if key[j] < best:
                best, off = key[j], dist
        assert dist <= lt
    return fin, entry_list


def entry_start(e, s, ev):
    """an entry's first window over the reduced list (k_entry_frame / k_entry_init): key from the minimum's record"""
    assert is_pending(s)   # (cycles only: an entry's window always leaves its tile)
    m = pend_min(s, e)
    return ((int(ev[m]) << 32) | m), pend_off(s), pend_dist(s), pend_slot(s)


def resolve_entries(fin, entry_list, ev):
    """the converged entry states (what k_entry_frame's / k_entry_jump's doubling reaches): plain walks over the reduced list"""
    start = {s: entry_start(e, fin[e], ev) for s, e in entry_list.items()}
    es = {}
    for s0 in start:
        key, off, dist, s = start[s0][0], start[s0][1], start[s0][2], start[s0][3]
        while s != s0:
            k, o, di, nxt = start[s]
            if k < key:
                key, off = k, dist + o
            dist += di
            s = nxt
        es[s0] = (key, off)
    return es


def finalize(fin, es):
    out = []
    for d, s in enumerate(fin):
        out.append(resolve_pending(s, d, *es[pend_slot(s)]) if is_pending(s) else s)
    return out


def list_ranking(succ, ev):
    n = len(succ)
    key = [(int(ev[d]) << 32) | d for d in range(n)]
    out = [None] * n
    for d in range(n):
        if out[d] is not None:
            continue
        cyc = [d]
        while int(succ[cyc[-1]]) != d:
            cyc.append(int(succ[cyc[-1]]))
        li = min(range(len(cyc)), key=lambda i: key[cyc[i]])
        leader = cyc[li]
        flag = FIN_EVENT if ev[leader] != NO_KEY else 0
        for i, x in enumerate(cyc):
            out[x] = (leader, ((li - i) % len(cyc)) | flag)
    return out


# ---- graphs ----
def _cycles_to_succ(cycles, n):
    succ = np.full(n, -1, np.int64)
    for c in cycles:
        for a, b in zip(c, c[1:] + c[:1]):
            succ[a] = b
    assert (succ >= 0).all()
    return succ


def _random_cycles(rng, n, lengths):
    perm = [int(x) for x in rng.permutation(n)]
    cycles, i = [], 0
    while i < n:
        k = min(int(rng.choice(lengths)), n - i)
        cycles.append(perm[i:i + k])
        i += k
    return cycles


def _local_cycles(rng, n, lt, span):
    """borders as the dart numbering makes them: runs of nearby indices (a border inside a tile, or crossing a few tiles)"""
    cycles, free = [], list(range(n))
    while free:
        k = min(len(free), int(rng.integers(1, span)))
        start = int(rng.integers(0, max(1, len(free) - k + 1)))
        c = free[start:start + k]
        del free[start:start + k]
        if rng.random() < 0.5:
            c = c[::-1]
        cycles.append(c)
    return cycles


def _events(rng, n, density):
    ev = np.full(n, NO_KEY, np.int64)
    has = rng.random(n) < density
    ev[has] = rng.permutation(np.arange(0, 2 * n, 2))[: int(has.sum())] + rng.integers(0, 2, int(has.sum()))
    return ev


_KINDS = ["random_short", "random_long", "local", "one_cycle", "tile_straddle"]


@pytest.mark.parametrize("lt", [1024, 2048])
@pytest.mark.parametrize("kind", _KINDS)
def test_pending_states_resolve_to_list_ranking(lt, kind):
    rng = np.random.default_rng(lt + _KINDS.index(kind))
    for trial in range(3):
        if kind == "random_short":
            n = int(rng.integers(3 * lt, 5 * lt))
            cycles = _random_cycles(rng, n, [1, 2, 3, 5, 8, 20])
        elif kind == "random_long":
            n = int(rng.integers(2 * lt, 4 * lt))
            cycles = _random_cycles(rng, n, [lt // 2, lt, 3 * lt])
        elif kind == "local":
            n = int(rng.integers(4 * lt, 6 * lt))
            cycles = _local_cycles(rng, n, lt, lt // 2)
        elif kind == "one_cycle":        # one border through every tile, windows of every length frozen at every tile exit
            n = int(rng.integers(2 * lt, 3 * lt))
            cycles = [[int(x) for x in rng.permutation(n)]]
        else:                            # long borders whose minimum sits right behind a tile boundary and right in front of one
            n = 4 * lt
            cycles = [list(range(a, b)) for a, b in [(0, lt - 3), (lt - 3, lt + 5), (lt + 5, 3 * lt + 1), (3 * lt + 1, n)]]
        succ = _cycles_to_succ(cycles, n)
        ev = _events(rng, n, [0.02, 0.3, 1.0][trial])
        fin, entry_list = local_states(succ, ev, lt, rng)
        n_pend = sum(is_pending(s) for s in fin)
        assert n_pend > 0 and (kind not in ("local", "tile_straddle") or n_pend < n)   # frozen windows, and wrapped ones
        got = finalize(fin, resolve_entries(fin, entry_list, ev))
        assert got == list_ranking(succ, ev)


def test_pending_packing_round_trips():
    """every field of a pending state at its extremes, for darts anywhere in a 2048-aligned block and far up the index range"""
    rng = np.random.default_rng(7)
    for _ in range(20000):
        lt = int(rng.choice([1024, 2048]))
        d = int(rng.integers(0, (1 << 30) - (1 << 16)))
        lo = d // lt * lt
        m = lo + int(rng.integers(0, lt))
        slot = int(rng.choice([0, PEND_SLOT, int(rng.integers(0, PEND_SLOT))]))
        dist = int(rng.choice([1, lt, int(rng.integers(1, lt + 1))]))
        off = int(rng.integers(0, dist))
        s = pend_pack(slot, dist, off, m)
        assert is_pending(s) and 0 <= s[0] < 2**32 and 0 <= s[1] < 2**32
        assert (pend_slot(s), pend_dist(s), pend_off(s), pend_min(s, d)) == (slot, dist, off, m)
    # a final state never reads as pending: leaders are dart indices below 2^30
    assert not is_pending(((1 << 30) - 1, FIN_EVENT | FIN_HOPS))
