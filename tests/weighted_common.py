"""The draw of mfsgd_sample_unseen_weighted (include/mfsgd.h, "weighted negatives") restated in numpy, uint64 throughout:
what tests/test_weighted_cpu.py checks against exhaustive enumeration and tests/test_weighted_gpu.py compares the device
with, bit for bit.  On top of tests/implicit_common.py, whose mix, pieces and row grouping these are."""
import numpy as np

from tests import implicit_common as IC

M64, M32 = IC.M64, np.uint64(0xFFFFFFFF)
_32 = np.uint64(32)


def mix64(seed, c):
    """z of the header: all 64 bits of splitmix64's output for the counters c (any integer array), as uint64."""
    c = np.asarray(c).astype(np.uint64)
    shape, c = c.shape, c.reshape(-1)  # (arrays wrap silently; a lone counter is an array of one)
    z = IC._u64(seed) + IC._u64(0x9E3779B97F4A7C15) * (c + np.uint64(1))
    z = (z ^ (z >> np.uint64(30))) * IC._u64(0xBF58476D1CE4E5B9)
    z = (z ^ (z >> np.uint64(27))) * IC._u64(0x94D049BB133111EB)
    return (z ^ (z >> np.uint64(31))).reshape(shape)


def mulhi64(a, b):
    """(a * b) >> 64 for a uint64 array a and one integer b in [0, 2^64): the upper half of the 128-bit product, from
    four 32 x 32 -> 64 bit products none of whose sums wraps."""
    a = np.asarray(a, np.uint64)
    b = IC._u64(b)
    al, ah, bl, bh = a & M32, a >> _32, b & M32, b >> _32
    ll, hl, lh, hh = al * bl, ah * bl, al * bh, ah * bh
    cross = (ll >> _32) + (hl & M32) + (lh & M32)
    return hh + (hl >> _32) + (lh >> _32) + (cross >> _32)


def prefix(w):
    """C: the exclusive prefix of the weights, len(w) + 1 entries, C[-1] = W."""
    return np.concatenate([np.zeros(1, np.uint64), np.cumsum(np.asarray(w, np.uint64), dtype=np.uint64)])


def mass_below(S, w):
    """g of the header: for every position q of the sorted, distinct list S, the weight of the items below S[q] that are
    not in S."""
    S = np.asarray(S, np.int64)
    C = prefix(w)
    seen_before = np.concatenate([np.zeros(1, np.uint64), np.cumsum(np.asarray(w, np.uint64)[S], dtype=np.uint64)])[:S.size]
    return C[S] - seen_before


def unseen_mass(S, w):
    """cnt of the header: the weight of the items that are not in S (a Python integer)."""
    S = np.asarray(S, np.int64)
    C = prefix(w)
    if S.size == 0:
        return int(C[-1])
    return int(mass_below(S, w)[-1]) + int(C[-1]) - int(C[S[-1] + 1])


def weighted_at(S, w, t):
    """The unseen item that holds position t (an array, every entry below unseen_mass(S, w)) of the unseen weight: the
    two searches of the header."""
    S = np.asarray(S, np.int64)
    t = np.asarray(t, np.uint64)
    C, g = prefix(w), mass_below(S, w)
    p = np.searchsorted(g, t, side="right")
    base = np.full(t.shape, int(C[-1]) - unseen_mass(S, w), np.uint64)
    inside = p < S.size
    base[inside] = (C[S] - g)[p[inside]]
    return (np.searchsorted(C, t + base, side="right") - 1).astype(np.int64)


def draw_weighted(S, w, seed, c):
    """The items drawn at the counters c for a user whose seen list is S under the weights w (int32, shape of c)."""
    c = np.asarray(c)
    cnt = unseen_mass(S, w)
    if cnt == 0:
        return np.full(c.shape, -1, np.int32)
    return weighted_at(S, w, mulhi64(mix64(seed, c), cnt)).astype(np.int32)


def sample_weighted(lists, w, users, m, seed=0, first=0, mass=False):
    """What sample_unseen_weighted(users, m, seed, first) must return when user u's list is lists(u) (a callable; sorted
    and distinct) and the weights are w; with mass, (items, int64 unseen weight per row).  Rows are grouped by user, as
    in implicit_common.sample."""
    users = np.asarray(users, np.int64)
    out, cnt = np.empty((users.size, m), np.int32), np.zeros(users.size, np.int64)
    d = np.arange(m, dtype=np.uint64)
    for u in np.unique(users):
        rows = np.flatnonzero(users == u)
        c = IC._u64(first) + rows.astype(np.uint64)[:, None] * np.uint64(m) + d  # first + x * m + d
        out[rows] = draw_weighted(lists(int(u)), w, seed, c)
        cnt[rows] = unseen_mass(lists(int(u)), w)
    return (out, cnt) if mass else out
