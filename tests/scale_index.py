"""One planted seen-item index with item weights at the smallest size that crosses every boundary of the weighted draw's
device code (tests/test_weighted_scale_cpu.py, tests/test_weighted_scale_gpu.py), and the draw restated from its
DEFINITION: enumerate a user's unseen items, accumulate their weights, look the rank up.  No g, no C, no second search:
what tests/weighted_common.py restates in the kernel's two searches is checked against this, and so is the device.

The boundaries (csrc/seen.hip, csrc/draw.hpp):
  * pair_weights_kernel, unseen_mass_kernel and item_counts_kernel stride over the pairs with at most 4096 workgroups of
    256 threads: the loop body runs a second time from position 2^20 on.  N > 2^20 + 2^16 distinct pairs.
  * between them one exclusive scan of 64-bit pair weights over the whole index, many blocks wide, whose sums wrap.
  * the two binary searches of a draw run over a list and over C: a list longer than 2^16 and I = 70 001 items give
    depth 17 to both.
Everything is a pure function of SEED; the arrays are built once per process and are read-only."""
import functools

import numpy as np

from tests import weighted_common as WC

SEED = 20
U, I = 3000, 70001
FIRST_PASS = 1 << 20  # pairs one pass of the grid-stride kernels covers: 4096 workgroups of 256 threads
BIG = 0xFFFFFFFF

# the special users: ZERO_LEFT and ONE_LEFT early, WHALE and EVERY late, so that EVERY's list lies beyond FIRST_PASS
BESIDE, ZERO_LEFT, ONE_LEFT, WHALE, EVERY = 7, 40, 41, 2900, 2950
WHALE_ITEMS = 66000
LEFT = 31337          # the one item of positive weight ONE_LEFT has not seen
HOT = 12345           # the item almost every user holds
RUN = (1000, 1010)    # a run of weightless items; BESIDE has seen its two neighbours and two items inside it
EMPTY = np.r_[0:5, 1400:1420, WHALE + 1:WHALE + 4, U - 6:U]  # users without pairs: at the start, in the middle, at the end
SPECIAL = np.array([0, BESIDE, ZERO_LEFT, ONE_LEFT, 1400, 1419, WHALE, WHALE + 1, EVERY, U - 7, U - 1], np.int32)


class Planted:
    """w uint32[I]; the pairs (eu, ei) as a caller would hand them in (shuffled, duplicates among them); keys, the sorted
    distinct user << 32 | item; ku, ki their halves; off int64[U + 1], the index's own offsets; N = off[U]."""

    def __init__(self, w, eu, ei):
        self.w, self.eu, self.ei = w, eu, ei
        self.keys = np.unique((eu.astype(np.int64) << 32) | ei)
        self.ku, self.ki = (self.keys >> 32).astype(np.int64), (self.keys & 0xFFFFFFFF).astype(np.int64)
        self.off = np.concatenate([[0], np.cumsum(np.bincount(self.ku, minlength=U))]).astype(np.int64)
        self.N = int(self.off[U])
        self.W = int(w.astype(np.uint64).sum())
        for a in (self.w, self.eu, self.ei, self.keys, self.ku, self.ki, self.off):
            a.setflags(write=False)

    def lists(self, u):
        return self.ki[self.off[u]:self.off[u + 1]]

    def row_mass(self):
        """int64[U]: W less the weight of what each user has seen -- every user at once, no prefix, no search."""
        seen = np.zeros(U, np.uint64)
        np.add.at(seen, self.ku, self.w[self.ki].astype(np.uint64))
        return (np.uint64(self.W) - seen).astype(np.int64)


def weights(rng):
    """Small values, 30 % zeros -- items 0 and I - 1 and the run RUN among them -- and 3 % of 2^32 - 1."""
    w = rng.integers(1, 10, I).astype(np.uint32)
    w[rng.random(I) < 0.03] = BIG
    w[rng.random(I) < 0.3] = 0
    w[[0, I - 1]] = 0
    w[RUN[0]:RUN[1]] = 0
    w[[RUN[0] - 1, RUN[1], LEFT, HOT]] = 3
    return w


@functools.lru_cache(maxsize=None)
def planted():
    rng = np.random.default_rng(SEED)
    w = weights(rng)
    special = (ZERO_LEFT, ONE_LEFT, WHALE, EVERY)
    plain = np.setdiff1d(np.arange(U), np.concatenate([EMPTY, special]))
    length = rng.integers(200, 441, plain.size)  # drawn with replacement: a few pairs come twice
    eu, ei = [np.repeat(plain, length)], [rng.integers(0, I, int(length.sum()))]
    heavy = np.flatnonzero(w > 0)
    lists = {
        ZERO_LEFT: np.concatenate([heavy, np.flatnonzero(w == 0)[::3]]),  # every item of weight, and some of none
        ONE_LEFT: np.setdiff1d(heavy, [LEFT]),
        WHALE: rng.permutation(I)[:WHALE_ITEMS],
        EVERY: np.arange(I),
        BESIDE: np.array([RUN[0] - 1, RUN[0] + 4, RUN[0] + 5, RUN[1]]),
    }
    for u, items in lists.items():
        eu.append(np.full(items.size, u))
        ei.append(items)
    holders = plain[plain % 50 != 3]  # almost everybody holds HOT
    eu.append(holders)
    ei.append(np.full(holders.size, HOT))
    eu, ei = np.concatenate(eu).astype(np.int32), np.concatenate(ei).astype(np.int32)
    order = rng.permutation(eu.size)
    return Planted(w, eu[order], ei[order])


def split_for_merge(p, rng):
    """(a, b): index arrays into the planted pairs.  a holds a little more than half of them; b the rest, some of its own
    twice and some that a holds already -- set_seen(a) then mark_seen(b) is the planted index, through the merge."""
    n = p.eu.size
    cut = n * 11 // 20
    order = rng.permutation(n)
    a, rest = order[:cut], order[cut:]
    b = np.concatenate([rest, rest[::97], a[::89]])
    return a, b[rng.permutation(b.size)]


# ---- the draw, from its definition ----------------------------------------------------------------------------------------------
def enumerate_draws(S, w, seed, c):
    """(items int32 of c's shape, cnt): the draws at the counters c for a user who has seen S.  unseen = every item not in
    S, ascending; cum = the running sum of their weights; the draw of rank t is the first unseen item whose running sum
    exceeds t.  -1 throughout when no weight is left."""
    c = np.asarray(c)
    mask = np.ones(w.size, bool)
    mask[np.asarray(S, np.int64)] = False
    unseen = np.flatnonzero(mask)
    cum = np.cumsum(w[unseen].astype(np.uint64), dtype=np.uint64)
    cnt = int(cum[-1]) if cum.size else 0
    if cnt == 0:
        return np.full(c.shape, -1, np.int32), 0
    t = WC.mulhi64(WC.mix64(seed, c), cnt)
    return unseen[np.searchsorted(cum, t, side="right")].astype(np.int32), cnt


def sample_enumerated(p, users, m, seed=0, first=0):
    """(items int32[n, m], mass int64[n]) that sample_unseen_weighted(users, m, seed, first, mass=True) must return on
    the planted index: enumerate_draws per user at the counters first + x * m + d of the user's rows x, and the mass of
    row_mass() -- the two are computed apart and must agree."""
    users = np.asarray(users, np.int64)
    out = np.empty((users.size, m), np.int32)
    mass = p.row_mass()
    d = np.arange(m, dtype=np.uint64)
    if users.size == 0:
        return out, mass[users]
    order = np.argsort(users, kind="stable")
    starts = np.flatnonzero(np.r_[True, users[order][1:] != users[order][:-1]])
    for rows in np.split(order, starts[1:]):
        u = int(users[rows[0]])
        c = np.uint64(int(first) & WC.M64) + rows.astype(np.uint64)[:, None] * np.uint64(m) + d
        out[rows], cnt = enumerate_draws(p.lists(u), p.w, seed, c)
        assert cnt == mass[u], (u, cnt, mass[u])
    return out, mass[users]
