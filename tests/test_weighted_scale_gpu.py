"""The weighted draw and its unseen-mass table at the size where their launch shapes matter: the planted index of
tests/scale_index.py -- 1.19 M distinct pairs, so that the grid-stride kernels of csrc/seen.hip take a second pass and the
scan between them is many blocks wide; a list of 66 000 and 70 001 items, so that both searches of a draw run to depth 17;
weights of 2^32 - 1 among small ones and zeros -- against the draw's definition (enumerate the unseen items, accumulate
their weights, look the rank up) and W less the seen weight, bit for bit.  No statistics, no tolerance.
The references are computed once per process and shared; every test builds its own handle."""
import functools
import gc

import numpy as np
import pytest

from tests import hardneg_common as HC
from tests import implicit_common as IC
from tests import scale_index as SI
from tests import warp_common as WPC

pytestmark = pytest.mark.gpu

LR, LAM = 0.01, 0.05
U, I = SI.U, SI.I
# (m, seed, first): every user once; the special users, every fourth other and the whale 400 times over
DRAWS = ((1, 3, 0), (5, -5, (1 << 40) + 11))


def _handle(mf, k=8):
    return mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1)


def _users(m):
    if m == 1:
        return np.arange(U, dtype=np.int32)
    others = np.setdiff1d(np.arange(U), SI.SPECIAL)[::4]
    # ... and the whale 400 times more, between the others: 2 000 draws whose first search runs over its 66 000 entries
    rows = np.concatenate([SI.SPECIAL, others, np.full(400, SI.WHALE)])
    return rows[np.random.default_rng(5).permutation(rows.size)].astype(np.int32)


@functools.lru_cache(maxsize=None)
def _reference(m, seed, first, alt=False):
    """(users, items, mass) of the enumeration on the planted index, under its weights or the small ones of _small()."""
    p = SI.planted() if not alt else _small()
    users = _users(m)
    items, mass = SI.sample_enumerated(p, users, m, seed, first)
    for a in (users, items, mass):
        a.setflags(write=False)
    return users, items, mass


@functools.lru_cache(maxsize=None)
def _small():
    """The planted pairs under other weights: none above 9, so that the draws land on every kind of item instead of on
    the 2^32 - 1 ones, which hold all but a billionth of the mass."""
    p = SI.planted()
    w = p.w.copy()
    big = w == SI.BIG
    w[big] = 1 + np.arange(int(big.sum())) % 9
    return SI.Planted(w, p.eu.copy(), p.ei.copy())


def _check(h, p, alt=False, draws=DRAWS, what=""):
    """The handle's draws and masses are the enumeration's on p; no draw is seen or weightless; -1 exactly where no weight
    is left.  Returns the rows checked that lie beyond the first pass of the grid-stride kernels."""
    late = 0
    for m, seed, first in draws:
        users, want, cnt = _reference(m, seed, first, alt)
        got, mass = h.sample_unseen_weighted(users, m, seed, first, mass=True)
        assert got.dtype == np.int32 and got.shape == (users.size, m) and mass.dtype == np.int64, what
        bad = np.flatnonzero((got != want).any(axis=1))
        assert bad.size == 0, f"{what} m {m}: the draws of {bad.size} rows differ, first users {users[bad[:8]]} " \
                              f"(their lists start at {p.off[users[bad[:8]]]}): {got[bad[:8], 0]} instead of {want[bad[:8], 0]}"
        bad = np.flatnonzero(mass != cnt)
        assert bad.size == 0, f"{what} m {m}: the masses of {bad.size} rows differ, first users {users[bad[:8]]}"
        assert ((got == -1) == (cnt == 0)[:, None]).all(), what
        hit = got >= 0
        assert (p.w[got[hit]] > 0).all(), what
        drawn = (np.broadcast_to(users[:, None].astype(np.int64), got.shape)[hit] << 32) | got[hit]
        assert not np.isin(drawn, p.keys).any(), what
        late += int(((p.off[users] >= SI.FIRST_PASS) & (p.off[users + 1] > p.off[users])).sum())
    return late


# ---- 1. bit for bit against the definition --------------------------------------------------------------------------------------
def test_the_draws_and_masses_of_every_user_are_the_definitions(mf):
    p = SI.planted()
    with _handle(mf) as h:
        h.set_seen(p.eu, p.ei)
        assert h.seen_size() == p.N > SI.FIRST_PASS + (1 << 16)
        h.set_item_weights(p.w)
        late = _check(h, p, what="set_seen, set_item_weights")
        assert late > 40  # users stored behind position 2^20 of the index were checked: by their off
        users, items, mass = _reference(*DRAWS[0])
        assert p.off[SI.EVERY] >= SI.FIRST_PASS and (items[users == SI.EVERY] == -1).all()
        assert (items[users == SI.ZERO_LEFT] == -1).all() and (items[users == SI.ONE_LEFT] == SI.LEFT).all()
        assert (mass[SI.EMPTY] == p.W).all() and mass[SI.ONE_LEFT] == 3 and p.W > 1 << 40
        assert (items[(mass > 0)] >= 0).all()
        assert np.array_equal(h.sample_unseen_weighted(users, 1, DRAWS[0][1], DRAWS[0][2]), items)  # without the mass
        # the index itself, where the lists are long or lie late
        ask = np.array([SI.WHALE, SI.WHALE + 1, SI.EVERY, U - 7, SI.ONE_LEFT], np.int32)
        ptr, items = h.seen(ask)
        assert np.array_equal(np.diff(ptr), np.diff(p.off)[ask])
        assert np.array_equal(items, np.concatenate([p.lists(u) for u in ask]))


# ---- 2. whichever way the index and the weights came ------------------------------------------------------------------------------
def test_weights_before_the_index(mf):
    p = SI.planted()
    with _handle(mf) as h:
        h.set_item_weights(p.w)  # before there is an index: the table comes with set_seen
        h.set_seen(p.eu, p.ei)
        _check(h, p, what="set_item_weights, set_seen")


def test_the_table_is_rebuilt_over_a_merged_index(mf):
    p = SI.planted()
    a, b = SI.split_for_merge(p, np.random.default_rng(2))
    first = np.unique((p.eu[a].astype(np.int64) << 32) | p.ei[a]).size
    assert first > 1 << 19 and b.size > p.eu.size - a.size + 5000
    with _handle(mf) as h:
        h.set_seen(p.eu[a], p.ei[a])
        assert h.seen_size() == first
        h.set_item_weights(p.w)
        h.mark_seen(p.eu[b], p.ei[b])  # duplicates and pairs already there among them
        assert h.seen_size() == p.N
        _check(h, p, what="set_seen of a half, set_item_weights, mark_seen of the rest")


def test_other_weights_and_back(mf):
    p, q = SI.planted(), _small()
    with _handle(mf) as h:
        h.set_seen(p.eu, p.ei)
        h.set_item_weights(q.w)
        assert np.array_equal(h.item_weights(), q.w)
        _check(h, q, alt=True, what="small weights")
        users, items, _ = _reference(*DRAWS[0], True)
        assert np.unique(items).size > 1000 and (q.w[items[items >= 0]] < 10).all()  # draws all over the catalogue
        users, items, _ = _reference(*DRAWS[1], True)
        whale = items[users == SI.WHALE]  # ... and all over the whale's 4 001 unseen items: a table entry a little off shows
        assert whale.size > 2000 and np.unique(whale).size > 1000 and not np.isin(whale, p.lists(SI.WHALE)).any()
        h.set_item_weights(p.w)
        assert np.array_equal(h.item_weights(), p.w)
        _check(h, p, what="set back")


# ---- 3. the histogram -----------------------------------------------------------------------------------------------------------
def test_seen_item_counts_past_one_pass_and_on_one_hot_address(mf):
    p = SI.planted()
    want = np.bincount(p.ki, minlength=I)
    assert want.sum() == p.N > SI.FIRST_PASS and want[SI.HOT] > 0.9 * U  # many atomics on one address
    with _handle(mf) as h:
        h.set_seen(p.eu, p.ei)
        got = h.seen_item_counts()
        assert got.dtype == np.int64 and np.array_equal(got, want)
        h.set_popularity_weights()
        assert np.array_equal(h.item_weights(), mf.popularity_weights(want))
        mass = h.sample_unseen_weighted(np.arange(U, dtype=np.int32), 1, mass=True)[1]
        pop = SI.Planted(mf.popularity_weights(want), p.eu.copy(), p.ei.copy())
        assert np.array_equal(mass, pop.row_mass())


# ---- 4. the other samplers at this search depth ------------------------------------------------------------------------------------
def test_the_uniform_hard_and_violating_draws_on_the_long_lists(mf, oracle):
    k, seed, first = 8, 6, (1 << 40) + 5
    m = 3  # L + 1 at k = 8
    p = SI.planted()
    rng = np.random.default_rng(4)
    users = np.repeat(np.array([SI.WHALE, SI.ONE_LEFT, SI.EVERY, SI.WHALE + 1], np.int32), (300, 100, 20, 100))
    users = users[rng.permutation(users.size)]
    pos = rng.integers(0, I, users.size).astype(np.int32)
    with _handle(mf, k) as h:
        h.init_factors()
        h.set_seen(p.eu, p.ei)
        P, Q = h.get_factors()
        scorer = lambda u, i: oracle.predict(P, Q, u, i)
        cand = h.sample_unseen(users, m, seed, first)
        assert np.array_equal(cand, IC.sample(p.lists, I, users, m, seed, first))
        whale = cand[users == SI.WHALE]
        assert not np.isin(whale, p.lists(SI.WHALE)).any() and np.unique(whale).size > 500 and (cand[users == SI.EVERY] == -1).all()
        got = h.sample_unseen_hard(users, m, seed, first, scores=True, draws=True)
        for g, w, name in zip(got, HC.hard(p.lists, I, users, m, seed, first, scorer), ("items", "scores", "draws")):
            assert g.tobytes() == w.tobytes(), name
        assert len(set(got[2][users == SI.WHALE].tolist())) == m  # every candidate number wins somewhere
        got = h.sample_unseen_violating(users, pos, m, 0.0, seed, first, draws=True, margins=True, ranks=True)
        want = WPC.violating(p.lists, I, users, pos, m, 0.0, seed, first, scorer)
        for g, w, name in zip(got, want, ("items", "draws", "margins", "ranks")):
            assert g.tobytes() == w.tobytes(), name
        sel = users == SI.WHALE
        assert (want[0][sel] >= 0).any() and (want[1][sel] == m).any() and (want[1][sel] > 0).any()


# ---- 5. what the handle holds ------------------------------------------------------------------------------------------------------
def test_memory_is_twelve_bytes_a_pair_and_the_prefix(mf):
    p = SI.planted()
    live = mf.debug_device_bytes
    gc.collect()
    before = live()
    with _handle(mf) as h:
        h.set_seen(p.eu, p.ei)
        h.set_item_weights(p.w)
        cap = h.capacity()[0]
        held = live() - before
        want = 12 * p.N + 8 * (I + 1)  # items int32, mass uint64; C uint64 -- and off, slot per user of capacity
        assert want + 12 * cap + 8 <= held <= want + 12 * (cap + 1) + 128
        h.sample_unseen_weighted(np.arange(U, dtype=np.int32), 5, 1, mass=True)  # a draw allocates staging only
        h.seen_item_counts()
        assert live() - before == held
    assert live() == before
