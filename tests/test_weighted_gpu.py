"""Weighted negatives on the device: sample_unseen_weighted against the numpy restatement of the draw
(tests/weighted_common.py), bit for bit -- no statistics, no tolerance -- across the pieces a call is staged in and after
everything that moves the index or the weights; what the handle holds for them; seen_item_counts; and
fit_implicit / fit_bpr with sampling="weighted" against the sequences of calls they are documented as.
The unseen mass cnt reaches about 2^40 here (every weight 2^32 - 1 over 300 items).  cnt near 2^63 needs 2^31 items and
cannot be reached at a testable item count: that end of the 128-bit product is covered on the CPU only
(tests/test_weighted_cpu.py)."""
import gc

import numpy as np
import pytest

from tests import implicit_common as IC
from tests import weighted_common as WC

pytestmark = pytest.mark.gpu

LR, LAM = 0.01, 0.05
STATE = -5
CHUNK = IC.SAMPLE_CHUNK
U1, I1 = 64, 300
EVERY, NONE, ZERO_LEFT, ONE_LEFT, LEFT = 5, 9, 12, 20, 137


def _handle(mf, U, I, k=8, lr=LR, lam=LAM, seed=1):
    return mf.MatrixFactorizationSGD(U, I, k, lr, lam, seed)


def _check(h, lists, w, users, m, seed=0, first=0, what=""):
    """The draws and the masses are the restatement's; no draw is seen or weightless; -1 exactly where no weight is left."""
    got, mass = h.sample_unseen_weighted(users, m, seed, first, mass=True)
    want, cnt = WC.sample_weighted(lists, w, users, m, seed, first, mass=True)
    assert got.dtype == np.int32 and got.shape == (len(users), m) and mass.dtype == np.int64, what
    assert np.array_equal(got, want), what
    assert np.array_equal(mass, cnt), what
    assert np.array_equal(h.sample_unseen_weighted(users, m, seed, first), got), what  # without the mass: the same draws
    w = np.asarray(w)
    for u in np.unique(users):
        mine = got[np.asarray(users) == u]
        assert not np.isin(mine, lists(int(u))).any(), (what, u)
        assert (mine == -1).all() if cnt[np.asarray(users) == u][0] == 0 else (w[mine] > 0).all(), (what, u)
    return got


def _planted(rng):
    """Weights 0 .. 9 with zeros at both ends, in a run beside and under seen items, and spread over a third of the rest;
    pairs with a user who has seen everything, one without pairs, one whose unseen items all weigh nothing and one with
    a single unseen item of positive weight."""
    w = rng.integers(1, 10, I1).astype(np.uint32)
    w[rng.random(I1) < 0.3] = 0
    w[[0, I1 - 1]] = 0
    w[100:110] = 0
    w[[99, 110, LEFT]] = 3
    eu, ei = rng.integers(0, U1, 3000).astype(np.int32), rng.integers(0, I1, 3000).astype(np.int32)
    keep = ~np.isin(eu, (EVERY, NONE, ZERO_LEFT, ONE_LEFT))
    heavy = np.flatnonzero(w > 0)
    zero_left = np.concatenate([heavy, np.flatnonzero(w == 0)[::3]])  # every item of weight, and some of none
    one_left = np.setdiff1d(heavy, [LEFT])
    beside = np.array([99, 104, 105, 110])  # user 0 sees the run's neighbours and two of its zeros
    eu = np.concatenate([eu[keep], np.full(I1, EVERY), np.full(zero_left.size, ZERO_LEFT), np.full(one_left.size, ONE_LEFT),
                         np.zeros(beside.size)]).astype(np.int32)
    ei = np.concatenate([ei[keep], np.arange(I1), zero_left, one_left, beside]).astype(np.int32)
    return w, eu, ei


# ---- 1. bit for bit against the restatement ---------------------------------------------------------------------------------
@pytest.mark.parametrize("m", [1, 5])
def test_draws_are_the_restatements_bit_for_bit(mf, m):
    rng = np.random.default_rng(41 + m)
    w, eu, ei = _planted(rng)
    lists = IC.lists_of(eu, ei)
    users = rng.permutation(U1).astype(np.int32)
    users = np.append(users, users[3])  # every user, in any order, one of them twice
    with _handle(mf, U1, I1) as h:
        h.set_seen(eu, ei)
        h.set_item_weights(w)
        assert np.array_equal(h.item_weights(), w)
        for seed in (0, 1, -5, 1 << 40):
            for first in (0, 1 << 40):
                got = _check(h, lists, w, users, m, seed, first, f"m {m} seed {seed} first {first}")
                assert (got[users == EVERY] == -1).all() and (got[users == ZERO_LEFT] == -1).all()
                assert (got[users == ONE_LEFT] == LEFT).all()
                assert (got[(users != EVERY) & (users != ZERO_LEFT)] >= 0).all()
        got, mass = h.sample_unseen_weighted(users, 40, 7, mass=True)
        assert (mass[users == NONE] == int(w.sum())).all() and (mass[users == ONE_LEFT] == 3).all()
        assert (mass[(users == EVERY) | (users == ZERO_LEFT)] == 0).all()
        assert np.array_equal(got, WC.sample_weighted(lists, w, users, 40, 7))


def test_every_weight_the_largest_there_is(mf):
    """W = 300 * (2^32 - 1), about 2^40: ranks, masses and prefix differences that need all 64 bits."""
    rng = np.random.default_rng(6)
    _, eu, ei = _planted(rng)
    w = np.full(I1, 0xFFFFFFFF, np.uint32)
    users = np.arange(U1, dtype=np.int32)
    with _handle(mf, U1, I1) as h:
        h.set_item_weights(w)  # before there is an index: the table comes with set_seen
        h.set_seen(eu, ei)
        assert np.array_equal(h.item_weights(), w)
        for m, seed, first in ((1, 0, 0), (5, -5, 1 << 40)):
            _check(h, IC.lists_of(eu, ei), w, users, m, seed, first, f"m {m}")
        _, mass = h.sample_unseen_weighted([NONE], 1, mass=True)
        assert int(mass[0]) == I1 * 0xFFFFFFFF > 1 << 40


def test_unit_weights_are_the_uniform_rule_on_the_64_bit_rank(mf):
    rng = np.random.default_rng(7)
    _, eu, ei = _planted(rng)
    lists = IC.lists_of(eu, ei)
    users, m, seed, first = np.arange(U1, dtype=np.int32), 5, 3, 1 << 33
    with _handle(mf, U1, I1) as h:
        h.set_seen(eu, ei)
        h.set_item_weights(np.ones(I1, np.uint32))
        got, mass = h.sample_unseen_weighted(users, m, seed, first, mass=True)
        for u in range(U1):
            S = lists(u)
            assert mass[u] == I1 - S.size
            if S.size == I1:
                assert (got[u] == -1).all()
                continue
            t = WC.mulhi64(WC.mix64(seed, first + u * m + np.arange(m)), I1 - S.size)
            assert np.array_equal(got[u], IC.unseen_at(S, t.astype(np.int64))), u


def test_an_empty_index_draws_among_all_the_items(mf):
    """No pairs: the index has no tables, p = 0 and base = 0 for everybody."""
    rng = np.random.default_rng(8)
    w = rng.integers(0, 5, I1).astype(np.uint32)
    w[[0, I1 - 1]] = 0
    users = rng.integers(0, U1, 200).astype(np.int32)
    with _handle(mf, U1, I1) as h:
        h.set_seen([], [])
        h.set_item_weights(w)
        got = _check(h, lambda u: np.empty(0, np.int64), w, users, 5, 2, 9)
        t = WC.mulhi64(WC.mix64(2, 9 + np.arange(users.size * 5)), int(w.sum()))
        assert np.array_equal(got.ravel(), np.searchsorted(WC.prefix(w), t, side="right") - 1)
        h.set_item_weights(np.zeros(I1, np.uint32))  # all zero is valid: nothing can be drawn
        got, mass = h.sample_unseen_weighted(users, 2, mass=True)
        assert (got == -1).all() and (mass == 0).all()


# ---- 2. cutting the call changes nothing --------------------------------------------------------------------------------------
def test_a_call_longer_than_a_piece_and_its_slices(mf):
    """Rows go up in pieces of CHUNK whole rows at m = 1: the last piece holds 3 rows."""
    U, I, m, seed, first = 8, 50, 1, 11, 1 << 33
    n = CHUNK + 3
    rng = np.random.default_rng(1)
    eu, ei = rng.integers(0, U - 1, 150).astype(np.int32), rng.integers(0, I, 150).astype(np.int32)  # user 7 has no pairs
    w = rng.integers(0, 6, I).astype(np.uint32)
    lists = IC.lists_of(eu, ei)
    users = rng.integers(0, U, n).astype(np.int32)
    with _handle(mf, U, I) as h:
        h.set_seen(eu, ei)
        h.set_item_weights(w)
        whole, mass = h.sample_unseen_weighted(users, m, seed, first, mass=True)
        want, cnt = WC.sample_weighted(lists, w, users, m, seed, first, mass=True)
        assert np.array_equal(whole, want) and np.array_equal(mass, cnt)
        for a, b in ((0, 7), (CHUNK - 2, CHUNK + 2), (CHUNK, n), (n - 1, n), (1000, 1000), (5, CHUNK + 1)):
            got, ms = h.sample_unseen_weighted(users[a:b], m, seed, first + a * m, mass=True)
            assert np.array_equal(got, whole[a:b]) and np.array_equal(ms, mass[a:b]), (a, b)


# ---- 3. the index and the weights move, the draws follow ----------------------------------------------------------------------
def test_the_draws_follow_the_index_and_the_weights(mf):
    U, I, m, seed = 6, 20, 64, 4
    rng = np.random.default_rng(8)
    eu, ei = rng.integers(0, U, 40).astype(np.int32), rng.integers(0, I, 40).astype(np.int32)
    eu, ei = np.concatenate([eu, np.full(I, 2)]).astype(np.int32), np.concatenate([ei, np.arange(I)]).astype(np.int32)
    w = rng.integers(0, 4, I).astype(np.uint32)
    with _handle(mf, U, I) as h:
        h.init_factors()
        h.reserve(users=U + 2)
        users = np.arange(U, dtype=np.int32)
        h.set_seen(eu, ei)
        h.set_item_weights(w)
        before = _check(h, IC.lists_of(eu, ei), w, users, m, seed, 0, "set_item_weights after set_seen")
        # mark_seen: what is newly seen is never drawn again; a batch that adds nothing changes nothing
        flat = before.ravel()
        nu, ni = np.repeat(users, m)[flat >= 0][::9], flat[flat >= 0][::9]
        h.mark_seen(nu, ni)
        eu, ei = np.concatenate([eu, nu]), np.concatenate([ei, ni])
        got = _check(h, IC.lists_of(eu, ei), w, users, m, seed, 0, "mark_seen")
        assert not np.isin((np.repeat(users, m).astype(np.int64) << 32) | got.ravel(), (nu.astype(np.int64) << 32) | ni).any()
        live = mf.debug_device_bytes()
        h.mark_seen(nu[:5], ni[:5])
        assert mf.debug_device_bytes() == live
        assert np.array_equal(_check(h, IC.lists_of(eu, ei), w, users, m, seed, 0, "mark_seen of nothing new"), got)
        # set_seen again; clear_seen then set_seen: the weights stay, the table is made anew
        eu, ei = eu[::2].copy(), ei[::2].copy()
        h.set_seen(eu, ei)
        _check(h, IC.lists_of(eu, ei), w, users, m, seed, 0, "set_seen again")
        h.clear_seen()
        with pytest.raises(mf.MfsgdError) as e:
            h.sample_unseen_weighted(users, m, seed)
        assert e.value.code == STATE and "sample_unseen_weighted: no seen set" in str(e.value)
        assert np.array_equal(h.item_weights(), w)
        eu, ei = np.concatenate([eu, [1, 3]]).astype(np.int32), np.concatenate([ei, [0, I - 1]]).astype(np.int32)
        h.set_seen(eu, ei)
        _check(h, IC.lists_of(eu, ei), w, users, m, seed, 0, "clear_seen then set_seen")
        # other weights
        w = rng.integers(0, 1000, I).astype(np.uint32)
        w[[0, 7, I - 1]] = 0
        h.set_item_weights(w)
        _check(h, IC.lists_of(eu, ei), w, users, m, seed, 0, "set_item_weights replaced")
        # add_users: inside the reserved capacity, then beyond it (the per-user tables move, the pairs do not)
        live = mf.debug_device_bytes()
        assert h.add_users(n=2) == U and h.capacity()[0] == U + 2
        assert mf.debug_device_bytes() == live
        users = np.arange(U + 2, dtype=np.int32)[::-1].copy()
        _check(h, IC.lists_of(eu, ei), w, users, m, seed, 0, "add_users inside the capacity")
        assert h.add_users(n=3) == U + 2 and h.capacity()[0] == U + 5
        users = np.arange(U + 5, dtype=np.int32)
        _check(h, IC.lists_of(eu, ei), w, users, m, seed, 0, "add_users beyond the capacity")
        h.mark_seen([U + 4, U + 1], [3, 4])
        eu, ei = np.concatenate([eu, [U + 4, U + 1]]).astype(np.int32), np.concatenate([ei, [3, 4]]).astype(np.int32)
        _check(h, IC.lists_of(eu, ei), w, users, m, seed, 0, "mark_seen of appended users")
        # add_items: the weights no longer cover the model, until they are set again
        assert h.add_items(n=5) == I
        for _ in range(2):
            with pytest.raises(mf.MfsgdError) as e:
                h.sample_unseen_weighted(users, m, seed)
            assert e.value.code == STATE and f"item weights cover {I} items, the model has {I + 5}" in str(e.value)
            assert np.array_equal(h.item_weights(), w)  # for the item count they were set for
            h.mark_seen([0, 2], [I + 1, I + 4])  # the index goes on working, new items included
        eu, ei = np.concatenate([eu, [0, 2]]).astype(np.int32), np.concatenate([ei, [I + 1, I + 4]]).astype(np.int32)
        assert np.array_equal(h.sample_unseen(users, 3, seed), IC.sample(IC.lists_of(eu, ei), I + 5, users, 3, seed))
        w = np.concatenate([w, [5, 0, 9, 1, 2]]).astype(np.uint32)
        h.set_item_weights(w)
        got = _check(h, IC.lists_of(eu, ei), w, users, m, seed, 0, "add_items, weights set again")
        assert (got >= I).any() and not (got == I + 1).any()  # the new items are drawn, but for the one of weight 0
        assert (got[2] != I + 4).all()  # ... and what was marked seen while the weights were stale
        # clear_item_weights: no weights, no draws; the uniform draw is as it was
        h.clear_item_weights()
        assert h.item_weights() is None
        with pytest.raises(mf.MfsgdError) as e:
            h.sample_unseen_weighted(users, m, seed)
        assert e.value.code == STATE and "no item weights" in str(e.value)
        assert np.array_equal(h.sample_unseen(users, 3, seed), IC.sample(IC.lists_of(eu, ei), I + 5, users, 3, seed))


# ---- 4. what the handle holds, and what a draw leaves alone ---------------------------------------------------------------------
def test_memory_is_the_index_plus_eight_bytes_a_pair_and_the_prefix(mf):
    U, I = 500, 400
    rng = np.random.default_rng(10)
    live = mf.debug_device_bytes
    gc.collect()
    before = live()
    su, si = rng.integers(0, U, 20000).astype(np.int32), rng.integers(0, I, 20000).astype(np.int32)
    users = rng.integers(0, U, 5000).astype(np.int32)
    with _handle(mf, U, I) as h:
        h.set_seen(su, si)
        d, cap = h.seen_size(), h.capacity()[0]
        index = live() - before
        assert 4 * d + 12 * cap + 8 <= index <= 4 * d + 12 * (cap + 1) + 64  # a handle without weights: the index's rule
        h.set_item_weights(rng.integers(0, 9, I))
        extra = 8 * d + 8 * (I + 1)
        assert extra <= live() - before - index <= extra + 64
        held = live()
        for m, mass in ((3, False), (1, True)):  # a draw allocates staging only
            h.sample_unseen_weighted(users, m, 5, mass=mass)
            assert live() == held
        with pytest.raises(mf.MfsgdError):  # a refused call holds nothing either
            h.sample_unseen_weighted([0, U], 3, 5)
        h.seen_item_counts()
        h.item_weights()
        assert live() == held
        h.set_item_weights(np.ones(I, np.uint32))  # replaced: the same size
        assert live() == held
        bu, bi = rng.integers(0, U, 3000).astype(np.int32), rng.integers(0, I, 3000).astype(np.int32)
        h.mark_seen(bu, bi)
        d2 = h.seen_size()
        assert d2 > d and 12 * d2 + 8 * (I + 1) <= live() - before <= 12 * d2 + 12 * (cap + 1) + 8 * (I + 1) + 128
        h.set_seen(su, si)
        assert live() == held
        h.clear_item_weights()
        assert live() - before == index
        h.set_item_weights(np.ones(I, np.uint32))
        h.clear_seen()  # the table leaves with the index, the prefix stays
        assert 8 * (I + 1) <= live() - before <= 8 * (I + 1) + 64
    assert live() == before


def test_seen_item_counts_is_the_histogram_of_the_distinct_pairs(mf):
    rng = np.random.default_rng(3)
    w, eu, ei = _planted(rng)
    keys = np.unique((eu.astype(np.int64) << 32) | ei)
    with _handle(mf, U1, I1) as h:
        h.set_seen(eu, ei)
        got = h.seen_item_counts()
        assert got.dtype == np.int64 and np.array_equal(got, np.bincount(keys & 0xFFFFFFFF, minlength=I1))
        assert got.sum() == h.seen_size() and got.min() >= 1  # (one user holds every item)
        h.mark_seen([NONE, NONE], [7, 7])
        assert h.seen_item_counts()[7] == got[7] + 1
        h.init_factors()
        h.add_items(n=3)  # the new items are seen by nobody
        assert np.array_equal(h.seen_item_counts()[I1:], [0, 0, 0])
        # set_popularity_weights is popularity_weights of these counts
        h.set_popularity_weights(alpha=0.5, resolution=4, least=0)
        counts = h.seen_item_counts()
        assert np.array_equal(h.item_weights(), mf.popularity_weights(counts, 0.5, 4, 0)) and (h.item_weights()[I1:] == 0).all()
        h.set_popularity_weights()
        assert np.array_equal(h.item_weights(), np.maximum(1, np.rint(16 * counts.astype(np.float64) ** 0.75)).astype(np.uint32))


def test_the_draws_touch_neither_the_model_nor_the_index(mf):
    U, I = 40, 90
    rng = np.random.default_rng(12)
    eu, ei = rng.integers(0, U, 900).astype(np.int32), rng.integers(0, I, 900).astype(np.int32)
    users = rng.integers(0, U, 5000).astype(np.int32)
    w = rng.integers(0, 50, I).astype(np.uint32)
    with _handle(mf, U, I) as h:
        h.set_seen(eu, ei)
        h.set_item_weights(w)
        h.init_factors()
        h.set_ratings(eu, ei, rng.random(eu.size, dtype=np.float32))
        h.fit(1)
        P, Q = h.get_factors()
        ptr, items = h.seen(np.arange(U))
        uniform = h.sample_unseen(users, 3, 5)
        assert np.array_equal(uniform, IC.sample(IC.lists_of(eu, ei), I, users, 3, 5))  # weights do not move the uniform draw
        got = h.sample_unseen_weighted(users, 3, 5)
        assert np.array_equal(got, WC.sample_weighted(IC.lists_of(eu, ei), w, users, 3, 5))
        h.seen_item_counts()
        P2, Q2 = h.get_factors()
        assert P.tobytes() == P2.tobytes() and Q.tobytes() == Q2.tobytes()
        ptr2, items2 = h.seen(np.arange(U))
        assert np.array_equal(ptr, ptr2) and np.array_equal(items, items2) and np.array_equal(h.item_weights(), w)
        assert h.debug_counters()["schedule_builds"] == 1


# ---- 5. the fits are the sequences they are documented as ----------------------------------------------------------------------
def _bits(m):
    P, Q = m.get_factors()
    return P.tobytes(), Q.tobytes()


def _positives(rng, U, I, full):
    pu, pi = rng.integers(0, U, 400).astype(np.int32), rng.integers(0, I, 400).astype(np.int32)  # duplicates among them
    pu, pi = np.concatenate([pu, np.full(I, full)]).astype(np.int32), np.concatenate([pi, np.arange(I)]).astype(np.int32)
    order = rng.permutation(pu.size)
    return pu[order], pi[order]


def test_fit_implicit_weighted_is_its_documented_sequence(mf):
    U, I, k, neg, epochs, seed, full = 60, 50, 8, 3, 3, 21, 17
    rng = np.random.default_rng(5)
    pu, pi = _positives(rng, U, I, full)
    n = pu.size
    with _handle(mf, U, I, k, lr=0.05) as a, _handle(mf, U, I, k, lr=0.05) as b, _handle(mf, U, I, k, lr=0.05) as c:
        for h in (a, b, c):
            h.set_seen(pu, pi)
            h.set_popularity_weights(least=0)
        w = a.item_weights()
        rmse = a.fit_implicit(pu, pi, epochs, neg, seed=seed, pos=1.0, neg=0.25, sampling="weighted")
        b.init_factors()
        want = []
        for e in range(epochs):
            J = b.sample_unseen_weighted(pu, neg, seed, first=e * n * neg)
            assert np.array_equal(J, WC.sample_weighted(IC.lists_of(pu, pi), w, pu, neg, seed, e * n * neg))
            assert (J[pu == full] == -1).all() and (J[pu != full] >= 0).all()
            keep = J.ravel() >= 0
            ju, ji = np.repeat(pu, neg)[keep], J.ravel()[keep]
            b.set_ratings(np.concatenate([pu, ju]), np.concatenate([pi, ji]),
                          np.concatenate([np.full(n, 1.0, np.float32), np.full(ji.size, 0.25, np.float32)]))
            want.append(b.fit(1)[0])
        assert rmse.tobytes() == np.array(want).tobytes() and _bits(a) == _bits(b)
        first = c.fit_implicit(pu, pi, 2, neg, seed=seed, neg=0.25, sampling="weighted")
        last = c.fit_implicit(pu, pi, 1, neg, seed=seed, neg=0.25, first_epoch=2, sampling="weighted")
        assert np.concatenate([first, last]).tobytes() == rmse.tobytes() and _bits(a) == _bits(c)
    # sampling="uniform" is the call without the keyword, weights or none
    with _handle(mf, U, I, k, lr=0.05) as a, _handle(mf, U, I, k, lr=0.05) as b:
        a.set_seen(pu, pi)
        a.set_popularity_weights()
        ra = a.fit_implicit(pu, pi, 2, neg, seed=seed, sampling="uniform")
        rb = b.fit_implicit(pu, pi, 2, neg, seed=seed)
        assert ra.tobytes() == rb.tobytes() and _bits(a) == _bits(b)


def test_fit_bpr_weighted_is_its_documented_sequence(mf):
    U, I, k, epochs, seed, full = 60, 50, 8, 3, 13, 17
    rng = np.random.default_rng(6)
    pu, pi = _positives(rng, U, I, full)
    n = pu.size
    with _handle(mf, U, I, k, lr=0.05) as a, _handle(mf, U, I, k, lr=0.05) as b, _handle(mf, U, I, k, lr=0.05) as c:
        for h in (a, b, c):
            h.set_seen(pu, pi)
            h.set_popularity_weights(least=0)
        w = a.item_weights()
        stats = a.fit_bpr(pu, pi, epochs, seed=seed, sampling="weighted")
        b.init_factors()
        loss, auc = [], []
        for e in range(epochs):
            J = b.sample_unseen_weighted(pu, 1, seed, first=e * n)[:, 0]
            assert np.array_equal(J, WC.sample_weighted(IC.lists_of(pu, pi), w, pu, 1, seed, e * n)[:, 0])
            keep = J >= 0
            assert not keep[pu == full].any() and keep[pu != full].all()
            x = b.partial_fit_pairwise(pu[keep], pi[keep], J[keep], margins=True).astype(np.float64)
            loss.append(np.logaddexp(0.0, -x).mean())
            auc.append((x > 0).mean())
        assert stats["loss"].tobytes() == np.array(loss).tobytes() and stats["auc"].tobytes() == np.array(auc).tobytes()
        assert _bits(a) == _bits(b)
        s1 = c.fit_bpr(pu, pi, 2, seed=seed, sampling="weighted")
        s2 = c.fit_bpr(pu, pi, 1, seed=seed, first_epoch=2, sampling="weighted")
        assert np.concatenate([s1["loss"], s2["loss"]]).tobytes() == stats["loss"].tobytes() and _bits(a) == _bits(c)
        assert c.fit_bpr(pu, pi, 1, seed=seed, first_epoch=3, stats=False, sampling="weighted") is None
    with _handle(mf, U, I, k, lr=0.05) as a, _handle(mf, U, I, k, lr=0.05) as b:
        a.set_seen(pu, pi)
        a.set_popularity_weights()
        sa = a.fit_bpr(pu, pi, 2, seed=seed, sampling="uniform")
        sb = b.fit_bpr(pu, pi, 2, seed=seed)
        assert sa["loss"].tobytes() == sb["loss"].tobytes() and _bits(a) == _bits(b)
        with pytest.raises(ValueError):
            a.fit_bpr(pu, pi, 1, candidates=4, sampling="weighted")
