"""Implicit feedback on the device: sample_unseen against the numpy restatement of the draw (tests/implicit_common.py),
bit for bit, across the pieces a call is staged in and after everything that moves the seen-item index; fit_implicit
against the sequence of calls it is documented as; and a planted one-class problem that negatives make learnable."""
import numpy as np
import pytest

from tests import implicit_common as IC

pytestmark = pytest.mark.gpu

LR, LAM = 0.01, 0.05
STATE = -5
CHUNK = IC.SAMPLE_CHUNK


def _handle(mf, U, I, k=8, lr=LR, lam=LAM, seed=1):
    return mf.MatrixFactorizationSGD(U, I, k, lr, lam, seed)


def _check(got, lists, n_items, users, m, seed, first, what=""):
    """got is the restatement's answer, holds no seen item and nothing outside [0, n_items) but the -1 of a full list."""
    assert got.dtype == np.int32 and got.shape == (len(users), m), what
    assert np.array_equal(got, IC.sample(lists, n_items, users, m, seed, first)), what
    assert got.max(initial=-1) < n_items, what
    for u in np.unique(users):
        mine = got[np.asarray(users) == u]
        S = lists(int(u))
        assert not np.isin(mine, S).any(), (what, u)
        assert ((mine == -1).all() if len(S) == n_items else (mine >= 0).all()), (what, u)


# ---- 1. bit for bit against the restatement ---------------------------------------------------------------------------------
U1, I1 = 64, 300
EVERY, NONE, ALL_BUT_ONE, ONLY_FIRST, ONLY_LAST, LEFT = 5, 9, 12, 20, 33, 137


def _planted_pairs(rng):
    eu, ei = rng.integers(0, U1, 3000).astype(np.int32), rng.integers(0, I1, 3000).astype(np.int32)
    keep = ~np.isin(eu, (EVERY, NONE, ALL_BUT_ONE, ONLY_FIRST, ONLY_LAST))
    rest = np.setdiff1d(np.arange(I1), [LEFT])
    eu = np.concatenate([eu[keep], np.full(I1, EVERY), np.full(rest.size, ALL_BUT_ONE), [ONLY_FIRST, ONLY_LAST]]).astype(np.int32)
    ei = np.concatenate([ei[keep], np.arange(I1), rest, [0, I1 - 1]]).astype(np.int32)
    return eu, ei


@pytest.mark.parametrize("m", [1, 5])
def test_draws_are_the_restatements_bit_for_bit(mf, m):
    rng = np.random.default_rng(31 + m)
    eu, ei = _planted_pairs(rng)
    lists = IC.lists_of(eu, ei)
    users = rng.permutation(U1).astype(np.int32)
    users = np.append(users, users[3])  # every user, in any order, one of them twice
    with _handle(mf, U1, I1) as h:
        h.set_seen(eu, ei)
        for seed in (0, 1, -5, 1 << 40):
            for first in (0, 1 << 40):
                got = h.sample_unseen(users, m, seed, first)
                _check(got, lists, I1, users, m, seed, first, f"m {m} seed {seed} first {first}")
                assert (got[users == EVERY] == -1).all()
                assert (got[users == ALL_BUT_ONE] == LEFT).all()
                assert (got[users == ONLY_FIRST] >= 1).all() and (got[users == ONLY_LAST] <= I1 - 2).all()
        # a user without pairs draws t itself, over all the items
        c = np.flatnonzero(users == NONE)[:, None] * 40 + np.arange(40)
        assert np.array_equal(h.sample_unseen(users, 40, 7)[users == NONE],
                              ((IC.mix32(7, c) * np.uint64(I1)) >> np.uint64(32)).astype(np.int32))


# ---- 2. cutting the call changes nothing --------------------------------------------------------------------------------------
@pytest.mark.parametrize("m, n", [(1, CHUNK + 3), (3, CHUNK // 3 + 2)])
def test_a_call_longer_than_a_piece_and_its_slices(mf, m, n):
    """Rows go up in pieces of CHUNK // m whole rows: with m = 1 the last piece holds 3 rows, with m = 3 a piece ends one
    draw short of CHUNK and the last holds 2 rows."""
    U, I, seed, first = 8, 50, 11, 1 << 33
    rng = np.random.default_rng(m)
    eu, ei = rng.integers(0, U - 1, 150).astype(np.int32), rng.integers(0, I, 150).astype(np.int32)  # user 7 has no pairs
    lists = IC.lists_of(eu, ei)
    users = rng.integers(0, U, n).astype(np.int32)
    rows = CHUNK // m
    assert n > rows and (n - rows) * m < 8
    with _handle(mf, U, I) as h:
        h.set_seen(eu, ei)
        whole = h.sample_unseen(users, m, seed, first)
        assert np.array_equal(whole, IC.sample(lists, I, users, m, seed, first))
        assert not (whole == -1).any()
        for a, b in ((0, 7), (rows - 2, rows + 2), (rows, n), (n - 1, n), (1000, 1000), (5, rows + 1)):
            assert np.array_equal(h.sample_unseen(users[a:b], m, seed, first + a * m), whole[a:b]), (a, b)


def test_one_row_longer_than_a_piece_is_a_piece_of_its_own(mf):
    U, I, seed = 3, 20, 2
    eu, ei = np.array([0, 0, 1, 1], np.int32), np.array([0, 7, 19, 3], np.int32)
    lists = IC.lists_of(eu, ei)
    m = CHUNK + 5
    with _handle(mf, U, I) as h:
        h.set_seen(eu, ei)
        users = np.array([1, 0], np.int32)
        got = h.sample_unseen(users, m, seed)
        assert np.array_equal(got, IC.sample(lists, I, users, m, seed))


# ---- 3. a long list -----------------------------------------------------------------------------------------------------------
def test_a_user_who_has_seen_all_but_ten_of_seventy_thousand(mf):
    U, I = 3, 70_000
    rng = np.random.default_rng(3)
    left = np.sort(rng.choice(I, 10, replace=False))
    left[0], left[-1] = 0, I - 1  # both ends among them
    seen = np.setdiff1d(np.arange(I), left).astype(np.int32)
    eu = np.concatenate([np.zeros(seen.size, np.int32), [1]]).astype(np.int32)
    ei = np.concatenate([seen, [41_234]]).astype(np.int32)
    lists = IC.lists_of(eu, ei)
    with _handle(mf, U, I) as h:
        h.set_seen(eu, ei)
        for users, m in ((np.zeros(1, np.int32), 1000), (np.array([1, 0] * 125, np.int32), 4), (np.array([2, 1, 0], np.int32), 333)):
            got = h.sample_unseen(users, m, seed=9, first=17)
            _check(got, lists, I, users, m, 9, 17)
            if m == 1000:
                assert np.array_equal(np.unique(got), left)  # 1 000 draws over 10 items: all of them
            assert np.isin(got[users == 0], left).all() and not (got[users == 1] == 41_234).any()


# ---- 4. the index moves, the draws follow -------------------------------------------------------------------------------------
def test_the_draws_follow_the_index(mf):
    U, I, m, seed = 6, 20, 64, 4
    rng = np.random.default_rng(8)
    full = 2
    eu, ei = rng.integers(0, U, 40).astype(np.int32), rng.integers(0, I, 40).astype(np.int32)
    eu, ei = np.concatenate([eu, np.full(I, full)]).astype(np.int32), np.concatenate([ei, np.arange(I)]).astype(np.int32)
    with _handle(mf, U, I) as h:
        h.init_factors()
        users = np.arange(U, dtype=np.int32)
        h.set_seen(eu, ei)
        _check(h.sample_unseen(users, m, seed), IC.lists_of(eu, ei), I, users, m, seed, 0, "set_seen")
        # mark_seen: what is newly seen is never drawn again
        before = h.sample_unseen(users, m, seed)
        nu, ni = np.repeat(users, m)[before.ravel() >= 0][::9], before.ravel()[before.ravel() >= 0][::9]
        h.mark_seen(nu, ni)
        eu, ei = np.concatenate([eu, nu]), np.concatenate([ei, ni])
        got = h.sample_unseen(users, m, seed)
        _check(got, IC.lists_of(eu, ei), I, users, m, seed, 0, "mark_seen")
        assert not np.isin((np.repeat(users, m).astype(np.int64) << 32) | got.ravel(), (nu.astype(np.int64) << 32) | ni).any()
        # add_items: the new indices are unseen by everybody, and all the user who had seen everything can get
        assert h.add_items(n=5) == I
        got = h.sample_unseen(users, m, seed)
        _check(got, IC.lists_of(eu, ei), I + 5, users, m, seed, 0, "add_items")
        assert (got[full] >= I).all() and (got >= I).any(axis=1).all()
        # add_users: the new users draw t itself
        assert h.add_users(n=2) == U
        users = np.arange(U + 2, dtype=np.int32)[::-1].copy()
        got = h.sample_unseen(users, m, seed)
        _check(got, IC.lists_of(eu, ei), I + 5, users, m, seed, 0, "add_users")
        t = (IC.mix32(seed, np.arange(2 * m).reshape(2, m)) * np.uint64(I + 5)) >> np.uint64(32)
        assert np.array_equal(got[:2], t.astype(np.int32))
        # reserve: other tables, the same draws -- and users appended inside the capacity
        h.reserve(users=50, items=60)
        assert np.array_equal(h.sample_unseen(users, m, seed), got)
        assert h.add_users(n=3) == U + 2
        users = np.arange(U + 5, dtype=np.int32)
        _check(h.sample_unseen(users, m, seed), IC.lists_of(eu, ei), I + 5, users, m, seed, 0, "reserve")
        # clear_seen: no index, no draws
        h.clear_seen()
        with pytest.raises(mf.MfsgdError) as e:
            h.sample_unseen(users, m, seed)
        assert e.value.code == STATE and "sample_unseen: no seen set" in str(e.value)
        # an empty index: t itself for everybody
        h.set_seen([], [])
        t = (IC.mix32(seed, np.arange(users.size * m).reshape(-1, m)) * np.uint64(I + 5)) >> np.uint64(32)
        assert np.array_equal(h.sample_unseen(users, m, seed), t.astype(np.int32))


# ---- 5. nothing is kept or changed --------------------------------------------------------------------------------------------
def test_a_call_keeps_no_device_memory_and_changes_neither_index_nor_model(mf):
    U, I = 40, 90
    rng = np.random.default_rng(12)
    eu, ei = rng.integers(0, U, 900).astype(np.int32), rng.integers(0, I, 900).astype(np.int32)
    users = rng.integers(0, U, 5000).astype(np.int32)
    with _handle(mf, U, I) as h:  # an index, but neither factors nor ratings
        h.set_seen(eu, ei)
        live = mf.debug_device_bytes()
        got = h.sample_unseen(users, 3, 5)
        assert mf.debug_device_bytes() == live
        assert np.array_equal(got, IC.sample(IC.lists_of(eu, ei), I, users, 3, 5))
        with pytest.raises(mf.MfsgdError):  # a refused call holds nothing either
            h.sample_unseen([0, U], 3, 5)
        assert mf.debug_device_bytes() == live
        h.init_factors()
        h.set_ratings(eu, ei, rng.random(eu.size, dtype=np.float32))
        h.fit(1)
        P, Q = h.get_factors()
        ptr, items = h.seen(np.arange(U))
        live = mf.debug_device_bytes()
        assert np.array_equal(h.sample_unseen(users, 3, 5), got)
        assert mf.debug_device_bytes() == live
        P2, Q2 = h.get_factors()
        assert np.array_equal(P.view(np.uint32), P2.view(np.uint32)) and np.array_equal(Q.view(np.uint32), Q2.view(np.uint32))
        ptr2, items2 = h.seen(np.arange(U))
        assert np.array_equal(ptr, ptr2) and np.array_equal(items, items2)
        assert h.debug_counters()["schedule_builds"] == 1


# ---- 6. fit_implicit is the sequence it is documented as -----------------------------------------------------------------------
def _bits(m):
    P, Q = m.get_factors()
    return P.view(np.uint32).copy(), Q.view(np.uint32).copy()


def _same_model(a, b):
    return all(np.array_equal(x, y) for x, y in zip(_bits(a), _bits(b)))


@pytest.mark.parametrize("k", [8, 20])
def test_fit_implicit_is_its_documented_sequence(mf, k):
    U, I, neg, epochs, seed, full = 60, 50, 3, 3, 21, 17
    rng = np.random.default_rng(k)
    pu, pi = rng.integers(0, U, 400).astype(np.int32), rng.integers(0, I, 400).astype(np.int32)  # duplicates among them
    pu, pi = np.concatenate([pu, np.full(I, full)]).astype(np.int32), np.concatenate([pi, np.arange(I)]).astype(np.int32)
    order = rng.permutation(pu.size)
    pu, pi = pu[order], pi[order]
    n = pu.size
    # held-out pairs that are no positives
    hu, hi = rng.integers(0, U, 200).astype(np.int32), rng.integers(0, I, 200).astype(np.int32)
    fresh = ~np.isin((hu.astype(np.int64) << 32) | hi, (pu.astype(np.int64) << 32) | pi)
    hu, hi = hu[fresh], hi[fresh]
    for held in (False, True):
        with _handle(mf, U, I, k, lr=0.05) as a, _handle(mf, U, I, k, lr=0.05) as b, _handle(mf, U, I, k, lr=0.05) as c:
            if held:  # the index also holds the held-out pairs: every handle gets it first
                for h in (a, b, c):
                    h.set_seen(np.concatenate([pu, hu]), np.concatenate([pi, hi]))
            builds = a.debug_counters()["schedule_builds"]
            rmse = a.fit_implicit(pu, pi, epochs, neg, seed=seed, pos=1.0, neg=0.25)
            assert rmse.shape == (epochs,) and rmse.dtype == np.float64
            assert a.debug_counters()["schedule_builds"] == builds + epochs
            if held:
                assert a.seen_size() == np.unique((np.concatenate([pu, hu]).astype(np.int64) << 32) | np.concatenate([pi, hi])).size
            else:  # a handle without an index got one: the distinct positives
                ptr, items = a.seen(np.arange(U))
                keys = np.unique((pu.astype(np.int64) << 32) | pi)
                assert np.array_equal(items, (keys & 0xFFFFFFFF).astype(np.int32))
                assert np.array_equal(ptr, np.searchsorted(keys >> 32, np.arange(U + 1)))
                b.set_seen(pu, pi)
            # the same steps written out
            b.init_factors()
            want = []
            for e in range(epochs):
                J = b.sample_unseen(pu, neg, seed, first=e * n * neg)
                assert (J[pu == full] == -1).all() and (J[pu != full] >= 0).all()
                if held:
                    assert not np.isin((np.repeat(pu, neg).astype(np.int64) << 32) | J.ravel(), (hu.astype(np.int64) << 32) | hi).any()
                keep = J.ravel() >= 0
                ju, ji = np.repeat(pu, neg)[keep], J.ravel()[keep]
                b.set_ratings(np.concatenate([pu, ju]), np.concatenate([pi, ji]),
                              np.concatenate([np.full(n, 1.0, np.float32), np.full(ji.size, 0.25, np.float32)]))
                want.append(b.fit(1)[0])
            assert np.array_equal(rmse.view(np.uint64), np.array(want).view(np.uint64))
            assert _same_model(a, b)
            assert a.schedule_info()["nnz"] == n + ji.size == b.schedule_info()["nnz"]  # the last epoch's set stays
            # two epochs and then the third: the same bits
            first = c.fit_implicit(pu, pi, 2, neg, seed=seed, neg=0.25)
            last = c.fit_implicit(pu, pi, 1, neg, seed=seed, neg=0.25, first_epoch=2)
            assert np.array_equal(np.concatenate([first, last]).view(np.uint64), rmse.view(np.uint64))
            assert _same_model(a, c)
            assert c.fit_implicit(pu, pi, 1, neg, seed=seed, first_epoch=3, rmse=False) is None


def test_fit_implicit_without_negatives_is_train_on_the_positives(mf):
    U, I, k = 30, 25, 8
    rng = np.random.default_rng(2)
    pu, pi = rng.integers(0, U, 200).astype(np.int32), rng.integers(0, I, 200).astype(np.int32)
    with _handle(mf, U, I, k) as a, _handle(mf, U, I, k) as b:
        rmse = a.fit_implicit(pu, pi, 4, negatives=0, pos=2.0)
        want = b.train(pu, pi, np.full(pu.size, 2.0, np.float32), 4)
        assert np.array_equal(rmse.view(np.uint64), want.view(np.uint64)) and _same_model(a, b)
        assert a.debug_counters()["schedule_builds"] == 1 and a.seen_size() == np.unique((pu.astype(np.int64) << 32) | pi).size


# ---- 7. it learns ---------------------------------------------------------------------------------------------------------------
def test_negatives_make_a_planted_one_class_problem_learnable(mf):
    """600 users, 400 items in 20 groups of 20; a user's 12 positives lie in the user's group, 11 to train on and 1 held
    out; k = 16, lambda = 0.01, lr = 0.05, 20 epochs.  Chance for the held-out item among the 389 unseen ones is 10 / 389
    = 0.026 at a cut-off of 10.  A plain sequential SGD in numpy gave 0.023 untrained, 0.035 to 0.04 on the positives
    alone and 1.0 with 4 negatives per positive; the library orders the ratings differently, so the bounds are wide: both
    baselines below 0.1 (about 4 x chance), the implicit model above 0.5 (half of what the restatement reached).
    Measured on an MI355X: untrained 0.02, positives alone 0.0333, 4 negatives 1.0."""
    U, I, G, k, lr, lam, seed = 600, 400, 20, 16, 0.05, 0.01, 3
    rng = np.random.default_rng(0)
    per = I // G
    its = np.stack([(u % G) * per + rng.choice(per, 12, replace=False) for u in range(U)]).astype(np.int32)
    hu, hi = np.arange(U, dtype=np.int32), its[:, 0].copy()
    pu, pi = np.repeat(hu, 11), its[:, 1:].ravel().copy()
    rate = {}
    for name, negatives in (("untrained", None), ("positives alone", 0), ("4 negatives", 4)):
        with _handle(mf, U, I, k, lr=lr, lam=lam, seed=seed) as h:
            h.set_seen(np.concatenate([pu, hu]), np.concatenate([pi, hi]))  # held-out positives are never negatives
            h.init_factors()
            if negatives is not None:
                h.fit_implicit(pu, pi, 20, negatives, seed=seed, rmse=False)
            rate[name] = h.evaluate_ranking(hu, hi, 10, exclude="seen")["hit_rate"]
    print("held-out hit rate at 10:", {name: round(v, 4) for name, v in rate.items()})
    assert rate["untrained"] < 0.1 and rate["positives alone"] < 0.1
    assert rate["4 negatives"] > 0.5
