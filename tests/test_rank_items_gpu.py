"""rank_items / rank_items_rows / evaluate_ranking -- mfsgd_rank_items and its kin -- against the CPU oracle: the
oracle's predictions of every item for the user, the excluded items dropped except the held-out one, and the rank is
#{j : s_j > s_t, or (s_j == s_t and j < t)}.  Ranks are integers and compared exactly."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LR, LAM = 0.01, 0.05
CAP = 512  # thresholds the kernel's on-chip table holds per user and round (csrc/rank.hip: kRankCap)


def _scores(oracle, P, Q, user):
    I = Q.shape[0]
    return oracle.predict(P, Q, np.full(I, user, np.int32), np.arange(I, dtype=np.int32))


def _ranks_ref(oracle, P, Q, u, i, eu, ei):
    """The rank of every pair by the definition; for a user with many pairs the same count taken from one sort of the
    user's items (position among all items minus the excluded ones ahead), checked against the definition on a few."""
    I = Q.shape[0]
    allitems = np.arange(I, dtype=np.int32)
    u, i = np.asarray(u, np.int32), np.asarray(i, np.int32)
    out = np.full(u.size, -1, np.int32)

    def by_definition(sc, excl, t):
        keep = ~excl
        keep[t] = True
        before = (sc > sc[t]) | ((sc == sc[t]) & (allitems < t))
        return np.count_nonzero(before & keep)

    for user in np.unique(u):
        sc = _scores(oracle, P, Q, user)
        assert not np.isnan(sc).any()
        excl = np.zeros(I, bool)
        excl[ei[eu == user]] = True
        mine = np.flatnonzero(u == user)
        if mine.size <= 64:
            for x in mine:
                out[x] = by_definition(sc, excl, i[x])
            continue
        order = np.lexsort((allitems, -sc.astype(np.float64)))  # best first, ties by the smaller item
        pos = np.empty(I, np.int64)
        pos[order] = np.arange(I)
        ahead = np.cumsum(excl[order]) - excl[order]  # excluded items strictly before each place
        out[mine] = pos[i[mine]] - ahead[pos[i[mine]]]
        for x in mine[:: max(1, mine.size // 16)]:
            assert out[x] == by_definition(sc, excl, i[x])
    return out


def _factors(I, topn, k):
    """The factors of test_recommend_excluding_matches_sorted_predictions: a third of Q alike, zero scores (all +0.0:
    the one -0.0 entry sums with +0.0 products; real -0.0 scores are in tests/test_serving_edges_gpu.py), a user (7)
    with an all-positive row."""
    rng = np.random.default_rng(I + topn)
    U = 40
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    Q[rng.integers(0, I, I // 3)] = Q[3 % I]
    if I > 100:
        Q[50:60] = 0.0
        Q[55, 0] = -0.0
        P[7] = np.abs(P[7])
        Q[60:5000:7] = -np.abs(Q[60:5000:7])
    return rng, P, Q


class _Pairs:
    def __init__(self):
        self.u, self.i = [], []

    def add(self, user, items):
        items = np.asarray(items, np.int32).ravel()
        self.u.append(np.full(items.size, user, np.int32))
        self.i.append(items)

    def arrays(self, rng=None, dup=False):
        u, i = np.concatenate(self.u), np.concatenate(self.i)
        if dup:
            d = rng.integers(0, u.size, max(1, u.size // 4))
            u, i = np.concatenate([u, u[d]]), np.concatenate([i, i[d]])
        if rng is not None:
            perm = rng.permutation(u.size)
            u, i = u[perm], i[perm]
        return u, i


def _case(oracle, I, k):
    """Held-out pairs of 7 distinct users and the exclusion pairs, both shuffled."""
    rng, P, Q = _factors(I, 10, k)
    U = P.shape[0]
    allitems = np.arange(I, dtype=np.int32)
    held, excl = _Pairs(), _Pairs()
    n_big = min(I, 5000)
    assert n_big > CAP or I < CAP  # the user below needs several rounds of the table wherever the catalogue allows
    # user 0: one pair, no exclusions
    held.add(0, rng.integers(0, I, 1))
    # user 7 (all-positive scores where I > 100): asked for twice with different items, and a pair given twice
    a, b = rng.choice(I, 2, replace=False)
    held.add(7, [a, b, a])
    excl.add(7, rng.choice(I, max(1, I // 50), replace=False))
    # user 13: its own top-1 and its last item
    s13 = _scores(oracle, P, Q, 13)
    order13 = np.lexsort((allitems, -s13.astype(np.float64)))
    held.add(13, [order13[0], order13[-1]])
    excl.add(13, order13[1:4])
    # user 3: members of the big tie group (a third of Q is one row), some of them excluded, one of those held out too
    s3 = _scores(oracle, P, Q, 3)
    tied = allitems[s3 == s3[3 % I]]
    assert tied.size >= 2 or I < 100
    held.add(3, tied[:6])
    excl.add(3, tied[1::2])
    if I > 100:  # the zero scores tie as well
        zeros = allitems[50:60]
        held.add(3, zeros[[0, 5, 9]])
        excl.add(3, zeros[[5, 6]])
    # user 21: more held-out items than the on-chip table holds
    held.add(21, rng.choice(I, n_big, replace=False))
    excl.add(21, rng.choice(I, max(1, I // 7), replace=False))
    # user 22: every item excluded -- each held-out item is alone, rank 0
    held.add(22, rng.choice(I, min(I, 5), replace=False))
    excl.add(22, allitems)
    # user 24: a tenth of the catalogue excluded, its held-out item among it
    tenth = rng.choice(I, max(1, I // 10), replace=False)
    held.add(24, tenth[:1])
    excl.add(24, tenth)
    # users nobody asks about
    excl.add(5, rng.integers(0, I, 300))
    excl.add(U - 2, allitems)
    u, i = held.arrays(rng)
    eu, ei = excl.arrays(rng, dup=True)
    assert np.unique(u).size == 7
    return rng, P, Q, u, i, eu, ei


@pytest.mark.parametrize("I,k", [(5, 16), (700, 3), (700, 8), (30000, 64), (9000, 256)])
def test_rank_items_matches_the_oracle(mf, oracle, I, k):
    rng, P, Q, u, i, eu, ei = _case(oracle, I, k)
    U = P.shape[0]
    # 37 distinct users with one or two pairs each, and one user alone: no count is a multiple of the users a
    # workgroup takes
    many_u = np.concatenate([np.arange(37), np.arange(0, 37, 5)]).astype(np.int32)
    many_i = rng.integers(0, I, many_u.size).astype(np.int32)
    perm = rng.permutation(many_u.size)
    many_u, many_i = many_u[perm], many_i[perm]
    one = u == 7
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        m.predict([0], [0])  # (the factors go to the device with the first call that needs them, and stay)
        before = mf.debug_device_bytes()
        got = m.rank_items(u, i, exclude=(eu, ei))
        got_many = m.rank_items(many_u, many_i, exclude=(eu, ei))
        got_one = m.rank_items(u[one], i[one], exclude=(eu, ei))
        got_plain = m.rank_items(u, i)
        got_empty = m.rank_items(u, i, exclude=(np.empty(0, np.int32), np.empty(0, np.int32)))
        other = np.isin(eu, u, invert=True)  # pairs of users nobody asks about only
        got_other = m.rank_items(u, i, exclude=(eu[other], ei[other]))
        assert mf.debug_device_bytes() == before
        P1, Q1 = m.get_factors()
    assert got.dtype == np.int32 and got.shape == u.shape
    np.testing.assert_array_equal(got, _ranks_ref(oracle, P, Q, u, i, eu, ei))
    np.testing.assert_array_equal(got_many, _ranks_ref(oracle, P, Q, many_u, many_i, eu, ei))
    np.testing.assert_array_equal(got_one, got[one])
    none = np.empty(0, np.int32)
    np.testing.assert_array_equal(got_plain, _ranks_ref(oracle, P, Q, u, i, none, none))
    np.testing.assert_array_equal(got_empty, got_plain)
    np.testing.assert_array_equal(got_other, got_plain)
    assert (got[u == 22] == 0).all()
    sel = np.flatnonzero(u == 7)
    dup = [x for x in sel if np.count_nonzero(i[sel] == i[x]) == 2]
    assert len(dup) == 2 and got[dup[0]] == got[dup[1]]
    assert P1.tobytes() == P.tobytes() and Q1.tobytes() == Q.tobytes()


def test_rank_is_the_place_in_the_shipped_ranking(mf, oracle):
    I, k = 700, 8
    rng, P, Q, u, i, eu, ei = _case(oracle, I, k)
    users = np.unique(u)
    with mf.MatrixFactorizationSGD(P.shape[0], I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        ranks = m.rank_items(u, i, exclude=(eu, ei))
        lists, _ = m.recommend(users, I, exclude=(eu, ei))
        plain = m.rank_items(u, i, exclude=None)
        empty = m.rank_items(u, i, exclude=(np.empty(0, np.int32), np.empty(0, np.int32)))
        plain_lists, _ = m.recommend(users, I)
    excluded = set(zip(eu.tolist(), ei.tolist()))
    checked = 0
    for x in range(u.size):
        row = int(np.searchsorted(users, u[x]))
        assert plain_lists[row, plain[x]] == i[x]
        if (int(u[x]), int(i[x])) in excluded:
            continue
        assert lists[row, ranks[x]] == i[x]
        checked += 1
    assert checked > 600
    np.testing.assert_array_equal(plain, empty)


@pytest.mark.parametrize("I,k", [(700, 8), (30000, 64)])
def test_rank_items_rows_of_p_equals_rank_items(mf, oracle, I, k):
    rng, P, Q, u, i, eu, ei = _case(oracle, I, k)
    sel = rng.permutation(np.unique(u)).astype(np.int32)  # the rows handed over: the users asked about, in another order
    row_of_user = np.full(P.shape[0], -1, np.int32)
    row_of_user[sel] = np.arange(sel.size, dtype=np.int32)
    mine = row_of_user[eu] >= 0  # (pairs of other users have no row to name)
    with mf.MatrixFactorizationSGD(P.shape[0], I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        want = m.rank_items(u, i, exclude=(eu, ei))
        got = m.rank_items_rows(P[sel], row_of_user[u], i, exclude=(row_of_user[eu[mine]], ei[mine]))
        want_plain = m.rank_items(u, i)
        got_plain = m.rank_items_rows(P[sel], row_of_user[u], i)
    np.testing.assert_array_equal(got, want)
    np.testing.assert_array_equal(got_plain, want_plain)


def test_rank_items_rows_of_folded_users_matches_the_oracle(mf, oracle):
    w = mf.synth.workload("cfg1_ml100k", scale=0.2)
    rng = np.random.default_rng(4)
    I, k, n_new = w["I"], w["k"], 20
    lens = rng.integers(0, 60, n_new)
    lens[0] = 0
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    rated = np.concatenate([rng.choice(I, n, replace=False) for n in lens]).astype(np.int32)
    ratings = rng.uniform(0.5, 5.0, rated.size).astype(np.float32)
    er = np.repeat(np.arange(n_new, dtype=np.int32), lens).astype(np.int32)
    row = np.repeat(np.arange(n_new, dtype=np.int32), 3)
    items = rng.integers(0, I, row.size).astype(np.int32)
    items[:6] = rated[-6:]  # (some held-out items that another row rated)
    with mf.MatrixFactorizationSGD(w["U"], I, k, LR, LAM, 7) as m:
        m.train(w["u"], w["i"], w["r"], 1)
        _, Q = m.get_factors()
        rows = m.fold_in(row_ptr, rated, ratings, 3)
        got = m.rank_items_rows(rows, row, items, exclude=(er, rated))
    np.testing.assert_array_equal(got, _ranks_ref(oracle, rows, Q, row, items, er, rated))


def test_evaluate_ranking_end_to_end(mf, oracle):
    from tests.test_rank_items_cpu import FIELDS, _assert_metrics, _metrics_ref

    w = mf.synth.workload("cfg1_ml100k", scale=0.2)
    u, i, r = w["u"].astype(np.int32), w["i"].astype(np.int32), w["r"]
    # distinct (user, item) pairs: the metrics mean nothing otherwise
    _, first = np.unique(u.astype(np.int64) * w["I"] + i, return_index=True)
    u, i, r = u[np.sort(first)], i[np.sort(first)], r[np.sort(first)]
    perm = np.random.default_rng(10).permutation(u.size)
    cut = u.size * 9 // 10
    tr, te = perm[:cut], perm[cut:]
    with mf.MatrixFactorizationSGD(w["U"], w["I"], w["k"], LR, LAM, 7) as m:
        m.train(u[tr], i[tr], r[tr], 2)
        P0, Q0 = m.get_factors()
        before = mf.debug_device_bytes()
        res = m.evaluate_ranking(u[te], i[te], 10, exclude=(u[tr], i[tr]))
        assert mf.debug_device_bytes() == before
        ranks = m.rank_items(u[te], i[te], exclude=(u[tr], i[tr]))
        P1, Q1 = m.get_factors()
    np.testing.assert_array_equal(res["ranks"], ranks)
    np.testing.assert_array_equal(ranks, _ranks_ref(oracle, P0, Q0, u[te], i[te], u[tr], i[tr]))
    again = mf.ranking_metrics(u[te], ranks, 10)
    for f in ("n_pairs", "n_users") + FIELDS:
        assert res[f] == again[f], f
    _assert_metrics(res, _metrics_ref(u[te], ranks, 10))
    assert res["n_pairs"] == te.size and res["n_users"] == np.unique(u[te]).size
    assert P0.tobytes() == P1.tobytes() and Q0.tobytes() == Q1.tobytes()
