"""recommend_users(items, topn, ...) -- mfsgd_recommend_users and its kin, top-N users for items -- against numpy over the
oracle, as tests/test_recommend_exclude_gpu.py does for the other side: per requested item the oracle's prediction of
every user with that item, the excluded users dropped (and those outside the candidates), sorted by score descending then
user ascending, cut at topn and padded with user -1 / score NaN.  Everything is compared bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LR, LAM = 0.01, 0.05
NONE = np.empty(0, np.int32)


def _expected(oracle, P, Q, items, topn, eu=NONE, ei=NONE, cands=None):
    """cands: None, or one array of users per request row."""
    U = P.shape[0]
    allusers = np.arange(U, dtype=np.int32)
    users = np.full((len(items), topn), -1, np.int32)
    scores = np.full((len(items), topn), np.nan, np.float32)
    for row, j in enumerate(items):
        sc = oracle.predict(P, Q, allusers, np.full(U, j, np.int32))
        keep = np.ones(U, bool)
        keep[eu[ei == j]] = False
        if cands is not None:
            among = np.zeros(U, bool)
            among[np.asarray(cands[row], np.int64)] = True
            keep &= among
        us = allusers[keep]
        order = us[np.lexsort((us, -sc[keep].astype(np.float64)))][:topn]
        users[row, :order.size] = order
        scores[row, :order.size] = sc[order]
    return users, scores


def _same(got, want, what=""):
    assert got[0].tobytes() == want[0].tobytes(), what
    assert got[1].tobytes() == want[1].tobytes(), what  # bit for bit, -0.0 and the NaN of the padding included


def _factors(U, topn, k):
    """What test_recommend_exclude_gpu's _factors carries, on the other side: a third of P's rows alike, a run of zero
    rows with one -0.0 entry (zero scores, all +0.0), and, for item 0, the alike rows as one tie group that scores above
    nearly everyone, so that it straddles the selection threshold."""
    rng = np.random.default_rng(U + topn)
    I = 40
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    P[rng.integers(0, U, U // 3)] = P[3 % U]
    if U > 100:
        P[50:60] = 0.0
        P[55, 0] = -0.0
        Q[7] = np.abs(Q[7])
        P[60:5000:7] = -np.abs(P[60:5000:7])
        Q[0] = P[3]
    return rng, P, Q


@pytest.mark.parametrize("U,topn,k", [(30000, 10, 64), (61000, 40, 32), (700, 128, 8), (700, 129, 8), (5, 5, 16)])
def test_recommend_users_matches_sorted_predictions(mf, oracle, U, topn, k):
    rng, P, Q = _factors(U, topn, k)
    I = Q.shape[0]
    items = np.array([0, 7, 7, I - 1, 13, 21], np.int32)  # 7 twice: one list for both rows
    plain = _expected(oracle, P, Q, items, topn)
    pu, pi = [], []

    def add(users, j):
        users = np.asarray(users, np.int32).ravel()
        pu.append(users)
        pi.append(np.full(users.size, j, np.int32))

    for row, j in enumerate(items):
        add(plain[0][row, :1], j)  # every row's current top-1
    # part of the tie group at item 0's selection threshold (every other member, so that the group still straddles it)
    allusers = np.arange(U, dtype=np.int32)
    s0 = oracle.predict(P, Q, allusers, np.zeros(U, np.int32))
    tied = allusers[s0 == s0[plain[0][0, -1]]]
    if U > 100:
        below = int((s0 > s0[tied[0]]).sum())
        assert below < topn < below + tied.size  # the group does straddle the threshold
    add(tied[::2], 0)
    # item 13: a tenth of the users, spread over every tile; item 7: a few from its ranking
    add(rng.choice(U, max(1, U // 10), replace=False), 13)
    add(plain[0][1, 1:topn:3], 7)
    # item 21: every user (the whole row is padded); item I - 1: all but topn // 2 (a partly padded row)
    add(allusers, 21)
    add(rng.permutation(U)[topn // 2:], I - 1)
    # items nobody asked about
    add(rng.integers(0, U, 300), 5)
    add(allusers, I - 2)
    eu, ei = np.concatenate(pu), np.concatenate(pi)
    dup = rng.integers(0, eu.size, eu.size // 4)  # duplicate pairs
    eu, ei = np.concatenate([eu, eu[dup]]), np.concatenate([ei, ei[dup]])
    perm = rng.permutation(eu.size)
    eu, ei = eu[perm], ei[perm]

    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        got = m.recommend_users(items, topn, exclude=(eu, ei))
        base = m.recommend_users(items, topn)
        none = m.recommend_users(items, topn, exclude=(NONE, NONE))
        other = np.isin(ei, items, invert=True)  # pairs of items that are not requested only: nothing is excluded
        oth = m.recommend_users(items, topn, exclude=(eu[other], ei[other]))
        with pytest.raises(mf.MfsgdError, match="topn exceeds the number of users"):
            m.recommend_users(items, U + 1, exclude=(eu, ei))
        there = got[0] >= 0
        pred = m.predict(got[0][there], np.repeat(items, topn).reshape(got[0].shape)[there])

    want = _expected(oracle, P, Q, items, topn, eu, ei)
    _same(got, want)
    assert (got[0][list(items).index(21)] == -1).all()
    assert (got[0][3, topn // 2:] == -1).all()
    _same(base, plain)
    _same(none, base, "empty pairs")
    _same(oth, base, "pairs of unrequested items")
    assert pred.tobytes() == got[1][there].tobytes()


def _index_pairs(rng, U, I):
    """Pairs for an index: users 0, 1500 and U - 1 without any, item 9 seen by nobody, user 77 with every other item, item 5
    seen by every other user, and duplicates.  (A user with EVERY item and an item nobody has seen cannot be in one index,
    nor an item EVERY user has seen and a user without a list: the test's mark_seen step completes user 77 and item 5.)"""
    u = rng.integers(0, U, 8 * U).astype(np.int32)
    i = rng.integers(0, I, 8 * U).astype(np.int32)
    u = np.concatenate([u, np.full(I, 77, np.int32), np.arange(U, dtype=np.int32)])
    i = np.concatenate([i, np.arange(I, dtype=np.int32), np.full(U, 5, np.int32)])
    keep = np.isin(u, [0, 1500, U - 1], invert=True) & (i != 9)
    u, i = u[keep], i[keep]
    dup = rng.integers(0, u.size, u.size // 5)
    return np.concatenate([u, u[dup]]), np.concatenate([i, i[dup]])


def test_exclude_seen_is_the_pair_call(mf, oracle):
    U, I, k, topn = 3000, 50, 16, 20
    rng = np.random.default_rng(5)
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    su, si = _index_pairs(rng, U, I)
    assert not np.isin([0, 1500, U - 1], su).any() and not (si == 9).any()
    assert np.unique(su[si == 5]).size == U - 3 and np.unique(si[su == 77]).size == I - 1

    def check(m, su, si, what):
        Pn, Qn = m.get_factors()
        items = np.arange(Qn.shape[0], dtype=np.int32)
        seen = m.recommend_users(items, topn, exclude="seen")
        _same(seen, m.recommend_users(items, topn, exclude=(su, si)), what + ": the pair call")
        _same(seen, _expected(oracle, Pn, Qn, items, topn, su, si), what + ": numpy")
        return seen

    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        with pytest.raises(mf.MfsgdError, match="recommend_users_unseen: no seen set"):
            m.recommend_users([0], topn, exclude="seen")
        m.set_seen(NONE, NONE)  # an empty index excludes nothing
        _same(m.recommend_users(np.arange(I), topn, exclude="seen"), m.recommend_users(np.arange(I), topn), "empty index")
        m.set_seen(su, si)
        seen = check(m, su, si, "set_seen")
        # item 5: the three users without a list are all that is left; item 9: the unrestricted row
        assert sorted(seen[0][5, :3].tolist()) == [0, 1500, U - 1] and (seen[0][5, 3:] == -1).all()
        assert seen[0][9].tobytes() == m.recommend_users([9], topn)[0].tobytes()
        # a merge of further pairs: now user 77 has seen every item, and every user item 5 (its row is all padding)
        mu = np.concatenate([rng.integers(0, U, 4000), [77, 0, 1500, U - 1]]).astype(np.int32)
        mi = np.concatenate([rng.integers(0, I, 4000), [9, 5, 5, 5]]).astype(np.int32)
        m.mark_seen(mu, mi)
        su, si = np.concatenate([su, mu]), np.concatenate([si, mi])
        seen = check(m, su, si, "mark_seen")
        assert (seen[0][5] == -1).all() and np.isnan(seen[1][5]).all() and 77 not in seen[0]
        # new users inside a reserved capacity: eligible, their lists empty
        m.reserve(users=U + 64)
        assert m.add_users(n=10) == U
        seen = check(m, su, si, "add_users")
        assert sorted(seen[0][5, :10].tolist()) == list(range(U, U + 10)) and (seen[0][5, 10:] == -1).all()
        # a new item: its row excludes nobody
        assert m.add_items(n=1) == I
        seen = check(m, su, si, "add_items")
        assert seen[0][I].tobytes() == m.recommend_users([I], topn)[0].tobytes()
        # ... until a pair names it, for one of the new users
        m.mark_seen([U + 3], [I])
        su, si = np.concatenate([su, [U + 3]]).astype(np.int32), np.concatenate([si, [I]]).astype(np.int32)
        seen = check(m, su, si, "a pair of a new user and the new item")
        assert U + 3 not in seen[0][I]


def test_an_index_longer_than_one_pass_of_the_launch(mf):
    """17 pairs for each of 70000 users: 1 190 000 pairs, more than the 4096 x 256 threads of one pass over the index."""
    U, I, k, per = 70000, 40, 8, 17
    rng = np.random.default_rng(11)
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    start, step = rng.integers(0, I, U), rng.choice([1, 3, 7, 9, 11, 13], U)  # (coprime to 40: 17 distinct items each)
    si = ((start[:, None] + step[:, None] * np.arange(per)[None, :]) % I).astype(np.int32).ravel()
    su = np.repeat(np.arange(U, dtype=np.int32), per)
    assert su.size > 4096 * 256
    items = np.arange(I, dtype=np.int32)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        m.set_seen(su, si)
        assert m.seen_size() == su.size
        seen = m.recommend_users(items, 10, exclude="seen")
        _same(seen, m.recommend_users(items, 10, exclude=(su, si)))
        # the last users of the index, whom only the second pass reaches, are left out where they should be
        tail = np.arange(U - 2000, U)
        got = m.recommend_users(items, 10, exclude="seen", candidates=tail)
        _same(got, m.recommend_users(items, 10, exclude=(su, si), candidates=tail))
        mask = np.zeros((U, I), bool)
        mask[su, si] = True
        rows = np.repeat(items, 10).reshape(I, 10)
        assert (got[0] >= U - 2000).all() and not mask[got[0], rows].any()


def test_candidates(mf, oracle):
    U, I, k, topn = 2000, 30, 16, 12
    rng = np.random.default_rng(21)
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    P[rng.integers(0, U, U // 4)] = P[1]  # ties, which go to the smaller user whatever the list's order
    items = np.array([4, 9, 9, 0, 29], np.int32)  # 9 twice, with two different lists
    shared = rng.integers(0, U, 500).astype(np.int32)  # unsorted, with repeats
    per_row = [rng.integers(0, U, 300), rng.permutation(U)[:40], np.array([7, 7, 7, 3, 1999, 3]), NONE, rng.integers(0, U, 5)]
    per_row = [np.asarray(c, np.int32) for c in per_row]
    ptr = np.concatenate([[0], np.cumsum([c.size for c in per_row])]).astype(np.int64)
    eu = rng.integers(0, U, 6000).astype(np.int32)
    ei = rng.integers(0, I, 6000).astype(np.int32)
    eu, ei = np.concatenate([eu, shared[:100], per_row[1][:10]]), np.concatenate([ei, np.full(100, 4, np.int32), np.full(10, 9, np.int32)])
    su, si = rng.integers(0, U, 9000).astype(np.int32), rng.integers(0, I, 9000).astype(np.int32)
    su, si = np.concatenate([su, shared[100:250]]), np.concatenate([si, np.full(150, 9, np.int32)])
    everyone = rng.permutation(U).astype(np.int32)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        m.set_seen(su, si)
        _same(m.recommend_users(items, topn, candidates=shared), _expected(oracle, P, Q, items, topn, cands=[shared] * 5), "shared")
        want = _expected(oracle, P, Q, items, topn, cands=per_row)
        _same(m.recommend_users(items, topn, candidates=(ptr, np.concatenate(per_row))), want, "CSR")
        _same(m.recommend_users(items, topn, candidates=per_row), want, "a list per row")
        assert (want[0][3] == -1).all()  # (the empty list, and the list of three distinct users)
        assert sorted(want[0][2][want[0][2] >= 0].tolist()) == [3, 7, 1999]
        # a list that names every user: the unrestricted bytes
        _same(m.recommend_users(items, topn, candidates=everyone), m.recommend_users(items, topn), "every user")
        _same(m.recommend_users(items, topn, exclude=(eu, ei), candidates=everyone), m.recommend_users(items, topn, exclude=(eu, ei)),
              "every user, with pairs")
        # with pairs, and with the index
        _same(m.recommend_users(items, topn, exclude=(eu, ei), candidates=shared),
              _expected(oracle, P, Q, items, topn, eu, ei, cands=[shared] * 5), "shared, with pairs")
        _same(m.recommend_users(items, topn, exclude=(eu, ei), candidates=per_row),
              _expected(oracle, P, Q, items, topn, eu, ei, cands=per_row), "per row, with pairs")
        for cand, cands in ((shared, [shared] * 5), (per_row, per_row)):
            got = m.recommend_users(items, topn, exclude="seen", candidates=cand)
            _same(got, _expected(oracle, P, Q, items, topn, su, si, cands=cands), "with the index")
            _same(got, m.recommend_users(items, topn, exclude=(su, si), candidates=cand), "the index as pairs")
        # no candidate at all: rows of padding
        for exclude in (None, (eu, ei), "seen"):
            got = m.recommend_users(items, topn, exclude=exclude, candidates=NONE)
            assert (got[0] == -1).all() and np.isnan(got[1]).all()
            _same(got, m.recommend_users(items, topn, exclude=exclude, candidates=[NONE] * 5))


def test_rows_of_new_items(mf):
    """k = 10: the device rows are padded (kp != k).  The rows call answers what add_items + recommend_users answers."""
    U, I, k, topn, n_new = 1500, 20, 10, 15, 6
    rng = np.random.default_rng(31)
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    lens = np.array([40, 0, 7, 300, 1, 25])
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    fu = rng.integers(0, U, ptr[-1]).astype(np.int32)
    fr = rng.uniform(1, 5, ptr[-1]).astype(np.float32)
    er = rng.integers(0, n_new, 2000).astype(np.int32)  # (row, user): for instance the users who rated the new item
    eu = rng.integers(0, U, 2000).astype(np.int32)
    cand = [rng.integers(0, U, 100).astype(np.int32) for _ in range(n_new)]
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        rows = m.fold_in_items(ptr, fu, fr, 3, seed=9)
        assert rows.shape == (n_new, k)
        got = m.recommend_users_rows(rows, topn, exclude=(er, eu))
        got_plain = m.recommend_users_rows(rows, topn)
        got_among = m.recommend_users_rows(rows, topn, exclude=(er, eu), candidates=cand)
        assert m.add_items(rows) == I
        new = np.arange(I, I + n_new, dtype=np.int32)
        _same(got, m.recommend_users(new, topn, exclude=(eu, I + er)))
        _same(got_plain, m.recommend_users(new, topn))
        _same(got_among, m.recommend_users(new, topn, exclude=(eu, I + er), candidates=cand))
        there = got[0] >= 0
        assert there.all() and m.predict(got[0].ravel(), np.repeat(new, topn)).tobytes() == got[1].tobytes()
        assert not (set(zip(er.tolist(), eu.tolist())) & {(r, int(u)) for r in range(n_new) for u in got[0][r]})


def test_nothing_else_changed(mf):
    U, I, k = 1200, 25, 12
    rng = np.random.default_rng(41)
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    su, si = rng.integers(0, U, 5000).astype(np.int32), rng.integers(0, I, 5000).astype(np.int32)
    items, users = np.array([3, 0, 3, 24], np.int32), np.arange(0, U, 7, dtype=np.int32)
    cand = rng.integers(0, U, 200).astype(np.int32)
    rows = rng.standard_normal((3, k)).astype(np.float32)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        m.set_seen(su, si)

        def state():
            Pn, Qn = m.get_factors()
            ptr, lst = m.seen(np.arange(U))
            rec = m.recommend(users, 5, exclude="seen")
            return (Pn.tobytes(), Qn.tobytes(), ptr.tobytes(), lst.tobytes(), rec[0].tobytes(), rec[1].tobytes(), m.seen_size(),
                    mf.debug_device_bytes())

        before = state()
        assert before[:2] == (P.tobytes(), Q.tobytes())
        calls = (lambda: m.recommend_users(items, 10), lambda: m.recommend_users(items, 10, exclude=(su, si)),
                 lambda: m.recommend_users(items, 200, exclude=(su, si)),  # the sort path
                 lambda: m.recommend_users(items, 10, exclude="seen"), lambda: m.recommend_users(items, 200, exclude="seen"),
                 lambda: m.recommend_users(items, 10, candidates=cand),
                 lambda: m.recommend_users(items, 10, exclude=(su, si), candidates=cand),
                 lambda: m.recommend_users(items, 10, exclude="seen", candidates=[cand[:9], NONE, cand, cand[50:]]),
                 lambda: m.recommend_users_rows(rows, 10), lambda: m.recommend_users_rows(rows, 10, exclude=([0, 2], [5, 6])),
                 lambda: m.recommend_users_rows(rows, 10, exclude=([0, 2], [5, 6]), candidates=cand))
        for x, call in enumerate(calls):
            call()
            assert state() == before, x
        with pytest.raises(mf.MfsgdError):
            m.recommend_users(items, U + 1, exclude="seen")
        with pytest.raises(mf.MfsgdError):
            m.recommend_users([I], 5)
        assert state() == before
        # the two halves are reported as for recommend: after a call that read the index, both took time
        m.recommend_users(items, 10, exclude="seen")
        lists_s, topn_s = m.serve_seconds()
        assert lists_s > 0.0 and topn_s > 0.0
