"""recommend(users, topn, exclude=(u, i)) -- mfsgd_recommend_excluding -- against numpy: the oracle's predictions
of every item, the excluded ones dropped, sorted by score descending then item ascending, cut at topn and padded
with item -1 / score NaN.  Both selection paths (fused kernel: one tile, several tiles; segmented sort: topn 129)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LR, LAM = 0.01, 0.05


def _expected(oracle, P, Q, users, topn, eu, ei):
    I = Q.shape[0]
    allitems = np.arange(I, dtype=np.int32)
    items = np.full((len(users), topn), -1, np.int32)
    scores = np.full((len(users), topn), np.nan, np.float32)
    for row, u in enumerate(users):
        sc = oracle.predict(P, Q, np.full(I, u, np.int32), allitems)
        keep = np.ones(I, bool)
        keep[ei[eu == u]] = False
        it = allitems[keep]
        order = it[np.lexsort((it, -sc[keep].astype(np.float64)))][:topn]
        items[row, :order.size] = order
        scores[row, :order.size] = sc[order]
    return items, scores


def _factors(I, topn, k):
    """The factors of test_recommend_fused_select_and_sort_paths: a third of Q alike, zero scores (all +0.0: the one
    -0.0 entry sums with +0.0 products; real -0.0 scores are in tests/test_serving_edges_gpu.py)."""
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


@pytest.mark.parametrize("I,topn,k", [(30000, 10, 64), (61000, 40, 32), (700, 128, 8), (700, 129, 8), (5, 5, 16)])
def test_recommend_excluding_matches_sorted_predictions(mf, oracle, I, topn, k):
    rng, P, Q = _factors(I, topn, k)
    U = P.shape[0]
    users = np.array([0, 7, 7, U - 1, 13, 21], np.int32)  # 7 twice: one list for both rows
    plain, _ = _expected(oracle, P, Q, users, topn, np.empty(0, np.int32), np.empty(0, np.int32))
    pu, pi = [], []

    def add(u, items):
        items = np.asarray(items, np.int32).ravel()
        pu.append(np.full(items.size, u, np.int32))
        pi.append(items)

    for row, u in enumerate(users):
        add(u, plain[row, :1])  # every row's current top-1
    # part of the tie group at user 0's selection threshold (every other member, so that the group still straddles it)
    allitems = np.arange(I, dtype=np.int32)
    s0 = oracle.predict(P, Q, np.zeros(I, np.int32), allitems)
    tied = allitems[s0 == s0[plain[0, -1]]]
    add(0, tied[::2])
    # user 13: a tenth of the catalogue, spread over every tile; user 7: a few from its ranking
    add(13, rng.choice(I, max(1, I // 10), replace=False))
    add(7, plain[1, 1:topn:3])
    # user 21: every item (the whole row is padded); user U - 1: all but topn // 2 (a partly padded row)
    add(21, allitems)
    add(U - 1, rng.permutation(I)[topn // 2:])
    # users nobody asked for
    add(5, rng.integers(0, I, 300))
    add(U - 2, allitems)
    eu, ei = np.concatenate(pu), np.concatenate(pi)
    dup = rng.integers(0, eu.size, eu.size // 4)  # duplicate pairs
    eu, ei = np.concatenate([eu, eu[dup]]), np.concatenate([ei, ei[dup]])
    perm = rng.permutation(eu.size)
    eu, ei = eu[perm], ei[perm]

    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        items, scores = m.recommend(users, topn, exclude=(eu, ei))
        base_items, base_scores = m.recommend(users, topn)
        none_items, none_scores = m.recommend(users, topn, exclude=(np.empty(0, np.int32), np.empty(0, np.int32)))
        # pairs of users that are not requested only: nothing is excluded
        other = np.isin(eu, users, invert=True)
        oth_items, oth_scores = m.recommend(users, topn, exclude=(eu[other], ei[other]))
        with pytest.raises(mf.MfsgdError):
            m.recommend(users, I + 1, exclude=(eu, ei))

    want_items, want_scores = _expected(oracle, P, Q, users, topn, eu, ei)
    np.testing.assert_array_equal(items, want_items)
    np.testing.assert_array_equal(scores, want_scores)
    assert (items[list(users).index(21)] == -1).all()
    assert (items[3, topn // 2:] == -1).all()
    for a, b in ((none_items, base_items), (oth_items, base_items)):
        np.testing.assert_array_equal(a, b)
    for a in (none_scores, oth_scores):
        assert a.tobytes() == base_scores.tobytes()  # bit for bit, -0.0 included
    np.testing.assert_array_equal(base_items, plain)


def test_recommend_unrated_after_training(mf):
    w = mf.synth.workload("cfg1_ml100k", scale=0.2)
    u, i = w["u"].astype(np.int32), w["i"].astype(np.int32)
    users = np.unique(u)[:: max(1, np.unique(u).size // 200)].astype(np.int32)
    with mf.MatrixFactorizationSGD(w["U"], w["I"], w["k"], LR, LAM, 7) as m:
        m.train(u, i, w["r"], 2)
        items, scores = m.recommend(users, 10, exclude=(u, i))
        pred = m.predict(np.repeat(users, 10), items.ravel())
    assert (items >= 0).all()
    seen = set(zip(u.tolist(), i.tolist()))
    for row, user in enumerate(users):
        assert not any((int(user), int(x)) in seen for x in items[row])
        assert len(set(items[row].tolist())) == 10
    assert pred.tobytes() == scores.ravel().tobytes()
