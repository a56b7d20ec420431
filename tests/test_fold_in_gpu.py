"""fold_in(...) -- mfsgd_fold_in_users -- and recommend_rows(...) -- mfsgd_recommend_rows -- against the CPU oracle.
Fold-in with Q fixed equals one ordinary oracle pass over a model in which every rating has a private copy of its
item row: the pass reads that copy once, writes an update nobody reads, and P sees exactly the fold-in step.  Rows
are compared bit for bit."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LR, LAM = 0.01, 0.05
STATE = -5


def fold_in_ref(oracle, Q, row_ptr, items, ratings, epochs, R0, lr, lam):
    R = R0.copy()
    n = items.size
    uo = np.repeat(np.arange(row_ptr.size - 1, dtype=np.int32), np.diff(row_ptr)).astype(np.int32)
    for _ in range(epochs):
        Qp = np.ascontiguousarray(Q[items])  # fresh private rows each epoch
        oracle.sgd_pass(R, Qp, uo, np.arange(n, dtype=np.int32), ratings, lr, lam)
    return R


def _csr(lens, I, rng):
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    items = rng.integers(0, I, int(row_ptr[-1])).astype(np.int32)
    ratings = rng.uniform(0.5, 5.0, items.size).astype(np.float32)
    return row_ptr, items, ratings


def _mixed_users(I, rng, n=150):
    """Lengths from 0 to a few hundred, shuffled so that neighbours differ widely; empty users; a repeated item."""
    lens = np.concatenate([rng.integers(0, 8, n // 3), rng.integers(0, 60, n // 3), rng.integers(100, 400, n - 2 * (n // 3))])
    rng.shuffle(lens)
    lens[0], lens[n // 2], lens[-1] = 0, 0, 0
    lens[3] = 17
    row_ptr, items, ratings = _csr(lens, I, rng)
    items[row_ptr[3] + 5] = items[row_ptr[3] + 2]   # the same item twice in one user's list, not adjacent
    items[row_ptr[3] + 9] = items[row_ptr[3] + 8]   # ... and adjacent
    return row_ptr, items, ratings


@pytest.mark.parametrize("k", [1, 3, 8, 12, 16, 33, 64, 100, 128, 200, 256])
def test_fold_in_matches_oracle_for_every_group_width(mf, oracle, k):
    rng = np.random.default_rng(100 + k)
    U, I = 20, 300
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = (rng.standard_normal((I, k)) * (0.5 / np.sqrt(k))).astype(np.float32)
    row_ptr, items, ratings = _mixed_users(I, rng)
    n_new = row_ptr.size - 1
    init = rng.standard_normal((n_new, k)).astype(np.float32)
    seeded, _ = oracle.init_factors(n_new, 0, k, 11)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 11) as m:
        m.set_factors(P, Q)
        for epochs in (0, 1, 3):
            got = m.fold_in(row_ptr, items, ratings, epochs, init=init)
            want = fold_in_ref(oracle, Q, row_ptr, items, ratings, epochs, init, LR, LAM)
            assert np.isfinite(want).all()
            assert np.array_equal(got, want), f"k={k} epochs={epochs} init given"
            got = m.fold_in(row_ptr, items, ratings, epochs)           # seeded with the model's seed
            want = fold_in_ref(oracle, Q, row_ptr, items, ratings, epochs, seeded, LR, LAM)
            assert np.array_equal(got, want), f"k={k} epochs={epochs} seeded"
        other, _ = oracle.init_factors(n_new, 0, k, 12345)
        assert np.array_equal(m.fold_in(row_ptr, items, ratings, 0, seed=12345), other)
        empty = np.flatnonzero(np.diff(row_ptr) == 0)
        assert empty.size >= 3
        assert np.array_equal(m.fold_in(row_ptr, items, ratings, 3, init=init)[empty], init[empty])
        # nobody has ratings: nothing to launch, the rows come back
        zero = np.zeros(n_new + 1, np.int64)
        assert np.array_equal(m.fold_in(zero, [], [], 2, init=init), init)


def test_fold_in_does_not_depend_on_the_order_of_the_users(mf):
    rng = np.random.default_rng(5)
    k, I = 33, 300
    Q = (rng.standard_normal((I, k)) * 0.1).astype(np.float32)
    row_ptr, items, ratings = _mixed_users(I, rng)
    n_new = row_ptr.size - 1
    init = rng.standard_normal((n_new, k)).astype(np.float32)
    lens = np.diff(row_ptr)
    rev_ptr = np.concatenate([[0], np.cumsum(lens[::-1])]).astype(np.int64)
    pieces = [slice(row_ptr[x], row_ptr[x + 1]) for x in range(n_new)][::-1]
    rev_items = np.concatenate([items[s] for s in pieces])
    rev_ratings = np.concatenate([ratings[s] for s in pieces])
    with mf.MatrixFactorizationSGD(4, I, k, LR, LAM, 1) as m:
        m.set_factors(np.zeros((4, k), np.float32), Q)
        a = m.fold_in(row_ptr, items, ratings, 2, init=init)
        b = m.fold_in(rev_ptr, rev_items, rev_ratings, 2, init=init[::-1])
    assert np.array_equal(a, b[::-1])


def test_fold_in_several_batches_and_a_dominant_user(mf, oracle):
    rng = np.random.default_rng(9)
    k, I, n_small = 8, 5000, 300_000
    lens = rng.integers(10, 51, n_small + 1)
    big = n_small // 3
    lens[big] = 200_000
    row_ptr, items, ratings = _csr(lens, I, rng)
    assert row_ptr[-1] > 2 * (1 << 22)
    Q = (rng.standard_normal((I, k)) * 0.3).astype(np.float32)
    with mf.MatrixFactorizationSGD(4, I, k, LR, LAM, 3) as m:
        m.set_factors(np.zeros((4, k), np.float32), Q)
        got = m.fold_in(row_ptr, items, ratings, 2)
    R0, _ = oracle.init_factors(lens.size, 0, k, 3)
    want = fold_in_ref(oracle, Q, row_ptr, items, ratings, 2, R0, LR, LAM)
    assert np.isfinite(want).all()
    assert np.array_equal(got[big], want[big])
    assert np.array_equal(got, want)


def test_fold_in_leaves_the_model_untouched(mf):
    w = mf.synth.workload("cfg1_ml100k", scale=0.2)
    rng = np.random.default_rng(2)
    row_ptr, items, ratings = _mixed_users(w["I"], rng)
    with mf.MatrixFactorizationSGD(w["U"], w["I"], w["k"], LR, LAM, 7) as m:
        m.train(w["u"], w["i"], w["r"], 1)
        P0, Q0 = m.get_factors()
        rmse0 = m.rmse()
        pred0 = m.predict(w["u"][:1000], w["i"][:1000])
        rows = m.fold_in(row_ptr, items, ratings, 3)
        P1, Q1 = m.get_factors()
        assert P0.tobytes() == P1.tobytes() and Q0.tobytes() == Q1.tobytes()
        assert m.rmse() == rmse0
        assert m.predict(w["u"][:1000], w["i"][:1000]).tobytes() == pred0.tobytes()
    assert rows.shape == (row_ptr.size - 1, w["k"])


def test_fold_in_learns_held_out_ratings(mf, oracle):
    """Rank-4 ground truth; the model is trained on 600 users, 100 further users are folded in from 40 ratings each and
    judged on 20 others.  The condition (held-out RMSE after 20 epochs below half its value at 0 epochs) is one on the
    method: the CPU reference on these inputs gives 2.98 -> 0.19 (training RMSE 0.15)."""
    rng = np.random.default_rng(42)
    U, Un, I, k = 600, 100, 400, 16
    A = rng.standard_normal((U + Un, 4)).astype(np.float32)
    B = rng.standard_normal((I, 4)).astype(np.float32)

    def sample(users, per):
        uu = np.repeat(users, per).astype(np.int32)
        ii = np.concatenate([rng.choice(I, per, replace=False) for _ in users]).astype(np.int32)
        rr = (np.einsum("ij,ij->i", A[uu], B[ii]) + 3.0 + 0.1 * rng.standard_normal(uu.size)).astype(np.float32)
        return uu, ii, rr

    u, i, r = sample(np.arange(U), 60)
    nu, ni, nr = sample(np.arange(U, U + Un), 60)
    nu -= U
    pos = np.tile(np.arange(60), Un)
    seen, held = pos < 40, pos >= 40
    row_ptr = (np.arange(Un + 1) * 40).astype(np.int64)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 7) as m:
        m.train(u, i, r, 30)
        _, Q = m.get_factors()
        rows0 = m.fold_in(row_ptr, ni[seen], nr[seen], 0)
        rows20 = m.fold_in(row_ptr, ni[seen], nr[seen], 20)
    before = oracle.rmse(rows0, Q, nu[held], ni[held], nr[held])
    after = oracle.rmse(rows20, Q, nu[held], ni[held], nr[held])
    print(f"held-out RMSE: {before:.4f} at 0 epochs, {after:.4f} at 20")
    assert after < 0.5 * before
    R0, _ = oracle.init_factors(Un, 0, k, 7)
    assert np.array_equal(rows20, fold_in_ref(oracle, Q, row_ptr, ni[seen], nr[seen], 20, R0, LR, LAM))


def _expected(oracle, P, Q, users, topn, eu, ei):
    """As tests/test_recommend_exclude_gpu.py builds it."""
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


@pytest.mark.parametrize("I,topn,k", [(30000, 10, 64), (700, 128, 8), (700, 129, 8), (5, 5, 16)])
def test_recommend_rows_equals_recommend_for_rows_of_p(mf, I, topn, k):
    rng = np.random.default_rng(I + topn)
    U = 40
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    Q[rng.integers(0, I, I // 3)] = Q[3 % I]   # ties
    users = np.array([0, 7, 7, U - 1, 13, 21], np.int32)
    # pairs by position in `users` (7 is there twice: both positions get its pairs)
    pos = [0, 4, 5, 3]
    per = [rng.choice(I, max(1, I // 10), replace=False), rng.choice(I, max(1, I // 3), replace=False),
           np.arange(I), rng.permutation(I)[topn // 2:]]     # a whole row excluded, and a partly padded one
    seven = rng.choice(I, max(1, I // 5), replace=False)
    er = np.concatenate([np.full(p.size, x, np.int32) for x, p in zip(pos, per)] + [np.full(seven.size, 1, np.int32),
                                                                                   np.full(seven.size, 2, np.int32)])
    ei = np.concatenate(per + [seven, seven]).astype(np.int32)
    perm = rng.permutation(er.size)
    er, ei = er[perm], ei[perm]
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        want_i, want_s = m.recommend(users, topn, exclude=(users[er], ei))
        got_i, got_s = m.recommend_rows(P[users], topn, exclude=(er, ei))
        plain_i, plain_s = m.recommend(users, topn)
        rows_i, rows_s = m.recommend_rows(P[users], topn)
    assert np.array_equal(got_i, want_i) and got_s.tobytes() == want_s.tobytes()
    assert np.array_equal(rows_i, plain_i) and rows_s.tobytes() == plain_s.tobytes()
    assert (got_i[5] == -1).all() and (got_i[3, topn // 2:] == -1).all()


@pytest.mark.parametrize("I,topn,k", [(30000, 10, 64), (700, 129, 8)])
def test_recommend_rows_of_folded_users_matches_sorted_predictions(mf, oracle, I, topn, k):
    rng = np.random.default_rng(I)
    Q = (rng.standard_normal((I, k)) * (0.5 / np.sqrt(k))).astype(np.float32)
    lens = np.array([0, 40, 3, 250, 17, 90])
    row_ptr, items, ratings = _csr(lens, I, rng)
    with mf.MatrixFactorizationSGD(4, I, k, LR, LAM, 5) as m:
        m.set_factors(np.zeros((4, k), np.float32), Q)
        rows = m.fold_in(row_ptr, items, ratings, 4)
        er = np.repeat(np.arange(lens.size, dtype=np.int32), lens).astype(np.int32)
        got_i, got_s = m.recommend_rows(rows, topn, exclude=(er, items))
    want_i, want_s = _expected(oracle, rows, Q, np.arange(lens.size), topn, er, items)
    np.testing.assert_array_equal(got_i, want_i)
    np.testing.assert_array_equal(got_s, want_s)
    for x in range(lens.size):
        assert not set(got_i[x].tolist()) & set(items[row_ptr[x]:row_ptr[x + 1]].tolist())


def test_partitioned_handles_are_a_state_error(mf):
    k = 8
    with mf.MatrixFactorizationSGD(6, 5, k, LR, LAM, 1, n_parts=2) as m:
        m.init_factors()
        with pytest.raises(mf.MfsgdError) as e:
            m.fold_in([0, 1, 2], [0, 1], [1.0, 2.0], 1)
        assert e.value.code == STATE
        with pytest.raises(mf.MfsgdError) as e:
            m.recommend_rows(np.ones((2, k), np.float32), 2)
        assert e.value.code == STATE
