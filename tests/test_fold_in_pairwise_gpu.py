"""Pairwise fold-in on the device (mfsgd_fold_in_users_pairwise, csrc/foldin_pairwise.hip) against the restatement of
tests/fold_in_pairwise_common.py: rows, margins and negatives bit for bit at every lane-group width, the draws those of
mfsgd_sample_unseen, calls split and reordered through `first`, chains of unequal length in one wave and across a batch
boundary, the pick at its edges, nothing else in the handle moved, and a planted problem on which it learns."""
import numpy as np
import pytest

from tests import fold_in_pairwise_common as FC
from tests import implicit_common as IC

pytestmark = pytest.mark.gpu

LR, LAM = 0.05, 0.01
N_ITEMS = 61


def _lists(rng, n_items=N_ITEMS, n_users=37):
    """The lists of the width test: the edge cases first, then random lengths up to 40 (items may repeat)."""
    lists = [[], [7], [5, 9, 5, 5, 2], list(rng.permutation(n_items)), [i for i in rng.permutation(n_items) if i != 33], [], [60],
             list(rng.integers(0, n_items, 40))]
    while len(lists) < n_users:
        lists.append(list(rng.integers(0, n_items, int(rng.integers(1, 41)))))
    return lists


def _same(got, want, what=""):
    for g, w, name in zip(got, want, ("rows", "margins", "negatives")):
        assert FC.same_bits(np.ascontiguousarray(g), np.ascontiguousarray(w)), f"{name} differ {what}"


def _same_or_nan(got, want, what=""):
    """Bit for bit where the restatement has a number, a NaN where it has a NaN (the host and the device need not agree
    on which NaN a sum of infinities or a NaN operand gives)."""
    for g, w, name in zip(got, want, ("rows", "margins", "negatives")):
        if g.dtype == np.int32:
            assert np.array_equal(g, w), f"{name} differ {what}"
            continue
        nan = np.isnan(w)
        assert np.array_equal(np.isnan(g), nan), f"{name}: NaNs differ {what}"
        assert g[~nan].tobytes() == w[~nan].tobytes(), f"{name} differ {what}"


def _model(mf, Q, k, users=4, seed=11):
    m = mf.MatrixFactorizationSGD(users, Q.shape[0], k, LR, LAM, seed)
    m.set_factors(np.zeros((users, k), np.float32), Q)
    return m


# ---- 1. every group width, bit for bit -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 3, 8, 12, 16, 33, 64, 100, 128, 200, 256])
def test_fold_in_pairwise_matches_the_restatement_for_every_group_width(mf, oracle, k):
    rng = np.random.default_rng(300 + k)
    lists = _lists(rng)
    row_ptr, items = FC.csr(lists)
    n_new, epochs, seed, first = len(lists), 3, 77, 12345
    assert n_new == 37 and max(len(a) for a in lists[5:]) <= 40
    Q = (rng.standard_normal((N_ITEMS, k)) * (1.0 / np.sqrt(k))).astype(np.float32)
    init = rng.standard_normal((n_new, k)).astype(np.float32)
    with _model(mf, Q, k) as m:
        for cand in (1, 4):
            want = FC.fold(Q, row_ptr, items, epochs, cand, init, LR, LAM, seed, first)
            assert np.isfinite(want[0]).all()
            got = m.fold_in_pairwise(row_ptr, items, epochs, candidates=cand, init=init, draw_seed=seed, first=first,
                                     margins=True, negatives=True)
            _same(got, want, f"k={k} m={cand}")
            # the list of every item: no step; of every item but one: every negative is that item
            o = row_ptr * epochs
            assert (got[2][o[3]:o[4]] == -1).all() and (got[1].view(np.uint32)[o[3]:o[4]] == FC.NAN_BITS).all()
            assert FC.same_bits(got[0][3], init[3]) and (got[2][o[4]:o[5]] == 33).all()
            # the rows alone, and one optional array alone
            assert FC.same_bits(m.fold_in_pairwise(row_ptr, items, epochs, candidates=cand, init=init, draw_seed=seed, first=first),
                                want[0])
            rows, negs = m.fold_in_pairwise(row_ptr, items, epochs, candidates=cand, init=init, draw_seed=seed, first=first,
                                            negatives=True)
            assert FC.same_bits(rows, want[0]) and FC.same_bits(negs, want[2])
        # seeded start rows are fold_in's, and epochs == 0 gives them back
        seeded, _ = oracle.init_factors(n_new, 0, k, 11)
        assert FC.same_bits(m.fold_in_pairwise(row_ptr, items, 0), seeded)
        _same(m.fold_in_pairwise(row_ptr, items, 1, margins=True, negatives=True), FC.fold(Q, row_ptr, items, 1, 1, seeded, LR, LAM))
        other, _ = oracle.init_factors(n_new, 0, k, 4321)
        assert FC.same_bits(m.fold_in_pairwise(row_ptr, items, 0, seed=4321), other)
        # nobody has positives: nothing to launch, the rows come back
        assert FC.same_bits(m.fold_in_pairwise(np.zeros(n_new + 1, np.int64), [], 2, init=init), init)


# ---- 2. the draws are the sampler's ------------------------------------------------------------------------------------------------
def test_the_negatives_are_sample_unseen_s_draws(mf):
    rng = np.random.default_rng(21)
    k, epochs, seed, first = 16, 2, -5, 999
    lists = _lists(rng)
    row_ptr, items = FC.csr(lists)
    Q = (rng.standard_normal((N_ITEMS, k)) * 0.25).astype(np.float32)
    init = rng.standard_normal((len(lists), k)).astype(np.float32)
    with _model(mf, Q, k) as m, mf.MatrixFactorizationSGD(len(lists), N_ITEMS, k, LR, LAM, 1) as twin:
        twin.set_seen(np.repeat(np.arange(len(lists)), np.diff(row_ptr)), items)
        _, negs = m.fold_in_pairwise(row_ptr, items, epochs, init=init, draw_seed=seed, first=first, negatives=True)
        for x, A in enumerate(lists):
            steps, o = len(A) * epochs, int(row_ptr[x]) * epochs
            if steps:
                want = twin.sample_unseen(np.full(steps, x, np.int32), 1, seed, first=first + o)[:, 0]
                assert np.array_equal(negs[o:o + steps], want), f"user {x}"
        assert (negs[row_ptr[3] * epochs:row_ptr[4] * epochs] == -1).all()


# ---- 3. splitting and order ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("cand", (1, 4))
def test_users_split_and_reordered_through_first(mf, cand):
    rng = np.random.default_rng(31)
    k, epochs, seed, first = 12, 3, 8, 50
    lists = _lists(rng)
    row_ptr, items = FC.csr(lists)
    n_new = len(lists)
    Q = (rng.standard_normal((N_ITEMS, k)) * 0.3).astype(np.float32)
    init = rng.standard_normal((n_new, k)).astype(np.float32)
    with _model(mf, Q, k) as m:
        kw = dict(candidates=cand, draw_seed=seed, margins=True, negatives=True)
        whole = m.fold_in_pairwise(row_ptr, items, epochs, init=init, first=first, **kw)
        _same(whole, FC.fold(Q, row_ptr, items, epochs, cand, init, LR, LAM, seed, first))

        def part(a, b):
            return m.fold_in_pairwise(row_ptr[a:b + 1] - row_ptr[a], items[row_ptr[a]:row_ptr[b]], epochs, init=init[a:b],
                                      first=first + int(row_ptr[a]) * epochs * cand, **kw)

        def of_whole(a, b):
            return whole[0][a:b], whole[1][row_ptr[a] * epochs:row_ptr[b] * epochs], whole[2][row_ptr[a] * epochs:row_ptr[b] * epochs]

        # the call cut in two
        cut = 17
        _same(part(0, cut), of_whole(0, cut), "first part")
        _same(part(cut, n_new), of_whole(cut, n_new), "second part")
        # the users in another order, one call each, their counters following them
        for x in rng.permutation(n_new):
            _same(part(x, x + 1), of_whole(x, x + 1), f"user {x} alone")


# ---- 4. unequal chains in one wave, and a batch boundary --------------------------------------------------------------------------
@pytest.mark.parametrize("cand", (1, 4))
def test_a_long_chain_among_short_ones_in_one_wave(mf, cand):
    rng = np.random.default_rng(41)
    k, n_items = 8, 2000  # L = 2: 32 groups a wave
    lists = [[int(rng.integers(0, n_items))] for _ in range(70)]
    lists[37] = list(rng.integers(0, n_items, 5000))
    row_ptr, items = FC.csr(lists)
    Q = (rng.standard_normal((n_items, k)) * 0.3).astype(np.float32)
    init = (rng.standard_normal((len(lists), k)) * 0.5).astype(np.float32)
    want = FC.fold(Q, row_ptr, items, 1, cand, init, LR, LAM, 3, 0)
    assert np.isfinite(want[0]).all()
    with _model(mf, Q, k) as m:
        got = m.fold_in_pairwise(row_ptr, items, 1, candidates=cand, init=init, draw_seed=3, margins=True, negatives=True)
    _same(got, want)


def test_fold_in_pairwise_across_a_batch_boundary(mf):
    rng = np.random.default_rng(42)
    k, n_items, n_new = 4, 5000, 1200
    lens = rng.integers(3200, 4201, n_new)
    lens[::97] = 0
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert row_ptr[-1] > (1 << 22)  # more than one batch
    items = rng.integers(0, n_items, int(row_ptr[-1])).astype(np.int32)
    Q = (rng.standard_normal((n_items, k)) * 0.3).astype(np.float32)
    init = (rng.standard_normal((n_new, k)) * 0.5).astype(np.float32)
    want = FC.fold(Q, row_ptr, items, 1, 1, init, LR, LAM, 9, 4)
    assert np.isfinite(want[0]).all()
    start = mf.debug_device_bytes()
    with _model(mf, Q, k) as m:
        got = m.fold_in_pairwise(row_ptr, items, 1, init=init, draw_seed=9, first=4, margins=True, negatives=True)
    assert mf.debug_device_bytes() == start
    _same(got, want)


# ---- 5. the pick at its edges ----------------------------------------------------------------------------------------------------
def _first_draws(row_ptr, lists, epochs, m, seed, first, n_items):
    out = np.full(int(row_ptr[-1]) * epochs, -1, np.int32)
    for x, A in enumerate(lists):
        S = np.unique(A)
        if len(A) and S.size < n_items:
            o = int(row_ptr[x]) * epochs
            out[o:o + len(A) * epochs] = IC.draw(S, n_items, seed, FC.counters(row_ptr, x, epochs, m, first))[:, 0]
    return out


def test_the_pick_at_its_edges(mf):
    rng = np.random.default_rng(51)
    k, epochs, cand, seed, first = 16, 2, 4, 6, 70
    lists = _lists(rng)
    row_ptr, items = FC.csr(lists)
    n_new = len(lists)
    init = rng.standard_normal((n_new, k)).astype(np.float32)
    kw = dict(candidates=cand, init=init, draw_seed=seed, first=first, margins=True, negatives=True)
    d0 = _first_draws(row_ptr, lists, epochs, cand, seed, first, N_ITEMS)
    # identical rows: every score ties, the tie goes to d = 0 (and the margin is 0: the row does not move but for the decay)
    Q = np.tile(rng.standard_normal(k).astype(np.float32), (N_ITEMS, 1))
    with _model(mf, Q, k) as m:
        got = m.fold_in_pairwise(row_ptr, items, epochs, **kw)
    _same(got, FC.fold(Q, row_ptr, items, epochs, cand, init, LR, LAM, seed, first), "identical rows")
    assert np.array_equal(got[2], d0)
    # rows of +0.0 and -0.0: the scores are zeros of either sign, which compare equal
    Q = np.where(rng.random((N_ITEMS, k)) < 0.5, np.float32(0.0), np.float32(-0.0)).astype(np.float32)
    with _model(mf, Q, k) as m:
        got = m.fold_in_pairwise(row_ptr, items, epochs, **kw)
    _same(got, FC.fold(Q, row_ptr, items, epochs, cand, init, LR, LAM, seed, first), "rows of zeros")
    assert np.array_equal(got[2], d0)
    # NaN rows of Q that are nobody's positive: a NaN loses; four NaNs pick d = 0, and the row is a NaN from there on
    Q = (rng.standard_normal((N_ITEMS, k)) * 0.25).astype(np.float32)
    bad = np.arange(30, N_ITEMS)
    Q[bad] = np.nan
    clean = [[int(i) % 30 for i in A] for A in lists]
    rp, it = FC.csr(clean)
    with _model(mf, Q, k) as m:
        got = m.fold_in_pairwise(rp, it, epochs, **kw)
    want = FC.fold(Q, rp, it, epochs, cand, init, LR, LAM, seed, first)
    _same_or_nan(got, want, "NaN rows in Q")
    # the case is there: steps whose row was a number, with a NaN row among their candidates, which lost
    cands = np.concatenate([IC.draw(np.unique(A), N_ITEMS, seed, FC.counters(rp, x, epochs, cand, first)) for x, A in enumerate(clean)])
    ok = ~np.isnan(want[1])
    assert (ok & np.isin(cands, bad).any(axis=1)).sum() > 100 and not np.isin(want[2][ok], bad).any()
    assert (np.isin(cands, bad).all(axis=1) & (want[2] == cands[:, 0])).sum() > 100  # ... and nothing but NaNs: d = 0
    assert np.isnan(want[0]).any() and np.isfinite(want[0]).any()
    # a NaN in a start row: every score is a NaN, the pick is d = 0 and the whole row a NaN after its first step
    Q = (rng.standard_normal((N_ITEMS, k)) * 0.25).astype(np.float32)
    poisoned = init.copy()
    poisoned[:, 5] = np.nan
    with _model(mf, Q, k) as m:
        got = m.fold_in_pairwise(row_ptr, items, epochs, **dict(kw, init=poisoned))
    _same_or_nan(got, FC.fold(Q, row_ptr, items, epochs, cand, poisoned, LR, LAM, seed, first), "a NaN start row")
    assert np.array_equal(got[2], d0)
    stepped = (np.diff(row_ptr) > 0) & (np.arange(n_new) != 3)
    assert np.isnan(got[0][stepped]).all() and np.isnan(got[1][got[2] >= 0]).all()


# ---- 6. nothing else moves ---------------------------------------------------------------------------------------------------------
def test_nothing_else_moves(mf):
    U, I, k = 40, N_ITEMS, 16
    rng = np.random.default_rng(61)
    eu, ei = rng.integers(0, U, 900).astype(np.int32), rng.integers(0, I, 900).astype(np.int32)
    lists = _lists(rng)
    row_ptr, items = FC.csr(lists)
    start = mf.debug_device_bytes()
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 2) as h:
        h.init_factors()
        h.set_ratings(eu, ei, rng.random(eu.size, dtype=np.float32))
        h.set_seen(eu, ei)
        h.set_item_weights(np.arange(1, I + 1, dtype=np.uint32))
        h.fit(1, rmse=False)
        P, Q = h.get_factors()
        ptr, seen = h.seen(np.arange(U))
        size, counters, weights, live = h.seen_size(), h.debug_counters(), h.item_weights(), mf.debug_device_bytes()
        assert live > start
        init = rng.standard_normal((len(lists), k)).astype(np.float32)
        for cand in (1, 4):
            got = h.fold_in_pairwise(row_ptr, items, 2, candidates=cand, init=init, margins=True, negatives=True)
            assert mf.debug_device_bytes() == live
            _same(got, FC.fold(Q, row_ptr, items, 2, cand, init, LR, LAM))
        with pytest.raises(mf.MfsgdError) as e:  # a refused call holds nothing either
            h.fold_in_pairwise([0, 1], [I], 1)
        assert e.value.code == -1 and mf.debug_device_bytes() == live
        P2, Q2 = h.get_factors()
        assert P2.tobytes() == P.tobytes() and Q2.tobytes() == Q.tobytes()
        ptr2, seen2 = h.seen(np.arange(U))
        assert h.seen_size() == size and np.array_equal(ptr, ptr2) and np.array_equal(seen, seen2)
        assert np.array_equal(h.item_weights(), weights)
        assert h.debug_counters() == counters  # schedule builds, cached graphs, the launch path
        assert mf.debug_device_bytes() == live
    assert mf.debug_device_bytes() == start
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 2, n_parts=2) as p:
        with pytest.raises(mf.MfsgdError) as e:
            p.fold_in_pairwise(row_ptr, items, 1)
        assert e.value.code == -5 and "single-partition handles only" in str(e.value)
    # neither an index nor ratings are needed
    Q = (rng.standard_normal((I, k)) * 0.25).astype(np.float32)
    with _model(mf, Q, k) as m:
        assert m.seen_size() == -1
        m.fold_in_pairwise(row_ptr, items, 1)
        assert m.seen_size() == -1


# ---- 7. it learns ------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def planted(mf):
    """The planted one-class problem of tests/test_pairwise_gpu.py (600 users, 400 items in 20 groups, 11 positives and one
    held-out item each; k = 16, lr 0.05, lambda 0.01), fit_bpr for 20 epochs on the first 500 users: Q and the rest."""
    U, I, G, k, lr, lam, seed, known = 600, 400, 20, 16, 0.05, 0.01, 3, 500
    rng = np.random.default_rng(0)
    per = I // G
    its = np.stack([(u % G) * per + rng.choice(per, 12, replace=False) for u in range(U)]).astype(np.int32)
    hu, hi = np.arange(known, dtype=np.int32), its[:known, 0].copy()
    pu, pi = np.repeat(hu, 11), its[:known, 1:].ravel().copy()
    with mf.MatrixFactorizationSGD(known, I, k, lr, lam, seed) as h:
        h.set_seen(np.concatenate([pu, hu]), np.concatenate([pi, hi]))  # held-out positives are never negatives
        h.init_factors()
        h.fit_bpr(pu, pi, 20, seed=seed)
        P, Q = h.get_factors()
    return dict(P=P, Q=Q, k=k, lr=lr, lam=lam, new=its[known:])


@pytest.mark.parametrize("cand", (1, 4))
def test_it_learns_new_users_of_a_planted_problem(mf, planted, cand):
    """The 100 users fit_bpr never saw, folded in from their 11 positives (20 epochs): the rank of each one's held-out item
    among the items they have not named is the rank the restatement's rows give, and the hit rate at 10 is strictly
    above that of the start rows.
    Measured on an MI355X: start rows 0.07, folded in 1.0 for m = 1 and for m = 4 ("Pairwise fold-in")."""
    k, Q, new = planted["k"], planted["Q"], planted["new"]
    n_new = new.shape[0]
    row_ptr, items = np.arange(n_new + 1, dtype=np.int64) * 11, new[:, 1:].ravel().copy()
    rows_of, held = np.arange(n_new, dtype=np.int32), new[:, 0].copy()
    excl = (np.repeat(rows_of, 11), items)
    with mf.MatrixFactorizationSGD(planted["P"].shape[0], Q.shape[0], k, planted["lr"], planted["lam"], 3) as h:
        h.set_factors(planted["P"], Q)
        start = h.fold_in_pairwise(row_ptr, items, 0)
        rows = h.fold_in_pairwise(row_ptr, items, 20, candidates=cand, draw_seed=5)
        want = FC.fold(Q, row_ptr, items, 20, cand, start, planted["lr"], planted["lam"], 5)[0]
        ranks0 = h.rank_items_rows(start, rows_of, held, exclude=excl)
        ranks = h.rank_items_rows(rows, rows_of, held, exclude=excl)
        ranks_want = h.rank_items_rows(want, rows_of, held, exclude=excl)
    before, after = float((ranks0 < 10).mean()), float((ranks < 10).mean())
    print(f"held-out hit rate at 10, m = {cand}: start rows {before:.4f}, folded in {after:.4f}")
    assert np.array_equal(ranks, ranks_want)
    assert after > before
    assert FC.same_bits(rows, want)


# ---- 8. sequence ---------------------------------------------------------------------------------------------------------------------
def test_fold_add_mark_recommend(mf, planted):
    k, Q, new = planted["k"], planted["Q"], planted["new"]
    n_new, topn = new.shape[0], 10
    row_ptr, items = np.arange(n_new + 1, dtype=np.int64) * 11, new[:, 1:].ravel().copy()
    pairs = (np.repeat(np.arange(n_new, dtype=np.int32), 11), items)
    with mf.MatrixFactorizationSGD(planted["P"].shape[0], Q.shape[0], k, planted["lr"], planted["lam"], 3) as h:
        h.set_factors(planted["P"], Q)
        rows = h.fold_in_pairwise(row_ptr, items, 5, candidates=4)
        want_items, want_scores = h.recommend_rows(rows, topn, exclude=pairs)
        first = h.add_users(rows)
        assert first == planted["P"].shape[0]
        h.mark_seen(first + pairs[0], pairs[1])
        got_items, got_scores = h.recommend(first + np.arange(n_new, dtype=np.int32), topn, exclude="seen")
    assert np.array_equal(got_items, want_items) and FC.same_bits(got_scores, want_scores)
    named = (pairs[0].astype(np.int64) << 32) | pairs[1]
    assert (got_items >= 0).all() and not np.isin((np.arange(n_new, dtype=np.int64)[:, None] << 32) | got_items, named).any()
