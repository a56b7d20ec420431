"""Hard negatives on the device (csrc/pick.hip, mfsgd_sample_unseen_hard): items, scores and draws against the numpy
restatement of the pick (tests/hardneg_common.py), byte for byte, for every lane-group size and the candidate counts around
it; the shapes of the seen-item index; ties, NaN and infinite scores; the pieces a call is staged in; that a live handle
stays whole; fit_bpr(candidates=m) against the sequence of calls it is documented as; and the planted one-class problem."""
import numpy as np
import pytest

from tests import hardneg_common as HC
from tests import implicit_common as IC

pytestmark = pytest.mark.gpu

LR, LAM, SEED = 0.05, 0.01, 4
CHUNK = IC.SAMPLE_CHUNK


def _group_lanes(k):
    """L: lanes per row, the power of two that holds k floats in chunks of four."""
    L = 1
    while 4 * L < k:
        L *= 2
    return L


def _keys(u, i):
    return (np.asarray(u).astype(np.int64) << 32) | np.asarray(i).astype(np.int64)


def _same(got, want, what):
    for g, w, name in zip(got, want, ("items", "scores", "draws")):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))
            raise AssertionError(f"{what}: {bad.size} {name} differ, first at rows {bad[:5]}: {g[bad[:5]]} instead of {w[bad[:5]]}")


def _compare(h, lists, n_items, users, m, seed, first, scorer, what=""):
    """One call with every output against the restatement; returns what the call gave."""
    got = h.sample_unseen_hard(users, m, seed, first, scores=True, draws=True)
    _same(got, HC.hard(lists, n_items, users, m, seed, first, scorer), what)
    return got


def _oracle_scorer(oracle, P, Q):
    return lambda u, i: oracle.predict(P, Q, u, i)


def _normal_factors(rng, U, I, k):
    return rng.standard_normal((U, k)).astype(np.float32), rng.standard_normal((I, k)).astype(np.float32)


# ---- 1. lane groups and candidate counts -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (1, 6, 16, 20, 64, 100, 256))  # L = 1, 2, 4, 8, 16, 32 (the permlane level of the dot), 64
def test_lane_groups_and_candidate_counts(mf, oracle, k):
    U, I, full, seed, first = 48, 130, 11, 5, (1 << 40) + 7
    L = _group_lanes(k)
    rng = np.random.default_rng(k)
    eu, ei = rng.integers(0, U - 1, 1500).astype(np.int32), rng.integers(0, I, 1500).astype(np.int32)  # the last user: no pairs
    eu, ei = np.concatenate([eu, np.full(I, full)]).astype(np.int32), np.concatenate([ei, np.arange(I)]).astype(np.int32)
    lists = IC.lists_of(eu, ei)
    P, Q = _normal_factors(rng, U, I, k)
    scorer = _oracle_scorer(oracle, P, Q)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as h:
        h.set_factors(P, Q)
        h.set_seen(eu, ei)
        for m in sorted({m for m in (1, 2, 3, L - 1, L, L + 1, 70) if m >= 1}):
            for n in sorted({n for n in (1, 256 // L - 1, 256 // L + 1, 1000) if n >= 1}):
                users = rng.integers(0, U, n).astype(np.int32)  # repeated, in any order
                items, scores, draws = _compare(h, lists, I, users, m, seed, first, scorer, f"k {k} m {m} n {n}")
                assert not np.isin(_keys(users, items), _keys(eu, ei)).any()
                assert ((items == -1) == (users == full)).all()
                assert np.array_equal(h.sample_unseen_hard(users, m, seed, first), items)  # without the other outputs
                if m == 1:
                    assert np.array_equal(items, h.sample_unseen(users, 1, seed, first)[:, 0])
                    ok = items >= 0
                    assert scores[ok].tobytes() == h.predict(users[ok], items[ok]).tobytes()
                    assert (draws[ok] == 0).all()


# ---- 2. the shapes of the index ----------------------------------------------------------------------------------------------------
def test_index_shapes(mf, oracle):
    U, I, k, m, seed = 20, 60, 6, 5, 9
    every, all_but_one, left = 3, 7, 41
    rng = np.random.default_rng(1)
    P, Q = _normal_factors(rng, U, I, k)
    users = np.append(rng.permutation(U), [every, all_but_one, 0]).astype(np.int32)
    nothing = lambda u: np.empty(0, np.int64)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as h:
        h.reserve(users=U + 4, items=I + 8)
        h.set_factors(P, Q)
        h.set_seen([], [])  # an empty index: every item is a candidate
        _compare(h, nothing, I, users, m, seed, 0, _oracle_scorer(oracle, P, Q), "an empty index")
        eu, ei = rng.integers(0, U, 300).astype(np.int32), rng.integers(0, I, 300).astype(np.int32)
        keep = ~np.isin(eu, (every, all_but_one))
        rest = np.setdiff1d(np.arange(I), [left])
        eu = np.concatenate([eu[keep], np.full(I, every), np.full(rest.size, all_but_one)]).astype(np.int32)
        ei = np.concatenate([ei[keep], np.arange(I), rest]).astype(np.int32)
        lists = IC.lists_of(eu, ei)
        h.set_seen(eu, ei)
        items, scores, draws = _compare(h, lists, I, users, m, seed, 0, _oracle_scorer(oracle, P, Q), "set_seen")
        sel = users == every  # seen everything
        assert (items[sel] == -1).all() and (draws[sel] == -1).all() and (scores.view(np.uint32)[sel] == HC.NAN_BITS).all()
        sel = users == all_but_one  # every candidate is the one item left: the first of them
        assert (items[sel] == left).all() and (draws[sel] == 0).all()
        # users appended with empty lists
        assert h.add_users(n=2, seed=3) == U
        P, Q = h.get_factors()
        more = np.append(users, [U + 1, U, U + 1]).astype(np.int32)
        _compare(h, lists, I, more, m, seed, 0, _oracle_scorer(oracle, P, Q), "add_users")
        # items appended inside the reserved capacity: they are drawn, the rows beyond the count never are
        assert h.add_items(n=5, seed=4) == I
        P, Q = h.get_factors()
        assert Q.shape[0] == I + 5 and h.capacity()[1] == I + 8
        items, _, _ = _compare(h, lists, I + 5, more, 16, seed, 0, _oracle_scorer(oracle, P, Q), "add_items")
        assert items.max() < I + 5 and (items[more == every] >= I).all()  # all that the user who had seen everything can get


# ---- 3. ties and specials ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (6, 64))
def test_ties_nan_and_infinite_scores(mf, k):
    """The handle's own predict is the scorer: its bits are pinned elsewhere, NaNs included."""
    U, I, seed = 12, 40, 2
    zero, minus_zero, nan_user, two_left = 1, 2, 3, 4
    nan_item, other_item, plus_inf, minus_inf = 10, 30, 20, 21
    rng = np.random.default_rng(k)
    P, Qb = _normal_factors(rng, U, 4, k)
    Q = Qb[np.arange(I) % 4].copy()  # four distinct rows: most candidates tie with another
    P[zero], P[minus_zero], P[nan_user, k // 2] = 0.0, -0.0, np.nan
    Q[nan_item, k - 1] = np.nan
    Q[plus_inf, 0], Q[minus_inf, 0] = np.inf, -np.inf
    rest = np.setdiff1d(np.arange(I), [nan_item, other_item])
    eu, ei = np.full(rest.size, two_left, np.int32), rest.astype(np.int32)  # candidates: the NaN item or one other
    lists = IC.lists_of(eu, ei)
    users = np.tile(np.arange(U, dtype=np.int32), 30)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as h:
        h.set_factors(P, Q)
        h.set_seen(eu, ei)
        for m in (2, 9, 40):
            items, scores, draws = _compare(h, lists, I, users, m, seed, 0, h.predict, f"k {k} m {m}")
            cand = IC.sample(lists, I, users, m, seed, 0)
            sc = h.predict(np.repeat(users, m), cand.ravel()).reshape(-1, m)
            plain = ~np.isin(users, (zero, minus_zero, nan_user, two_left)) & ~np.isnan(sc).all(axis=1)
            # duplicated rows of Q: the smaller d wins, and the case occurs
            best = np.nanmax(sc[plain], axis=1)
            assert np.array_equal(draws[plain], np.argmax(sc[plain] == best[:, None], axis=1))
            assert m == 2 or ((sc[plain] == best[:, None]).sum(axis=1) > 1).any()
            # infinite scores: +inf wins wherever it is a candidate, -inf only against nothing else
            sel = plain & np.isin(cand, [plus_inf, minus_inf]).any(axis=1)
            assert sel.any() and np.isinf(sc[sel]).any()
            assert np.array_equal(scores[plain], best)
            # a P row of zeros: every score is +0.0 or -0.0 (or a NaN, against the NaN and infinite items), the draw is the
            # first number
            for user in (zero, minus_zero):
                sel = users == user
                assert ((sc[sel] == 0) | np.isnan(sc[sel])).all()
                assert np.array_equal(draws[sel], np.argmax(~np.isnan(sc[sel]), axis=1))
                assert (draws[sel] == 0).sum() > 0
            # a NaN row of P: every score is a NaN, the draw is 0
            sel = users == nan_user
            assert np.isnan(sc[sel]).all() and (draws[sel] == 0).all() and np.isnan(scores[sel]).all()
            assert np.array_equal(items[sel], cand[sel, 0])
            # a NaN row of Q among the candidates loses
            sel = users == two_left
            assert np.isin(cand[sel], [nan_item, other_item]).all()
            has_other = (cand[sel] == other_item).any(axis=1)
            assert (items[sel][has_other] == other_item).all() and (items[sel][~has_other] == nan_item).all()
            assert (draws[sel][~has_other] == 0).all() and has_other.any()


# ---- 4. cutting the call changes nothing -----------------------------------------------------------------------------------------
def _small_index(rng, U, I):
    eu, ei = rng.integers(0, U - 1, 4 * U).astype(np.int32), rng.integers(0, I, 4 * U).astype(np.int32)
    return eu, ei, IC.lists_of(eu, ei)


def test_rows_of_a_call_are_the_call_on_those_rows(mf, oracle):
    U, I, k, m, seed, first = 40, 90, 16, 3, 11, 1 << 33
    rng = np.random.default_rng(6)
    eu, ei, lists = _small_index(rng, U, I)
    users = rng.integers(0, U, 1000).astype(np.int32)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as h:
        h.init_factors()
        h.set_seen(eu, ei)
        P, Q = h.get_factors()
        whole = _compare(h, lists, I, users, m, seed, first, _oracle_scorer(oracle, P, Q))
        for a, b in ((0, 7), (63, 65), (500, 1000), (999, 1000), (300, 300)):
            part = h.sample_unseen_hard(users[a:b], m, seed, first + a * m, scores=True, draws=True)
            _same(part, tuple(w[a:b] for w in whole), (a, b))


def test_a_call_longer_than_a_piece(mf):
    """k = 4, m = 4, n = 2^20 + 3: a piece is 2^20 rows, the last holds 3.  The handle's predict is the scorer."""
    U, I, k, m, seed, first = 300, 200, 4, 4, 11, 1 << 33
    n = CHUNK // m + 3
    rng = np.random.default_rng(4)
    eu, ei, lists = _small_index(rng, U, I)
    users = rng.integers(0, U, n).astype(np.int32)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as h:
        h.init_factors()
        h.set_seen(eu, ei)
        whole = _compare(h, lists, I, users, m, seed, first, h.predict)
        rows = CHUNK // m
        for a, b in ((rows - 2, rows + 2), (rows, n), (5, rows + 1)):
            part = h.sample_unseen_hard(users[a:b], m, seed, first + a * m, scores=True, draws=True)
            _same(part, tuple(w[a:b] for w in whole), (a, b))


def test_one_row_longer_than_a_piece_is_a_piece_of_its_own(mf):
    """m = 2^22 + 5 and two rows: each is a piece.  One lane group walks a row's candidates in rounds of L draws, so the
    test takes k = 64 (L = 16) where k = 4 would walk four million dependent draws one after the other."""
    U, I, k, seed = 300, 200, 64, 2
    m = CHUNK + 5
    rng = np.random.default_rng(9)
    eu, ei, lists = _small_index(rng, U, I)
    users = np.array([1, 0], np.int32)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as h:
        h.init_factors()
        h.set_seen(eu, ei)
        _compare(h, lists, I, users, m, seed, 3, h.predict)


# ---- 5. a live handle stays whole ------------------------------------------------------------------------------------------------
def test_side_effects(mf, oracle):
    U, I, k, m, seed = 40, 90, 16, 6, 5
    rng = np.random.default_rng(12)
    eu, ei = rng.integers(0, U, 900).astype(np.int32), rng.integers(0, I, 900).astype(np.int32)
    lists = IC.lists_of(eu, ei)
    users = rng.integers(0, U, 3000).astype(np.int32)
    start = mf.debug_device_bytes()
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as h:
        h.init_factors()
        h.set_ratings(eu, ei, rng.random(eu.size, dtype=np.float32))
        h.set_seen(eu, ei)
        h.fit(1, rmse=False)
        P, Q = h.get_factors()
        ptr, seen = h.seen(np.arange(U))
        size, counters, live = h.seen_size(), h.debug_counters(), mf.debug_device_bytes()
        assert live > start
        got = _compare(h, lists, I, users, m, seed, 0, _oracle_scorer(oracle, P, Q))
        assert mf.debug_device_bytes() == live
        again = h.sample_unseen_hard(users, m, seed, 0, scores=True, draws=True)
        _same(again, got, "the same call twice")
        with pytest.raises(mf.MfsgdError) as e:  # a refused call holds nothing either
            h.sample_unseen_hard([0, U], m, seed)
        assert e.value.code == -1 and mf.debug_device_bytes() == live
        P2, Q2 = h.get_factors()
        assert P2.tobytes() == P.tobytes() and Q2.tobytes() == Q.tobytes()
        ptr2, seen2 = h.seen(np.arange(U))
        assert h.seen_size() == size and np.array_equal(ptr, ptr2) and np.array_equal(seen, seen2)
        assert h.debug_counters() == counters  # schedule builds, cached graphs, the launch path
        # the rows move, the picks follow
        ok = got[0] >= 0
        tu, tj = users[ok][:400], got[0][ok][:400]
        ti = ((tj + 1 + rng.integers(0, I - 1, tj.size)) % I).astype(np.int32)  # any item but the negative
        h.partial_fit_pairwise(tu, ti, tj)
        P3, Q3 = h.get_factors()
        assert P3.tobytes() != P.tobytes() and Q3.tobytes() != Q.tobytes()
        moved = _compare(h, lists, I, users, m, seed, 0, _oracle_scorer(oracle, P3, Q3), "after partial_fit_pairwise")
        assert moved[1].tobytes() != got[1].tobytes() and not np.array_equal(moved[0], got[0])
        assert mf.debug_device_bytes() == live
    assert mf.debug_device_bytes() == start


# ---- 6. fit_bpr(candidates=m) is the sequence it is documented as ------------------------------------------------------------------
def _bits(m):
    P, Q = m.get_factors()
    return P.tobytes(), Q.tobytes()


@pytest.mark.parametrize("refresh", (None, 128))
@pytest.mark.parametrize("held", (False, True))
def test_fit_bpr_with_candidates_is_its_documented_sequence(mf, held, refresh):
    U, I, k, epochs, seed, full, m = 60, 50, 8, 3, 21, 17, 3
    rng = np.random.default_rng(5)
    pu, pi = rng.integers(0, U, 400).astype(np.int32), rng.integers(0, I, 400).astype(np.int32)  # duplicates among them
    pu, pi = np.concatenate([pu, np.full(I, full)]).astype(np.int32), np.concatenate([pi, np.arange(I)]).astype(np.int32)
    order = rng.permutation(pu.size)
    pu, pi = pu[order], pi[order]
    n = pu.size
    step = n if refresh is None else refresh
    assert refresh is None or n % refresh != 0
    hu, hi = rng.integers(0, U, 200).astype(np.int32), rng.integers(0, I, 200).astype(np.int32)
    fresh = ~np.isin(_keys(hu, hi), _keys(pu, pi))
    hu, hi = hu[fresh], hi[fresh]
    new = lambda: mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED)
    with new() as a, new() as b, new() as c:
        if held:  # the index also holds the held-out pairs: every handle gets it first
            for h in (a, b, c):
                h.set_seen(np.concatenate([pu, hu]), np.concatenate([pi, hi]))
            size = a.seen_size()
        stats = a.fit_bpr(pu, pi, epochs, seed=seed, candidates=m, refresh=refresh)
        assert sorted(stats) == ["auc", "loss"] and all(v.shape == (epochs,) and v.dtype == np.float64 for v in stats.values())
        assert a.debug_counters()["schedule_builds"] == 0  # no rating set was made
        if held:
            assert a.seen_size() == size
        else:  # a handle without an index got one: the distinct positives
            assert a.seen_size() == np.unique(_keys(pu, pi)).size
            b.set_seen(pu, pi)
        # the same steps written out
        b.init_factors()
        for e in range(epochs):
            xs = []
            for lo in range(0, n, step):
                bu, bi = pu[lo:lo + step], pi[lo:lo + step]
                J = b.sample_unseen_hard(bu, m, seed, first=e * n * m + lo * m)
                assert (J[bu == full] == -1).all() and (J[bu != full] >= 0).all()
                if held:
                    assert not np.isin(_keys(bu, J), _keys(hu, hi)).any()
                keep = J >= 0
                xs.append(b.partial_fit_pairwise(bu[keep], bi[keep], J[keep], margins=True))
            x = np.concatenate(xs).astype(np.float64)
            assert x.size == n - (pu == full).sum()
            np.testing.assert_allclose(stats["loss"][e], np.log1p(np.exp(-x)).mean(), rtol=1e-12)
            assert stats["auc"][e] == (x > 0).mean()
        assert _bits(a) == _bits(b)
        # two epochs and then the third: the same bits
        first = c.fit_bpr(pu, pi, 2, seed=seed, candidates=m, refresh=refresh)
        last = c.fit_bpr(pu, pi, 1, seed=seed, first_epoch=2, candidates=m, refresh=refresh)
        for name in ("loss", "auc"):
            assert np.concatenate([first[name], last[name]]).tobytes() == stats[name].tobytes()
        assert _bits(a) == _bits(c)
        assert c.fit_bpr(pu, pi, 1, seed=seed, first_epoch=3, stats=False, candidates=m, refresh=refresh) is None
        assert c.fit_bpr(pu, pi, 0, seed=seed, candidates=m)["loss"].shape == (0,)


def test_the_picks_depend_on_refresh_and_the_candidates_do_not(mf):
    U, I, k, seed, m = 60, 50, 8, 21, 3
    rng = np.random.default_rng(15)
    pu, pi = rng.integers(0, U, 400).astype(np.int32), rng.integers(0, I, 400).astype(np.int32)
    new = lambda: mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED)
    with new() as a, new() as b:
        a.fit_bpr(pu, pi, 1, seed=seed, candidates=m)
        b.fit_bpr(pu, pi, 1, seed=seed, candidates=m, refresh=100)
        assert _bits(a) != _bits(b)
        # the second epoch's candidates for the rows of a block are one slice of sample_unseen, whatever the blocks were
        n = pu.size
        cand = a.sample_unseen(pu, m, seed, first=n * m)
        J = a.sample_unseen_hard(pu[100:200], m, seed, first=n * m + 100 * m, draws=True)
        assert np.array_equal(J[0], cand[100:200][np.arange(100), J[1]])


def test_one_candidate_is_the_call_without_the_argument(mf):
    U, I, k, seed = 60, 50, 8, 21
    rng = np.random.default_rng(16)
    pu, pi = rng.integers(0, U, 400).astype(np.int32), rng.integers(0, I, 400).astype(np.int32)
    new = lambda: mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED)
    with new() as a, new() as b:
        sa = a.fit_bpr(pu, pi, 2, seed=seed)
        sb = b.fit_bpr(pu, pi, 2, seed=seed, candidates=1, refresh=7)
        assert _bits(a) == _bits(b)
        assert all(sa[name].tobytes() == sb[name].tobytes() for name in ("loss", "auc"))


# ---- 7. it learns ------------------------------------------------------------------------------------------------------------------
def test_bpr_with_hard_negatives_learns_the_planted_one_class_problem(mf):
    """The planted problem of tests/test_pairwise_gpu.py, same data, k, lr and lambda: 600 users, 400 items in 20 groups of
    20; a user's 12 positives lie in the user's group, 11 to train on and 1 held out (and kept in the seen-item index, so
    never drawn); 20 epochs of fit_bpr with candidates=4.  A plain sequential BPR in numpy with the best of 4 unseen
    candidates reached a held-out hit rate at 10 of 1.0 after 20 epochs; the library's draws differ, so the bounds are
    that test's: untrained below 0.1, trained above 0.5, and the loss falling.
    Measured on an MI355X: untrained 0.02, after fit_bpr(candidates=4) 1.0 (mean loss 0.691 in the first epoch, 0.121 in
    the last: the negatives are chosen to be hard)."""
    U, I, G, k, lr, lam, seed = 600, 400, 20, 16, 0.05, 0.01, 3
    rng = np.random.default_rng(0)
    per = I // G
    its = np.stack([(u % G) * per + rng.choice(per, 12, replace=False) for u in range(U)]).astype(np.int32)
    hu, hi = np.arange(U, dtype=np.int32), its[:, 0].copy()
    pu, pi = np.repeat(hu, 11), its[:, 1:].ravel().copy()
    with mf.MatrixFactorizationSGD(U, I, k, lr, lam, seed) as h:
        h.set_seen(np.concatenate([pu, hu]), np.concatenate([pi, hi]))  # held-out positives are never negatives
        h.init_factors()
        untrained = h.evaluate_ranking(hu, hi, 10, exclude="seen")["hit_rate"]
        stats = h.fit_bpr(pu, pi, 20, seed=seed, candidates=4)
        trained = h.evaluate_ranking(hu, hi, 10, exclude="seen")["hit_rate"]
    print("held-out hit rate at 10: untrained", round(untrained, 4), "after fit_bpr(candidates=4)", round(trained, 4))
    print("loss per epoch:", np.round(stats["loss"], 4).tolist(), "auc:", np.round(stats["auc"], 4).tolist())
    assert untrained < 0.1
    assert trained > 0.5
    assert stats["loss"][-1] < stats["loss"][0]
