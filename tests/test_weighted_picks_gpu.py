"""Weighted picks on the device: mfsgd_sample_unseen_hard_weighted and mfsgd_sample_unseen_violating_weighted (csrc/pick.hip
under the weighted draw) and mfsgd_fold_in_users_pairwise_weighted (csrc/foldin_pairwise.hip under it) against the
restatements of tests/weighted_pick_common.py, every output byte for byte -- no tolerance, no statistics -- for every
lane-group size and the candidate counts around it; the shapes of weights and index; ties, NaN and infinite scores and
margins; the pieces a call is staged in; that a live handle stays whole; and fit_warp(sampling="weighted"),
fit_bpr(candidate_sampling="weighted") against the sequences of calls they are documented as.  The scorer is the
handle's own predict: its bits are pinned elsewhere."""
import numpy as np
import pytest

from tests import fold_in_pairwise_common as FC
from tests import implicit_common as IC
from tests import weighted_common as WM
from tests import weighted_pick_common as WP

pytestmark = pytest.mark.gpu

LR, LAM, SEED = 0.05, 0.01, 4
STATE = -5
CHUNK = IC.SAMPLE_CHUNK
U1, I1 = 40, 300
EVERY, NONE, ZERO_LEFT, ONE_LEFT, LEFT = 5, 9, 12, 20, 137
HARD_NAMES = ("items", "scores", "draws", "mass")
VIOL_NAMES = ("items", "draws", "margins", "ranks", "mass")
KS = (1, 6, 16, 20, 64, 100, 256)  # L = 1, 2, 4, 8, 16, 32, 64


def _group_lanes(k):
    L = 1
    while 4 * L < k:
        L *= 2
    return L


def _counts(L):
    """Round boundaries (a round is L draws) and chunks of the gather depth that do not divide m."""
    return sorted({m for m in (1, 2, L - 1, L, L + 1, 2 * L + 3, 37) if m >= 1})


def _keys(u, i):
    return (np.asarray(u).astype(np.int64) << 32) | np.asarray(i).astype(np.int64)


def _normal_factors(rng, U, I, k):
    return rng.standard_normal((U, k)).astype(np.float32), rng.standard_normal((I, k)).astype(np.float32)


def _pairs(rng):
    """About 1 500 pairs with a user who has seen everything, one without pairs, one whose unseen items all weigh nothing
    under _popular (while unseen items exist) and one with a single unseen item of positive weight."""
    eu, ei = rng.integers(0, U1, 1500).astype(np.int32), (I1 * rng.random(1500) ** 2).astype(np.int32)  # a long tail
    return eu, ei


def _popular(rng, eu, ei):
    """(w, eu, ei): popularity ** 0.75 of the pairs, with items that weigh nothing (the unpopular ones, and a planted run),
    and the pairs of the planted users on top."""
    counts = np.bincount(ei, minlength=I1)
    w = np.floor(counts.astype(np.float64) ** 0.75 * 16).astype(np.uint32)
    w[100:110] = 0
    w[[99, 110, LEFT]] = np.maximum(w[[99, 110, LEFT]], 3)
    assert (w == 0).sum() >= 10
    keep = ~np.isin(eu, (EVERY, NONE, ZERO_LEFT, ONE_LEFT))
    heavy = np.flatnonzero(w > 0)
    zero_left = np.concatenate([heavy, np.flatnonzero(w == 0)[::3]])  # every item of weight, and some of none
    one_left = np.setdiff1d(heavy, [LEFT])
    eu = np.concatenate([eu[keep], np.full(I1, EVERY), np.full(zero_left.size, ZERO_LEFT), np.full(one_left.size, ONE_LEFT)])
    ei = np.concatenate([ei[keep], np.arange(I1), zero_left, one_left])
    return w, eu.astype(np.int32), ei.astype(np.int32)


def _hard(h, lists, w, users, m, seed, first, what=""):
    got = h.sample_unseen_hard(users, m, seed, first, scores=True, draws=True, sampling="weighted", mass=True)
    WP.same(got, WP.hard(lists, w, users, m, seed, first, h.predict), HARD_NAMES, "hard " + what)
    return got


def _violating(h, lists, w, n_items, users, pos, m, margin, seed, first, what=""):
    got = h.sample_unseen_violating(users, pos, m, margin, seed, first, draws=True, margins=True, ranks=True, sampling="weighted",
                                    mass=True)
    WP.same(got, WP.violating(lists, w, n_items, users, pos, m, margin, seed, first, h.predict), VIOL_NAMES, "violating " + what)
    return got


# ---- 1. lane groups and candidate counts, popularity weights -------------------------------------------------------------------
@pytest.mark.parametrize("k", KS)
def test_lane_groups_and_candidate_counts(mf, k):
    L = _group_lanes(k)
    rng = np.random.default_rng(k)
    w, eu, ei = _popular(rng, *_pairs(rng))
    lists = IC.lists_of(eu, ei)
    P, Q = _normal_factors(rng, U1, I1, k)
    seed, first = 5, (1 << 40) + 7
    planted = np.array([EVERY, NONE, ZERO_LEFT, ONE_LEFT], np.int32)
    with mf.MatrixFactorizationSGD(U1, I1, k, LR, LAM, SEED) as h:
        h.set_factors(P, Q)
        h.set_seen(eu, ei)
        h.set_item_weights(w)
        for m in _counts(L):
            n = 256 // L + 9 if m > 2 else 300  # more than one block; every planted user among the rows
            users = np.concatenate([planted, rng.integers(0, U1, n).astype(np.int32)])
            pos = rng.integers(0, I1, users.size).astype(np.int32)
            what = f"k {k} m {m}"
            items, scores, draws, mass = _hard(h, lists, w, users, m, seed, first, what)
            none = (users == EVERY) | (users == ZERO_LEFT)
            assert ((items == -1) == none).all() and ((mass == 0) == none).all()
            assert (w[items[~none]] > 0).all()  # an item that weighs nothing is never returned
            assert not np.isin(_keys(users, items), _keys(eu, ei)).any()
            assert (items[users == ONE_LEFT] == LEFT).all() and (mass[users == ONE_LEFT] == w[LEFT]).all()
            assert np.array_equal(h.sample_unseen_hard(users, m, seed, first, sampling="weighted"), items)
            if m == 1:  # the weighted sampler's column, predict's scores
                col, col_mass = h.sample_unseen_weighted(users, 1, seed, first, mass=True)
                assert np.array_equal(items, col[:, 0]) and np.array_equal(mass, col_mass)
                assert scores[~none].tobytes() == h.predict(users[~none], items[~none]).tobytes() and (draws[~none] == 0).all()
            for margin in (1.0, -0.5):
                v_items, v_draws, _, v_ranks, v_mass = _violating(h, lists, w, I1, users, pos, m, margin, seed, first, what)
                assert np.array_equal(v_mass, mass) and (v_draws[none] == -1).all() and (v_draws[~none] >= 0).all()
                hit = v_items >= 0
                assert (w[v_items[hit]] > 0).all() and (v_items[hit] != pos[hit]).all()
                assert not np.isin(_keys(users[hit], v_items[hit]), _keys(eu, ei)).any()
                assert ((v_ranks > 0) == hit).all()
            assert hit.any()
            assert np.array_equal(h.sample_unseen_violating(users, pos, m, -0.5, seed, first, sampling="weighted"), v_items)


# ---- 2. the shapes of the weights and of the index --------------------------------------------------------------------------------
def test_weights_and_index_shapes(mf):
    k, m, seed = 6, 5, 9
    rng = np.random.default_rng(1)
    eu, ei = _pairs(rng)
    popular, pu, pi = _popular(rng, eu, ei)
    P, Q = _normal_factors(rng, U1, I1, k)
    users = np.append(rng.permutation(U1), [EVERY, ZERO_LEFT, 0]).astype(np.int32)
    pos = rng.integers(0, I1, users.size).astype(np.int32)
    nothing = lambda u: np.empty(0, np.int64)
    with mf.MatrixFactorizationSGD(U1, I1, k, LR, LAM, SEED) as h:
        h.set_factors(P, Q)
        # an empty index: no offsets, no mass table; every item of weight is a candidate
        h.set_seen([], [])
        h.set_item_weights(popular)
        items, _, _, mass = _hard(h, nothing, popular, users, m, seed, 0, "an empty index")
        assert (mass == int(popular.sum())).all() and (popular[items] > 0).all()
        _violating(h, nothing, popular, I1, users, pos, m, 0.5, seed, 0, "an empty index")
        h.set_seen(pu, pi)
        lists = IC.lists_of(pu, pi)
        # every weight the largest there is: masses of about 2^40
        big = np.full(I1, 0xFFFFFFFF, np.uint32)
        h.set_item_weights(big)
        items, _, _, mass = _hard(h, lists, big, users, m, seed, 1 << 40, "the largest weights")
        assert int(mass[users == NONE][0]) == I1 * 0xFFFFFFFF and ((items == -1) == (users == EVERY)).all()
        _violating(h, lists, big, I1, users, pos, m, 0.5, seed, 1 << 40, "the largest weights")
        # all zero: every row is -1
        zeros = np.zeros(I1, np.uint32)
        h.set_item_weights(zeros)
        items, scores, draws, mass = _hard(h, lists, zeros, users, m, seed, 0, "no weight at all")
        assert (items == -1).all() and (draws == -1).all() and (mass == 0).all() and (scores.view(np.uint32) == WP.NAN_BITS).all()
        v = _violating(h, lists, zeros, I1, users, pos, m, 0.5, seed, 0, "no weight at all")
        assert (v[0] == -1).all() and (v[1] == -1).all() and (v[3] == 0).all() and (v[2].view(np.uint32) == WP.NAN_BITS).all()
        # cnt_w == 0 with unseen items left, beside a user who has seen everything
        h.set_item_weights(popular)
        assert I1 - len(lists(ZERO_LEFT)) > 0 and len(lists(EVERY)) == I1
        v = _violating(h, lists, popular, I1, users, pos, m, np.inf, seed, 0, "planted users")
        for user in (ZERO_LEFT, EVERY):
            sel = users == user
            assert (v[0][sel] == -1).all() and (v[1][sel] == -1).all() and (v[3][sel] == 0).all() and (v[4][sel] == 0).all()
        sel = v[0] >= 0  # an infinite margin: the first candidate that is not the positive; N is the unseen COUNT
        assert sel[(users != ZERO_LEFT) & (users != EVERY) & (users != ONE_LEFT)].all()
        unseen = np.array([I1 - len(lists(int(u))) for u in users])
        assert np.array_equal(v[3][sel], np.maximum(1, unseen[sel] // (v[1][sel] + 1)))


# ---- 3. ties and specials ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (6, 64))
def test_ties_nan_and_infinite_scores_and_margins(mf, k):
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
    w = rng.integers(1, 9, I).astype(np.uint32)
    w[[5, 6, 7]] = 0
    users = np.tile(np.arange(U, dtype=np.int32), 30)
    # positives that come out among the candidates: heavy items, the one other item of two_left included
    pos = np.where(users == two_left, other_item, rng.choice(np.flatnonzero(w > 6), users.size)).astype(np.int32)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as h:
        h.set_factors(P, Q)
        h.set_seen(eu, ei)
        h.set_item_weights(w)
        for m in (2, 9, 40):
            items, scores, draws, _ = _hard(h, lists, w, users, m, seed, 0, f"k {k} m {m}")
            cand = WM.sample_weighted(lists, w, users, m, seed, 0)
            assert (w[cand] > 0).all()
            sc = h.predict(np.repeat(users, m), cand.ravel()).reshape(-1, m)
            plain = ~np.isin(users, (zero, minus_zero, nan_user, two_left)) & ~np.isnan(sc).all(axis=1)
            best = np.nanmax(sc[plain], axis=1)  # duplicated rows of Q: the smaller d wins, and the case occurs
            assert np.array_equal(draws[plain], np.argmax(sc[plain] == best[:, None], axis=1))
            assert m == 2 or ((sc[plain] == best[:, None]).sum(axis=1) > 1).any()
            assert np.isinf(sc[plain & np.isin(cand, [plus_inf, minus_inf]).any(axis=1)]).any()
            assert np.array_equal(scores[plain], best)
            sel = users == nan_user  # every score a NaN: d = 0
            assert np.isnan(sc[sel]).all() and (draws[sel] == 0).all() and np.array_equal(items[sel], cand[sel, 0])
            sel = users == two_left  # a NaN row of Q among the candidates loses
            has_other = (cand[sel] == other_item).any(axis=1)
            assert (items[sel][has_other] == other_item).all() and (items[sel][~has_other] == nan_item).all() and has_other.any()
            for margin in (0.0, 1.5, np.inf, -np.inf):
                v = _violating(h, lists, w, I, users, pos, m, margin, seed, 0, f"k {k} m {m} margin {margin}")
                if margin == np.inf:
                    # the positive among the candidates is skipped; two_left draws its positive or the NaN item: never a pick
                    skipped = (cand == pos[:, None]) & (np.arange(m) < v[1][:, None])
                    assert skipped.any() and (v[0] != pos).all() and (v[0][users == two_left] == -1).all()
                if margin == -np.inf:
                    assert (v[0] == -1).all() and (v[1] == m).all()
                assert (v[0][users == nan_user] == -1).all()  # NaN margins never violate


# ---- 4. cutting the call changes nothing -------------------------------------------------------------------------------------------
def _small(rng, U, I, pairs):
    eu, ei = rng.integers(0, U - 1, pairs).astype(np.int32), rng.integers(0, I, pairs).astype(np.int32)
    w = rng.integers(0, 1 << 20, I).astype(np.uint32)
    w[rng.random(I) < 0.2] = 0
    return eu, ei, IC.lists_of(eu, ei), w


def test_rows_of_a_call_are_the_call_on_those_rows(mf):
    U, I, k, m, seed, first = 40, 90, 16, 3, 11, 1 << 33
    rng = np.random.default_rng(6)
    eu, ei, lists, w = _small(rng, U, I, 160)
    users, pos = rng.integers(0, U, 1000).astype(np.int32), rng.integers(0, I, 1000).astype(np.int32)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as h:
        h.init_factors()
        h.set_seen(eu, ei)
        h.set_item_weights(w)
        whole = _hard(h, lists, w, users, m, seed, first)
        v_whole = _violating(h, lists, w, I, users, pos, m, 0.25, seed, first)
        for a, b in ((0, 7), (63, 65), (500, 1000), (999, 1000), (300, 300)):
            part = h.sample_unseen_hard(users[a:b], m, seed, first + a * m, scores=True, draws=True, sampling="weighted", mass=True)
            WP.same(part, tuple(x[a:b] for x in whole), HARD_NAMES, (a, b))
            part = h.sample_unseen_violating(users[a:b], pos[a:b], m, 0.25, seed, first + a * m, draws=True, margins=True,
                                             ranks=True, sampling="weighted", mass=True)
            WP.same(part, tuple(x[a:b] for x in v_whole), VIOL_NAMES, (a, b))


def test_a_call_longer_than_a_piece(mf):
    """n = 4 099 rows of m = 1 025 candidates, more than 2^22 in all: a piece is 4 092 rows, the last holds 7."""
    U, I, k, m, seed, first, n = 8, 200, 64, 1025, 11, 1 << 33, 4099
    rows = CHUNK // m
    assert n * m > CHUNK and 0 < n - rows < rows
    rng = np.random.default_rng(4)
    eu, ei, lists, w = _small(rng, U + 1, I, 300)
    users, pos = rng.integers(0, U, n).astype(np.int32), rng.integers(0, I, n).astype(np.int32)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as h:
        h.init_factors()
        h.set_seen(eu, ei)
        h.set_item_weights(w)
        kw = dict(sampling="weighted", mass=True)
        whole = h.sample_unseen_hard(users, m, seed, first, scores=True, draws=True, **kw)
        v_whole = h.sample_unseen_violating(users, pos, m, 0.0, seed, first, draws=True, margins=True, ranks=True, **kw)
        for a, b in ((rows - 2, rows + 2), (rows, n), (5, rows + 1)):  # across the boundary, and cut elsewhere
            part = h.sample_unseen_hard(users[a:b], m, seed, first + a * m, scores=True, draws=True, **kw)
            WP.same(part, tuple(x[a:b] for x in whole), HARD_NAMES, (a, b))
            part = h.sample_unseen_violating(users[a:b], pos[a:b], m, 0.0, seed, first + a * m, draws=True, margins=True, ranks=True, **kw)
            WP.same(part, tuple(x[a:b] for x in v_whole), VIOL_NAMES, (a, b))
        sampled = np.unique(np.concatenate([[0, rows - 1, rows, n - 1], rng.integers(0, n, 60)]))[:64]
        for x in sampled:
            want = WP.hard(lists, w, users[x:x + 1], m, seed, first + int(x) * m, h.predict)
            WP.same(tuple(a[x:x + 1] for a in whole), want, HARD_NAMES, f"row {x}")
            want = WP.violating(lists, w, I, users[x:x + 1], pos[x:x + 1], m, 0.0, seed, first + int(x) * m, h.predict)
            WP.same(tuple(a[x:x + 1] for a in v_whole), want, VIOL_NAMES, f"row {x}")


def test_one_row_longer_than_a_piece_is_a_piece_of_its_own(mf):
    """m = 2^22 + 5: one lane group walks the row's candidates in rounds of L = 16 draws."""
    U, I, k, seed = 30, 200, 64, 2
    m = CHUNK + 5
    rng = np.random.default_rng(9)
    eu, ei, lists, w = _small(rng, U, I, 300)
    users = np.array([1], np.int32)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as h:
        h.init_factors()
        h.set_seen(eu, ei)
        h.set_item_weights(w)
        _hard(h, lists, w, users, m, seed, 3)
        # a margin nothing falls below: the whole row is walked
        got = _violating(h, lists, w, I, users, np.array([7], np.int32), m, -1e30, seed, 3)
        assert got[1][0] == m


# ---- 5. a live handle stays whole --------------------------------------------------------------------------------------------------
def test_side_effects(mf):
    U, I, k, m, seed = 40, 90, 16, 6, 5
    rng = np.random.default_rng(12)
    eu, ei = rng.integers(0, U, 900).astype(np.int32), rng.integers(0, I, 900).astype(np.int32)
    lists = IC.lists_of(eu, ei)
    w = rng.integers(0, 50, I).astype(np.uint32)
    users, pos = rng.integers(0, U, 3000).astype(np.int32), rng.integers(0, I, 3000).astype(np.int32)
    row_ptr, new_items = FC.csr([[1, 5, 5], [], [8]])
    start = mf.debug_device_bytes()
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as h:
        h.init_factors()
        h.set_ratings(eu, ei, rng.random(eu.size, dtype=np.float32))
        h.set_seen(eu, ei)
        h.set_item_weights(w)
        h.fit(1, rmse=False)
        P, Q = h.get_factors()
        ptr, seen = h.seen(np.arange(U))
        table = h.sample_unseen_weighted(users, 2, 1, mass=True)  # what the mass table gives
        size, counters, live = h.seen_size(), h.debug_counters(), mf.debug_device_bytes()
        assert live > start
        got = _hard(h, lists, w, users, m, seed, 0)
        assert mf.debug_device_bytes() == live
        v_got = _violating(h, lists, w, I, users, pos, m, 0.5, seed, 0)
        assert mf.debug_device_bytes() == live
        h.fold_in_pairwise(row_ptr, new_items, 2, candidates=3, sampling="weighted", margins=True, negatives=True)
        assert mf.debug_device_bytes() == live
        WP.same(h.sample_unseen_hard(users, m, seed, 0, scores=True, draws=True, sampling="weighted", mass=True), got, HARD_NAMES, "twice")
        for refused in (lambda: h.sample_unseen_hard([0, U], m, seed, sampling="weighted"),
                        lambda: h.sample_unseen_violating([0, 1], [0, I], m, sampling="weighted"),
                        lambda: h.fold_in_pairwise([0, 1], [I], 1, sampling="weighted")):
            with pytest.raises(mf.MfsgdError) as e:  # a refused call holds nothing either
                refused()
            assert e.value.code == -1 and mf.debug_device_bytes() == live
        P2, Q2 = h.get_factors()
        assert P2.tobytes() == P.tobytes() and Q2.tobytes() == Q.tobytes()
        ptr2, seen2 = h.seen(np.arange(U))
        assert h.seen_size() == size and np.array_equal(ptr, ptr2) and np.array_equal(seen, seen2)
        assert np.array_equal(h.item_weights(), w)
        again = h.sample_unseen_weighted(users, 2, 1, mass=True)
        assert np.array_equal(again[0], table[0]) and np.array_equal(again[1], table[1])
        assert h.debug_counters() == counters  # schedule builds, cached graphs, the launch path
        # the uniform calls are the uniform calls, weights or none
        uniform = h.sample_unseen_hard(users, m, seed, 0, scores=True, draws=True)
        assert np.array_equal(uniform[0], h.sample_unseen_hard(users, m, seed, 0, sampling="uniform"))
        # items appended: the weights no longer cover the model, and every weighted call says so until they are set again
        h.add_items(n=3, seed=2)
        for stale in (lambda: h.sample_unseen_hard(users, m, seed, sampling="weighted"),
                      lambda: h.sample_unseen_violating(users, pos, m, sampling="weighted"),
                      lambda: h.fold_in_pairwise(row_ptr, new_items, 1, sampling="weighted")):
            with pytest.raises(mf.MfsgdError) as e:
                stale()
            assert e.value.code == STATE and f"item weights cover {I} items, the model has {I + 3}" in str(e.value)
        with pytest.raises(ValueError):
            h.fit_warp(eu, ei, 1, sampling="weighted")
        w3 = np.append(w, [7, 0, 9]).astype(np.uint32)
        h.set_item_weights(w3)
        items, _, _, _ = _hard(h, lists, w3, users, m, seed, 0, "after add_items")
        _violating(h, lists, w3, I + 3, users, pos, m, 0.5, seed, 0, "after add_items")
        assert (h.sample_unseen_weighted(users, m, seed) == I).any() and not (items == I + 1).any()
    assert mf.debug_device_bytes() == start


# ---- 6. the fits are the sequences they are documented as ------------------------------------------------------------------------
def _bits(m):
    P, Q = m.get_factors()
    return P.tobytes(), Q.tobytes()


def _positives(rng, U, I, full):
    pu, pi = rng.integers(0, U, 400).astype(np.int32), rng.integers(0, I, 400).astype(np.int32)  # duplicates among them
    pu, pi = np.concatenate([pu, np.full(I, full)]).astype(np.int32), np.concatenate([pi, np.arange(I)]).astype(np.int32)
    order = rng.permutation(pu.size)
    return pu[order], pi[order]


@pytest.mark.parametrize("refresh", (None, 128))
def test_fit_warp_weighted_is_its_documented_sequence(mf, refresh):
    U, I, k, epochs, seed, full, m, margin = 60, 50, 8, 3, 21, 17, 5, 0.5
    rng = np.random.default_rng(5)
    pu, pi = _positives(rng, U, I, full)
    n = pu.size
    step = n if refresh is None else refresh
    assert refresh is None or n % refresh != 0
    new = lambda: mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED)
    with new() as a, new() as b, new() as c:
        for h in (a, b, c):
            h.set_seen(pu, pi)
            h.set_popularity_weights(least=0)
        w = a.item_weights()
        lists = IC.lists_of(pu, pi)
        kw = dict(candidates=m, margin=margin, refresh=refresh, seed=seed, sampling="weighted")
        stats = a.fit_warp(pu, pi, epochs, **kw)
        b.init_factors()
        violating, trials = [], []
        for e in range(epochs):
            hits = draws = 0
            for lo in range(0, n, step):
                bu, bi = pu[lo:lo + step], pi[lo:lo + step]
                first = (e * n + lo) * m
                J, d, _, rk, _ = _violating(b, lists, w, I, bu, bi, m, margin, seed, first, f"epoch {e} block {lo}")
                assert (J[bu == full] == -1).all()
                keep = J >= 0
                b.partial_fit_pairwise(bu[keep], bi[keep], J[keep], weights=mf.warp_weights(rk[keep]))
                hits += int(keep.sum())
                draws += int(d[keep].astype(np.int64).sum()) + int(keep.sum())
            violating.append(hits / n)
            trials.append(draws / hits if hits else 0.0)
        assert stats["violating"].tobytes() == np.array(violating).tobytes() and stats["trials"].tobytes() == np.array(trials).tobytes()
        assert _bits(a) == _bits(b) and stats["violating"][0] > 0
        s1 = c.fit_warp(pu, pi, 2, **kw)
        s2 = c.fit_warp(pu, pi, 1, first_epoch=2, **kw)
        for name in ("violating", "trials"):
            assert np.concatenate([s1[name], s2[name]]).tobytes() == stats[name].tobytes()
        assert _bits(a) == _bits(c)
    with new() as a, new() as b:  # sampling="uniform" is the call without the keyword, weights or none
        a.set_seen(pu, pi)
        a.set_popularity_weights()
        sa = a.fit_warp(pu, pi, 2, candidates=m, seed=seed, refresh=refresh, sampling="uniform")
        sb = b.fit_warp(pu, pi, 2, candidates=m, seed=seed, refresh=refresh)
        assert sa["trials"].tobytes() == sb["trials"].tobytes() and _bits(a) == _bits(b)


@pytest.mark.parametrize("refresh", (None, 128))
def test_fit_bpr_with_weighted_candidates_is_its_documented_sequence(mf, refresh):
    U, I, k, epochs, seed, full, m = 60, 50, 8, 3, 13, 17, 4
    rng = np.random.default_rng(6)
    pu, pi = _positives(rng, U, I, full)
    n = pu.size
    step = n if refresh is None else refresh
    new = lambda: mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED)
    with new() as a, new() as b, new() as c:
        for h in (a, b, c):
            h.set_seen(pu, pi)
            h.set_popularity_weights(least=0)
        w = a.item_weights()
        lists = IC.lists_of(pu, pi)
        kw = dict(candidates=m, refresh=refresh, seed=seed, candidate_sampling="weighted")
        stats = a.fit_bpr(pu, pi, epochs, **kw)
        b.init_factors()
        loss, auc = [], []
        for e in range(epochs):
            xs = []
            for lo in range(0, n, step):
                bu, bi = pu[lo:lo + step], pi[lo:lo + step]
                J = _hard(b, lists, w, bu, m, seed, (e * n + lo) * m, f"epoch {e} block {lo}")[0]
                keep = J >= 0
                assert not keep[bu == full].any() and (w[J[keep]] > 0).all()
                xs.append(b.partial_fit_pairwise(bu[keep], bi[keep], J[keep], margins=True))
            x = np.concatenate(xs).astype(np.float64)
            loss.append(np.logaddexp(0.0, -x).mean())
            auc.append((x > 0).mean())
        assert stats["loss"].tobytes() == np.array(loss).tobytes() and stats["auc"].tobytes() == np.array(auc).tobytes()
        assert _bits(a) == _bits(b)
        s1 = c.fit_bpr(pu, pi, 2, **kw)
        s2 = c.fit_bpr(pu, pi, 1, first_epoch=2, **kw)
        for name in ("loss", "auc"):
            assert np.concatenate([s1[name], s2[name]]).tobytes() == stats[name].tobytes()
        assert _bits(a) == _bits(c)
        assert c.fit_bpr(pu, pi, 1, first_epoch=3, stats=False, **kw) is None
        with pytest.raises(ValueError):  # still refused, as it was
            c.fit_bpr(pu, pi, 1, candidates=m, sampling="weighted")
    with new() as a, new() as b:  # candidate_sampling="uniform" is the call without the keyword, weights or none
        a.set_seen(pu, pi)
        a.set_popularity_weights()
        sa = a.fit_bpr(pu, pi, 2, candidates=m, seed=seed, refresh=refresh, candidate_sampling="uniform")
        sb = b.fit_bpr(pu, pi, 2, candidates=m, seed=seed, refresh=refresh)
        assert sa["loss"].tobytes() == sb["loss"].tobytes() and _bits(a) == _bits(b)


# ---- 7. the weighted fold-in -----------------------------------------------------------------------------------------------------------
N_ITEMS = 61


def _fold_weights(rng):
    w = rng.integers(1, 1 << 16, N_ITEMS).astype(np.uint32)
    w[rng.random(N_ITEMS) < 0.25] = 0
    w[[0, 33, N_ITEMS - 1]] = (0, 9, 0)
    return w


def _fold_lists(rng, w, n_users=21):
    """The edge cases first -- no positives; one; an item twice (and three times); every item; every item of positive weight
    (no unseen weight, unseen items left); every such item but one -- then random lengths up to 12."""
    heavy = [int(i) for i in rng.permutation(np.flatnonzero(w > 0))]
    lists = [[], [7], [5, 9, 5, 5, 2, 9], [int(i) for i in rng.permutation(N_ITEMS)], heavy, [i for i in heavy if i != 33], []]
    while len(lists) < n_users:
        lists.append([int(i) for i in rng.integers(0, N_ITEMS, int(rng.integers(1, 13)))])
    return lists


def _model(mf, Q, k, w, users=4, seed=11):
    m = mf.MatrixFactorizationSGD(users, Q.shape[0], k, LR, LAM, seed)
    m.set_factors(np.zeros((users, k), np.float32), Q)
    m.set_item_weights(w)
    return m


def _same_fold(got, want, what=""):
    for g, x, name in zip(got, want, ("rows", "margins", "negatives")):
        assert FC.same_bits(np.ascontiguousarray(g), np.ascontiguousarray(x)), f"{name} differ {what}"


@pytest.mark.parametrize("k", KS)
def test_weighted_fold_in_matches_the_restatement_for_every_group_width(mf, k):
    L = _group_lanes(k)
    rng = np.random.default_rng(300 + k)
    w = _fold_weights(rng)
    lists = _fold_lists(rng, w)
    row_ptr, items = FC.csr(lists)
    n_new, seed, first = len(lists), 77, 12345
    Q = (rng.standard_normal((N_ITEMS, k)) * (1.0 / np.sqrt(k))).astype(np.float32)
    init = rng.standard_normal((n_new, k)).astype(np.float32)
    start = mf.debug_device_bytes()
    with _model(mf, Q, k, w) as m:
        m.predict([0], [0])  # (factors still staged on the host move to the device with the first call that reads them)
        model, live = _bits(m), mf.debug_device_bytes()
        for cand in sorted({1, 3, L + 1}):
            for epochs in (0, 1, 3):
                what = f"k={k} m={cand} epochs={epochs}"
                want = WP.fold(Q, w, row_ptr, items, epochs, cand, init, LR, LAM, seed, first)
                assert np.isfinite(want[0]).all()
                kw = dict(candidates=cand, draw_seed=seed, margins=True, negatives=True, sampling="weighted")
                got = m.fold_in_pairwise(row_ptr, items, epochs, init=init, first=first, **kw)
                _same_fold(got, want, what)
                assert mf.debug_device_bytes() == live
                o = row_ptr * epochs
                # no unseen weight (every item named, or every item of weight): no step; one such item left: always that one
                for x in (3, 4):
                    assert (got[2][o[x]:o[x + 1]] == -1).all() and (got[1].view(np.uint32)[o[x]:o[x + 1]] == WP.NAN_BITS).all()
                    assert FC.same_bits(got[0][x], init[x])
                assert (got[2][o[5]:o[6]] == 33).all() and FC.same_bits(got[0][0], init[0])
                assert (w[got[2][got[2] >= 0]] > 0).all()  # never a negative that weighs nothing
                # the call split by users, row_ptr and first rebased: the whole call
                cut = 9
                for a, b in ((0, cut), (cut, n_new)):
                    part = m.fold_in_pairwise(row_ptr[a:b + 1] - row_ptr[a], items[row_ptr[a]:row_ptr[b]], epochs, init=init[a:b],
                                              first=first + int(row_ptr[a]) * epochs * cand, **kw)
                    _same_fold(part, (got[0][a:b], got[1][o[a]:o[b]], got[2][o[a]:o[b]]), what + f" users {a}:{b}")
        # the rows alone; and the uniform call is the uniform call on a handle with weights
        assert FC.same_bits(m.fold_in_pairwise(row_ptr, items, 1, init=init, draw_seed=seed, sampling="weighted"),
                            WP.fold(Q, w, row_ptr, items, 1, 1, init, LR, LAM, seed, 0)[0])
        _same_fold(m.fold_in_pairwise(row_ptr, items, 1, init=init, draw_seed=seed, margins=True, negatives=True, sampling="uniform"),
                   FC.fold(Q, row_ptr, items, 1, 1, init, LR, LAM, seed, 0), "uniform")
        assert _bits(m) == model and np.array_equal(m.item_weights(), w) and m.seen_size() == -1
        assert mf.debug_device_bytes() == live
    assert mf.debug_device_bytes() == start


def test_weighted_fold_in_negatives_are_the_weighted_sampler_s(mf):
    rng = np.random.default_rng(21)
    k, epochs, seed, first = 16, 2, -5, 999
    w = _fold_weights(rng)
    lists = _fold_lists(rng, w)
    row_ptr, items = FC.csr(lists)
    Q = (rng.standard_normal((N_ITEMS, k)) * 0.25).astype(np.float32)
    init = rng.standard_normal((len(lists), k)).astype(np.float32)
    with _model(mf, Q, k, w) as m, mf.MatrixFactorizationSGD(len(lists), N_ITEMS, k, LR, LAM, 1) as twin:
        twin.set_seen(np.repeat(np.arange(len(lists)), np.diff(row_ptr)), items)
        twin.set_item_weights(w)
        _, negs = m.fold_in_pairwise(row_ptr, items, epochs, init=init, draw_seed=seed, first=first, negatives=True, sampling="weighted")
        for x, A in enumerate(lists):
            steps, o = len(A) * epochs, int(row_ptr[x]) * epochs
            if steps:
                want = twin.sample_unseen_weighted(np.full(steps, x, np.int32), 1, seed, first=first + o)[:, 0]
                assert np.array_equal(negs[o:o + steps], want), f"user {x}"
