"""WARP on the device: mfsgd_sample_unseen_violating (csrc/pick.hip) against the numpy restatement of its rule
(tests/warp_common.py) -- items, draws, margins and ranks, byte for byte -- for the lane-group sizes, the candidate counts
around a round and the margins that are special; the shapes of the seen-item index; that a call may be cut and leaves a
live handle whole; mfsgd_apply_triples_weighted against the sequential loop restated in C; and fit_warp against the loop it
is documented as."""
import functools

import numpy as np
import pytest

from tests import implicit_common as IC
from tests import warp_common as WC

pytestmark = pytest.mark.gpu

LR, LAM, SEED = 0.05, 0.01, 4
U, I = 24, 40
EVERY, ONE_LEFT, LEFT, OUTSIDE, ZERO = 3, 7, 29, 11, 5  # users who have seen all / all but LEFT; whose positive is unseen; -0.0
NAN_ITEM = 17
NAMES = ("items", "draws", "margins", "ranks")


def _group_lanes(k):
    """L: lanes per row, the power of two that holds k floats in chunks of four."""
    L = 1
    while 4 * L < k:
        L *= 2
    return L


def _same(got, want, what):
    for g, w, name in zip(got, want, NAMES):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name)
        if g.tobytes() != w.tobytes():
            bad = np.flatnonzero(g.view(np.uint32) != w.view(np.uint32))
            raise AssertionError(f"{what}: {bad.size} {name} differ, first at rows {bad[:5]}: {g[bad[:5]]} instead of {w[bad[:5]]}")


def _call(h, users, pos, m, margin, seed, first):
    return h.sample_unseen_violating(users, pos, m, margin, seed, first, draws=True, margins=True, ranks=True)


def _compare(h, lists, n_items, users, pos, m, margin, seed, first, scorer, what=""):
    """One call with every output against the restatement; returns what the call gave."""
    got = _call(h, users, pos, m, margin, seed, first)
    _same(got, WC.violating(lists, n_items, users, pos, m, margin, seed, first, scorer), what)
    return got


def _index(rng):
    """A few pairs per user; EVERY has seen every item, ONE_LEFT all but LEFT."""
    eu, ei = rng.integers(0, U, 4 * U).astype(np.int32), rng.integers(0, I, 4 * U).astype(np.int32)
    keep = ~np.isin(eu, (EVERY, ONE_LEFT)) & ~((eu == OUTSIDE) & (ei == I - 3))  # (OUTSIDE's positive is I - 3: test 1)
    rest = np.setdiff1d(np.arange(I), [LEFT])
    eu = np.concatenate([eu[keep], np.full(I, EVERY), np.full(rest.size, ONE_LEFT)]).astype(np.int32)
    ei = np.concatenate([ei[keep], np.arange(I), rest]).astype(np.int32)
    return eu, ei


def _ranked_factors(rng, k):
    """Every user scores the items in ascending order of their number, 0.5 apart but for a little noise, and the last one
    5 above the rest: how soon a candidate violates is then a matter of where the row's positive stands -- a low one is
    overtaken by the first draw, a high one after many draws, the last one by none."""
    P, Q = (0.01 * rng.standard_normal((U, k))).astype(np.float32), (0.01 * rng.standard_normal((I, k))).astype(np.float32)
    P[:, 0], Q[:, 0] = 1.0, 0.5 * np.arange(I)
    Q[I - 1, 0] += 5.0
    return P, Q


# ---- 1. lane groups, candidate counts and margins -----------------------------------------------------------------------------
def _mixed_waves(items, draws, m, rows):
    """How many waves -- `rows` consecutive rows, from a multiple of `rows` on -- hold both a row whose first draw is its
    pick and a live row that walks all m draws without one (draws == m: not a user who has seen everything, whose group
    never enters the rounds): the groups of such a wave leave the rounds at different trips, by the ballot."""
    n = items.size // rows * rows
    first = ((items >= 0) & (draws == 0))[:n].reshape(-1, rows).any(axis=1)
    never = ((items < 0) & (draws == m))[:n].reshape(-1, rows).any(axis=1)
    return int((first & never).sum())


# L = 1, 4 and 8 (64, 16 and 8 rows to a wave: each finds its pick in a round of its own); pad columns and L = 2; L = 16;
# the permlane level; one group per wave
@pytest.mark.parametrize("k", (3, 5, 12, 20, 64, 128, 256))
def test_lane_groups_candidate_counts_and_margins(mf, oracle, k):
    seed, first, n = 5, (1 << 40) + 7, 700
    L = _group_lanes(k)
    rng = np.random.default_rng(k)
    eu, ei = _index(rng)
    lists = IC.lists_of(eu, ei)
    P, Q = _ranked_factors(rng, k)
    P[ZERO] = -0.0  # a row of -0.0: every difference is +0.0 or -0.0
    scorer = lambda u, i: oracle.predict(P, Q, u, i)
    users = rng.integers(0, U, n).astype(np.int32)  # repeated, in any order
    pos = rng.integers(0, I, n).astype(np.int32)
    pos[::9] = I - 1  # the item nobody overtakes
    pos[1::9] = I - 2  # ... and the one a single item does: a violator turns up late
    out = np.flatnonzero(users == OUTSIDE)
    pos[out] = I - 3  # not in OUTSIDE's list (below), and high: it is drawn before anything violates
    assert not np.isin(I - 3, lists(OUTSIDE)) and out.size > 10
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as h:
        h.set_factors(P, Q)
        h.set_seen(eu, ei)
        for m in sorted({m for m in (1, L - 1, L, L + 1, 2 * L + 3) if m >= 1}):
            cand = IC.sample(lists, I, users, m, seed, first)
            for margin in (0.0, 1.0, np.inf, -np.inf):
                what = f"k {k} m {m} margin {margin}"
                items, draws, margins, ranks = _compare(h, lists, I, users, pos, m, margin, seed, first, scorer, what)
                assert np.array_equal(h.sample_unseen_violating(users, pos, m, margin, seed, first), items)  # without the rest
                full = users == EVERY
                assert (items[full] == -1).all() and (draws[full] == -1).all() and (ranks[full] == 0).all()
                assert (margins.view(np.uint32)[items < 0] == WC.NAN_BITS).all()
                hit = items >= 0
                assert not np.isin((users[hit].astype(np.int64) << 32) | items[hit], (eu.astype(np.int64) << 32) | ei).any()
                assert (items[hit] != pos[hit]).all()
                one = users == ONE_LEFT
                assert np.isin(items[one], (LEFT, -1)).all() and (ranks[one & hit] == 1).all() and (draws[one & hit] == 0).all()
                if margin == -np.inf:
                    assert not hit.any() and (draws[~full] == m).all()
                    continue
                assert (draws[hit] == 0).any()
                # the reference reaches the places the kernel can go wrong in: a pick in a later round, none at all, and
                # the positive drawn before the pick
                if m == 2 * L + 3 and margin != np.inf:
                    assert (draws[hit] >= L).any(), what
                if margin != np.inf:
                    assert (draws[~full] == m).any(), what
                if L <= 8 and margin != np.inf:  # (the outputs are the reference's by now) many rows to a wave, and in some
                    # waves a pick at the first draw beside a row without any: the ballot exit with mixed groups
                    assert _mixed_waves(items, draws, m, 64) > 0 and _mixed_waves(items, draws, m, 64 // L) > 0, what
                if m > 1 and margin == 1.0:  # (its own difference is 0: below the margin, were it not passed over)
                    upto = np.where(hit, draws, m)[out]
                    assert any((cand[r, :d] == pos[r]).any() for r, d in zip(out, upto)), what
                if margin == 1.0:
                    zero = users == ZERO
                    assert (zero & hit).any() and (margins[zero & hit] == 0).all()
                if margin == 0.0:
                    assert not (hit & (users == ZERO)).any()  # -0.0 < +0.0 is false
                if m == 1 and margin == np.inf:  # the draw itself, wherever the candidate is not the positive
                    column = h.sample_unseen(users, 1, seed, first)[:, 0]
                    ok = (column != pos) & (column >= 0)
                    assert np.array_equal(items[ok], column[ok]) and (items[~ok] == -1).all()


# ---- 2. NaN scores: the handle's own predict is the scorer ----------------------------------------------------------------------
@pytest.mark.parametrize("k", (5, 64))
def test_a_nan_row_of_q(mf, k):
    seed, n, m = 2, 600, 9
    rng = np.random.default_rng(100 + k)
    eu, ei = _index(rng)
    lists = IC.lists_of(eu, ei)
    P, Q = _ranked_factors(rng, k)
    Q[NAN_ITEM, k - 1] = np.nan
    users, pos = rng.integers(0, U, n).astype(np.int32), rng.integers(0, I, n).astype(np.int32)
    pos[::5] = NAN_ITEM  # a NaN positive: nothing violates
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as h:
        h.set_factors(P, Q)
        h.set_seen(eu, ei)
        for margin in (1.0, np.inf):
            items, draws, margins, ranks = _compare(h, lists, I, users, pos, m, margin, seed, 0, h.predict, f"k {k} margin {margin}")
            assert (items != NAN_ITEM).all() and not np.isnan(margins[items >= 0]).any()
            assert (items[pos == NAN_ITEM] == -1).all()
            cand = IC.sample(lists, I, users, m, seed, 0)
            passed = [(cand[r, :draws[r]] == NAN_ITEM).any() for r in np.flatnonzero(items >= 0)]
            assert any(passed)  # a NaN candidate was passed over on the way to a pick


# ---- 3. the shapes of the index ---------------------------------------------------------------------------------------------------
def test_an_empty_index_and_appended_rows(mf, oracle):
    k, m, seed = 5, 6, 9
    rng = np.random.default_rng(1)
    P, Q = _ranked_factors(rng, k)
    users, pos = rng.integers(0, U, 300).astype(np.int32), rng.integers(0, I, 300).astype(np.int32)
    nothing = lambda u: np.empty(0, np.int64)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as h:
        h.reserve(users=U + 4, items=I + 8)
        h.set_factors(P, Q)
        h.set_seen([], [])  # an empty index: every item is a candidate
        _compare(h, nothing, I, users, pos, m, 1.0, seed, 0, lambda u, i: oracle.predict(P, Q, u, i), "an empty index")
        eu, ei = _index(rng)
        lists = IC.lists_of(eu, ei)
        h.set_seen(eu, ei)
        assert h.add_users(n=2, seed=3) == U and h.add_items(n=5, seed=4) == I
        P2, Q2 = h.get_factors()
        more = np.append(users, [U + 1, U, EVERY]).astype(np.int32)
        mpos = np.append(pos, [I + 4, 0, I]).astype(np.int32)
        items, _, _, _ = _compare(h, lists, I + 5, more, mpos, 16, np.inf, seed, 0, lambda u, i: oracle.predict(P2, Q2, u, i), "grown")
        assert items.max() < I + 5 and (items[more == EVERY] >= I).all()  # all that the user who had seen everything can get


# ---- 4. cutting the call changes nothing ---------------------------------------------------------------------------------------------
def test_rows_of_a_call_are_the_call_on_those_rows(mf, oracle):
    k, m, seed, first = 64, 19, 11, 1 << 33
    rng = np.random.default_rng(6)
    eu, ei = _index(rng)
    lists = IC.lists_of(eu, ei)
    P, Q = _ranked_factors(rng, k)
    users, pos = rng.integers(0, U, 1000).astype(np.int32), rng.integers(0, I, 1000).astype(np.int32)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as h:
        h.set_factors(P, Q)
        h.set_seen(eu, ei)
        whole = _compare(h, lists, I, users, pos, m, 1.0, seed, first, lambda u, i: oracle.predict(P, Q, u, i))
        for a, b in ((0, 7), (15, 17), (500, 1000), (999, 1000), (300, 300)):
            part = _call(h, users[a:b], pos[a:b], m, 1.0, seed, first + a * m)
            _same(part, tuple(w[a:b] for w in whole), (a, b))


def test_a_call_longer_than_a_piece(mf):
    """k = 4, m = 4, n = 2^20 + 3: a piece is 2^20 rows, the last holds 3.  The handle's predict is the scorer."""
    UU, II, k, m, seed, first = 300, 200, 4, 4, 11, 1 << 33
    n = IC.SAMPLE_CHUNK // m + 3
    rng = np.random.default_rng(4)
    eu, ei = rng.integers(0, UU - 1, 4 * UU).astype(np.int32), rng.integers(0, II, 4 * UU).astype(np.int32)
    lists = IC.lists_of(eu, ei)
    users, pos = rng.integers(0, UU, n).astype(np.int32), rng.integers(0, II, n).astype(np.int32)
    with mf.MatrixFactorizationSGD(UU, II, k, LR, LAM, SEED) as h:
        h.init_factors()
        h.set_seen(eu, ei)
        whole = _compare(h, lists, II, users, pos, m, 0.0, seed, first, h.predict)
        assert (whole[0] >= 0).any() and (whole[1] == m).any()
        rows = IC.SAMPLE_CHUNK // m
        for a, b in ((rows - 2, rows + 2), (rows, n)):
            part = _call(h, users[a:b], pos[a:b], m, 0.0, seed, first + a * m)
            _same(part, tuple(w[a:b] for w in whole), (a, b))


# ---- 5. a live handle stays whole ----------------------------------------------------------------------------------------------------
def test_side_effects(mf, oracle):
    k, m, seed = 16, 6, 5
    rng = np.random.default_rng(12)
    eu, ei = _index(rng)
    lists = IC.lists_of(eu, ei)
    users, pos = rng.integers(0, U, 3000).astype(np.int32), rng.integers(0, I, 3000).astype(np.int32)
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
        got = _compare(h, lists, I, users, pos, m, 0.0, seed, 0, lambda u, i: oracle.predict(P, Q, u, i))
        assert mf.debug_device_bytes() == live
        _same(_call(h, users, pos, m, 0.0, seed, 0), got, "the same call twice")
        assert h.sample_unseen_violating(users, pos, m, 0.0, seed).dtype == np.int32 and mf.debug_device_bytes() == live
        for bad_u, bad_i in (([0, U], [0, 0]), ([0, 1], [0, I])):  # a refused call holds nothing either
            with pytest.raises(mf.MfsgdError) as e:
                h.sample_unseen_violating(bad_u, bad_i, m, 0.0, seed)
            assert e.value.code == -1 and mf.debug_device_bytes() == live
        P2, Q2 = h.get_factors()
        assert P2.tobytes() == P.tobytes() and Q2.tobytes() == Q.tobytes()
        ptr2, seen2 = h.seen(np.arange(U))
        assert h.seen_size() == size and np.array_equal(ptr, ptr2) and np.array_equal(seen, seen2)
        assert h.debug_counters() == counters  # schedule builds, cached graphs, the launch path
        # the margin of a pick is the margin apply_triples reports for the triple under the same factors
        ok = np.flatnonzero(got[0] >= 0)
        _, first_of = np.unique(users[ok], return_index=True)  # one triple per user: level 0 is the factors as they are ...
        rows = ok[first_of]
        _, a = np.unique(pos[rows], return_index=True)
        rows = rows[a]
        rows = rows[~np.isin(got[0][rows], pos[rows])]
        _, a = np.unique(got[0][rows], return_index=True)  # ... when no item is named twice either
        rows = rows[a]
        assert rows.size >= 3
        x, info = h.partial_fit_pairwise(users[rows], pos[rows], got[0][rows], weights=np.zeros(rows.size), margins=True, info=True)
        assert info["levels"] == 1 and x.tobytes() == got[2][rows].tobytes()
        assert mf.debug_device_bytes() == live
    assert mf.debug_device_bytes() == start


# ---- 6. the weighted step ------------------------------------------------------------------------------------------------------------
def _nan_alike(got, want, what):
    """NaN payloads and signs are not part of the contract: which entries are NaN is, and every other bit."""
    for g, w in zip(got, want):
        assert np.array_equal(np.isnan(g), np.isnan(w)), what
        assert np.array_equal(g.view(np.uint32)[~np.isnan(w)], w.view(np.uint32)[~np.isnan(w)]), what


def _hot_batch(rng, n=400):
    """A few hundred triples over few rows, every fifth on user 1 and every seventh on item 2: many levels."""
    UU, II = 30, 26
    u, i = rng.integers(0, UU, n).astype(np.int32), rng.integers(0, II, n).astype(np.int32)
    u[::5], i[::7] = 1, 2
    j = ((i + rng.integers(1, II, n)) % II).astype(np.int32)
    return UU, II, u, i, j


@pytest.mark.parametrize("k", (1, 5, 16, 20, 64, 100, 256))  # L = 1, 2, 4, 8, 16, 32, 64
def test_the_weighted_step_is_the_sequential_loop(mf, oracle, k):
    rng = np.random.default_rng(k)
    UU, II, u, i, j = _hot_batch(rng)
    w = rng.standard_normal(u.size).astype(np.float32)  # negative weights among them
    w[::11] = 0.0
    w[5] = -0.0
    with mf.MatrixFactorizationSGD(UU, II, k, LR, LAM, SEED) as h:
        h.init_factors()
        P0, Q0 = h.get_factors()
        levels, want_info = h.triple_levels(u, i, j)
        assert want_info["levels"] > 20
        x, info = h.partial_fit_pairwise(u, i, j, weights=w, margins=True, info=True)
        P, Q, want_x = WC.c_pass(P0, Q0, u, i, j, w, LR, LAM)
        got = h.get_factors()
        assert x.tobytes() == want_x.tobytes() and got[0].tobytes() == P.tobytes() and got[1].tobytes() == Q.tobytes()
        assert info.pop("launches") >= 1 and want_info.pop("launches") == 0 and info == want_info  # weights do not enter
        assert h.partial_fit_pairwise(u[:9], i[:9], j[:9], weights=w[:9]) is None  # without the margins
        P, Q, _ = WC.c_pass(P, Q, u[:9], i[:9], j[:9], w[:9], LR, LAM)
        got = h.get_factors()
        assert got[0].tobytes() == P.tobytes() and got[1].tobytes() == Q.tobytes()
        # an infinite weight is plain arithmetic: Inf, and NaN where Inf meets 0 or Inf
        w2 = w.copy()
        w2[[3, 200]] = np.inf
        x = h.partial_fit_pairwise(u, i, j, weights=w2, margins=True)
        P, Q, want_x = WC.c_pass(P, Q, u, i, j, w2, LR, LAM)
        assert np.isinf(P).any() or np.isnan(P).any()
        _nan_alike((x,) + h.get_factors(), (want_x, P, Q), f"k {k}: infinite weights")


@pytest.mark.parametrize("k", (5, 9, 64, 65))  # 9 and 65: lanes that hold padding only (L = 4, L = 32)
def test_a_nan_weight_is_canonical_at_the_door(mf, oracle, k):
    """A weight of 0xFFFFFFFF would hand the word the training kernels read as "not posted yet" to three factor rows.  The
    factors are read, not trained on.  A second batch with finite weights then goes over the rows of the NaN steps and over
    rows still finite, and every pair is predicted, against the sequential loop: the state after a NaN step goes on
    working.  (A NaN step makes every real column of its rows NaN, so this cannot tell whether a pad column took the NaN
    too: test_an_infinite_step_leaves_the_pad_columns_zero can.)"""
    rng = np.random.default_rng(k)
    UU, II, u, i, j = _hot_batch(rng, 60)
    w = rng.standard_normal(u.size).astype(np.float32)
    w.view(np.uint32)[[2, 31]] = 0xFFFFFFFF
    pu, pi = np.repeat(np.arange(UU, dtype=np.int32), II), np.tile(np.arange(II, dtype=np.int32), UU)
    with mf.MatrixFactorizationSGD(UU, II, k, LR, LAM, SEED) as h:
        h.init_factors()
        P0, Q0 = h.get_factors()
        x = h.partial_fit_pairwise(u, i, j, weights=w, margins=True)
        P, Q = h.get_factors()
        wP, wQ, wx = WC.c_pass(P0, Q0, u, i, j, w, LR, LAM)
        _nan_alike((x, P, Q), (wx, wP, wQ), f"k {k}")
        assert np.isnan(P[u[2]]).all() and np.isnan(Q[i[2]]).all() and np.isnan(Q[j[2]]).all()
        for M in (P, Q):
            bits = M.view(np.uint32)[np.isnan(M)]
            assert bits.size and ((bits & 0x3FFFFF) != 0x3FFFFF).all()
        finite = ~np.isnan(h.predict(u, i))  # the pad columns stayed +0.0: rows the NaN never reached have finite dots
        assert finite.any()
        _nan_alike((h.predict(pu, pi),), (oracle.predict(wP, wQ, pu, pi),), f"k {k}: predict")
        # the second batch: four triples over rows that are still finite, the two NaN steps' triples, 20 of the batch again
        fu, fi = np.flatnonzero(~np.isnan(wP).any(axis=1)), np.flatnonzero(~np.isnan(wQ).any(axis=1))
        assert fu.size >= 4 and fi.size >= 2
        pick = np.r_[2, 31, 0:20]
        u2 = np.concatenate([fu[:4], u[pick]]).astype(np.int32)
        i2 = np.concatenate([np.full(4, fi[0]), i[pick]]).astype(np.int32)
        j2 = np.concatenate([np.full(4, fi[1]), j[pick]]).astype(np.int32)
        w2 = rng.standard_normal(u2.size).astype(np.float32)
        x2 = h.partial_fit_pairwise(u2, i2, j2, weights=w2, margins=True)
        wP2, wQ2, wx2 = WC.c_pass(wP, wQ, u2, i2, j2, w2, LR, LAM)
        assert np.isnan(wx2[4:6]).all() and not np.isnan(wx2[:4]).any() and not np.isnan(wP2).all()
        pred = h.predict(pu, pi)
        _nan_alike((x2,) + h.get_factors() + (pred,), (wx2, wP2, wQ2, oracle.predict(wP2, wQ2, pu, pi)), f"k {k}: a finite batch after")
        assert np.isnan(pred).any() and not np.isnan(pred).all()


@pytest.mark.parametrize("k", (1, 5, 9, 20, 65, 100))  # pad columns beside real ones in a lane, and lanes of padding only
def test_an_infinite_step_leaves_the_pad_columns_zero(mf, oracle, k):
    """Where a pad column left non-zero can be seen.  A step of weight +Inf makes every real column of its three rows
    +Inf or -Inf (none NaN: no column of q_i - q_j or p is 0 here), while fma(Inf, 0, c * 0) in a pad column is NaN.  A
    row chosen to agree in sign with such a row, column by column, then has the dot +Inf in the sequential loop, which has
    no pad columns -- and NaN on the device if one of its pad columns took the step."""
    UU, II = 6, 8
    rng = np.random.default_rng(k)
    P0 = rng.uniform(0.5, 1.5, (UU, k)).astype(np.float32) * rng.choice([-1.0, 1.0], (UU, k)).astype(np.float32)
    Q0 = rng.uniform(0.5, 1.5, (II, k)).astype(np.float32) * rng.choice([-1.0, 1.0], (II, k)).astype(np.float32)
    Q0[1] = -Q0[0] * np.float32(0.5)  # the triple (0, 0, 1): q_i - q_j has the signs of q_i
    Q0[2] = Q0[0]  # agrees with the new P[0]
    P0[1] = P0[0]  # agrees with the new Q[0], disagrees with the new Q[1]
    u, i, j, w = np.array([0], np.int32), np.array([0], np.int32), np.array([1], np.int32), np.array([np.inf], np.float32)
    wP, wQ, wx = WC.c_pass(P0, Q0, u, i, j, w, LR, LAM)
    assert np.isinf(wP[0]).all() and np.isinf(wQ[0]).all() and np.isinf(wQ[1]).all() and np.isfinite(wx).all()
    pu, pi = np.array([0, 1, 1], np.int32), np.array([2, 0, 1], np.int32)
    want = oracle.predict(wP, wQ, pu, pi)
    assert list(want) == [np.inf, np.inf, -np.inf]
    with mf.MatrixFactorizationSGD(UU, II, k, LR, LAM, SEED) as h:
        h.set_factors(P0, Q0)
        x = h.partial_fit_pairwise(u, i, j, weights=w, margins=True)
        P, Q = h.get_factors()
        assert x.tobytes() == wx.tobytes() and P.tobytes() == wP.tobytes() and Q.tobytes() == wQ.tobytes()
        assert h.predict(pu, pi).tobytes() == want.tobytes()
        # a finite step over the same three rows: Inf - Inf in the margin, and NaN from there on, as in the loop
        x2 = h.partial_fit_pairwise(u, i, j, weights=np.ones(1, np.float32), margins=True)
        wP2, wQ2, wx2 = WC.c_pass(wP, wQ, u, i, j, np.ones(1, np.float32), LR, LAM)
        _nan_alike((x2,) + h.get_factors(), (wx2, wP2, wQ2), f"k {k}: a finite step after")


@pytest.mark.parametrize("k", (5, 64))
def test_bpr_weights_reproduce_apply_triples_on_rows_that_share_nothing(mf, k):
    n = 90
    rng = np.random.default_rng(k)
    u = rng.permutation(n).astype(np.int32)
    items = rng.permutation(2 * n).astype(np.int32)
    i, j = items[:n].copy(), items[n:].copy()
    new = lambda: mf.MatrixFactorizationSGD(n, 2 * n, k, LR, LAM, SEED)
    with new() as a, new() as b:
        a.init_factors()
        b.init_factors()
        x, info = a.partial_fit_pairwise(u, i, j, margins=True, info=True)
        assert info["levels"] == 1
        x2 = b.partial_fit_pairwise(u, i, j, weights=mf.bpr_weights(x), margins=True)
        assert x2.tobytes() == x.tobytes()
        for A, B in zip(a.get_factors(), b.get_factors()):
            assert A.tobytes() == B.tobytes()


# ---- 7. fit_warp is the loop it is documented as ---------------------------------------------------------------------------------------
FU, FI, FK, FM, FSEED, EPOCHS = 48, 64, 8, 8, 21, 4
FLR, FLAM, FMARGIN = 0.1, 0.01, 0.5


def _planted():
    """48 users in 8 groups, 64 items in 8 blocks of 8: a user's 6 positives lie in the block of the user's group."""
    rng = np.random.default_rng(0)
    its = np.stack([(u % 8) * 8 + rng.choice(8, 6, replace=False) for u in range(FU)]).astype(np.int32)
    pu, pi = np.repeat(np.arange(FU, dtype=np.int32), 6), its.ravel().copy()
    order = rng.permutation(pu.size)
    return pu[order], pi[order]


@functools.lru_cache(maxsize=None)
def _reference(refresh):
    """The restated loop from seeded factors, computed once per refresh: (P, Q, stats) after EPOCHS epochs."""
    from tests.oracle_bind import Oracle

    oracle = Oracle()
    pu, pi = _planted()
    P0, Q0 = oracle.init_factors(FU, FI, FK, SEED)
    return WC.fit_warp(oracle, P0, Q0, IC.lists_of(pu, pi), pu, pi, EPOCHS, FLR, FLAM, candidates=FM, margin=FMARGIN,
                       refresh=refresh, seed=FSEED)


def _factor_bits(h):
    P, Q = h.get_factors()
    return P.tobytes(), Q.tobytes()


@pytest.mark.parametrize("refresh", (None, 7))
def test_fit_warp_is_its_documented_loop(mf, refresh):
    pu, pi = _planted()
    P, Q, want = _reference(refresh)
    # a condition on the reference: the model learns, so fewer positives have a violator among their m draws
    assert want["violating"][-1] < want["violating"][0] and want["trials"][-1] > want["trials"][0]
    new = lambda: mf.MatrixFactorizationSGD(FU, FI, FK, FLR, FLAM, SEED)
    with new() as a, new() as b:
        stats = a.fit_warp(pu, pi, EPOCHS, candidates=FM, margin=FMARGIN, refresh=refresh, seed=FSEED)
        assert sorted(stats) == ["trials", "violating"] and all(v.shape == (EPOCHS,) and v.dtype == np.float64 for v in stats.values())
        assert a.seen_size() == pu.size and a.debug_counters()["schedule_builds"] == 0  # an index was made, a rating set was not
        assert _factor_bits(a) == (P.tobytes(), Q.tobytes())
        for name in ("violating", "trials"):
            assert stats[name].tobytes() == want[name].tobytes(), name
        # three epochs and then the fourth: the same bits
        first = b.fit_warp(pu, pi, EPOCHS - 1, candidates=FM, margin=FMARGIN, refresh=refresh, seed=FSEED)
        last = b.fit_warp(pu, pi, 1, candidates=FM, margin=FMARGIN, refresh=refresh, seed=FSEED, first_epoch=EPOCHS - 1)
        for name in ("violating", "trials"):
            assert np.concatenate([first[name], last[name]]).tobytes() == want[name].tobytes(), name
        assert _factor_bits(b) == _factor_bits(a)
        assert b.fit_warp(pu, pi, 1, candidates=FM, margin=FMARGIN, seed=FSEED, first_epoch=EPOCHS, stats=False) is None
        assert b.fit_warp(pu, pi, 0, candidates=FM)["violating"].shape == (0,)
