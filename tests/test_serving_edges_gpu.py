"""The serving kernels (csrc/recommend.hip, csrc/rank.hip) at every lane-group width and on every boundary of their
tables: each template instance L = 1 .. 64 on the fused path, the sort path and in rank_items; item counts on and around
a tile edge of the fused kernel, a short last tile, a tile whose items are all excluded; the switch between the two
selection paths where the candidate table is exactly full; more users than one launch / one staging batch takes; scores
that are -0.0, infinite or subnormal; pair counts on and around the size of rank.hip's threshold table.

The reference is the one of the existing serving tests: the oracle's predictions of the whole catalogue for the user,
np.lexsort((items, -scores)); items compare exactly and scores bit for bit, ranks as integers."""
import numpy as np
import pytest

from tests import edge_inputs as E
from tests.test_rank_items_gpu import _case, _ranks_ref

pytestmark = pytest.mark.gpu

LR, LAM = 0.01, 0.05
TILE = 14336   # csrc/recommend.hip: kTopnTile, items per tile of the fused kernel
CAND = 2048    # ... kTopnCand: candidates kept across tiles; fused while tiles * topn <= CAND (and topn <= 128)
RANK_CAP = 512  # csrc/rank.hip: kRankCap, thresholds per user and round
NONE = np.empty(0, np.int32)


def _model(mf, P, Q):
    m = mf.MatrixFactorizationSGD(P.shape[0], Q.shape[0], P.shape[1], LR, LAM, 1)
    m.set_factors(P, Q)
    return m


# ---- C1: every L on every path ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 4, 8, 16, 32, 64, 100, 129, 256])  # L = 1, 1, 2, 4, 8, 16, 32, 64, 64
def test_every_group_width_on_the_fused_and_the_sort_path(mf, oracle, k):
    U, I = 40, 700
    rng, P, Q = E.tied_factors(U, I, k, 700 + k)
    users = np.array([0, 7, 7, U - 1, 13, 21], np.int32)
    rows = {}
    with _model(mf, P, Q) as m:
        for topn in (128, 129):  # the largest fused topn; the smallest of the sort path
            plain = E.recommend_ref(oracle, P, Q, users, topn, score_rows=rows)
            eu, ei = E.exclusions_like_the_exclude_test(rng, oracle, P, Q, users, topn, plain[0])
            excl = E.recommend_ref(oracle, P, Q, users, topn, eu, ei, score_rows=rows)
            assert (excl[0][5] == -1).all() and (excl[0][3, topn // 2:] == -1).all() and (excl[0][3, :topn // 2 - 1] >= 0).all()
            E.assert_recommend(m.recommend(users, topn), plain, f"plain, topn {topn}")
            E.assert_recommend(m.recommend(users, topn, exclude=(eu, ei)), excl, f"excluding, topn {topn}")
            # the same rows handed over as rows that are not in the model: a pair names its row's position in `users`
            er = np.concatenate([np.full(np.count_nonzero(eu == x), j, np.int32) for j, x in enumerate(users)])
            ej = np.concatenate([ei[eu == x] for x in users])
            E.assert_recommend(m.recommend_rows(P[users], topn), plain, f"rows, topn {topn}")
            E.assert_recommend(m.recommend_rows(P[users], topn, exclude=(er, ej)), excl, f"rows excluding, topn {topn}")


@pytest.mark.parametrize("k", [32, 100])  # L = 8 and 32: the widths no other rank test reaches
def test_rank_items_at_the_missing_group_widths(mf, oracle, k):
    rng, P, Q, u, i, eu, ei = _case(oracle, 700, k)
    with _model(mf, P, Q) as m:
        got = m.rank_items(u, i, exclude=(eu, ei))
        plain = m.rank_items(u, i)
    np.testing.assert_array_equal(got, _ranks_ref(oracle, P, Q, u, i, eu, ei))
    np.testing.assert_array_equal(plain, _ranks_ref(oracle, P, Q, u, i, NONE, NONE))


# ---- C2: tile edges of the fused kernel -----------------------------------------------------------------------------------
@pytest.mark.parametrize("I", [TILE - 1, TILE, TILE + 1, 2 * TILE, 2 * TILE + 3])
def test_fused_kernel_on_and_around_a_tile_edge(mf, oracle, I):
    """One item short of a tile, a full tile, a second tile of one item, two full tiles, and a third tile of 3 items --
    fewer than topn, and the best three of user 2 (they must come out of the short tile)."""
    k, topn = 8, 10
    rng, P, Q = E.tied_factors(4, I, k, I)
    Q[I - 3:] = np.outer([60.0, 50.0, 70.0], P[2]).astype(np.float32)
    users = np.arange(4, dtype=np.int32)
    want = E.recommend_ref(oracle, P, Q, users, topn)
    assert sorted(want[0][2, :3].tolist()) == [I - 3, I - 2, I - 1]
    with _model(mf, P, Q) as m:
        E.assert_recommend(m.recommend(users, topn), want)


def test_fused_kernel_exclusions_on_tile_boundaries(mf, oracle):
    k, topn, I = 8, 10, 30000  # tiles [0, TILE), [TILE, 2 TILE), [2 TILE, 30000)
    rng, P, Q = E.tied_factors(4, I, k, I)
    users = np.arange(4, dtype=np.int32)
    middle = np.arange(TILE, 2 * TILE, dtype=np.int32)       # user 0: the whole middle tile, nothing else
    edge = np.array([TILE - 1, TILE], np.int32)              # user 1: the two items either side of a tile edge
    first = rng.permutation(TILE)[3:].astype(np.int32)       # user 2: all but 3 items of the first tile (< topn left)
    eu = np.concatenate([np.zeros(middle.size), np.ones(edge.size), np.full(first.size, 2)]).astype(np.int32)
    ei = np.concatenate([middle, edge, first])               # user 3: none, in the same call
    perm = rng.permutation(eu.size)
    eu, ei = eu[perm], ei[perm]
    # ... and each of them matters: the items taken away would have been recommended
    Q[[TILE + 5, 2 * TILE - 1]] = np.outer([40.0, 45.0], P[0]).astype(np.float32)
    Q[edge] = np.outer([40.0, 45.0], P[1]).astype(np.float32)
    rows = {}
    plain = E.recommend_ref(oracle, P, Q, users, topn, score_rows=rows)
    want = E.recommend_ref(oracle, P, Q, users, topn, eu, ei, score_rows=rows)
    assert set(plain[0][0, :2]) == {TILE + 5, 2 * TILE - 1} and not np.isin(want[0][0], middle).any()
    assert set(plain[0][1, :2]) == set(edge.tolist()) and not np.isin(want[0][1], edge).any()
    assert np.array_equal(want[0][3], plain[0][3]) and (want[0] >= 0).all()
    with _model(mf, P, Q) as m:
        E.assert_recommend(m.recommend(users, topn, exclude=(eu, ei)), want)
        E.assert_recommend(m.recommend(users, topn), plain)


# ---- C3: the switch between the two selection paths ---------------------------------------------------------------------
@pytest.mark.parametrize("I", [16 * TILE, 16 * TILE + 1])
def test_the_switch_between_the_fused_and_the_sort_path(mf, oracle, I):
    """topn = 128 and 16 full tiles: 2048 candidates, the table exactly full and the bitonic sort unpadded -- still
    fused; one item more is a 17th tile, and the sort path.  User 0's top 128 are 8 items of each of the 16 tiles; the
    last item of the catalogue (the 17th tile where there is one) is user 1's best."""
    k, topn = 4, 128
    assert 16 * topn == CAND
    rng, P, Q = E.tied_factors(3, I, k, 229376)
    spread = (np.arange(16)[:, None] * TILE + rng.choice(TILE, 8, replace=False)[None, :]).ravel()
    Q[spread] = np.outer(rng.permutation(128) + 100.0, P[0]).astype(np.float32)
    Q[I - 1] = (30.0 * P[1]).astype(np.float32)
    users = np.arange(3, dtype=np.int32)
    want = E.recommend_ref(oracle, P, Q, users, topn)
    assert np.unique(want[0][0] // TILE).size == 16 and set(want[0][0].tolist()) == set(spread.tolist())
    assert want[0][1, 0] == I - 1
    with _model(mf, P, Q) as m:
        E.assert_recommend(m.recommend(users, topn), want)


# ---- C4: more users than one launch, or one staging batch, takes ----------------------------------------------------------------
def test_fused_path_more_users_than_one_launch(mf, oracle):
    U, I, k, topn = 70000, 5, 4, 5  # a launch takes 65 535 users (csrc/serve_topn.cpp, kLaunchRows): the second one has 4 465
    rng = np.random.default_rng(70000)
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    Q[3] = Q[1]  # a tie in every row
    users = np.arange(U, dtype=np.int32)
    with _model(mf, P, Q) as m:
        items, scores = m.recommend(users, topn)
    sc = oracle.predict(P, Q, np.repeat(users, I), np.tile(np.arange(I, dtype=np.int32), U))
    row, item = np.repeat(users, I), np.tile(np.arange(I), U)
    order = np.lexsort((item, -sc.astype(np.float64), row))
    np.testing.assert_array_equal(items, item[order].reshape(U, I))
    assert scores.tobytes() == sc[order].tobytes()
    some = np.array([0, 65534, 65535, 65536, 69999], np.int32)
    want = E.recommend_ref(oracle, P, Q, some, topn)
    E.assert_recommend((items[some], scores[some]), want)


def test_sort_path_more_users_than_one_staging_batch(mf, oracle):
    """csrc/serve_topn.cpp, topn_batches: the sort path stages kSortCells / I = ((int64_t)64 << 20) / I scores' worth of users per batch;
    at I = 229 377 that is 292 users, so 300 users are a batch of 292 and one of 8."""
    I, k, topn, n_users = 16 * TILE + 1, 4, 129, 300
    assert (64 << 20) // I == 292
    rng, P, Q = E.tied_factors(n_users, I, k, 300)
    users = rng.permutation(n_users).astype(np.int32)
    with _model(mf, P, Q) as m:
        got = m.recommend(users, topn)
    E.assert_recommend(got, E.recommend_ref(oracle, P, Q, users, topn))


# ---- C5: scores at the edges of fp32 -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 64])
@pytest.mark.parametrize("kind", E.SCORE_KINDS)
def test_scores_at_the_edges_of_fp32(mf, oracle, kind, k):
    """-0.0 scores tie with +0.0 ones (the smaller item first); +inf scores tie at the top and -inf ones at the bottom,
    in item order; subnormal scores keep their order (a kernel that flushed them would answer 0, 1, 2, ...).  Fused
    path (topn 128), sort path (129, and the whole catalogue so that the bottom shows), each with and without
    exclusions, and rank_items of every item."""
    P, Q, user = E.edge_score_factors(kind, k)
    I = Q.shape[0]
    rows = {}
    sc = rows[user] = E.all_scores(oracle, P, Q, user)
    E.check_edge_scores(kind, sc)
    users = np.array([user, 0, user], np.int32)
    if kind == "infinite":
        users = np.array([user, user], np.int32)  # (another row's scores of the +-3e38 items may be NaN)
    rng = np.random.default_rng(k)
    ei = np.concatenate([rng.choice(I, 50, replace=False), E.ZERO_ITEMS[[0, 3]], E.POS_INF_ITEMS[:1], E.NEG_INF_ITEMS[:1]])
    ei = ei.astype(np.int32)
    eu = np.full(ei.size, user, np.int32)
    allitems = np.arange(I, dtype=np.int32)
    with _model(mf, P, Q) as m:
        for topn in (128, 129, I):
            want = E.recommend_ref(oracle, P, Q, users, topn, score_rows=rows)
            E.assert_recommend(m.recommend(users, topn), want, f"topn {topn}")
            want_x = E.recommend_ref(oracle, P, Q, users, topn, eu, ei, score_rows=rows)
            E.assert_recommend(m.recommend(users, topn, exclude=(eu, ei)), want_x, f"excluding, topn {topn}")
        ranks = m.rank_items(np.full(I, user, np.int32), allitems)
        ranks_x = m.rank_items(np.full(I, user, np.int32), allitems, exclude=(eu, ei))
    full = want[0][0]  # the user's whole catalogue, best first
    if kind == "negative_zero":
        at = int(np.flatnonzero(full == E.ZERO_ITEMS[0])[0])
        np.testing.assert_array_equal(full[at:at + E.ZERO_ITEMS.size], E.ZERO_ITEMS)  # one tie group, in item order
        assert at + E.ZERO_ITEMS.size <= 128
    if kind == "infinite":
        np.testing.assert_array_equal(full[:4], np.sort(E.POS_INF_ITEMS))
        np.testing.assert_array_equal(full[-4:], np.sort(E.NEG_INF_ITEMS))
    np.testing.assert_array_equal(ranks, _ranks_ref(oracle, P, Q, np.full(I, user, np.int32), allitems, NONE, NONE))
    np.testing.assert_array_equal(ranks_x, _ranks_ref(oracle, P, Q, np.full(I, user, np.int32), allitems, eu, ei))
    assert np.array_equal(ranks[full], np.arange(I))  # the rank is the place in the shipped list


# ---- C6: table boundaries of rank.hip --------------------------------------------------------------------------------------
def test_rank_items_pair_counts_around_the_table_size(mf, oracle):
    """Users with 1, CAP - 1, CAP, CAP + 1, 2 CAP - 1, 2 CAP, 2 CAP + 1 and 3000 held-out items in one call: a round
    whose table is exactly full, one with a single threshold left for the next round, and five full rounds + 440."""
    I, k = 3000, 16
    rng, P, Q = E.tied_factors(40, I, k, 3000)
    counts = [1, RANK_CAP - 1, RANK_CAP, RANK_CAP + 1, 2 * RANK_CAP - 1, 2 * RANK_CAP, 2 * RANK_CAP + 1, I]
    who = [3, 30, 7, 11, 0, 21, 39, 16]
    u = np.concatenate([np.full(n, x, np.int32) for n, x in zip(counts, who)])
    i = np.concatenate([rng.choice(I, n, replace=False) for n in counts]).astype(np.int32)
    perm = rng.permutation(u.size)
    u, i = u[perm], i[perm]
    ex7, ex39 = rng.choice(I, I // 5, replace=False), rng.choice(I, I // 2, replace=False)  # the users with CAP, 2 CAP + 1
    eu = np.concatenate([np.full(ex7.size, 7), np.full(ex39.size, 39)]).astype(np.int32)
    ei = np.concatenate([ex7, ex39]).astype(np.int32)
    with _model(mf, P, Q) as m:
        got = m.rank_items(u, i, exclude=(eu, ei))
        plain = m.rank_items(u, i)
    np.testing.assert_array_equal(got, _ranks_ref(oracle, P, Q, u, i, eu, ei))
    np.testing.assert_array_equal(plain, _ranks_ref(oracle, P, Q, u, i, NONE, NONE))
