"""The serving calls across the limits of their host-side staging (csrc/serve_topn.cpp, serve_rank.cpp, serve_fold.cpp): more ranked pairs than one launch of
rank_items takes, one user whose own pairs exceed a launch, more exclusion pairs and more candidates than one upload, each
with the pointer or offset that the second piece re-bases.  Every expectation is the oracle's canonical scores and a plain
numpy selection, never another call of the library; where a test also runs exclude="seen" it is compared with the same
reference.  Items and ranks compare exactly, scores bit for bit, padding (-1, NaN) by position.

The constants below are the library's, named with their source: each test asserts the number of launches or uploads they
imply, so that a change in the library fails that arithmetic instead of quietly leaving the seam uncrossed.
(tests/test_seen_gpu.py has the batches of request rows and the strides of the index's gather.)"""
import time

import numpy as np
import pytest

from tests import edge_inputs as E
from tests.test_rank_items_gpu import _ranks_ref

pytestmark = pytest.mark.gpu

LR, LAM = 0.01, 0.05
TILE = 14336           # csrc/recommend.hip: kTopnTile, positions per tile of the fused kernel
CAND = 2048            # csrc/recommend.hip: kTopnCand; fused while tiles * topn <= CAND and topn <= 128
CHUNK = 1 << 22        # csrc/handle.hpp: kExclChunk, exclusion pairs / candidates per upload
RANK_CHUNK = 1 << 22   # csrc/serve_rank.cpp: kRankChunk, pairs of one rank launch (whole users)
RANK_CAP = 512         # csrc/rank.hip: kRankCap, thresholds per user and round
NONE = np.empty(0, np.int32)


def _model(mf, P, Q):
    m = mf.MatrixFactorizationSGD(P.shape[0], Q.shape[0], P.shape[1], LR, LAM, 1)
    m.set_factors(P, Q)
    return m


def _uploads(n):
    return -(-n // CHUNK)


# ---- the references ---------------------------------------------------------------------------------------------------------
def score_matrix(oracle, P, Q, users):
    """[len(users), I]: the oracle's canonical score of every item for each of the users, in one call."""
    users = np.asarray(users, np.int32)
    I = Q.shape[0]
    sc = oracle.predict(P, Q, np.repeat(users, I), np.tile(np.arange(I, dtype=np.int32), users.size))
    assert not np.isnan(sc).any()
    return sc.reshape(users.size, I)


class RankRef:
    """tests/test_rank_items_gpu.py's _ranks_ref for millions of pairs: one stable sort per row of the score matrix (best
    first, ties by the smaller item), and the rank of (row, t) is t's place minus the excluded items strictly before it
    (t itself counts as eligible even if excluded)."""

    def __init__(self, S):
        I = S.shape[1]
        self.order = np.argsort(-S.astype(np.float64), axis=1, kind="stable")
        self.pos = np.empty_like(self.order)
        np.put_along_axis(self.pos, self.order, np.broadcast_to(np.arange(I), S.shape), axis=1)

    def ranks(self, row, i, X=None):
        p = self.pos[row, i]
        if X is None:
            return p.astype(np.int32)
        xo = np.take_along_axis(X, self.order, axis=1)
        ahead = np.cumsum(xo, axis=1) - xo
        return (p - ahead[row, p]).astype(np.int32)


def topn_ref(S, X, topn):
    """(items, scores) [rows, topn]: per row of S the topn eligible items (X: True where an item is excluded or no
    candidate), the larger score first, ties by the smaller item (edge_inputs.top_of), padded with -1 / NaN."""
    items = np.full((S.shape[0], topn), -1, np.int32)
    scores = np.full((S.shape[0], topn), np.nan, np.float32)
    for row in range(S.shape[0]):
        top = E.top_of(S[row], topn, np.flatnonzero(X[row]) if X is not None else None)
        items[row, :top.size] = top
        scores[row, :top.size] = S[row][top]
    return items, scores


def rank_launches(u):
    """The users of each launch of rank_core (csrc/serve_rank.cpp) for the pairs' users u as given: a slot per distinct user in
    the order of first appearance, the slots stably sorted by pair count (most first), launches of whole users of at most
    RANK_CHUNK pairs -- a single user with more is a launch of its own."""
    counts = np.bincount(u)
    first = np.full(counts.size, u.size)
    first[u[::-1]] = np.arange(u.size)[::-1]  # (the last write is the first appearance)
    users = np.flatnonzero(counts)
    by_first = np.argsort(first[users], kind="stable")
    users = users[by_first]
    counts = counts[users]
    by_count = np.argsort(-counts, kind="stable")
    users, counts = users[by_count], counts[by_count]
    off = np.concatenate([[0], np.cumsum(counts)])
    launches, s = [], 0
    while s < users.size:
        s1 = max(s + 1, int(np.searchsorted(off, off[s] + RANK_CHUNK, side="right")) - 1)
        launches.append(users[s:s1])
        s = s1
    return launches


def _mask(shape, row, item):
    X = np.zeros(shape, bool)
    X[row, item] = True
    return X


# ---- A1: rank_items over more than one launch -------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [4, 64])
def test_rank_items_over_more_than_one_launch(mf, oracle, k):
    """8 292 users of RANK_CAP pairs, three of 1 300 (several rounds) and five of one: 4.25 M pairs, shuffled.  Sorted by
    pair count the three come first, so the first launch takes them and 8 184 users, the second the other 108 and the five;
    d_slot_rows + b0, d_off + b0, base, and exb.off += b0 for a pair list but not for the index, all run with b0 > 0.
    (300 items, not more: the reference sorts every user's row, and the seam is in the pairs.)"""
    U, I = 8300, 300
    rng, P, Q = E.tied_factors(U, I, k, 8300 + k)
    heavy, single = np.array([11, 4000, 8290]), np.array([5, 17, 4100, 8200, 8299])
    counts = np.full(U, RANK_CAP)
    counts[heavy], counts[single] = 1300, 1
    u = np.repeat(np.arange(U, dtype=np.int32), counts)
    i = rng.integers(0, I, u.size).astype(np.int32)  # (duplicates: 512 draws of 300 items)
    perm = rng.permutation(u.size)
    u, i = np.ascontiguousarray(u[perm]), np.ascontiguousarray(i[perm])
    launches = rank_launches(u)
    assert u.size > RANK_CHUNK and RANK_CHUNK // RANK_CAP == 8192
    assert [x.size for x in launches] == [3 + (RANK_CHUNK - 3 * 1300) // RANK_CAP, U - 3 - (RANK_CHUNK - 3 * 1300) // RANK_CAP]
    assert set(launches[0][:3].tolist()) == set(heavy.tolist()) and set(launches[1][-5:].tolist()) == set(single.tolist())
    assert not np.array_equal(np.concatenate(launches), np.arange(U))  # the slot order is not the user order
    in_second = np.zeros(U, bool)
    in_second[launches[1]] = True
    second = in_second[u]
    eu = np.repeat(np.arange(U, dtype=np.int32), 30)
    ei = rng.integers(0, I, eu.size).astype(np.int32)
    perm = rng.permutation(eu.size)
    eu, ei = np.ascontiguousarray(eu[perm]), np.ascontiguousarray(ei[perm])
    t0 = time.perf_counter()
    ref = RankRef(score_matrix(oracle, P, Q, np.arange(U)))
    want_plain, want_excl = ref.ranks(u, i), ref.ranks(u, i, _mask((U, I), eu, ei))
    few = np.array([heavy[0], single[0], 3, launches[1][0], launches[1][50]])  # ... which is _ranks_ref's, pair for pair
    is_few = np.zeros(U, bool)
    is_few[few] = True
    sel, selx = is_few[u], is_few[eu]
    np.testing.assert_array_equal(want_excl[sel], _ranks_ref(oracle, P, Q, u[sel], i[sel], eu[selx], ei[selx]))
    np.testing.assert_array_equal(want_plain[sel], _ranks_ref(oracle, P, Q, u[sel], i[sel], NONE, NONE))
    assert (want_plain[second] != want_excl[second]).any()  # a second launch that ignored its lists would show
    t1 = time.perf_counter()
    with _model(mf, P, Q) as m:
        got_plain = m.rank_items(u, i)
        got_list = m.rank_items(u, i, exclude=(eu, ei))
        m.set_seen(eu, ei)
        if k == 64:
            got_seen = m.rank_items(u, i, exclude="seen")
        else:  # the same ranks through evaluate_ranking, and the metrics of the reference's ranks
            res = m.evaluate_ranking(u, i, 10, exclude="seen")
            got_seen = res.pop("ranks")
            assert res == mf.ranking_metrics(u, want_excl, 10)
    print(f"k {k}: reference {t1 - t0:.2f} s, four calls {time.perf_counter() - t1:.2f} s")
    np.testing.assert_array_equal(got_plain, want_plain)
    np.testing.assert_array_equal(got_list, want_excl)
    np.testing.assert_array_equal(got_seen, want_excl)
    assert (got_list[second] != got_plain[second]).any() and (got_seen[second] != got_plain[second]).any()


# ---- A2: one user whose own pairs exceed a launch ---------------------------------------------------------------------------
def test_one_user_with_more_pairs_than_a_launch(mf, oracle):
    """User 2 has RANK_CHUNK + 600 pairs: a launch of its own (8 194 rounds in one workgroup), the four ordinary users,
    two before it and two after it in user id, in a second one.  (Measured on an MI355X: the call takes 0.13 s without
    exclusions and 0.14 s against the index; the whole test 0.44 s.)"""
    U, I, k = 5, 64, 4
    rng, P, Q = E.tied_factors(U, I, k, 64)
    counts = np.array([3, 700, RANK_CHUNK + 600, 1, 520])
    u = np.repeat(np.arange(U, dtype=np.int32), counts)
    i = rng.integers(0, I, u.size).astype(np.int32)
    perm = rng.permutation(u.size)
    u, i = np.ascontiguousarray(u[perm]), np.ascontiguousarray(i[perm])
    launches = rank_launches(u)
    assert [x.tolist() for x in launches] == [[2], [1, 4, 0, 3]]
    assert -(-int(counts[2]) // RANK_CAP) == 8194
    eu = np.concatenate([np.full(20, 2), np.full(9, 0), np.full(30, 1), np.full(5, 4)]).astype(np.int32)  # user 3: none
    ei = np.concatenate([rng.choice(I, n, replace=False) for n in (20, 9, 30, 5)]).astype(np.int32)
    ref = RankRef(score_matrix(oracle, P, Q, np.arange(U)))
    want_plain, want_seen = ref.ranks(u, i), ref.ranks(u, i, _mask((U, I), eu, ei))
    for user in (2, 1, 3):
        assert (want_plain[u == user] != want_seen[u == user]).any() == (user != 3)
    with _model(mf, P, Q) as m:
        t0 = time.perf_counter()
        got_plain = m.rank_items(u, i)
        t1 = time.perf_counter()
        m.set_seen(eu, ei)
        t2 = time.perf_counter()
        got_seen = m.rank_items(u, i, exclude="seen")
        t3 = time.perf_counter()
    print(f"rank_items of {u.size} pairs, {counts[2]} of one user: {t1 - t0:.2f} s plain, {t3 - t2:.2f} s against the index")
    np.testing.assert_array_equal(got_plain, want_plain)
    np.testing.assert_array_equal(got_seen, want_seen)


# ---- A3: exclusion pairs past one upload ------------------------------------------------------------------------------------
def test_exclusion_pairs_past_one_upload(mf, oracle):
    """CHUNK + 1000 exclusion pairs over 3 000 users, 200 of them requested: count_exclusions and the filter drop the
    rest.  The first pair of the second upload takes away user a's best item, the last pair of all user b's."""
    U = I = 3000
    k, n_excl = 8, CHUNK + 1000
    assert _uploads(n_excl) == 2 and _uploads(n_excl - 1001) == 1
    rng, P, Q = E.tied_factors(U, I, k, 3000)
    users = rng.choice(U, 200, replace=False).astype(np.int32)
    users[150] = users[20]  # one user twice: one list for both rows
    uniq, row_of_req = np.unique(users, return_inverse=True)
    row_of_user = np.full(U, -1)
    row_of_user[uniq] = np.arange(uniq.size)
    a, b = int(users[3]), int(users[77])
    S = score_matrix(oracle, P, Q, uniq)
    top_a, top_b = (int(E.top_of(S[row_of_user[x]], 1)[0]) for x in (a, b))
    eu, ei = rng.integers(0, U, n_excl).astype(np.int32), rng.integers(0, I, n_excl).astype(np.int32)
    for x, top in ((a, top_a), (b, top_b)):
        hit = (eu == x) & (ei == top)
        ei[hit] = (top + 1) % I
        assert not ((eu == x) & (ei == top)).any()
    eu[CHUNK], ei[CHUNK] = a, top_a          # the first pair of the second upload
    eu[n_excl - 1], ei[n_excl - 1] = b, top_b  # the last pair
    mine = row_of_user[eu] >= 0
    assert 0 < np.count_nonzero(mine) < n_excl // 10  # (most pairs belong to users nobody asked for)
    X = _mask(S.shape, row_of_user[eu[mine]], ei[mine])
    hu = users[rng.integers(0, users.size, 2000)]
    hi = rng.integers(0, I, 2000).astype(np.int32)
    hu[:2], hi[:2] = (a, b), (top_a, top_b)  # (ranked although excluded)
    ref = RankRef(S)
    want_ranks = ref.ranks(row_of_user[hu], hi, X)
    assert (want_ranks != ref.ranks(row_of_user[hu], hi)).any() and want_ranks[0] == want_ranks[1] == 0
    want = {}
    for topn in (10, 129):  # the fused path; the sort path
        want[topn] = topn_ref(S[row_of_req], X[row_of_req], topn)
        plain = topn_ref(S[row_of_req], None, topn)
        for row, top in ((3, top_a), (77, top_b)):  # each of the two pairs changes the answer
            assert plain[0][row, 0] == top and top not in want[topn][0][row]
    with _model(mf, P, Q) as m:
        for topn in (10, 129):
            got = m.recommend(users, topn, exclude=(eu, ei))
            E.assert_recommend(got, want[topn], f"topn {topn}")
            assert top_a not in got[0][3] and top_b not in got[0][77]
        np.testing.assert_array_equal(m.rank_items(hu, hi, exclude=(eu, ei)), want_ranks)
        res = m.evaluate_ranking(hu, hi, 10, exclude=(eu, ei))
    np.testing.assert_array_equal(res.pop("ranks"), want_ranks)
    assert res == mf.ranking_metrics(hu, want_ranks, 10)


# ---- A4: candidates past one upload -----------------------------------------------------------------------------------------
def test_candidates_past_one_upload(mf, oracle):
    """CHUNK + 1000 candidates: as per-row lists (CSR) of which row 292 straddles entry CHUNK and rows 293 .. 299 lie in
    the second upload, where recommend_cand_keys finds their rows in cand_ptr from x0 = CHUNK; and as one shared list.
    The last candidate of row 292, and of the shared list, is a row's best item."""
    I, k, topn, n_rows = 20000, 8, 10, 300
    n_cand = CHUNK + 1000
    assert _uploads(n_cand) == 2
    rng, P, Q = E.tied_factors(n_rows, I, k, 20000)
    users = rng.permutation(n_rows).astype(np.int32)
    lens = np.array([14400] * 290 + [10000, 8000, 700, 300, 200, 0, 50, 30, 20, 4])
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert ptr[-1] == n_cand and ptr[292] < CHUNK < ptr[293] and lens[295] == 0
    z, z2 = 19990, 19995  # the decisive candidates: in no list but where they are put below
    items = rng.integers(0, 19000, n_cand).astype(np.int32)
    items[ptr[293] - 1] = z
    Q[z] = (50.0 * P[users[292]]).astype(np.float32)
    subset = rng.choice(19000, 9000, replace=False).astype(np.int32)
    shared = subset[rng.integers(0, subset.size, n_cand)]
    shared[-1] = z2
    Q[z2] = (50.0 * P[users[0]]).astype(np.float32)
    S = score_matrix(oracle, P, Q, users)
    lists = [items[ptr[b]:ptr[b + 1]] for b in range(n_rows)]
    C = np.zeros((n_rows, I), bool)  # the rows' distinct candidates
    C[np.repeat(np.arange(n_rows), lens), items] = True
    assert max(C.sum(axis=1).max(), np.unique(shared).size) < TILE and topn <= 128 and 1 * topn <= CAND  # one tile: fused
    assert C.sum(axis=1)[0] < lens[0]  # (duplicates)
    want = topn_ref(S, ~C, topn)
    assert want[0][292, 0] == z and z not in lists[292][:-1] and (want[0][295] == -1).all()
    Cs = np.zeros(I, bool)
    Cs[shared] = True
    want_shared = topn_ref(S, np.broadcast_to(~Cs, S.shape), topn)
    assert want_shared[0][0, 0] == z2 and z2 not in shared[:-1]
    # exclusions: every row's two best candidates, and 2 000 random pairs
    eu = np.concatenate([np.repeat(users, 2), rng.integers(0, n_rows, 2000)]).astype(np.int32)
    ei = np.concatenate([want[0][:, :2].ravel(), rng.integers(0, I, 2000)]).astype(np.int32)
    eu, ei = eu[ei >= 0], ei[ei >= 0]  # (the empty row has no best candidate)
    row_of_user = np.empty(n_rows, np.int64)
    row_of_user[users] = np.arange(n_rows)
    X = _mask(S.shape, row_of_user[eu], ei)
    want_excl = topn_ref(S, ~C | X, topn)
    assert z not in want_excl[0][292] and not np.array_equal(want_excl[0], want[0])
    with _model(mf, P, Q) as m:
        E.assert_recommend(m.recommend(users, topn, candidates=(ptr, items)), want, "per-row lists")
        E.assert_recommend(m.recommend(users, topn, candidates=shared), want_shared, "one shared list")
        E.assert_recommend(m.recommend(users, topn, candidates=(ptr, items), exclude=(eu, ei)), want_excl, "lists, pairs")
        m.set_seen(eu, ei)
        E.assert_recommend(m.recommend(users, topn, candidates=(ptr, items), exclude="seen"), want_excl, "lists, the index")
