"""The seen-item index on the device: set_seen / mark_seen / seen against numpy's unique of the same pairs, and the serving
calls with exclude="seen" against the same calls given the index's pairs as a list, which build their lists per call and
do not read the index.  Items and ranks compare exactly, scores bit for bit, padding (-1, NaN) by position.
Tests 9 to 11 do not compare the library with itself: batches of request rows with exclusions (a pair list, the index) and
with per-row candidates against the oracle's scores and numpy (tests/test_serving_limits_gpu.py has the other staging
limits), and lists read back past the strides of the gather kernel."""
import gc

import numpy as np
import pytest

from tests import edge_inputs as E

pytestmark = pytest.mark.gpu

LR, LAM = 0.01, 0.05
TILE = 14336      # csrc/recommend.hip: kTopnTile, positions per tile of the fused kernel
CHUNK = 1 << 22   # csrc/handle.hpp: kExclChunk, pairs per upload of set_seen / mark_seen
LAUNCH_ROWS = 65535     # csrc/serve_topn.cpp, topn_batches: kLaunchRows, request rows per launch
SORT_CELLS = 64 << 20   # csrc/serve_topn.cpp: kSortCells, scores one batch of the sort path materialises
GATHER_ROWS = 4096      # csrc/seen.hip, seen_gather: grid.x, the rows a pass of the gather takes
GATHER_SPAN = 64 * 256  # ... grid.y parts of kSeenThreads positions: what a pass takes of one list
INVALID_ARG = -1


def _model(mf, P, Q):
    m = mf.MatrixFactorizationSGD(P.shape[0], Q.shape[0], P.shape[1], LR, LAM, 1)
    m.set_factors(P, Q)
    return m


def _factors(U, I, k, seed):
    rng = np.random.default_rng(seed)
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    Q[rng.integers(0, I, I // 3)] = Q[3]  # a third of the items alike: ties everywhere
    return rng, P, Q


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), what
    pad = want[0] < 0
    assert np.isnan(got[1][pad]).all(), what
    assert np.array_equal(got[1].view(np.uint32)[~pad], want[1].view(np.uint32)[~pad]), what


def _csr(u, i, U):
    """(row_ptr int64[U + 1], items int32) of the distinct pairs: what seen(arange(U)) must return."""
    keys = np.unique((np.asarray(u, np.int64) << 32) | np.asarray(i, np.int64))
    ptr = np.searchsorted(keys >> 32, np.arange(U + 1)).astype(np.int64)
    return ptr, (keys & 0xFFFFFFFF).astype(np.int32)


def _seen_is(m, u, i, what=""):
    ptr, items = _csr(u, i, m.users)
    got = m.seen(np.arange(m.users))
    assert got[0].dtype == np.int64 and got[1].dtype == np.int32
    assert np.array_equal(got[0], ptr) and np.array_equal(got[1], items), what
    assert m.seen_size() == items.size, what


# ---- 1. every lane-group width: L = 1, a padded row, 16 and 64; fused and sort path ---------------------------------------
@pytest.mark.parametrize("k", [3, 20, 64, 256])
def test_recommend_unseen_is_recommend_excluding_at_every_group_width(mf, k):
    U, I = 64, 300
    rng, P, Q = _factors(U, I, k, 900 + k)
    eu, ei = rng.integers(0, U, 3000).astype(np.int32), rng.integers(0, I, 3000).astype(np.int32)
    every, none = 5, 9  # one user has seen every item: a row of padding; one has seen none
    keep = eu != none
    eu, ei = np.concatenate([eu[keep], np.full(I, every, np.int32)]), np.concatenate([ei[keep], np.arange(I, dtype=np.int32)])
    users = rng.permutation(U).astype(np.int32)
    users = np.append(users, users[0])  # every user, in any order, one of them twice
    shared = rng.integers(0, I, 120).astype(np.int32)
    lists = [rng.integers(0, I, rng.integers(0, I + 1)).astype(np.int32) for _ in range(users.size)]
    ptr = np.zeros(users.size + 1, np.int64)
    np.cumsum([c.size for c in lists], out=ptr[1:])
    csr = (ptr, np.concatenate(lists))
    with _model(mf, P, Q) as m:
        m.set_seen(eu, ei)
        _seen_is(m, eu, ei)
        for topn in (1, 10, 300):  # 300 takes the sort path: kTopnFused = 128
            got = m.recommend(users, topn, exclude="seen")
            _same(got, m.recommend(users, topn, exclude=(eu, ei)), f"k {k} topn {topn}")
            row = int(np.flatnonzero(users == every)[0])
            assert (got[0][row] == -1).all() and np.isnan(got[1][row]).all()
            row = int(np.flatnonzero(users == none)[0])
            _same((got[0][row:row + 1], got[1][row:row + 1]), m.recommend([none], topn), "a user who has seen nothing")
            for name, cand in (("shared", shared), ("csr", csr)):
                _same(m.recommend(users, topn, exclude="seen", candidates=cand),
                      m.recommend(users, topn, exclude=(eu, ei), candidates=cand), f"k {k} topn {topn} {name}")


# ---- 2. tiles -------------------------------------------------------------------------------------------------------------
def test_lists_that_cross_the_tiles_of_the_fused_kernel(mf):
    U, I, k, topn = 4, 2 * TILE + 5, 8, 50
    rng, P, Q = _factors(U, I, k, 77)
    edge = np.array([TILE - 1, TILE, 2 * TILE])  # the unseen items straddle both boundaries
    left = np.concatenate([edge, rng.choice(np.setdiff1d(np.arange(I), edge), 37, replace=False)])
    all_but_40 = np.setdiff1d(np.arange(I), left).astype(np.int32)  # one list longer than a tile
    last_tile = np.arange(2 * TILE, I, dtype=np.int32)[[0, 2, 4]]    # one list inside the last, 5-item tile
    some = rng.integers(0, I, 5000).astype(np.int32)
    eu = np.concatenate([np.zeros(all_but_40.size, np.int32), np.ones(last_tile.size, np.int32), np.full(some.size, 3, np.int32)])
    ei = np.concatenate([all_but_40, last_tile, some])
    users = np.array([0, 1, 2, 3, 0], np.int32)
    with _model(mf, P, Q) as m:
        m.set_seen(eu, ei)
        got = m.recommend(users, topn, exclude="seen")
        _same(got, m.recommend(users, topn, exclude=(eu, ei)))
        assert (got[0][0][:40] >= 0).all() and (got[0][0][40:] == -1).all()  # the first row pads after 40
        assert sorted(got[0][0][:40].tolist()) == sorted(left.tolist())
        assert not np.isin(got[0][1], last_tile).any()


# ---- 3. ranks ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", [3, 64])
def test_rank_items_unseen_is_rank_items_with_the_pairs(mf, k):
    U, I = 37, 500
    rng, P, Q = _factors(U, I, k, 40 + k)
    eu, ei = rng.integers(0, U, 6000).astype(np.int32), rng.integers(0, I, 6000).astype(np.int32)
    hu, hi = rng.integers(0, U, 400).astype(np.int32), rng.integers(0, I, 400).astype(np.int32)
    keep = eu != 7  # one user without anything seen
    eu, ei = eu[keep], ei[keep]
    hu[:50], hi[:50] = eu[:50], ei[:50]  # held-out pairs that are themselves in the index
    hu[50:60], hi[50:60] = hu[60:70], hi[60:70]  # duplicates
    hu[390:] = 7
    with _model(mf, P, Q) as m:
        m.set_seen(eu, ei)
        want = m.rank_items(hu, hi, exclude=(eu, ei))
        got = m.rank_items(hu, hi, exclude="seen")
        assert got.dtype == np.int32 and np.array_equal(got, want)
        assert not np.array_equal(got, m.rank_items(hu, hi))  # (the exclusions matter)
        a, b = m.evaluate_ranking(hu, hi, 10, exclude="seen"), m.evaluate_ranking(hu, hi, 10, exclude=(eu, ei))
        assert a.keys() == b.keys()
        for key in a:
            assert np.array_equal(a[key], b[key]), key
        # an empty index excludes nothing
        m.set_seen([], [])
        assert np.array_equal(m.rank_items(hu, hi, exclude="seen"), m.rank_items(hu, hi))
        _same(m.recommend(hu[:9], 10, exclude="seen"), m.recommend(hu[:9], 10))


# ---- 4. the merge -----------------------------------------------------------------------------------------------------------
def test_mark_seen_merges_into_the_index(mf):
    U, I = 50, 70  # dense: batches overlap the index heavily
    rng = np.random.default_rng(5)
    with mf.MatrixFactorizationSGD(U, I, 4, LR, LAM, 1) as m:
        # mark_seen on a handle without an index is set_seen
        au, ai = rng.integers(0, 40, 600).astype(np.int32), rng.integers(0, I, 600).astype(np.int32)  # users 40 .. 49: empty
        m.mark_seen(au, ai)
        _seen_is(m, au, ai, "mark_seen without an index")
        m.clear_seen()
        m.set_seen(au, ai)
        _seen_is(m, au, ai, "set_seen")
        su, si = au, ai
        for rd in range(20):
            n = int(rng.integers(0, 501))
            bu, bi = rng.integers(0, 45, n).astype(np.int32), rng.integers(0, I, n).astype(np.int32)
            if rd == 2:
                bu, bi = bu[:0], bi[:0]  # an empty batch
            elif rd == 3:
                pick = rng.integers(0, su.size, 300)
                bu, bi = su[pick], si[pick]  # entirely contained in the index
            elif rd == 4:
                bu, bi = rng.integers(45, 49, 60).astype(np.int32), rng.integers(0, I, 60).astype(np.int32)  # empty lists only
            elif rd in (5, 11):
                bu = np.concatenate([bu, [U - 1, U - 1, 0]]).astype(np.int32)  # the last user and the last item
                bi = np.concatenate([bi, [I - 1, 0, I - 1]]).astype(np.int32)
            size = m.seen_size()
            m.mark_seen(bu, bi)
            su, si = np.concatenate([su, bu]), np.concatenate([si, bi])
            _seen_is(m, su, si, f"round {rd}")
            if rd in (2, 3):
                assert m.seen_size() == size
            m.mark_seen(bu, bi)  # the same batch again changes nothing
            _seen_is(m, su, si, f"round {rd}, applied twice")
        assert m.seen_size() > 600
        # a failed check (a bad last pair) leaves the index as it was
        for call in (m.mark_seen, m.set_seen):
            with pytest.raises(mf.MfsgdError) as e:
                call(np.array([0, 1, U], np.int32), np.array([0, 1, 0], np.int32))
            assert e.value.code == INVALID_ARG and "pair 2 out of range" in str(e.value)
            _seen_is(m, su, si, "after a refused call")
        # requests in any order, with repeats
        users = np.array([49, 3, 3, 44, 0], np.int32)
        ptr, items = m.seen(users)
        all_ptr, all_items = _csr(su, si, U)
        assert np.array_equal(np.diff(ptr), np.diff(all_ptr)[users])
        for b, u in enumerate(users):
            assert np.array_equal(items[ptr[b]:ptr[b + 1]], all_items[all_ptr[u]:all_ptr[u + 1]])


# ---- 5. more pairs than one upload ----------------------------------------------------------------------------------------
def test_set_and_mark_seen_across_the_chunk_boundary(mf):
    U = I = 3000
    n = CHUNK + 1000
    rng = np.random.default_rng(6)
    with mf.MatrixFactorizationSGD(U, I, 4, LR, LAM, 1) as m:
        au, ai = rng.integers(0, U, n).astype(np.int32), rng.integers(0, I, n).astype(np.int32)
        au[-1], ai[-1] = U - 1, I - 1  # (the last pair of the second chunk)
        m.set_seen(au, ai)
        _seen_is(m, au, ai, "set_seen")
        bu, bi = rng.integers(0, U, n).astype(np.int32), rng.integers(0, I, n).astype(np.int32)
        bu[-1], bi[-1] = 0, 0
        m.mark_seen(bu, bi)
        _seen_is(m, np.concatenate([au, bu]), np.concatenate([ai, bi]), "mark_seen")


# ---- 6. growth --------------------------------------------------------------------------------------------------------------
def test_the_index_follows_a_growing_model(mf):
    U, I, k = 40, 30, 8
    rng = np.random.default_rng(8)
    ru, ri = rng.integers(0, U, 900).astype(np.int32), rng.integers(0, I, 900).astype(np.int32)
    rr = rng.uniform(1, 5, 900).astype(np.float32)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as m:
        m.reserve(U + 8, I + 8)
        m.set_ratings(ru, ri, rr)
        m.init_factors()
        m.fit(1)
        m.set_seen(ru, ri)
        su, si = ru, ri
        graphs, live = m.debug_counters()["graphs"], mf.debug_device_bytes()
        first = m.add_users(n=4)  # inside the capacity: nothing allocated, the cached graphs stay
        assert first == U and m.users == U + 4
        assert m.debug_counters()["graphs"] == graphs and mf.debug_device_bytes() == live
        new = np.arange(U, U + 4, dtype=np.int32)
        _same(m.recommend(new, 10, exclude="seen"), m.recommend(new, 10))
        _seen_is(m, su, si, "after an append inside the capacity")
        # the new users, and after add_items the new items, are valid in mark_seen
        with pytest.raises(mf.MfsgdError) as e:
            m.mark_seen([0, U + 4], [0, 0])  # a user that equals the count
        assert e.value.code == INVALID_ARG and "pair 1 out of range" in str(e.value)
        with pytest.raises(mf.MfsgdError):
            m.mark_seen([0], [I])
        m.mark_seen([U + 3, U, U], [I - 1, 0, 4])
        su, si = np.concatenate([su, [U + 3, U, U]]), np.concatenate([si, [I - 1, 0, 4]])
        _seen_is(m, su, si, "new users marked")
        assert m.add_items(n=2) == I
        m.mark_seen([U + 3, 2], [I + 1, I])
        su, si = np.concatenate([su, [U + 3, 2]]), np.concatenate([si, [I + 1, I]])
        _seen_is(m, su, si, "new items marked")
        _same(m.recommend(np.arange(U + 4), 5, exclude="seen"), m.recommend(np.arange(U + 4), 5, exclude=(su, si)))
        # beyond the capacity: the tables are copied, every list is kept
        old = m.seen(np.arange(U + 4))
        m.add_users(n=8)
        assert m.users == U + 12 and m.capacity()[0] == U + 12
        again = m.seen(np.arange(U + 4))
        assert old[0].tobytes() == again[0].tobytes() and old[1].tobytes() == again[1].tobytes()
        _seen_is(m, su, si, "after a reallocating append")
        m.reserve(U + 40)
        _seen_is(m, su, si, "after reserve")
        m.mark_seen([U + 11], [3])
        su, si = np.concatenate([su, [U + 11]]), np.concatenate([si, [3]])
        _seen_is(m, su, si, "the last new user marked")
        _same(m.recommend(np.arange(U + 12), 5, exclude="seen"), m.recommend(np.arange(U + 12), 5, exclude=(su, si)))
        assert np.isfinite(m.fit(1)).all()
        _seen_is(m, su, si, "after fit")


# ---- 7. the index and the model do not touch each other ---------------------------------------------------------------------
def test_the_index_and_the_model_are_independent(mf):
    U, I, k = 30, 25, 8
    rng = np.random.default_rng(9)

    def triples(n):
        return (rng.integers(0, U, n).astype(np.int32), rng.integers(0, I, n).astype(np.int32),
                rng.uniform(1, 5, n).astype(np.float32))
    t1, t2, t3, t4 = triples(500), triples(400), triples(60), triples(50)
    su, si = rng.integers(0, U, 300).astype(np.int32), rng.integers(0, I, 300).astype(np.int32)
    P0 = rng.standard_normal((U, k)).astype(np.float32)
    Q0 = rng.standard_normal((I, k)).astype(np.float32)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as a, mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as b:
        a.set_seen(su, si)  # b never has an index
        steps = [
            lambda m: m.init_factors(),
            lambda m: m.set_ratings(*t1),
            lambda m: m.fit(1),
            lambda m: m.set_ratings(*t2),
            lambda m: m.set_hyper(0.02, 0.01),
            lambda m: m.fit(2),
            lambda m: m.set_factors(P0, Q0),
            lambda m: m.partial_fit(*t3),
            lambda m: m.fit(1),
            lambda m: m.init_factors(3),
            lambda m: m.fit(1),
        ]
        for x, step in enumerate(steps):
            step(a)
            step(b)
            _seen_is(a, su, si, f"step {x}")
            a.recommend([0, 1], 3, exclude="seen")  # (reading the index between the steps changes nothing either)
            Pa, Qa = a.get_factors()
            Pb, Qb = b.get_factors()
            assert Pa.tobytes() == Pb.tobytes() and Qa.tobytes() == Qb.tobytes(), f"step {x}"
        # partial_fit(seen=True) adds exactly its pairs, and applies what partial_fit applies
        a.partial_fit(*t4, seen=True)
        b.partial_fit(*t4)
        _seen_is(a, np.concatenate([su, t4[0]]), np.concatenate([si, t4[1]]), "partial_fit(seen=True)")
        assert a.get_factors()[0].tobytes() == b.get_factors()[0].tobytes()
        assert a.get_factors()[1].tobytes() == b.get_factors()[1].tobytes()
        assert b.seen_size() == -1


# ---- 8. memory --------------------------------------------------------------------------------------------------------------
def test_the_index_holds_what_the_bound_says_and_the_calls_keep_nothing(mf):
    U, I, k = 500, 400, 16
    rng, P, Q = _factors(U, I, k, 10)
    live = mf.debug_device_bytes
    gc.collect()
    before = live()
    m = _model(mf, P, Q)
    try:
        m.reserve(U + 100)
        m.recommend([0], 5)  # the factors are on the device from here on
        level = live()

        def bound(d):
            return 4 * d + 12 * (m.capacity()[0] + 1) + 64
        su, si = rng.integers(0, U, 20000).astype(np.int32), rng.integers(0, I, 20000).astype(np.int32)
        m.set_seen(su, si)
        d = m.seen_size()
        assert d == _csr(su, si, U)[1].size
        assert 4 * d <= live() - level <= bound(d)
        bu, bi = rng.integers(0, U, 30000).astype(np.int32), rng.integers(0, I, 30000).astype(np.int32)
        m.mark_seen(bu, bi)
        d2 = m.seen_size()
        assert d2 > d and 4 * d2 <= live() - level <= bound(d2)
        held = live()
        m.mark_seen(bu[:100], bi[:100])  # nothing new: nothing moves
        assert live() == held
        users = np.arange(0, U, 7, dtype=np.int32)
        for call in (lambda: m.recommend(users, 10, exclude="seen"), lambda: m.recommend(users, 200, exclude="seen"),
                     lambda: m.recommend(users, 10, exclude="seen", candidates=np.arange(50)),
                     lambda: m.rank_items(users, users % I, exclude="seen"),
                     lambda: m.evaluate_ranking(users, users % I, 10, exclude="seen"), lambda: m.seen(users)):
            call()
            assert live() == held
        m.set_seen(su, si)  # replaced: back to the first size
        assert live() - level <= bound(d) and m.seen_size() == d
        m.clear_seen()
        assert live() == level and m.seen_size() == -1
        m.set_seen([], [])  # an empty index holds nothing
        assert live() == level
        m.set_seen(su, si)
    finally:
        m.close()
    assert live() == before


# ---- 9. batches of request rows: the fused path -----------------------------------------------------------------------------
def test_fused_path_batches_with_exclusions_and_candidates(mf, oracle):
    """The shape of test_fused_path_more_users_than_one_launch (tests/test_serving_edges_gpu.py): 70 000 request rows are a
    launch of 65 535 and one of 4 465.  Across the cut `ex` stays as it is while the users restart at the batch, for a
    pair list and for the index's identity slot table, and am.off += done re-bases the per-row candidate lists."""
    U, I, k, topn = 70000, 5, 4, 5
    assert -(-U // LAUNCH_ROWS) == 2
    rng = np.random.default_rng(70001)
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    Q[3] = Q[1]  # a tie in every row
    users = rng.permutation(U).astype(np.int32)  # (request row b is user users[b]: the lists go by user, not by row)
    edge = np.array([65534, 65535, 65536, 69999])
    half = np.unique(np.concatenate([rng.choice(U, U // 2, replace=False), edge, users[edge]])).astype(np.int32)
    eu, ei = np.repeat(half, 2), rng.integers(0, I, 2 * half.size).astype(np.int32)
    perm = rng.permutation(eu.size)
    eu, ei = np.ascontiguousarray(eu[perm]), np.ascontiguousarray(ei[perm])
    cand = np.argsort(rng.random((U, I)), axis=1)[:, :3].astype(np.int32)  # three of the five items per request row
    ptr = 3 * np.arange(U + 1, dtype=np.int64)
    sc = oracle.predict(P, Q, np.repeat(users, I), np.tile(np.arange(I, dtype=np.int32), U)).reshape(U, I)
    item = np.broadcast_to(np.arange(I, dtype=np.int32), (U, I))
    row_of_user = np.empty(U, np.int64)
    row_of_user[users] = np.arange(U)
    X = np.zeros((U, I), bool)
    X[row_of_user[eu], ei] = True
    C = np.zeros((U, I), bool)
    np.put_along_axis(C, cand.astype(np.int64), True, axis=1)

    def ref(out):
        """per row: the items that are not `out`, the larger score first, ties by the smaller item; -1 / NaN behind them"""
        order = np.lexsort((item, -sc.astype(np.float64), out), axis=1)
        pad = np.take_along_axis(out, order, axis=1)
        return (np.where(pad, -1, order).astype(np.int32), np.where(pad, np.float32(np.nan), np.take_along_axis(sc, order, axis=1)))
    want_x, want_c, want_cx = ref(X), ref(~C), ref(~C | X)
    plain = ref(np.zeros((U, I), bool))
    some = np.array([0, 65534, 65535, 65536, 69999])
    E.assert_recommend((want_x[0][some], want_x[1][some]), E.recommend_ref(oracle, P, Q, users[some], topn, eu, ei))
    second = np.arange(LAUNCH_ROWS, U)
    for want in (want_x, want_c, want_cx):  # the second launch's lists change its rows
        assert (want[0][second] != plain[0][second]).any(axis=1).sum() > second.size // 3
    assert (want_cx[0][second] != want_c[0][second]).any() and X[edge].any(axis=1).all()
    with _model(mf, P, Q) as m:
        _same(m.recommend(users, topn, exclude=(eu, ei)), want_x, "a pair list")
        _same(m.recommend(users, topn, candidates=(ptr, cand.ravel())), want_c, "per-row candidates")
        m.set_seen(eu, ei)
        got = m.recommend(users, topn, exclude="seen")
        _same(got, want_x, "the index")
        for b in edge:
            assert not np.isin(ei[eu == users[b]], got[0][b]).any()
        _same(m.recommend(users, topn, exclude="seen", candidates=(ptr, cand.ravel())), want_cx, "candidates and the index")


# ---- 10. batches of request rows: the sort path -----------------------------------------------------------------------------
def test_sort_path_batches_with_exclusions(mf, oracle):
    """The shape of test_sort_path_more_users_than_one_staging_batch: a batch of 292 users and one of 8, every user's
    three best items and 1 000 random ones excluded, as a pair list and from the index."""
    I, k, topn, n_users = 16 * TILE + 1, 4, 129, 300
    assert SORT_CELLS // I == 292 and topn > 128
    rng, P, Q = E.tied_factors(n_users, I, k, 301)
    users = rng.permutation(n_users).astype(np.int32)
    rows = {}
    best = {int(u): E.top_of(rows.setdefault(int(u), E.all_scores(oracle, P, Q, int(u))), 3) for u in users}
    eu = np.repeat(users, 1003)
    ei = np.concatenate([np.concatenate([best[int(u)], rng.integers(0, I, 1000)]) for u in users]).astype(np.int32)
    perm = rng.permutation(eu.size)
    eu, ei = np.ascontiguousarray(eu[perm]), np.ascontiguousarray(ei[perm])
    want = E.recommend_ref(oracle, P, Q, users, topn, eu, ei, score_rows=rows)
    for b in range(292, n_users):  # the second batch: the best items would have led the row
        assert not np.isin(best[int(users[b])], want[0][b]).any()
    with _model(mf, P, Q) as m:
        got = m.recommend(users, topn, exclude=(eu, ei))
        E.assert_recommend(got, want, "a pair list")
        m.set_seen(eu, ei)
        seen = m.recommend(users, topn, exclude="seen")
        E.assert_recommend(seen, want, "the index")
    for b in range(292, n_users):
        assert not np.isin(best[int(users[b])], got[0][b]).any() and not np.isin(best[int(users[b])], seen[0][b]).any()


# ---- 11. lists read back past the strides of the gather ---------------------------------------------------------------------
def test_seen_reads_back_past_the_strides_of_the_gather(mf):
    """gather_kernel strides over a list in at most 64 parts of 256 positions and over the request rows in at most 4 096
    workgroups: a list of 17 000 and one of 20 000 items, asked for at request rows beyond 4 096, take second trips of both
    loops.  Then a merge that adds 3 000 keys to the long user, interleaved with its old ones."""
    U, I = 5000, 20000
    long_user, full_user = 4321, 77
    rng = np.random.default_rng(11)
    assert 17000 > GATHER_SPAN and I > GATHER_SPAN and U + 200 > GATHER_ROWS
    has = rng.permutation(I)[:17000].astype(np.int32)
    lens = rng.integers(0, 6, U)
    lens[[long_user, full_user]] = 0
    su = np.concatenate([np.repeat(np.arange(U), lens), np.full(has.size, long_user), np.full(I, full_user)]).astype(np.int32)
    si = np.concatenate([rng.integers(0, I, int(lens.sum())), has, np.arange(I)]).astype(np.int32)
    perm = rng.permutation(su.size)
    su, si = su[perm], si[perm]
    users = rng.permutation(U).astype(np.int32)
    for at, user in ((4500, long_user), (4999, full_user)):  # the long lists at request rows of the second trip
        users[np.flatnonzero(users == user)[0]] = users[at]
        users[at] = user
    users = np.concatenate([users, rng.integers(0, U, 198), [long_user, 3]]).astype(np.int32)
    assert users.size == U + 200 and np.flatnonzero(users == long_user).min() >= GATHER_ROWS
    assert np.flatnonzero(users == full_user).min() >= GATHER_ROWS and np.array_equal(np.unique(users), np.arange(U))

    def check(m, su, si, what):
        all_ptr, all_items = _csr(su, si, U)
        ptr, items = m.seen(users)
        assert np.array_equal(np.diff(ptr), np.diff(all_ptr)[users]), what
        want = np.concatenate([all_items[all_ptr[u]:all_ptr[u + 1]] for u in users])
        assert np.array_equal(items, want), what
        ptr, items = m.seen([long_user])  # one request row, many parts
        assert ptr.tolist() == [0, all_ptr[long_user + 1] - all_ptr[long_user]], what
        assert np.array_equal(items, all_items[all_ptr[long_user]:all_ptr[long_user + 1]]), what
        return items.size
    with mf.MatrixFactorizationSGD(U, I, 4, LR, LAM, 1) as m:
        m.set_seen(su, si)
        assert check(m, su, si, "set_seen") == 17000
        _seen_is(m, su, si, "set_seen")
        more = np.concatenate([np.setdiff1d(np.arange(I), has), has[:500]]).astype(np.int32)  # 3 000 new, 500 it has
        rng.shuffle(more)
        bu, bi = np.full(more.size, long_user, np.int32), more
        m.mark_seen(bu, bi)
        su, si = np.concatenate([su, bu]), np.concatenate([si, bi])
        assert check(m, su, si, "mark_seen") == I
        _seen_is(m, su, si, "mark_seen")


# ---- 12. growth with the factors on host staging ----------------------------------------------------------------------------
def test_the_index_follows_appends_on_host_staging(mf, oracle):
    """set_factors leaves the factors on host staging until the first compute call (csrc/handle.cpp, Where::Host); the
    index is on the device all the same, and an append that reallocates, a reserve and an append in place move or keep
    its per-user tables as they do with the factors on the device."""
    U, I, k = 40, 30, 8
    rng, P, Q = _factors(U, I, k, 12)
    su, si = rng.integers(0, U, 500).astype(np.int32), rng.integers(0, I, 500).astype(np.int32)
    new = rng.standard_normal((8, k)).astype(np.float32)
    with _model(mf, P, Q) as m:
        m.set_seen(su, si)
        assert m.add_users(new[:6]) == U and m.capacity()[0] == U + 6  # beyond the capacity
        _seen_is(m, su, si, "after a reallocating append on host staging")
        m.mark_seen([U + 5, U, 0], [3, I - 1, 0])
        su, si = np.concatenate([su, [U + 5, U, 0]]).astype(np.int32), np.concatenate([si, [3, I - 1, 0]]).astype(np.int32)
        _seen_is(m, su, si, "new users marked")
        m.reserve(U + 20)
        _seen_is(m, su, si, "after reserve")
        assert m.add_users(new[6:]) == U + 6 and m.capacity()[0] == U + 20  # in place
        _seen_is(m, su, si, "after an append in place on host staging")
        users = np.arange(U + 8, dtype=np.int32)
        got = m.recommend(users, 5, exclude="seen")  # (the first compute call: the factors go up now)
        _seen_is(m, su, si, "after the upload")
    want = E.recommend_ref(oracle, np.vstack([P, new]), Q, users, 5, su, si)
    assert not np.array_equal(want[0], E.recommend_ref(oracle, np.vstack([P, new]), Q, users, 5)[0])
    E.assert_recommend(got, want)
