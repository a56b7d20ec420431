"""The seen-item index on the device: set_seen / mark_seen / seen against numpy's unique of the same pairs, and the serving
calls with exclude="seen" against the same calls given the index's pairs as a list, which build their lists per call and
do not read the index.  Items and ranks compare exactly, scores bit for bit, padding (-1, NaN) by position."""
import gc

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LR, LAM = 0.01, 0.05
TILE = 14336      # csrc/recommend.hip: kTopnTile, positions per tile of the fused kernel
CHUNK = 1 << 22   # csrc/handle.hpp: kExclChunk, pairs per upload of set_seen / mark_seen
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
