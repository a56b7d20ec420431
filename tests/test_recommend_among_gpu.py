"""recommend(users, topn, exclude, candidates=...) -- mfsgd_recommend_among / mfsgd_recommend_rows_among -- against two
references that do not run the gathered kernel:
(a) the contract itself: recommend(users, n_items, exclude) from the existing whole-catalogue path, every item outside
    the row's list deleted on the host, cut or padded to topn;
(b) predict() of every (user, candidate) pair, ordered on the host by score descending (-0.0 equal to +0.0), then item
    ascending.
Items compare exactly, scores bit for bit, padding (-1, NaN) by position."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LR, LAM = 0.01, 0.05
TILE = 14336  # csrc/recommend.hip: kTopnTile, positions per tile of the fused kernel
NONE = np.empty(0, np.int32)


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


def _padded(rows, topn):
    items = np.full((len(rows), topn), -1, np.int32)
    scores = np.full((len(rows), topn), np.nan, np.float32)
    for b, (it, sc) in enumerate(rows):
        items[b, :it.size] = it
        scores[b, :it.size] = sc
    return items, scores


def _ref_a(full, lists, topn):
    """From (items, scores) of recommend(users, n_items, exclude): what is left of each row inside its list."""
    rows = []
    for b, cand in enumerate(lists):
        keep = np.isin(full[0][b], cand)  # (the row's padding, -1, is in no list)
        rows.append((full[0][b][keep][:topn], full[1][b][keep][:topn]))
    return _padded(rows, topn)


def _ref_b(predict, users, lists, topn, eu=NONE, ei=NONE):
    """predict(u, i) of every (row's user, distinct candidate the user does not exclude), one call for all rows."""
    cands = []
    for u, cand in zip(users, lists):
        c = np.unique(np.asarray(cand, np.int32))
        cands.append(c[~np.isin(c, ei[eu == u])])
    pu = np.concatenate([np.full(c.size, u, np.int32) for u, c in zip(users, cands)])
    pi = np.concatenate(cands) if cands else NONE
    sc = predict(pu, pi) if pu.size else np.empty(0, np.float32)
    rows, at = [], 0
    for c in cands:
        s = sc[at:at + c.size]
        at += c.size
        order = np.lexsort((c, -s.astype(np.float64)))[:topn]
        rows.append((c[order], s[order]))
    return _padded(rows, topn)


def _same(got, want, what=""):
    assert np.array_equal(got[0], want[0]), what
    pad = want[0] < 0
    assert np.isnan(got[1][pad]).all(), what
    assert np.array_equal(got[1].view(np.uint32)[~pad], want[1].view(np.uint32)[~pad]), what


def _check(m, users, lists, topn, exclude=None, full=None, form="csr", what=""):
    """recommend(..., candidates=lists) in the given form against both references; returns what it gave."""
    eu, ei = (NONE, NONE) if exclude is None else exclude
    if form == "shared":
        cand = np.asarray(lists[0], np.int32)
    elif form == "csr":
        ptr = np.zeros(len(lists) + 1, np.int64)
        np.cumsum([len(c) for c in lists], out=ptr[1:])
        cand = (ptr, np.concatenate([np.asarray(c, np.int32) for c in lists]))
    else:
        cand = [np.asarray(c, np.int32) for c in lists]
    got = m.recommend(users, topn, exclude=exclude, candidates=cand)
    if full is None:
        full = m.recommend(users, m.items, exclude=exclude)
    _same(got, _ref_a(full, lists, topn), f"{what} topn {topn} {form}: against the filtered whole-catalogue order")
    _same(got, _ref_b(m.predict, users, lists, topn, eu, ei), f"{what} topn {topn} {form}: against sorted predictions")
    return got


def _random_lists(rng, n, I):
    """Unsorted, with duplicates, of length 0 .. I; the first two (one user asked twice) differ, the third is empty."""
    lists = [rng.integers(0, I, rng.integers(0, I + 1)).astype(np.int32) for _ in range(n)]
    lists[0] = rng.integers(0, I // 2, 40).astype(np.int32)
    lists[1] = rng.integers(I // 2, I, 200).astype(np.int32)
    lists[2] = NONE
    return lists


# ---- every lane-group width: L = 1, a padded row, 16 and 64 ----------------------------------------------------------
@pytest.mark.parametrize("k", [3, 20, 64, 256])
def test_per_row_lists_at_every_group_width(mf, k):
    U, I = 64, 300
    rng, P, Q = _factors(U, I, k, 300 + k)
    users = rng.permutation(U).astype(np.int32)
    users[1] = users[0]  # the same user twice, with two different lists
    lists = _random_lists(rng, U, I)
    eu, ei = rng.integers(0, U, 3000).astype(np.int32), rng.integers(0, I, 3000).astype(np.int32)
    with _model(mf, P, Q) as m:
        full, full_x = m.recommend(users, I), m.recommend(users, I, exclude=(eu, ei))
        for topn in (1, 10):
            got = _check(m, users, lists, topn, full=full, form="csr")
            _check(m, users, lists, topn, exclude=(eu, ei), full=full_x, form="sequence")
            assert not np.array_equal(got[0][0], got[0][1])  # the two rows of one user answer their own lists
            assert (got[0][2] == -1).all() and np.isnan(got[1][2]).all()


@pytest.mark.parametrize("k", [3, 20, 64, 256])
def test_one_shared_list_shorter_than_a_pass_of_the_lane_groups(mf, k):
    U, I, topn = 300, 300, 10
    rng, P, Q = _factors(U, I, k, 37 + k)
    users = np.arange(U, dtype=np.int32)
    shared = rng.choice(I, 37, replace=False).astype(np.int32)
    # pairs that hit the list for the even users only; the odd users exclude items outside it
    outside = np.setdiff1d(np.arange(I, dtype=np.int32), shared)
    eu = np.repeat(users, 30)
    ei = np.where(eu % 2 == 0, rng.choice(shared, eu.size), rng.choice(outside, eu.size)).astype(np.int32)
    with _model(mf, P, Q) as m:
        plain = _check(m, users, [shared] * U, topn, form="shared")
        excl = _check(m, users, [shared] * U, topn, exclude=(eu, ei), form="shared")
    assert np.array_equal(excl[0][1::2], plain[0][1::2]) and not np.array_equal(excl[0][0::2], plain[0][0::2])


# ---- padding ---------------------------------------------------------------------------------------------------------
def test_short_empty_and_wholly_excluded_lists_are_padded(mf):
    U, I, k, topn = 8, 300, 20, 10
    rng, P, Q = _factors(U, I, k, 5)
    users = np.array([0, 1, 2, 3, 2], np.int32)
    gone = rng.choice(I, 25, replace=False).astype(np.int32)
    lists = [np.array([5, 3], np.int32), NONE, gone[::-1], np.arange(I, dtype=np.int32), gone]
    eu, ei = np.full(gone.size, 2, np.int32), gone  # user 2 excludes all of its list, in both of its rows
    with _model(mf, P, Q) as m:
        got = _check(m, users, lists, topn, exclude=(eu, ei))
        empty = m.recommend(users[:3], topn, candidates=NONE)  # one shared empty list
        _same(m.recommend(users, topn, candidates=lists), _ref_b(m.predict, users, lists, topn))
    assert sorted(got[0][0][:2]) == [3, 5] and (got[0][0][2:] == -1).all()
    for b in (1, 2, 4):
        assert (got[0][b] == -1).all() and np.isnan(got[1][b]).all()
    assert (got[0][3] >= 0).all()
    assert (empty[0] == -1).all() and np.isnan(empty[1]).all()


# ---- a list that names every item is recommend_excluding's row, bit for bit --------------------------------------------
@pytest.mark.parametrize("topn", [10, 128, 300])  # fused; the largest fused topn; the sort path (topn == n_items)
def test_a_full_list_is_recommend_excluding(mf, topn):
    U, I, k = 12, 300, 20
    rng, P, Q = _factors(U, I, k, topn)
    users = np.array([3, 0, 11, 3, 7], np.int32)
    every = [rng.permutation(I).astype(np.int32) for _ in users]
    eu = np.concatenate([np.full(I, 7), rng.integers(0, U, 500)]).astype(np.int32)  # user 7 excludes everything
    ei = np.concatenate([np.arange(I), rng.integers(0, I, 500)]).astype(np.int32)
    with _model(mf, P, Q) as m:
        for exclude in (None, (eu, ei)):
            want = m.recommend(users, topn, exclude=exclude)
            _same(m.recommend(users, topn, exclude=exclude, candidates=every), want)
            _same(m.recommend(users, topn, exclude=exclude, candidates=every[0]), want)


# ---- ties --------------------------------------------------------------------------------------------------------------
def test_ties_go_to_the_smaller_item_not_to_the_earlier_place_in_the_list(mf):
    U, I, k, topn = 4, 300, 8, 10
    rng = np.random.default_rng(11)
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = np.repeat(rng.standard_normal((I // 6, k)).astype(np.float32), 6, axis=0)  # groups of six identical rows
    # user 0 is all zeros and the rows of Q have one sign each: its scores are +0.0 and -0.0, one tie group
    P[0] = 0.0
    Q[:120] = np.abs(Q[:120]) * np.where(np.arange(120) % 2 == 0, 1.0, -1.0).astype(np.float32)[:, None]
    users = np.array([0, 1, 2, 0], np.int32)
    down = np.arange(I - 1, -1, -1, dtype=np.int32)  # descending: the larger index of a group comes first in the list
    lists = [down[down < 120], down[::2], down, rng.permutation(np.arange(0, 120, 3)).astype(np.int32)]
    with _model(mf, P, Q) as m:
        zero = m.predict(np.zeros(120, np.int32), np.arange(120, dtype=np.int32))
        assert (zero == 0).all() and np.signbit(zero).any() and not np.signbit(zero).all()
        got = _check(m, users, lists, topn)
        got129 = _check(m, users, lists, 129)  # the sort path
    assert np.array_equal(got[0][0], np.arange(topn)) and np.array_equal(got[0][3], np.arange(0, 3 * topn, 3))
    assert np.array_equal(got129[0][0][:120], np.arange(120))
    for b in (1, 2):  # inside a group of identical rows the smaller index comes first
        it, sc = got[0][b], got[1][b]
        tied = sc[1:] == sc[:-1]
        assert tied.any() and (it[1:][tied] > it[:-1][tied]).all()


# ---- the tile boundary of the fused kernel ---------------------------------------------------------------------------------
@pytest.mark.parametrize("topn", [10, 128])
def test_lists_of_one_tile_and_of_one_tile_and_one_item(mf, topn):
    U, I, k = 4, 20000, 8
    rng = np.random.default_rng(TILE + topn)
    P = np.abs(rng.standard_normal((U, k))).astype(np.float32) + 0.1
    Q = rng.standard_normal((I, k)).astype(np.float32)
    over = np.sort(rng.choice(I, TILE + 1, replace=False)).astype(np.int32)   # two tiles: the second holds one item
    exact = np.sort(rng.choice(I - 100, TILE, replace=False)).astype(np.int32)  # exactly one tile, its end another item
    assert over[TILE - 1] > exact[TILE - 1]
    # the best scores of every user at the last position of each list and at the last of the first tile
    planted = [over[TILE], over[TILE - 1], exact[TILE - 1]]
    Q[planted] = np.array([[9.0], [8.0], [7.0]], np.float32)
    users = np.array([0, 1, 2, 3], np.int32)
    lists = [rng.permutation(over), rng.permutation(exact), rng.permutation(exact), rng.permutation(over)]
    with _model(mf, P, Q) as m:
        full = m.recommend(users, I)
        got = _check(m, users, lists, topn, full=full)
        shared = _check(m, users, [lists[0]] * 4, topn, full=full, form="shared")
    for b, cand in enumerate((over, exact, exact, over)):
        want = [x for x in planted if x in cand]
        assert list(got[0][b][:len(want)]) == want
    assert list(shared[0][2][:2]) == planted[:2]


# ---- past the fused limits: the sort path, its segments the lists ---------------------------------------------------------
def test_topn_129_takes_the_sort_path_with_segments_of_unequal_length(mf):
    U, I, k, topn = 8, 300, 20, 129
    rng, P, Q = _factors(U, I, k, 129)
    users = np.array([0, 5, 5, 1, 2, 3, 4, 7, 6], np.int32)
    lengths = [300, 0, 1, 150, 129, 128, 0, 299, 0]
    lists = [rng.permutation(I)[:n].astype(np.int32) for n in lengths]
    lists[3] = np.concatenate([lists[3], lists[3][:70]])  # duplicates
    eu, ei = rng.integers(0, U, 600).astype(np.int32), rng.integers(0, I, 600).astype(np.int32)
    with _model(mf, P, Q) as m:
        _check(m, users, lists, topn)
        _check(m, users, lists, topn, exclude=(eu, ei))
        _check(m, users[:1], lists[:1], topn, form="shared")
        _check(m, users, [lists[4]] * users.size, topn, exclude=(eu, ei), form="shared")
        nothing = m.recommend(users[:2], topn, candidates=[NONE, NONE])
    assert (nothing[0] == -1).all() and np.isnan(nothing[1]).all()


def test_a_list_of_more_tiles_than_the_candidate_table_holds_takes_the_sort_path(mf):
    U, I, k, topn = 2, 250000, 4, 128  # 18 tiles x 128 > kTopnCand = 2048
    rng = np.random.default_rng(245)
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    Q[rng.integers(0, I, I // 3)] = Q[3]
    users = np.array([1, 0], np.int32)
    big = rng.permutation(I)[:245000].astype(np.int32)
    with _model(mf, P, Q) as m:
        _check(m, users, [big, big[::-1]], topn)
        _check(m, users, [big] * 2, topn, form="shared")


# ---- rows that are not in the model --------------------------------------------------------------------------------------
def test_recommend_rows_among_for_folded_in_rows(mf):
    U, I, k, topn, n_new = 10, 300, 20, 10, 6
    rng, P, Q = _factors(U, I, k, 66)
    counts = rng.integers(1, 30, n_new)
    ptr = np.concatenate([[0], np.cumsum(counts)]).astype(np.int64)
    rated = rng.integers(0, I, ptr[-1]).astype(np.int32)
    lists = _random_lists(rng, n_new, I)
    er = np.repeat(np.arange(n_new, dtype=np.int32), counts)  # a row never gets back what it rated
    with _model(mf, P, Q) as m:
        rows = m.fold_in(ptr, rated, rng.uniform(1, 5, rated.size).astype(np.float32), 3)
        full = m.recommend_rows(rows, I, exclude=(er, rated))
        got = m.recommend_rows(rows, topn, exclude=(er, rated), candidates=lists)
        shared = m.recommend_rows(rows, topn, candidates=lists[1])
        full_plain = m.recommend_rows(rows, I)
    _same(got, _ref_a(full, lists, topn))
    _same(shared, _ref_a(full_plain, [lists[1]] * n_new, topn))
    with _model(mf, rows, Q) as as_users:  # (b): the rows as the users of a model of their own
        who = np.arange(n_new, dtype=np.int32)
        _same(got, _ref_b(as_users.predict, who, lists, topn, er, rated))
        _same(shared, _ref_b(as_users.predict, who, [lists[1]] * n_new, topn))


# ---- a model that grew -----------------------------------------------------------------------------------------------------
def test_appended_items_are_candidates(mf):
    U, I, k, n_new = 6, 300, 20, 7
    rng, P, Q = _factors(U, I, k, 77)
    users = np.array([0, 5, 2], np.int32)
    with _model(mf, P, Q) as m:
        m.recommend(users, 3)  # the factors are on the device from here on
        new_rows = rng.standard_normal((n_new, k)).astype(np.float32)
        first = m.add_items(new_rows)
        assert first == I and m.items == I + n_new
        new = np.arange(first, first + n_new, dtype=np.int32)
        got = _check(m, users, [new[::-1]] * 3, n_new + 2, form="shared")
        with pytest.raises(mf.MfsgdError, match="recommend_among: candidate 1 out of range"):
            m.recommend(users, 3, candidates=[0, I + n_new])
    assert (np.sort(got[0][:, :n_new], axis=1) == new).all() and (got[0][:, n_new:] == -1).all()


# ---- nothing kept, nothing changed -----------------------------------------------------------------------------------------
def test_no_device_memory_is_kept_and_the_model_is_not_modified(mf):
    U, I, k = 16, 20000, 8
    rng = np.random.default_rng(8)
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    users = np.arange(U, dtype=np.int32)
    eu, ei = rng.integers(0, U, 5000).astype(np.int32), rng.integers(0, I, 5000).astype(np.int32)
    short = [rng.integers(0, I, 100).astype(np.int32) for _ in users]
    long = [rng.permutation(I)[:TILE + 500].astype(np.int32) for _ in users]
    with _model(mf, P, Q) as m:
        m.recommend(users, 3)  # the factors go to the device
        before, live = [f.tobytes() for f in m.get_factors()], mf.debug_device_bytes()
        calls = [
            lambda: m.recommend(users, 10, candidates=short),                         # the fused kernel
            lambda: m.recommend(users, 10, candidates=long, exclude=(eu, ei)),        # ... over two tiles
            lambda: m.recommend(users, 10, candidates=short[0], exclude=(eu, ei)),    # one shared list
            lambda: m.recommend(users, 129, candidates=long, exclude=(eu, ei)),       # the sort path
            lambda: m.recommend(users, 129, candidates=short),
            lambda: m.recommend(users, 10, candidates=NONE),                          # nothing to do
            lambda: m.recommend_rows(P[:4], 10, candidates=short[:4], exclude=(eu[eu < 4], ei[eu < 4])),
        ]
        for x, call in enumerate(calls):
            call()
            assert mf.debug_device_bytes() == live, x
        for bad in (dict(candidates=[0, I]), dict(candidates=short, exclude=(eu, ei + I))):
            with pytest.raises(mf.MfsgdError):
                m.recommend(users, 10, **bad)
            assert mf.debug_device_bytes() == live
        assert [f.tobytes() for f in m.get_factors()] == before


def test_candidates_none_is_todays_call(mf):
    U, I, k = 12, 300, 20
    rng, P, Q = _factors(U, I, k, 1)
    users = np.array([3, 0, 11], np.int32)
    eu, ei = rng.integers(0, U, 300).astype(np.int32), rng.integers(0, I, 300).astype(np.int32)
    with _model(mf, P, Q) as m:
        for n in (10, 129):
            _same(m.recommend(users, n, candidates=None), m.recommend(users, n))
            _same(m.recommend(users, n, exclude=(eu, ei), candidates=None), m.recommend(users, n, (eu, ei)))
            _same(m.recommend_rows(P[:3], n, candidates=None), m.recommend_rows(P[:3], n))
