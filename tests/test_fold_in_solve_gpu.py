"""gram(...), fold_in_exact(...), fold_in_implicit(...), their item-side mirrors, fit_als(...) and fit_ials(...) --
mfsgd_gram and mfsgd_fold_in_solve -- against the C restatement of the rule (tests/solve_common.py), bit for bit."""
import functools

import numpy as np
import pytest

from tests import solve_common as sc

pytestmark = pytest.mark.gpu

LR, LAM = 0.01, 0.05


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    return np.array_equal(_bits(got), _bits(want))


@pytest.mark.parametrize("k", [1, 3, 12, 64, 200, 256])
def test_gram_of_both_sides_at_the_tile_edges(mf, k):
    rng = np.random.default_rng(50 + k)
    for n in (1, 255, 256, 257, 1000):
        P, Q = sc.fixed_side(n, k, rng), sc.fixed_side(n + 3, k, rng)
        with mf.MatrixFactorizationSGD(n, n + 3, k, LR, LAM, 1) as m:
            m.set_factors(P, Q)
            gp, gq = m.gram("users"), m.gram("items")
        assert _same(gp, sc.gram(P)), f"users n={n}"
        assert _same(gq, sc.gram(Q)), f"items n={n + 3}"
        assert np.array_equal(gq, gq.T)


def test_gram_where_the_tile_size_doubles(mf):
    rng = np.random.default_rng(6)
    n, k = 65537, 8
    F = sc.fixed_side(n, k, rng)
    with mf.MatrixFactorizationSGD(4, n, k, LR, LAM, 1) as m:
        m.set_factors(np.zeros((4, k), np.float32), F)
        assert _same(m.gram("items"), sc.gram(F))
        assert not m.gram("users").any()


@functools.lru_cache(maxsize=2)
def _reference(k):
    """The restatement's rows of the three forms on the inputs of case(k): computed once, shared by both sides."""
    c = sc.case(k)
    ref = dict(exact=sc.exact(c["F"], c["row_ptr"], c["ids"], c["r"], LAM),
               weighted=sc.exact(c["F"], c["row_ptr"], c["ids"], c["r"], LAM, c["w"]),
               implicit=sc.implicit(c["F"], c["row_ptr"], c["ids"], c["c"], sc.LAM_IMPLICIT))
    for rows, st in ref.values():
        assert not st.any() and np.isfinite(rows).all()
    return c, ref


@pytest.mark.parametrize("side", ["users", "items"])
@pytest.mark.parametrize("k", sc.K_ALL)
def test_every_form_matches_the_restatement_at_every_group_width(mf, k, side):
    """New users against Q = F, or new items against P = F: the same lists, so the same rows."""
    c, ref = _reference(k)
    assert sc.LAM_EXACT == LAM
    F, ptr, ids = c["F"], c["row_ptr"], c["ids"]
    other = np.zeros((20, k), np.float32)
    users = side == "users"
    with (mf.MatrixFactorizationSGD(20, sc.N_FIXED, k, LR, LAM, 11) if users else
          mf.MatrixFactorizationSGD(sc.N_FIXED, 20, k, LR, LAM, 11)) as m:
        m.set_factors(*((other, F) if users else (F, other)))
        exact = m.fold_in_exact if users else m.fold_in_items_exact
        implicit = m.fold_in_implicit if users else m.fold_in_items_implicit
        got = dict(exact=exact(ptr, ids, c["r"], status=True),                     # lam: the handle's
                   weighted=exact(ptr, ids, c["r"], LAM, weights=c["w"], status=True),
                   implicit=implicit(ptr, ids, c["c"], sc.LAM_IMPLICIT, status=True))
        for name, (rows, st) in got.items():
            assert not st.any(), f"{name}: status {st[st != 0]} of rows {np.flatnonzero(st)}"
            assert _same(rows, ref[name][0]), f"{name} k={k}: rows {np.flatnonzero((_bits(rows) != _bits(ref[name][0])).any(1))}"
        assert _same(exact(ptr, ids, c["r"]), ref["exact"][0])                     # status=False: the rows alone
        empty = np.diff(ptr) == 0
        assert empty.sum() >= 2 and not _bits(got["implicit"][0][empty]).any()
        # the result does not depend on the order of the rows
        rptr, rids, rr, rw, rc = sc.reversed_rows(ptr, ids, c["r"], c["w"], c["c"])
        assert _same(exact(rptr, rids, rr, weights=rw)[::-1], ref["weighted"][0])
        assert _same(implicit(rptr, rids, rc, sc.LAM_IMPLICIT)[::-1], ref["implicit"][0])


def _nan_rows(rows):
    return (_bits(rows) == 0x7FC00000).all(axis=1)


def test_refused_rows_are_reported_and_leave_the_others_alone(mf):
    rng = np.random.default_rng(21)
    k, I = 16, 300
    Q = sc.fixed_side(I, k, rng)
    lens = np.array([40, 5, 60, 0, 5, 33])
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = rng.integers(0, I, int(ptr[-1])).astype(np.int32)
    r = rng.uniform(0.5, 5.0, ids.size).astype(np.float32)
    want, want_st = sc.exact(Q, ptr, ids, r, 0.0)
    assert want_st[[0, 2, 3, 5]].tolist() == [0] * 4 and (want_st[[1, 4]] > 5).all()   # rank 5: five pivots at least
    keep = np.repeat(np.array([True, False, True, True, False, True]), lens)
    ptr_ok = np.concatenate([[0], np.cumsum(lens[[0, 2, 3, 5]])]).astype(np.int64)
    with mf.MatrixFactorizationSGD(4, I, k, LR, LAM, 1) as m:
        m.set_factors(np.zeros((4, k), np.float32), Q)
        got, st = m.fold_in_exact(ptr, ids, r, lam=0.0, status=True)        # alpha = ridge = ridge_per_entry = 0
        assert np.array_equal(st, want_st) and _same(got, want)
        assert _nan_rows(got).tolist() == [False, True, False, False, True, False]
        alone = m.fold_in_exact(ptr_ok, ids[keep], r[keep], lam=0.0)
        assert _same(got[[0, 2, 3, 5]], alone)
        assert _nan_rows(m.fold_in_exact(ptr, ids, r, lam=0.0))[[1, 4]].all()      # without a status array too
        # a NaN row of Q reaches the rows that name it, and those alone
        clean = m.fold_in_exact(ptr, ids, r, status=True)
        Qn = Q.copy()
        Qn[ids[ptr[2] + 7]] = np.nan
        names = np.array([(ids[ptr[x]:ptr[x + 1]] == ids[ptr[2] + 7]).any() for x in range(lens.size)])
        assert names[2] and not names.all()
        m.set_factors(np.zeros((4, k), np.float32), Qn)
        got, st = m.fold_in_exact(ptr, ids, r, status=True)
        want, want_st = sc.exact(Qn, ptr, ids, r, LAM)
        assert np.array_equal(st, want_st) and (st[names] == 1).all() and _nan_rows(got)[names].all()
        assert _same(got[~names], clean[0][~names]) and not st[~names].any()


def test_several_batches_and_a_dominant_row(mf):
    rng = np.random.default_rng(9)
    k, I, n_small = 8, 5000, 300_000
    lens = rng.integers(10, 51, n_small + 1)
    big = n_small // 3
    lens[big] = 200_000
    ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    assert ptr[-1] > 2 * (1 << 22)
    ids = rng.integers(0, I, int(ptr[-1])).astype(np.int32)
    r = rng.uniform(0.5, 5.0, ids.size).astype(np.float32)
    Q = sc.fixed_side(I, k, rng)
    with mf.MatrixFactorizationSGD(4, I, k, LR, LAM, 3) as m:
        m.set_factors(np.zeros((4, k), np.float32), Q)
        got, st = m.fold_in_exact(ptr, ids, r, status=True)
    want, want_st = sc.exact(Q, ptr, ids, r, LAM)
    assert not want_st.any() and np.isfinite(want).all()
    assert not st.any()
    assert _same(got[big], want[big])
    assert _same(got, want)


def test_the_calls_leave_the_handle_alone(mf):
    rng = np.random.default_rng(2)
    U, I, k = 50, 300, 16
    c = sc.case(k)
    P, Q = sc.fixed_side(U, k, rng), c["F"]
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 7) as m:
        m.set_factors(P, Q)
        m.set_seen(rng.integers(0, U, 200), rng.integers(0, I, 200))
        m.set_item_weights(rng.integers(1, 9, I).astype(np.uint32))
        m.set_validation(rng.integers(0, U, 30), rng.integers(0, I, 30), rng.uniform(1, 5, 30).astype(np.float32))
        m.gram("items")  # (the factors are on the device from here on)

        def state():
            P1, Q1 = m.get_factors()
            return (P1.tobytes(), Q1.tobytes(), m.seen_size(), m.item_weights().tobytes(), m.validation_size(),
                    mf.debug_device_bytes())

        before = state()
        m.fold_in_exact(c["row_ptr"], c["ids"], c["r"], weights=c["w"])
        m.fold_in_implicit(c["row_ptr"], c["ids"], c["c"], 0.1)
        users = rng.integers(0, U, c["ids"].size).astype(np.int32)
        m.fold_in_items_exact(c["row_ptr"], users, c["r"])
        m.fold_in_items_implicit(c["row_ptr"], users, c["c"], 0.1)
        m.gram("users")
        assert state() == before
        rows, st = m.fold_in_exact([0, 5, 45], c["ids"][:45], c["r"][:45], lam=0.0, status=True)   # row 0 is refused
        assert st[0] > 0 and st[1] == 0
        assert state() == before


def test_fit_als_and_fit_ials_are_the_loop_over_the_restatement(mf):
    u, i, r, c, P0, Q0 = sc.als_case()
    U, I, k, lam = sc.ALS_U, sc.ALS_I, sc.ALS_K, sc.ALS_LAM
    with mf.MatrixFactorizationSGD(U, I, k, LR, lam, 5) as m:
        m.set_factors(P0, Q0)
        obj = m.fit_als(u, i, r, 3)                                     # lam: the handle's
        P, Q = m.get_factors()
        wP, wQ, wobj = sc.als_loop(P0, Q0, u, i, r, 3, lambda F, ptr, ids, v: sc.exact(F, ptr, ids, v, lam),
                                   lambda A, B: sc.als_objective(A, B, u, i, r, lam))
        assert _same(P, wP) and _same(Q, wQ)
        assert np.array_equal(obj, wobj) and (np.diff(obj) < 0).all()
        # rows folded in from the users' own ratings are P's (Q is what the last half-sweep left: not the same system as
        # the one P came from, so not P itself), and serving them agrees with predict
        order = np.argsort(u, kind="stable")
        ptr = np.concatenate([[0], np.cumsum(np.bincount(u, minlength=U))]).astype(np.int64)
        rows = m.fold_in_exact(ptr, i[order], r[order])
        assert _same(rows, sc.exact(Q, ptr, i[order], r[order], lam)[0])
        m.set_factors(rows, Q)
        items, scores = m.recommend_rows(rows, 5)
        assert (items >= 0).all()
        pred = m.predict(np.repeat(np.arange(U, dtype=np.int32), 5), items.ravel())
        assert _same(scores.ravel(), pred)

        m.set_factors(P0, Q0)
        obj = m.fit_ials(u, i, 3, confidence=c, lam=sc.LAM_IMPLICIT)
        P, Q = m.get_factors()
        wP, wQ, wobj = sc.als_loop(P0, Q0, u, i, c, 3, lambda F, ptr, ids, v: sc.implicit(F, ptr, ids, v, sc.LAM_IMPLICIT),
                                   lambda A, B: sc.ials_objective(A, B, u, i, c, sc.LAM_IMPLICIT, 1.0))
        assert _same(P, wP) and _same(Q, wQ)
        assert np.array_equal(obj, wobj) and (np.diff(obj) < 0).all()
        # a system that is not positive definite stops the fit
        with pytest.raises(mf.MfsgdError):
            m.fit_als(u, i, r, 1, lam=0.0)
