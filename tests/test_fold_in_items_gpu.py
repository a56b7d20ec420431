"""fold_in_items(...) -- mfsgd_fold_in_items -- against the CPU oracle: the mirror of tests/test_fold_in_gpu.py with P as
the fixed side.  Fold-in of an item with P fixed equals one ordinary oracle pass over a model in which every rating
has a private copy of its user row: the pass reads that copy once, writes an update nobody reads, and Q -- the new
rows -- sees exactly the fold-in step, as the q of the oracle's update.  Rows are compared bit for bit."""
import ctypes as C

import numpy as np
import pytest

from tests.test_fold_in_gpu import _mixed_users, fold_in_ref

pytestmark = pytest.mark.gpu

LR, LAM = 0.01, 0.05
INVALID, STATE = -1, -5


def fold_in_items_ref(oracle, P, row_ptr, users, ratings, epochs, R0, lr, lam):
    R = R0.copy()
    n = users.size
    io = np.repeat(np.arange(row_ptr.size - 1, dtype=np.int32), np.diff(row_ptr)).astype(np.int32)
    for _ in range(epochs):
        Pp = np.ascontiguousarray(P[users])  # fresh private rows each epoch
        oracle.sgd_pass(Pp, R, np.arange(n, dtype=np.int32), io, ratings, lr, lam)
    return R


@pytest.mark.parametrize("k", [1, 3, 8, 12, 16, 33, 64, 100, 128, 200, 256])
def test_fold_in_items_matches_oracle_for_every_group_width(mf, oracle, k):
    rng = np.random.default_rng(200 + k)
    U, I = 300, 20
    P = (rng.standard_normal((U, k)) * (0.5 / np.sqrt(k))).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    row_ptr, users, ratings = _mixed_users(U, rng)   # lengths 0 .. 400, empty lists, one user twice (adjacent and not)
    n_new = row_ptr.size - 1
    init = rng.standard_normal((n_new, k)).astype(np.float32)
    seeded, _ = oracle.init_factors(n_new, 0, k, 11)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 11) as m:
        m.set_factors(P, Q)
        for epochs in (0, 1, 3):
            got = m.fold_in_items(row_ptr, users, ratings, epochs, init=init)
            want = fold_in_items_ref(oracle, P, row_ptr, users, ratings, epochs, init, LR, LAM)
            assert np.isfinite(want).all()
            assert np.array_equal(got, want), f"k={k} epochs={epochs} init given"
            got = m.fold_in_items(row_ptr, users, ratings, epochs)           # seeded with the model's seed
            want = fold_in_items_ref(oracle, P, row_ptr, users, ratings, epochs, seeded, LR, LAM)
            assert np.array_equal(got, want), f"k={k} epochs={epochs} seeded"
        other, _ = oracle.init_factors(n_new, 0, k, 12345)
        assert np.array_equal(m.fold_in_items(row_ptr, users, ratings, 0, seed=12345), other)
        empty = np.flatnonzero(np.diff(row_ptr) == 0)
        assert empty.size >= 3
        assert np.array_equal(m.fold_in_items(row_ptr, users, ratings, 3, init=init)[empty], init[empty])
        zero = np.zeros(n_new + 1, np.int64)
        assert np.array_equal(m.fold_in_items(zero, [], [], 2, init=init), init)


def test_the_user_fold_in_has_not_moved(mf, oracle):
    rng = np.random.default_rng(7)
    k, U, I = 33, 40, 300
    P = (rng.standard_normal((U, k)) * 0.1).astype(np.float32)
    Q = (rng.standard_normal((I, k)) * 0.1).astype(np.float32)
    row_ptr, items, ratings = _mixed_users(I, rng)
    ip_ptr, users, uratings = _mixed_users(U, rng)
    init = rng.standard_normal((row_ptr.size - 1, k)).astype(np.float32)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 3) as m:
        m.set_factors(P, Q)
        got_i = m.fold_in_items(ip_ptr, users, uratings, 2, init=init)
        got_u = m.fold_in(row_ptr, items, ratings, 2, init=init)
    assert np.array_equal(got_u, fold_in_ref(oracle, Q, row_ptr, items, ratings, 2, init, LR, LAM))
    assert np.array_equal(got_i, fold_in_items_ref(oracle, P, ip_ptr, users, uratings, 2, init, LR, LAM))


def test_fold_in_items_is_independent_of_item_order_and_leaves_the_model_alone(mf):
    rng = np.random.default_rng(5)
    k, U, I = 33, 300, 6
    P = (rng.standard_normal((U, k)) * 0.1).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    row_ptr, users, ratings = _mixed_users(U, rng)
    n_new = row_ptr.size - 1
    init = rng.standard_normal((n_new, k)).astype(np.float32)
    lens = np.diff(row_ptr)
    rev_ptr = np.concatenate([[0], np.cumsum(lens[::-1])]).astype(np.int64)
    pieces = [slice(row_ptr[x], row_ptr[x + 1]) for x in range(n_new)][::-1]
    rev_users = np.concatenate([users[s] for s in pieces])
    rev_ratings = np.concatenate([ratings[s] for s in pieces])
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        m.predict([0], [0])                        # the factors are on the device from here on
        a = m.fold_in_items(row_ptr, users, ratings, 2, init=init)
        b = m.fold_in_items(rev_ptr, rev_users, rev_ratings, 2, init=init[::-1])
        P1, Q1 = m.get_factors()
        assert (m.users, m.items) == (U, I)
    assert np.array_equal(a, b[::-1])
    assert P1.tobytes() == P.tobytes() and Q1.tobytes() == Q.tobytes()


def test_errors(mf):
    k, U, I = 8, 6, 5
    rng = np.random.default_rng(1)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as m:
        m.set_factors(rng.standard_normal((U, k)).astype(np.float32), rng.standard_normal((I, k)).astype(np.float32))

        def fails(code, text, *a):
            with pytest.raises(mf.MfsgdError) as e:
                m.fold_in_items(*a)
            assert e.value.code == code and f": fold_in_items: {text}" in str(e.value), str(e.value)

        fails(INVALID, "user of rating 2 out of range", [0, 2, 3], [0, 5, U], [1.0, 2.0, 3.0], 1)   # (5 is an item count)
        fails(INVALID, "user of rating 1 out of range", [0, 2, 3], [0, -1, 2], [1.0, 2.0, 3.0], 1)
        fails(INVALID, "row_ptr decreases at item 1", [0, 2, 1], [0], [1.0], 1)
        fails(INVALID, "row_ptr[0] is not 0", [1, 2, 3], [0, 1, 2], [1.0, 2.0, 3.0], 1)
        fails(INVALID, "epochs is negative", [0, 1], [0], [1.0], -1)
        call, h = m._lib.mfsgd_fold_in_items, m._h
        rp = (C.c_int64 * 2)(0, 1)
        us, rs, out = (C.c_int32 * 1)(0), (C.c_float * 1)(1.0), (C.c_float * k)()
        err = lambda: m._lib.mfsgd_last_error(h).decode()
        assert call(h, -1, rp, us, rs, 1, None, 0, out) == INVALID and err().startswith("fold_in_items: n_new")
        assert call(h, 1, None, us, rs, 1, None, 0, out) == INVALID and err().startswith("fold_in_items: row_ptr or out_rows")
        assert call(h, 1, rp, us, rs, 1, None, 0, None) == INVALID and err().startswith("fold_in_items: row_ptr or out_rows")
        assert call(h, 1, rp, None, rs, 1, None, 0, out) == INVALID and err().startswith("fold_in_items: users or ratings")
        assert call(h, 1, rp, us, None, 1, None, 0, out) == INVALID and err().startswith("fold_in_items: users or ratings")
        assert m.fold_in_items([0], [], [], 1).shape == (0, k)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as m:      # factors never set
        with pytest.raises(mf.MfsgdError) as e:
            m.fold_in_items([0, 1], [0], [1.0], 1)
        assert e.value.code == STATE and "fold_in_items: " in str(e.value)
        m.init_p_offset(3, 0)                                      # P alone: no Q in the handle
        with pytest.raises(mf.MfsgdError) as e:
            m.fold_in_items([0, 1], [0], [1.0], 1)
        assert e.value.code == STATE and "fold_in_items: Q is not initialised" in str(e.value)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1, n_parts=2) as m:
        m.init_factors()
        with pytest.raises(mf.MfsgdError) as e:
            m.fold_in_items([0, 1], [0], [1.0], 1)
        assert e.value.code == STATE
