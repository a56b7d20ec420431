"""Pairwise fold-in, as far as it goes without a GPU: mfsgd_fold_in_users_pairwise exists, checks its arguments before any
device work in the order include/mfsgd.h states and never answers on the CPU; the Python wrapper shapes its results; and
the restatement the GPU tests compare with (tests/fold_in_pairwise_common.py) is the P line of the pairwise step."""
import ctypes as C

import numpy as np
import pytest

from tests import fold_in_pairwise_common as FC
from tests import hardneg_common as HC
from tests import implicit_common as IC
from tests import pairwise_common as PC
from tests.conftest import have_gpu

OK, INVALID_ARG, NO_DEVICE, STATE = 0, -1, -2, -5
U, I, K = 6, 5, 8
I64_MAX = (1 << 63) - 1
I32_MAX = (1 << 31) - 1
UNTOUCHED = -77
PRE = "fold_in_pairwise: "


def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def _fold(m, row_ptr=(0, 2, 3), items=(1, 4, 0), n_new=None, epochs=2, cand=3, first=0, rows=True, extra=True):
    """(rc, message, untouched) of one raw call; untouched: every output array is still as it was."""
    rp = None if row_ptr is None else np.ascontiguousarray(row_ptr, np.int64)
    ii = None if items is None else np.ascontiguousarray(items, np.int32)
    if n_new is None:
        n_new = rp.size - 1
    out = np.full((8, K), UNTOUCHED, np.float32)
    mg, ng = np.full(64, UNTOUCHED, np.float32), np.full(64, UNTOUCHED, np.int32)
    rc = m._lib.mfsgd_fold_in_users_pairwise(m._handle(), n_new, _ptr(rp, C.c_int64), _ptr(ii, C.c_int32), epochs, cand, None, 0,
                                             0, first, _ptr(out, C.c_float) if rows else None,
                                             _ptr(mg, C.c_float) if extra else None, _ptr(ng, C.c_int32) if extra else None)
    untouched = bool((out == UNTOUCHED).all() and (mg == UNTOUCHED).all() and (ng == UNTOUCHED).all())
    return rc, m._lib.mfsgd_last_error(m._h).decode(), untouched


@pytest.fixture
def bare(mf):
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        yield m


@pytest.fixture
def ready(bare):
    """Seeded factors: a valid state that needs no GPU to reach.  No index, no ratings: the call wants neither."""
    bare.init_factors()
    return bare


def test_the_symbol_is_there(mf):
    assert hasattr(mf.load_library(), "mfsgd_fold_in_users_pairwise")
    assert callable(getattr(mf.MatrixFactorizationSGD, "fold_in_pairwise"))


def test_one_broken_argument_at_a_time(ready):
    m = ready
    for args, msg in ((dict(n_new=-1), "n_new is negative"),
                      (dict(epochs=-1), "epochs is negative"),
                      (dict(cand=0), "m is below 1"),
                      (dict(cand=-2), "m is below 1"),
                      (dict(first=-1), "first is negative"),
                      (dict(first=I64_MAX - 17), "first + T * epochs * m exceeds 2^63 - 1"),  # T * epochs * m = 18
                      (dict(epochs=I32_MAX, cand=I32_MAX), "first + T * epochs * m exceeds 2^63 - 1"),
                      (dict(row_ptr=None, n_new=2), "row_ptr or out_rows is null"),
                      (dict(rows=False), "row_ptr or out_rows is null"),
                      (dict(row_ptr=(1, 2, 3)), "row_ptr[0] is not 0"),
                      (dict(row_ptr=(0, 4, 3)), "row_ptr decreases at user 1"),
                      (dict(items=None), "items is null"),
                      (dict(items=(1, 4, I)), "item of positive 2 out of range"),
                      (dict(items=(1, -1, 0)), "item of positive 1 out of range")):
        rc, got, untouched = _fold(m, **args)
        assert (rc, got) == (INVALID_ARG, PRE + msg), args
        assert untouched
    # the largest counter range there is passes the checks, and so do null out_margin and out_neg, a user without
    # positives, epochs == 0 and a list that names every item
    want = OK if have_gpu() else NO_DEVICE
    assert _fold(m, first=I64_MAX - 18)[0] == want
    assert _fold(m, extra=False)[0] == want
    assert _fold(m, row_ptr=(0, 0, 3))[0] == want
    assert _fold(m, epochs=0)[0] == want
    assert _fold(m, row_ptr=(0, I), items=np.arange(I))[0] == want
    assert _fold(m, row_ptr=(0, 0), items=None)[0] == want  # (no positives at all: items is not needed)


def test_the_checks_come_in_the_stated_order(mf, bare):
    m = bare  # (factors never initialised: whatever is refused here is refused before the state is looked at)
    # 1 - 3. n_new and epochs, then m, then first and the counter range
    assert _fold(m, n_new=-1, epochs=-1, cand=0, first=-1)[1] == PRE + "n_new is negative"
    assert _fold(m, epochs=-1, cand=0, first=-1)[1] == PRE + "epochs is negative"
    assert _fold(m, cand=0, first=-1, row_ptr=None, n_new=2)[1] == PRE + "m is below 1"
    assert _fold(m, first=-1, row_ptr=None, n_new=2)[1] == PRE + "first is negative"
    assert _fold(m, first=I64_MAX, rows=False)[1] == PRE + "first + T * epochs * m exceeds 2^63 - 1"
    # 4. the arrays and row_ptr, before the items are looked at
    assert _fold(m, row_ptr=None, n_new=2, items=(I, I, I))[:2] == (INVALID_ARG, PRE + "row_ptr or out_rows is null")
    assert _fold(m, row_ptr=(1, 2, 3), items=(I, I, I))[1] == PRE + "row_ptr[0] is not 0"
    assert _fold(m, row_ptr=(0, 4, 3), items=(I, I, I))[1] == PRE + "row_ptr decreases at user 1"
    assert _fold(m, row_ptr=(0, 2, 1, 3), items=(I, I, I))[1] == PRE + "row_ptr decreases at user 1"
    # 5. the items, named by position, before the state
    rc, msg, untouched = _fold(m, items=(0, I, I))
    assert (rc, msg) == (INVALID_ARG, PRE + "item of positive 1 out of range") and untouched
    # 6. the state, whatever n_new is: fold_in's
    for kw in (dict(), dict(row_ptr=(0,), items=None)):
        assert _fold(m, **kw)[:2] == (STATE, PRE + "factors not initialised")
    m.init_p_offset(1, 0)  # P alone
    for kw in (dict(), dict(row_ptr=(0,), items=None)):
        rc, msg, untouched = _fold(m, **kw)
        assert rc == STATE and msg.startswith(PRE + "Q is not initialised") and untouched
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as p:
        for kw in (dict(), dict(row_ptr=(0,), items=None)):
            assert _fold(p, **kw)[:2] == (STATE, PRE + "single-partition handles only")
        assert _fold(p, cand=0)[:2] == (INVALID_ARG, PRE + "m is below 1")
    # 7. n_new == 0 is fine and reads nothing
    m.init_factors()
    rc, msg, untouched = _fold(m, row_ptr=(0,), items=None)
    assert rc == OK and untouched
    assert _fold(m, row_ptr=None, items=None, n_new=0, rows=False, extra=False)[0] == OK
    out = np.zeros(K, np.float32)
    rp = np.zeros(2, np.int64)
    assert mf.load_library().mfsgd_fold_in_users_pairwise(None, 1, _ptr(rp, C.c_int64), None, 1, 1, None, 0, 0, 0,
                                                          _ptr(out, C.c_float), None, None) == INVALID_ARG


@pytest.mark.skipif(have_gpu(), reason="checks the no-device error path")
def test_a_valid_call_needs_the_device(ready):
    rc, msg, untouched = _fold(ready)
    assert rc == NO_DEVICE and "no CPU fallback" in msg and untouched
    with pytest.raises(Exception) as e:
        ready.fold_in_pairwise([0, 2, 3], [1, 4, 0], 2, candidates=3)
    assert e.value.code == NO_DEVICE


def test_the_wrapper_shapes_its_results(ready):
    m = ready
    rows = m.fold_in_pairwise([0], [], 3)
    assert rows.shape == (0, K) and rows.dtype == np.float32
    rows, mg, ng = m.fold_in_pairwise([0], [], 3, candidates=4, margins=True, negatives=True)
    assert (rows.shape, mg.shape, ng.shape, mg.dtype, ng.dtype) == ((0, K), (0,), (0,), np.float32, np.int32)
    assert len(m.fold_in_pairwise([0], [], 3, negatives=True)) == 2
    for bad in (dict(row_ptr=[[0, 1]], items=[1]), dict(row_ptr=[], items=[]), dict(row_ptr=[0, 2], items=[1]),
                dict(row_ptr=[0, 1], items=[[1]]), dict(row_ptr=[0, 1], items=[1], init=np.zeros((2, K), np.float32)),
                dict(row_ptr=[0, 1], items=[1], init=np.zeros((1, K + 1), np.float32))):
        with pytest.raises(ValueError):
            m.fold_in_pairwise(bad.pop("row_ptr"), bad.pop("items"), 1, **bad)
    with pytest.raises(Exception) as e:  # the library's refusals come through
        m.fold_in_pairwise([0, 1], [1], 1, candidates=0)
    assert e.value.code == INVALID_ARG
    assert m.seen_size() == -1  # no index was made


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_the_restatement_is_the_p_line_of_the_pairwise_step():
    """One user, given negatives: the P row of pairwise_common.c_pass on a copy of Q that is restored after every step is
    the restatement's row, margins included."""
    rng = np.random.default_rng(4)
    lr, lam = 0.05, 0.01
    for k in (1, 3, 8, 13):
        Q = rng.standard_normal((9, k)).astype(np.float32)
        row = rng.standard_normal(k).astype(np.float32)
        pos = np.array([0, 3, 3, 8, 1, 0, 5], np.int32)
        neg = np.array([2, 4, 7, 6, 2, 4, 6], np.int32)
        got_row, got_x = FC.chain(row, Q, pos, neg, lr, lam)
        P, xs = row[None].copy(), []
        for i, j in zip(pos, neg):
            P, _, x = PC.c_pass(P, Q, [0], [i], [j], lr, lam)  # (c_pass works on copies: Q is the same for every step)
            xs.append(x[0])
        assert FC.same_bits(got_row, P[0]) and FC.same_bits(got_x, np.array(xs, np.float32))
        assert not FC.same_bits(got_row, row)


def test_fold_on_a_hand_made_problem():
    """fold() against the rule spelt out step by step in Python: the counters, the draws, the pick, what is written where."""
    rng = np.random.default_rng(6)
    n_items, k, epochs, lr, lam, seed, first = 7, 5, 2, 0.1, 0.02, 99, 1000
    Q = rng.standard_normal((n_items, k)).astype(np.float32)
    lists = [[3, 1, 3], [], list(range(n_items)), [0, 1, 2, 4, 5, 6], [6]]
    row_ptr, items = FC.csr(lists)
    init = rng.standard_normal((len(lists), k)).astype(np.float32)
    for m in (1, 3):
        rows, mg, ng = FC.fold(Q, row_ptr, items, epochs, m, init, lr, lam, seed, first)
        assert mg.shape == ng.shape == (row_ptr[-1] * epochs,)
        for x, A in enumerate(lists):
            o, S, row = int(row_ptr[x]) * epochs, np.unique(A), init[x].copy()
            if len(S) == n_items:  # no step: the start row, NaN bits and -1
                assert FC.same_bits(rows[x], init[x]) and (ng[o:o + len(A) * epochs] == -1).all()
                assert (mg.view(np.uint32)[o:o + len(A) * epochs] == FC.NAN_BITS).all()
                continue
            for tau in range(len(A) * epochs):
                c = first + (o + tau) * m + np.arange(m)
                cand = IC.draw(S, n_items, seed, c)
                assert not np.isin(cand, S).any()
                sc = np.empty(m, np.float32)
                cand = np.ascontiguousarray(cand)
                FC.restatement().fp_scores(row.ctypes.data_as(FC._f), Q.ctypes.data_as(FC._f), k, cand.ctypes.data_as(FC._i), m,
                                           sc.ctypes.data_as(FC._f))
                j = cand[HC.pick(sc[None])[0]]
                row, xm = FC.chain(row, Q, [A[tau % len(A)]], [j], lr, lam)
                assert ng[o + tau] == j and FC.same_bits(mg[o + tau:o + tau + 1], xm)
                if len(S) == n_items - 1:  # one unseen item: every draw is that item
                    assert j == 3
            assert FC.same_bits(rows[x], row)
    # users [a, b) of a call are the call on row_ptr rebased to a with first + row_ptr[a] * epochs * m
    whole = FC.fold(Q, row_ptr, items, epochs, 3, init, lr, lam, seed, first)
    a, b = 3, 5
    part = FC.fold(Q, row_ptr[a:b + 1] - row_ptr[a], items[row_ptr[a]:row_ptr[b]], epochs, 3, init[a:b], lr, lam, seed,
                   first + int(row_ptr[a]) * epochs * 3)
    assert FC.same_bits(whole[0][a:b], part[0])
    for w, p in zip(whole[1:], part[1:]):
        assert FC.same_bits(w[row_ptr[a] * epochs:row_ptr[b] * epochs], p)
