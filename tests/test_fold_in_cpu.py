"""mfsgd_fold_in_users and mfsgd_recommend_rows check their arguments before any device work, so that these checks
run without a GPU; a valid call without a device fails with MFSGD_ERR_NO_DEVICE, never with a CPU result."""
import ctypes as C

import numpy as np
import pytest

from tests.conftest import have_gpu

OK, INVALID_ARG, NO_DEVICE, STATE = 0, -1, -2, -5
U, I, K = 6, 5, 8


def _ptr(a, dtype, ctype):
    """None stands for a NULL pointer."""
    return None if a is None else np.ascontiguousarray(a, dtype).ctypes.data_as(C.POINTER(ctype))


def _fold(m, n_new, row_ptr, items, ratings, epochs=1, init=None, out=True):
    rows = np.zeros((max(1, n_new), K), np.float32) if out else None
    return m._lib.mfsgd_fold_in_users(m._handle(), n_new, _ptr(row_ptr, np.int64, C.c_int64),
                                      _ptr(items, np.int32, C.c_int32), _ptr(ratings, np.float32, C.c_float), epochs,
                                      _ptr(init, np.float32, C.c_float), 3, _ptr(rows, np.float32, C.c_float))


def _rec_rows(m, rows, n_rows, topn, er, ei, n_excl):
    items = np.empty(max(1, n_rows * max(topn, 1)), np.int32)
    scores = np.empty(max(1, n_rows * max(topn, 1)), np.float32)
    return m._lib.mfsgd_recommend_rows(m._handle(), _ptr(rows, np.float32, C.c_float), n_rows, topn,
                                       _ptr(er, np.int32, C.c_int32), _ptr(ei, np.int32, C.c_int32), n_excl,
                                       _ptr(items, np.int32, C.c_int32), _ptr(scores, np.float32, C.c_float))


def _err(m):
    return m._lib.mfsgd_last_error(m._h).decode()


@pytest.fixture
def model(mf):
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        m.init_factors()
        yield m


@pytest.mark.parametrize("kw,names", [
    (dict(n_new=-1, row_ptr=[0], items=[], ratings=[]), "n_new"),
    (dict(n_new=2, row_ptr=[0, 1, 2], items=[0, 1], ratings=[1, 2], epochs=-1), "epochs"),
    (dict(n_new=2, row_ptr=None, items=[0, 1], ratings=[1, 2]), "row_ptr"),
    (dict(n_new=2, row_ptr=[0, 1, 2], items=[0, 1], ratings=[1, 2], out=False), "out_rows"),
    (dict(n_new=2, row_ptr=[1, 1, 2], items=[0, 1], ratings=[1, 2]), "row_ptr[0]"),
    (dict(n_new=3, row_ptr=[0, 2, 1, 3], items=[0, 1, 2], ratings=[1, 2, 3]), "user 1"),
    (dict(n_new=2, row_ptr=[0, 1, 2], items=None, ratings=[1, 2]), "items"),
    (dict(n_new=2, row_ptr=[0, 1, 2], items=[0, 1], ratings=None), "ratings"),
    (dict(n_new=2, row_ptr=[0, 1, 3], items=[0, 1, -1], ratings=[1, 2, 3]), "rating 2"),
    (dict(n_new=2, row_ptr=[0, 1, 3], items=[0, I, 1], ratings=[1, 2, 3]), "rating 1"),
])
def test_bad_fold_in_arguments_are_invalid(model, kw, names):
    assert _fold(model, **kw) == INVALID_ARG
    msg = _err(model)
    assert msg.startswith("fold_in:") and names in msg


def _fold_raw(m, fn, n_new, row_ptr, ids, ratings, epochs=1, out=True):
    """(status, message) of one raw call of mfsgd_fold_in_users or mfsgd_fold_in_items."""
    rows = np.zeros((max(1, n_new), K), np.float32) if out else None
    rc = getattr(m._lib, fn)(m._handle(), n_new, _ptr(row_ptr, np.int64, C.c_int64), _ptr(ids, np.int32, C.c_int32),
                             _ptr(ratings, np.float32, C.c_float), epochs, None, 3, _ptr(rows, np.float32, C.c_float))
    return rc, _err(m)


# (the C function, how it names itself, a new row, an id and the ids, and how many rows the fixed side has)
@pytest.mark.parametrize("fn,call,row,id_,ids,n_fixed", [
    ("mfsgd_fold_in_users", "fold_in", "user", "item", "items", I),
    ("mfsgd_fold_in_items", "fold_in_items", "item", "user", "users", U),
])
def test_the_fold_in_checks_come_in_their_order(mf, fn, call, row, id_, ids, n_fixed):
    """Two faults in one call, one case for each neighbouring pair of the order: n_new, epochs, the null row_ptr / out_rows,
    the state of the factors (before row_ptr is read, and before n_new == 0 is answered), row_ptr[0], a decreasing
    row_ptr, the null ids / ratings, an id out of range.  The earlier fault is the one reported."""
    pre = call + ": "
    two, bad = dict(ids=[0, 1], ratings=[1, 2]), [0, n_fixed, 1]

    def go(m, n_new, row_ptr, ids, ratings, **kw):
        return _fold_raw(m, fn, n_new, row_ptr, ids, ratings, **kw)

    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:  # factors never set: what passes here is asked before the state
        assert go(m, -1, [0], [], [], epochs=-1) == (INVALID_ARG, pre + "n_new is negative")
        assert go(m, 2, None, epochs=-1, **two) == (INVALID_ARG, pre + "epochs is negative")
        assert go(m, 2, [0, 1, 2], epochs=-1, out=False, **two) == (INVALID_ARG, pre + "epochs is negative")
        assert go(m, 2, None, **two) == (INVALID_ARG, pre + "row_ptr or out_rows is null")
        assert go(m, 2, [0, 1, 2], out=False, **two) == (INVALID_ARG, pre + "row_ptr or out_rows is null")
        # the state before anything of row_ptr is read, and whatever n_new is
        assert go(m, 2, [1, 1, 2], **two) == (STATE, pre + "factors not initialised")
        assert go(m, 0, [0], None, None) == (STATE, pre + "factors not initialised")
        m.init_p_offset(1, 0)  # P alone
        for args in ((2, [1, 1, 2], [0, 1], [1, 2]), (0, [0], None, None)):
            rc, msg = go(m, *args)
            assert rc == STATE and msg.startswith(pre + "Q is not initialised")
        assert go(m, 2, None, **two) == (INVALID_ARG, pre + "row_ptr or out_rows is null")
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as m:
        assert go(m, 2, [1, 1, 2], **two) == (STATE, pre + "single-partition handles only")
        assert go(m, 0, [0], None, None) == (STATE, pre + "single-partition handles only")
        assert go(m, 2, [0, 1, 2], out=False, **two) == (INVALID_ARG, pre + "row_ptr or out_rows is null")
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        m.init_factors()
        assert go(m, 2, [1, 3, 2], bad, None) == (INVALID_ARG, pre + "row_ptr[0] is not 0")
        assert go(m, 3, [0, 2, 1, 3], None, [1, 2, 3]) == (INVALID_ARG, pre + f"row_ptr decreases at {row} 1")
        assert go(m, 3, [0, 2, 1, 3], bad, None) == (INVALID_ARG, pre + f"row_ptr decreases at {row} 1")
        assert go(m, 3, [0, 2, 1, 3], bad, [1, 2, 3]) == (INVALID_ARG, pre + f"row_ptr decreases at {row} 1")
        assert go(m, 2, [0, 1, 3], bad, None) == (INVALID_ARG, pre + f"{ids} or ratings is null")
        assert go(m, 2, [0, 1, 3], None, [1, 2, 3]) == (INVALID_ARG, pre + f"{ids} or ratings is null")
        assert go(m, 2, [0, 1, 3], bad, [1, 2, 3]) == (INVALID_ARG, pre + f"{id_} of rating 1 out of range")
        assert go(m, 2, [0, 1, 3], [0, 1, -1], [1, 2, 3]) == (INVALID_ARG, pre + f"{id_} of rating 2 out of range")
        assert go(m, 0, [1], bad, None)[0] == OK  # nobody to fold in: row_ptr is not read


def test_fold_in_null_handle(model):
    rp = np.zeros(1, np.int64)
    assert model._lib.mfsgd_fold_in_users(None, 0, _ptr(rp, np.int64, C.c_int64), None, None, 1, None, 0,
                                          None) == INVALID_ARG
    assert model._lib.mfsgd_recommend_rows(None, None, 0, 1, None, None, 0, None, None) == INVALID_ARG


def test_fold_in_of_nobody_is_ok(model):
    assert _fold(model, 0, [0], None, None) == OK
    assert _fold(model, 0, None, None, None, out=False) == OK
    assert model.fold_in([0], [], [], 2).shape == (0, K)


ROWS = np.ones((3, K), np.float32)


@pytest.mark.parametrize("rows,n_rows,topn,er,ei,n_excl", [
    (None, 3, 2, None, None, 0),            # NULL rows
    (ROWS, -1, 2, None, None, 0),           # negative count
    (ROWS, 3, 0, None, None, 0),            # topn below 1
    (ROWS, 3, I + 1, None, None, 0),        # topn above the number of items
    (ROWS, 3, 2, [0], [1], -1),             # negative pair count
    (ROWS, 3, 2, None, [1], 1),             # NULL row array
    (ROWS, 3, 2, [0], None, 1),             # NULL item array
    (ROWS, 3, 2, [0, -1], [1, 1], 2),       # row below range
    (ROWS, 3, 2, [0, 3], [1, 1], 2),        # row above range (3 rows, although the model has 6 users)
    (ROWS, 3, 2, [0, 1], [1, -1], 2),       # item below range
    (ROWS, 3, 2, [0, 1], [1, I], 2),        # item above range
])
def test_bad_recommend_rows_arguments_are_invalid(model, rows, n_rows, topn, er, ei, n_excl):
    assert _rec_rows(model, rows, n_rows, topn, er, ei, n_excl) == INVALID_ARG
    assert _err(model).startswith("recommend")


def test_recommend_rows_of_nothing_is_ok(model):
    assert _rec_rows(model, None, 0, 2, None, None, 0) == OK
    items, scores = model.recommend_rows(np.empty((0, K), np.float32), 2)
    assert items.shape == (0, 2) and scores.shape == (0, 2)


def test_uninitialised_factors_are_a_state_error(mf):
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        assert _fold(m, 2, [0, 1, 2], [0, 1], [1, 2]) == STATE
        assert _err(m).startswith("fold_in:")
        assert _rec_rows(m, ROWS, 3, 2, None, None, 0) == STATE
        assert _err(m).startswith("recommend")


def test_python_shapes_are_checked(model):
    with pytest.raises(ValueError):
        model.fold_in([0, 1, 2], [0, 1, 2], [1.0, 2.0], 1)        # items and ratings differ
    with pytest.raises(ValueError):
        model.fold_in([0, 1, 3], [0, 1], [1.0, 2.0], 1)           # row_ptr ends elsewhere
    with pytest.raises(ValueError):
        model.fold_in([[0, 1, 2]], [0, 1], [1.0, 2.0], 1)         # row_ptr not 1-d
    with pytest.raises(ValueError):
        model.fold_in([0, 1, 2], [0, 1], [1.0, 2.0], 1, init=np.zeros((3, K), np.float32))
    with pytest.raises(ValueError):
        model.fold_in([0, 1, 2], [0, 1], [1.0, 2.0], 1, init=np.zeros((2, K + 1), np.float32))
    with pytest.raises(ValueError):
        model.recommend_rows(np.zeros((2, K + 1), np.float32), 2)
    with pytest.raises(ValueError):
        model.recommend_rows(np.zeros(K, np.float32), 2)
    with pytest.raises(ValueError):
        model.recommend_rows(ROWS, 2, exclude=([0, 1], [1]))


@pytest.mark.skipif(have_gpu(), reason="checks the no-device error path")
def test_valid_calls_without_device_fail_loudly(model, mf):
    assert _fold(model, 3, [0, 2, 2, 3], [0, 4, 0], [1, 2, 3], epochs=2) == NO_DEVICE
    assert _fold(model, 2, [0, 0, 0], None, None, epochs=0, init=np.ones((2, K), np.float32)) == NO_DEVICE
    assert _rec_rows(model, ROWS, 3, 2, [0, 2], [1, 4], 2) == NO_DEVICE
    with pytest.raises(mf.MfsgdError) as e:
        model.fold_in([0, 2, 3], [0, 4, 0], [1.0, 2.0, 3.0], 2)
    assert e.value.code == NO_DEVICE
    with pytest.raises(mf.MfsgdError) as e:
        model.recommend_rows(ROWS, 2, exclude=([0, 2], [1, 4]))
    assert e.value.code == NO_DEVICE
