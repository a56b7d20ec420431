"""mfsgd_similar_items / _users / _rows and mfsgd_row_inv_norms check their arguments before any device work, so that
these checks run without a GPU; a valid call without a device fails with MFSGD_ERR_NO_DEVICE, never with a CPU result."""
import ctypes as C

import numpy as np
import pytest

from tests.conftest import have_gpu

INVALID_ARG, NO_DEVICE, STATE = -1, -2, -5
U, I, K = 6, 5, 8
USERS, ITEMS = 0, 1


def _ptr(a, dtype, ctype):
    return None if a is None else np.ascontiguousarray(a, dtype).ctypes.data_as(C.POINTER(ctype))


def _outs(n, topn, with_out):
    cells = max(1, n * max(1, topn))
    index, scores = np.empty(cells, np.int32), np.empty(cells, np.float32)
    if not with_out:
        return None, None
    return _ptr(index, np.int32, C.c_int32), _ptr(scores, np.float32, C.c_float)


def _by_index(m, call, queries, n, topn, with_out=True):
    """The raw C-ABI call of similar_items / similar_users: None stands for a NULL pointer."""
    oi, os_ = _outs(max(n, 0), topn, with_out)
    return getattr(m._lib, "mfsgd_" + call)(m._handle(), _ptr(queries, np.int32, C.c_int32), n, topn, oi, os_)


def _by_rows(m, side, rows, n_rows, topn, with_out=True):
    oi, os_ = _outs(max(n_rows, 0), topn, with_out)
    return m._lib.mfsgd_similar_rows(m._handle(), side, _ptr(rows, np.float32, C.c_float), n_rows, topn, oi, os_)


def _message(m):
    return m._lib.mfsgd_last_error(m._h).decode()


@pytest.fixture
def model(mf):
    """A handle without ratings: the calls need factors only."""
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        m.init_factors()
        yield m


@pytest.mark.parametrize("call,size", [("similar_items", I), ("similar_users", U)])
def test_bad_arguments_of_the_index_calls(model, call, size):
    bad = [
        dict(queries=[0, 1], n=-1, topn=2),                  # negative n
        dict(queries=None, n=2, topn=2),                     # NULL queries
        dict(queries=[0, 1], n=2, topn=2, with_out=False),   # NULL outputs
        dict(queries=[0, -1], n=2, topn=2),                  # index below range
        dict(queries=[0, size], n=2, topn=2),                # index above range
        dict(queries=[0, 1], n=2, topn=0),                   # topn < 1
        dict(queries=[0, 1], n=2, topn=size + 1),            # topn above the side's size
    ]
    for kw in bad:
        assert _by_index(model, call, **kw) == INVALID_ARG, kw
        assert _message(model).startswith(call + ": "), (kw, _message(model))
    # the other side's size is not this side's: U - 1 is a user, not an item
    assert (_by_index(model, call, [U - 1], 1, 1) == INVALID_ARG) == (call == "similar_items")


def test_bad_arguments_of_similar_rows(model):
    rows = np.ones((2, K), np.float32)
    for kw in [
        dict(side=2, rows=rows, n_rows=2, topn=2),            # a side that is neither
        dict(side=-1, rows=rows, n_rows=2, topn=2),
        dict(side=ITEMS, rows=rows, n_rows=-1, topn=2),       # negative n_rows
        dict(side=ITEMS, rows=None, n_rows=2, topn=2),        # NULL rows
        dict(side=ITEMS, rows=rows, n_rows=2, topn=2, with_out=False),
        dict(side=ITEMS, rows=rows, n_rows=2, topn=0),
        dict(side=ITEMS, rows=rows, n_rows=2, topn=I + 1),    # topn bound: the side's size, not the other's
        dict(side=USERS, rows=rows, n_rows=2, topn=U + 1),
    ]:
        assert _by_rows(model, **kw) == INVALID_ARG, kw
        assert _message(model).startswith("similar_rows: "), (kw, _message(model))


def test_bad_arguments_of_row_inv_norms(model):
    out = np.empty(U, np.float32)
    for side, o in [(2, out), (-1, out), (ITEMS, None), (USERS, None)]:
        assert model._lib.mfsgd_row_inv_norms(model._handle(), side, _ptr(o, np.float32, C.c_float)) == INVALID_ARG
        assert _message(model).startswith("row_inv_norms: ")


def test_dsgd_handles_are_a_state_error(mf):
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as m:
        assert _by_index(m, "similar_items", [0], 1, 2) == STATE and _message(m).startswith("similar_items: ")
        assert _by_index(m, "similar_users", [0], 1, 2) == STATE and _message(m).startswith("similar_users: ")
        assert _by_rows(m, ITEMS, np.ones((1, K), np.float32), 1, 2) == STATE and _message(m).startswith("similar_rows: ")
        out = np.empty(U, np.float32)
        assert m._lib.mfsgd_row_inv_norms(m._handle(), USERS, _ptr(out, np.float32, C.c_float)) == STATE
        assert _message(m).startswith("row_inv_norms: ")


def test_factors_never_set_are_a_state_error(mf):
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        assert _by_index(m, "similar_items", [0], 1, 2) == STATE and _message(m).startswith("similar_items: ")
        assert _by_rows(m, USERS, np.ones((1, K), np.float32), 1, 2) == STATE and _message(m).startswith("similar_rows: ")
        out = np.empty(I, np.float32)
        assert m._lib.mfsgd_row_inv_norms(m._handle(), ITEMS, _ptr(out, np.float32, C.c_float)) == STATE
        assert _message(m).startswith("row_inv_norms: ")


def test_no_queries_is_ok_and_touches_nothing(model, mf):
    before = mf.debug_device_bytes()
    assert _by_index(model, "similar_items", None, 0, 3, with_out=False) == 0
    assert _by_index(model, "similar_users", None, 0, 3, with_out=False) == 0
    assert _by_rows(model, ITEMS, None, 0, 3, with_out=False) == 0
    for index, scores in (model.similar_items([], 3), model.similar_users([], 2),
                          model.similar_rows(np.empty((0, K), np.float32), 3, side="users")):
        assert index.shape == scores.shape and index.shape[0] == 0
    assert mf.debug_device_bytes() == before


def test_python_shapes_are_checked(model):
    with pytest.raises(ValueError):
        model.similar_rows(np.ones((2, K + 1), np.float32), 2)
    with pytest.raises(ValueError):
        model.similar_rows(np.ones(K, np.float32), 2)
    with pytest.raises(ValueError):
        model.similar_rows(np.ones((2, K), np.float32), 2, side="neither")
    with pytest.raises(ValueError):
        model.row_inv_norms("neither")
    with pytest.raises(ValueError):
        model.similar_items(np.zeros((2, 2), np.int32), 2)


@pytest.mark.skipif(have_gpu(), reason="checks the no-device error path")
def test_valid_calls_without_device_fail_loudly(model, mf):
    assert _by_index(model, "similar_items", [0, 2], 2, 3) == NO_DEVICE
    assert _by_index(model, "similar_users", [0, 2], 2, 3) == NO_DEVICE
    assert _by_rows(model, ITEMS, np.ones((2, K), np.float32), 2, 3) == NO_DEVICE
    for call in (lambda: model.similar_items([0, 2], 3), lambda: model.similar_users([1], U),
                 lambda: model.similar_rows(np.ones((1, K), np.float32), 2, side="users"),
                 lambda: model.row_inv_norms("items"), lambda: model.row_inv_norms("users")):
        with pytest.raises(mf.MfsgdError) as err:
            call()
        assert err.value.code == NO_DEVICE
