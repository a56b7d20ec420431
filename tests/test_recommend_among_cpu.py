"""mfsgd_recommend_among / mfsgd_recommend_rows_among check their arguments before any device work, in
mfsgd_recommend_excluding's order with the candidates after the users and before the exclusion pairs, so these checks
run without a GPU; a valid call without a device fails with MFSGD_ERR_NO_DEVICE, never with a CPU result."""
import ctypes as C

import numpy as np
import pytest

from tests.conftest import have_gpu

OK, INVALID_ARG, NO_DEVICE, STATE = 0, -1, -2, -5
U, I, K = 6, 5, 8


def _ptr(a, dtype, ctype):
    return None if a is None else np.ascontiguousarray(a, dtype).ctypes.data_as(C.POINTER(ctype))


def _among(m, users, topn, cand_ptr, cand_items, n_cand, eu=None, ei=None, n_excl=0):
    """The raw C-ABI call: None stands for a NULL pointer.  Returns (status, message)."""
    uu = np.ascontiguousarray(users, np.int32)
    items = np.empty(max(1, uu.size * max(topn, 1)), np.int32)
    scores = np.empty(items.size, np.float32)
    rc = m._lib.mfsgd_recommend_among(m._handle(), _ptr(uu, np.int32, C.c_int32), uu.size, topn,
                                      _ptr(cand_ptr, np.int64, C.c_int64), _ptr(cand_items, np.int32, C.c_int32), n_cand,
                                      _ptr(eu, np.int32, C.c_int32), _ptr(ei, np.int32, C.c_int32), n_excl,
                                      _ptr(items, np.int32, C.c_int32), _ptr(scores, np.float32, C.c_float))
    return rc, m._lib.mfsgd_last_error(m._h).decode()


def _rows_among(m, rows, topn, cand_ptr, cand_items, n_cand, er=None, ei=None, n_excl=0):
    rows = np.ascontiguousarray(rows, np.float32)
    n = rows.shape[0]
    items = np.empty(max(1, n * max(topn, 1)), np.int32)
    scores = np.empty(items.size, np.float32)
    rc = m._lib.mfsgd_recommend_rows_among(m._handle(), _ptr(rows, np.float32, C.c_float), n, topn,
                                           _ptr(cand_ptr, np.int64, C.c_int64), _ptr(cand_items, np.int32, C.c_int32),
                                           n_cand, _ptr(er, np.int32, C.c_int32), _ptr(ei, np.int32, C.c_int32), n_excl,
                                           _ptr(items, np.int32, C.c_int32), _ptr(scores, np.float32, C.c_float))
    return rc, m._lib.mfsgd_last_error(m._h).decode()


@pytest.fixture
def model(mf):
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        m.init_factors()
        yield m


# users [0, 2]: two request rows
@pytest.mark.parametrize("topn,cand_ptr,cand_items,n_cand,message", [
    (3, [1, 2, 3], [0, 1, 2], 3, "recommend_among: cand_ptr[0] is not 0"),
    (3, [0, 2, 1], [0, 1, 2], 1, "recommend_among: cand_ptr decreases at row 1"),
    (3, [0, 1, 2], [0, 1, 2], 3, "recommend_among: cand_ptr ends at 2, not at n_cand"),
    (3, [0, 2, 4], [0, 1, 2], 3, "recommend_among: cand_ptr ends at 4, not at n_cand"),
    (3, None, None, 2, "recommend_among: cand_items is null"),
    (3, [0, 1, 2], None, 2, "recommend_among: cand_items is null"),
    (3, None, [0, 1], -1, "recommend_among: n_cand is negative"),
    (3, None, [0, 1, I, 2], 4, "recommend_among: candidate 2 out of range"),
    (3, [0, 1, 4], [0, 1, 3, -1], 4, "recommend_among: candidate 3 out of range"),
    (0, None, [0, 1], 2, "recommend_among: bad argument"),
    (-4, [0, 1, 2], [0, 1], 2, "recommend_among: bad argument"),
    (I + 1, None, [0, 1], 2, "recommend_among: topn exceeds the number of items"),
])
def test_bad_candidates_are_invalid_arguments_with_their_message(model, topn, cand_ptr, cand_items, n_cand, message):
    assert _among(model, [0, 2], topn, cand_ptr, cand_items, n_cand) == (INVALID_ARG, message)


def test_the_rows_call_names_itself(model):
    rows = np.ones((2, K), np.float32)
    assert _rows_among(model, rows, 3, [0, 1, 1], [0, I], 2) == (INVALID_ARG, "recommend_rows_among: cand_ptr ends at 1, not at n_cand")
    assert _rows_among(model, rows, 3, None, [0, I], 2) == (INVALID_ARG, "recommend_rows_among: candidate 1 out of range")
    assert _rows_among(model, rows, 0, None, [0], 1) == (INVALID_ARG, "recommend_rows_among: bad argument")
    assert _rows_among(model, rows, I + 1, None, [0], 1) == (INVALID_ARG, "recommend_rows_among: topn exceeds the number of items")
    assert _rows_among(model, rows, 2, None, [0], 1, [2], [0], 1) == (INVALID_ARG, "recommend_rows_among: excluded pair 0 out of range")


def test_checks_run_in_recommends_order_candidates_between_users_and_exclusions(model):
    bad_user, bad_cand, bad_pair = [0, U], [0, I], ([0, U], [1, 1])
    # everything wrong at once: the user is reported
    assert _among(model, bad_user, 2, None, bad_cand, 2, *bad_pair, 2) == (INVALID_ARG, "recommend_among: user 1 out of range")
    # a good user: the candidate comes before the pair
    assert _among(model, [0, 1], 2, None, bad_cand, 2, *bad_pair, 2) == (INVALID_ARG, "recommend_among: candidate 1 out of range")
    assert _among(model, [0, 1], 2, [0, 1, 1], bad_cand, 2, *bad_pair, 2) == (
        INVALID_ARG, "recommend_among: cand_ptr ends at 1, not at n_cand")
    # good candidates: the pair
    assert _among(model, [0, 1], 2, None, [0, 1], 2, *bad_pair, 2) == (INVALID_ARG, "recommend_among: excluded pair 1 out of range")
    # topn is recommend's own check and comes before all three
    assert _among(model, bad_user, I + 1, None, bad_cand, 2, *bad_pair, 2) == (
        INVALID_ARG, "recommend_among: topn exceeds the number of items")


def test_no_users_is_ok(model):
    assert _among(model, [], 3, None, [0, 1], 2)[0] == OK
    assert _among(model, [], 3, [0], None, 0)[0] == OK
    assert _rows_among(model, np.empty((0, K), np.float32), 3, [0], None, 0)[0] == OK


def test_state_errors(mf):
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as m:
        assert _among(m, [0], 2, None, [0, 1], 2) == (STATE, "recommend_among: single-partition handles only")
        assert _rows_among(m, np.ones((1, K), np.float32), 2, None, [0, 1], 2) == (
            STATE, "recommend_rows_among: single-partition handles only")
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:  # factors never set
        assert _rows_among(m, np.ones((1, K), np.float32), 2, None, [0, 1], 2) == (
            STATE, "recommend_rows_among: factors not initialised")
        # the users' call reports it exactly as mfsgd_recommend_excluding does, whatever that is on this machine
        uu, out_i, out_s = np.zeros(1, np.int32), np.empty(2, np.int32), np.empty(2, np.float32)
        want = m._lib.mfsgd_recommend_excluding(m._handle(), _ptr(uu, np.int32, C.c_int32), 1, 2, None, None, 0,
                                                _ptr(out_i, np.int32, C.c_int32), _ptr(out_s, np.float32, C.c_float))
        want_msg = m._lib.mfsgd_last_error(m._h).decode()
        rc, msg = _among(m, [0], 2, None, [0, 1], 2)
        assert want != OK and rc == want and msg == want_msg.replace("recommend:", "recommend_among:", 1)


@pytest.mark.skipif(have_gpu(), reason="checks the no-device error path")
def test_valid_call_without_device_fails_loudly(model, mf):
    assert _among(model, [0, 2], 3, None, [4, 0, 0, 1], 4)[0] == NO_DEVICE
    assert _among(model, [0, 2], 3, [0, 0, 2], [4, 0], 2, [0], [4], 1)[0] == NO_DEVICE
    assert _among(model, [0, 2], I, None, None, 0)[0] == NO_DEVICE  # (a topn above the list's length is no error)
    assert _rows_among(model, np.ones((2, K), np.float32), 3, None, [1], 1)[0] == NO_DEVICE
    for cand in ([1, 2], ([0, 1, 2], [3, 4]), [[1], []]):
        with pytest.raises(mf.MfsgdError) as e:
            model.recommend([0, 2], 3, candidates=cand)
        assert e.value.code == NO_DEVICE
        with pytest.raises(mf.MfsgdError) as e:
            model.recommend_rows(np.ones((2, K), np.float32), 3, candidates=cand)
        assert e.value.code == NO_DEVICE


@pytest.mark.parametrize("cand", [
    np.zeros((2, 2), np.int32),            # a 2-d array
    np.array([0.5, 1.0]),                  # not integers
    ([0, 1, 2],),                          # a tuple that is no (ptr, items)
    ([0, 1], [0]),                         # ptr of the wrong length for two rows
    ([0, 1, 2], [[0, 1]]),                 # items not 1-d
    ([0.0, 1.0, 2.0], [0, 1]),             # ptr not integers
    [[0, 1]],                              # one list for two rows
    [[0, 1], [[2]]],                       # a row's list not 1-d
    [[0, 1], [0.5]],                       # a row's list not integers
])
def test_python_candidate_shapes_are_checked(model, cand):
    with pytest.raises(ValueError):
        model.recommend([0, 2], 2, candidates=cand)
    with pytest.raises(ValueError):
        model.recommend_rows(np.ones((2, K), np.float32), 2, candidates=cand)


def test_appended_items_are_candidates_and_the_reserve_beyond_them_is_not(mf):
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        m.init_factors()  # host staging: no device yet
        m.reserve(items=I + 8)
        assert m.add_items(n=3) == I
        bad_pair = ([0], [I + 3])  # reported only once every candidate has passed
        rc, msg = _among(m, [0], 2, None, [I, I + 2, 0], 3, *bad_pair, 1)
        assert (rc, msg) == (INVALID_ARG, "recommend_among: excluded pair 0 out of range")
        # the new count is the first index that is none, however much room was reserved
        assert _among(m, [0], 2, None, [I, I + 3], 2) == (INVALID_ARG, "recommend_among: candidate 1 out of range")
        assert _among(m, [0], I + 3, None, [I], 1, *bad_pair, 1)[1] == "recommend_among: excluded pair 0 out of range"
        assert _among(m, [0], I + 4, None, [I], 1)[1] == "recommend_among: topn exceeds the number of items"
