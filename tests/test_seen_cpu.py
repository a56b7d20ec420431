"""The seen-item index under the C-ABI, as far as it goes without a GPU: every new call checks its arguments before any
device work, "no seen set" is a state error that comes before the device is asked for, an empty index is host-only, and
a valid call that needs the device fails with MFSGD_ERR_NO_DEVICE and leaves the index as it was (with a GPU the same
call succeeds: there is never a CPU result)."""
import ctypes as C

import numpy as np
import pytest

from tests.conftest import have_gpu

OK, INVALID_ARG, NO_DEVICE, STATE = 0, -1, -2, -5
U, I, K = 6, 5, 8


def _ptr(a, dtype, ctype):
    return None if a is None else np.ascontiguousarray(a, dtype).ctypes.data_as(C.POINTER(ctype))


def _i32(a):
    return _ptr(a, np.int32, C.c_int32)


def _err(m, rc):
    return rc, m._lib.mfsgd_last_error(m._h).decode()


def _update(m, call, u, i, n):
    return _err(m, getattr(m._lib, "mfsgd_" + call)(m._handle(), _i32(u), _i32(i), n))


def _size(m):
    n = C.c_int64(-7)
    assert m._lib.mfsgd_seen_size(m._handle(), C.byref(n)) == OK
    return n.value


def _get(m, users, n_users, row_ptr=True, items=None, capacity=0):
    ptr = np.full(max(n_users, 0) + 1, -9, np.int64)
    rc = m._lib.mfsgd_get_seen(m._handle(), _i32(users), n_users, _ptr(ptr, np.int64, C.c_int64) if row_ptr else None,
                               _i32(items), capacity)
    return _err(m, rc)


def _recommend(m, users, n_users, topn, out=True):
    items, scores = np.empty(64, np.int32), np.empty(64, np.float32)
    rc = m._lib.mfsgd_recommend_unseen(m._handle(), _i32(users), n_users, topn, _i32(items) if out else None,
                                       _ptr(scores, np.float32, C.c_float))
    return _err(m, rc)


def _among(m, users, n_users, topn, cand_ptr, cand_items, n_cand):
    items, scores = np.empty(64, np.int32), np.empty(64, np.float32)
    rc = m._lib.mfsgd_recommend_unseen_among(m._handle(), _i32(users), n_users, topn, _ptr(cand_ptr, np.int64, C.c_int64),
                                             _i32(cand_items), n_cand, _i32(items), _ptr(scores, np.float32, C.c_float))
    return _err(m, rc)


def _rank(m, users, items, n, out=True):
    ranks = np.empty(16, np.int32)
    return _err(m, m._lib.mfsgd_rank_items_unseen(m._handle(), _i32(users), _i32(items), n, _i32(ranks) if out else None))


def _evaluate(m, users, items, n, topn, metrics=True):
    from mfsgd_amd import _lib

    out, ranks = _lib.RankingMetrics(), np.empty(16, np.int32)
    rc = m._lib.mfsgd_evaluate_ranking_unseen(m._handle(), _i32(users), _i32(items), n, topn,
                                              C.byref(out) if metrics else None, _i32(ranks))
    return _err(m, rc)


@pytest.fixture
def model(mf):
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        m.init_factors()
        yield m


@pytest.fixture
def indexed(model):
    """... with an empty index: a valid state that needs no GPU."""
    assert _update(model, "set_seen", None, None, 0)[0] == OK
    return model


# ---- set_seen / mark_seen ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("call", ["set_seen", "mark_seen"])
def test_bad_pairs_are_invalid_arguments_with_the_calls_prefix(model, call):
    assert _update(model, call, [0], [0], -1) == (INVALID_ARG, f"{call}: n is negative")
    assert _update(model, call, None, [0], 1) == (INVALID_ARG, f"{call}: u or i is null")
    assert _update(model, call, [0], None, 1) == (INVALID_ARG, f"{call}: u or i is null")
    assert _update(model, call, [0, U, 1], [0, 0, 0], 3) == (INVALID_ARG, f"{call}: pair 1 out of range")
    assert _update(model, call, [0, -1], [0, 0], 2) == (INVALID_ARG, f"{call}: pair 1 out of range")
    assert _update(model, call, [0, 1], [I, 0], 2) == (INVALID_ARG, f"{call}: pair 0 out of range")
    # a bad pair in the last position of a list longer than one block of the check names that position
    n = 3 * 4096 + 17
    u, i = np.arange(n, dtype=np.int32) % U, np.arange(n, dtype=np.int32) % I
    i[-1] = -1
    assert _update(model, call, u, i, n) == (INVALID_ARG, f"{call}: pair {n - 1} out of range")
    assert _size(model) == -1  # nothing was created on the way


def test_an_empty_index_is_host_only(model):
    assert _size(model) == -1
    assert _update(model, "set_seen", None, None, 0)[0] == OK
    assert _size(model) == 0
    assert _update(model, "mark_seen", None, None, 0)[0] == OK and _size(model) == 0
    assert model._lib.mfsgd_clear_seen(model._handle()) == OK and _size(model) == -1
    assert model._lib.mfsgd_clear_seen(model._handle()) == OK  # (works in every state)
    # mark_seen of nothing gives a handle without an index an empty one
    assert _update(model, "mark_seen", None, None, 0)[0] == OK and _size(model) == 0


@pytest.mark.parametrize("call", ["set_seen", "mark_seen"])
def test_a_valid_update_needs_the_device_and_leaves_the_index_as_it_was_without_one(mf, call):
    # (needs neither ratings nor factors)
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        for before in (-1, 0):
            rc, msg = _update(m, call, [0, 1, 1], [0, 2, 2], 3)
            if have_gpu():
                assert (rc, _size(m)) == (OK, 2), msg
                assert m._lib.mfsgd_clear_seen(m._handle()) == OK
            else:
                assert rc == NO_DEVICE and _size(m) == before, msg
            m.set_seen([], [])  # the second round starts from an empty index


def test_seen_size_wants_its_output(model):
    assert _err(model, model._lib.mfsgd_seen_size(model._handle(), None)) == (INVALID_ARG, "seen_size: pairs is null")


# ---- get_seen --------------------------------------------------------------------------------------------------------
def test_get_seen_checks_then_state_then_users(model):
    assert _get(model, [0], -1) == (INVALID_ARG, "get_seen: n_users is negative")
    assert _get(model, [0], 1, row_ptr=False) == (INVALID_ARG, "get_seen: row_ptr is null")
    assert _get(model, None, 1) == (INVALID_ARG, "get_seen: users is null")
    assert _get(model, [0], 1, items=[0], capacity=-1) == (INVALID_ARG, "get_seen: items_capacity is negative")
    assert _get(model, [0], 1) == (STATE, "get_seen: no seen set")
    assert _get(model, [U], 1) == (STATE, "get_seen: no seen set")  # (the state comes before the users)
    model.set_seen([], [])
    assert _get(model, [0, U], 2) == (INVALID_ARG, "get_seen: user 1 out of range")
    assert _get(model, [0, -1], 2) == (INVALID_ARG, "get_seen: user 1 out of range")
    assert _get(model, None, 0)[0] == OK
    ptr, items = model.seen([3, 0, 3])  # an empty index answers on the host
    assert ptr.tolist() == [0, 0, 0, 0] and items.size == 0


# ---- the unseen calls: the base call's checks under the new name, "no seen set" after n_parts ---------------------------
def test_recommend_unseen_checks(indexed):
    m = indexed
    assert _recommend(m, [0], -1, 3) == (INVALID_ARG, "recommend_unseen: bad argument")
    assert _recommend(m, [0], 1, 0) == (INVALID_ARG, "recommend_unseen: bad argument")
    assert _recommend(m, None, 1, 3) == (INVALID_ARG, "recommend_unseen: bad argument")
    assert _recommend(m, [0], 1, 3, out=False) == (INVALID_ARG, "recommend_unseen: bad argument")
    assert _recommend(m, [0], 1, I + 1) == (INVALID_ARG, "recommend_unseen: topn exceeds the number of items")
    assert _recommend(m, [0, U], 2, 3) == (INVALID_ARG, "recommend_unseen: user 1 out of range")
    assert _recommend(m, None, 0, 3)[0] == OK


def test_recommend_unseen_among_checks(indexed):
    m = indexed
    name = "recommend_unseen_among"
    assert _among(m, [0, 2], 2, 0, None, [0], 1) == (INVALID_ARG, f"{name}: bad argument")
    assert _among(m, [0, U], 2, 2, None, [0], 1) == (INVALID_ARG, f"{name}: user 1 out of range")
    assert _among(m, [0, 2], 2, 2, None, [0], -1) == (INVALID_ARG, f"{name}: n_cand is negative")
    assert _among(m, [0, 2], 2, 2, None, None, 1) == (INVALID_ARG, f"{name}: cand_items is null")
    assert _among(m, [0, 2], 2, 2, [1, 1, 1], [0], 1) == (INVALID_ARG, f"{name}: cand_ptr[0] is not 0")
    assert _among(m, [0, 2], 2, 2, [0, 1, 0], [0], 1) == (INVALID_ARG, f"{name}: cand_ptr decreases at row 1")
    assert _among(m, [0, 2], 2, 2, [0, 1, 2], [0], 1) == (INVALID_ARG, f"{name}: cand_ptr ends at 2, not at n_cand")
    assert _among(m, [0, 2], 2, 2, None, [0, I], 2) == (INVALID_ARG, f"{name}: candidate 1 out of range")
    assert _among(m, None, 0, 2, None, [0], 1)[0] == OK


def test_rank_and_evaluate_unseen_checks(indexed):
    m = indexed
    assert _rank(m, [0], [0], -1) == (INVALID_ARG, "rank_items_unseen: n is negative")
    assert _rank(m, None, [0], 1) == (INVALID_ARG, "rank_items_unseen: users, items or out_rank is null")
    assert _rank(m, [0], [0], 1, out=False) == (INVALID_ARG, "rank_items_unseen: users, items or out_rank is null")
    assert _rank(m, [0, U], [0, 0], 2) == (INVALID_ARG, "rank_items_unseen: pair 1 out of range")
    assert _rank(m, [0, 1], [0, I], 2) == (INVALID_ARG, "rank_items_unseen: pair 1 out of range")
    assert _rank(m, None, None, 0)[0] == OK
    name = "evaluate_ranking_unseen"
    assert _evaluate(m, [0], [0], 1, 0) == (INVALID_ARG, f"{name}: topn is below 1")
    assert _evaluate(m, [0], [0], 1, 3, metrics=False) == (INVALID_ARG, f"{name}: the metrics struct is null")
    assert _evaluate(m, [0], [0], -1, 3) == (INVALID_ARG, f"{name}: n is negative")
    assert _evaluate(m, [0, 1], [0, I], 2, 3) == (INVALID_ARG, f"{name}: pair 1 out of range")
    assert _evaluate(m, None, None, 0, 3)[0] == OK


def test_no_seen_set_is_a_state_error_before_the_device_and_the_factors(mf):
    """A handle without an index, and without factors: the missing index is reported, not the factors and not the
    device -- and before the argument checks that follow the n_parts check."""
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        assert _recommend(m, [0], 1, 3) == (STATE, "recommend_unseen: no seen set")
        assert _recommend(m, [U], 1, I + 1) == (STATE, "recommend_unseen: no seen set")
        assert _among(m, [0], 1, 3, None, [0], 1) == (STATE, "recommend_unseen_among: no seen set")
        assert _rank(m, [0], [0], 1) == (STATE, "rank_items_unseen: no seen set")
        assert _evaluate(m, [0], [0], 1, 3) == (STATE, "evaluate_ranking_unseen: no seen set")
        assert _recommend(m, [0], 1, 0) == (INVALID_ARG, "recommend_unseen: bad argument")  # (those before it stay first)
        # with an (empty) index the call goes on to what the base call reports
        m.set_seen([], [])
        rc, msg = _recommend(m, [0], 1, 3)  # (mfsgd_recommend asks for the device first, then for the factors)
        assert rc == (STATE if have_gpu() else NO_DEVICE) and "no seen set" not in msg
        assert _rank(m, [0], [0], 1) == (STATE, "rank_items_unseen: factors not initialised")


def test_a_valid_unseen_call_needs_the_device(indexed):
    want = OK if have_gpu() else NO_DEVICE
    assert _recommend(indexed, [0, 1], 2, 3)[0] == want
    assert _among(indexed, [0, 1], 2, 3, None, [0, 1], 2)[0] == want
    assert _rank(indexed, [0], [1], 1)[0] == want
    assert _evaluate(indexed, [0], [1], 1, 3)[0] == want


# ---- DSGD handles, null handles --------------------------------------------------------------------------------------
def test_partitioned_handles_are_a_state_error_everywhere(mf):
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as m:
        only = "single-partition handles only"
        assert _update(m, "set_seen", [0], [0], 1) == (STATE, f"set_seen: {only}")
        assert _update(m, "set_seen", None, None, 0) == (STATE, f"set_seen: {only}")
        assert _update(m, "mark_seen", [0], [0], 1) == (STATE, f"mark_seen: {only}")
        assert _err(m, m._lib.mfsgd_clear_seen(m._handle())) == (STATE, f"clear_seen: {only}")
        n = C.c_int64()
        assert _err(m, m._lib.mfsgd_seen_size(m._handle(), C.byref(n))) == (STATE, f"seen_size: {only}")
        assert _get(m, [0], 1) == (STATE, f"get_seen: {only}")
        assert _recommend(m, [0], 1, 3) == (STATE, f"recommend_unseen: {only}")
        assert _among(m, [0], 1, 3, None, [0], 1) == (STATE, f"recommend_unseen_among: {only}")
        assert _rank(m, [0], [0], 1) == (STATE, f"rank_items_unseen: {only}")
        assert _evaluate(m, [0], [0], 1, 3) == (STATE, f"evaluate_ranking_unseen: {only}")


def test_a_null_handle_is_an_invalid_argument(mf):
    lib = mf.load_library()
    n = C.c_int64()
    one = _i32([0])
    ptr = _ptr([0, 0], np.int64, C.c_int64)
    f = _ptr([0.0], np.float32, C.c_float)
    from mfsgd_amd import _lib

    met = _lib.RankingMetrics()
    assert lib.mfsgd_set_seen(None, one, one, 1) == INVALID_ARG
    assert lib.mfsgd_mark_seen(None, one, one, 1) == INVALID_ARG
    assert lib.mfsgd_clear_seen(None) == INVALID_ARG
    assert lib.mfsgd_seen_size(None, C.byref(n)) == INVALID_ARG
    assert lib.mfsgd_get_seen(None, one, 1, ptr, None, 0) == INVALID_ARG
    assert lib.mfsgd_recommend_unseen(None, one, 1, 1, one, f) == INVALID_ARG
    assert lib.mfsgd_recommend_unseen_among(None, one, 1, 1, None, one, 1, one, f) == INVALID_ARG
    assert lib.mfsgd_rank_items_unseen(None, one, one, 1, one) == INVALID_ARG
    assert lib.mfsgd_evaluate_ranking_unseen(None, one, one, 1, 1, C.byref(met), one) == INVALID_ARG


# ---- the Python plumbing -----------------------------------------------------------------------------------------------
def test_exclude_takes_the_string_seen_and_no_other(indexed):
    m = indexed
    for call in (lambda e: m.recommend([0], 2, exclude=e), lambda e: m.recommend([0], 2, exclude=e, candidates=[0, 1]),
                 lambda e: m.rank_items([0], [1], exclude=e), lambda e: m.evaluate_ranking([0], [1], 2, exclude=e)):
        for bad in ("unseen", "", "Seen"):
            with pytest.raises(ValueError, match='exclude must be None, \\(u, i\\) or "seen"'):
                call(bad)
    # "seen" reaches the _unseen calls: on a handle without an index they say so
    m.clear_seen()
    for call, name in ((lambda: m.recommend([0], 2, exclude="seen"), "recommend_unseen"),
                       (lambda: m.recommend([0], 2, exclude="seen", candidates=[0, 1]), "recommend_unseen_among"),
                       (lambda: m.rank_items([0], [1], exclude="seen"), "rank_items_unseen"),
                       (lambda: m.evaluate_ranking([0], [1], 2, exclude="seen"), "evaluate_ranking_unseen")):
        with pytest.raises(Exception) as e:
            call()
        assert e.value.code == STATE and f"{name}: no seen set" in str(e.value)
    assert m.seen_size() == -1
