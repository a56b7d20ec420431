"""Online updates without a GPU (include/mfsgd.h, "online updates"): mfsgd_online_levels against a restatement of its
definition; that no level holds a user or an item twice; the theorem the device path rests on -- the levels in ascending
order, each in any order, give the bits of the sequential loop -- on the oracle alone; the argument and state checks of
both calls, which come before any device work; and that a valid mfsgd_apply_ratings without a device fails loudly."""
import ctypes as C

import numpy as np
import pytest

from tests import online_common as oc
from tests.conftest import have_gpu

OK, INVALID_ARG, NO_DEVICE, STATE = 0, -1, -2, -5
LR, LAM, SEED = 0.01, 0.05, 4

BATCHES = {
    "random": oc.random_batch,
    "distinct": oc.distinct_batch,
    "one_item": oc.one_item_batch,
    "one_user": oc.one_user_batch,
    "same_pair": oc.same_pair_batch,
    "hot_item": oc.hot_item_batch,
    "widths_16": lambda: oc.widths_batch(oc.boundary_widths(16)),
    "two_pieces": lambda: oc.two_piece_batch(5),
}
_made = {}


def batch(name):
    """(U, I, u, i, r, levels by the restatement): built once, never modified."""
    if name not in _made:
        U, I, u, i, r = BATCHES[name]()
        _made[name] = (U, I, u, i, r, oc.py_levels(u, i))
        for a in _made[name][2:]:
            a.setflags(write=False)
    return _made[name]


def _handle(mf, U, I, k=8, **kw):
    return mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED, **kw)


# -- 1. the levels ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_levels_equal_the_restatement(mf, name):
    U, I, u, i, r, want = batch(name)
    with _handle(mf, U, I) as m:  # no ratings, no factors, no GPU
        for _ in range(2):  # (the second call finds the handle's scratch as the first left it: all reset)
            got, info = m.online_levels(u, i)
            assert np.array_equal(got, want)
            assert info == dict(oc.py_info(want), launches=0)
        # a prefix that ends inside the list is levelled on its own
        got, info = m.online_levels(u[:7], i[:7])
        assert np.array_equal(got, oc.py_levels(u[:7], i[:7])) and info["n"] == 7


def test_the_shapes_the_batches_are_there_for(mf):
    def info(name):
        U, I, u, i, r, level = batch(name)
        return oc.py_info(level), level

    got, _ = info("distinct")
    assert got["levels"] == 1 and got["max_width"] == got["n"] == 5000
    for name in ("one_item", "one_user"):
        got, _ = info(name)
        assert got["levels"] == 600 and got["max_width"] == 1
    got, _ = info("same_pair")
    assert got["levels"] == 300 and got["max_width"] == 1
    got, level = info("two_pieces")
    assert got["pieces"] == 2 and got["n"] == oc.PIECE + 5 and level[oc.PIECE] == 0 and level[oc.PIECE - 1] > 0
    got, level = info("widths_16")
    assert list(np.bincount(level)) == oc.boundary_widths(16)


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_no_level_holds_a_row_twice(name):
    U, I, u, i, r, level = batch(name)
    key = (np.arange(u.size, dtype=np.int64) // oc.PIECE) * (int(level.max()) + 1) + level  # (piece, level)
    for rows, size in ((u, U), (i, I)):
        pairs = key * size + rows
        assert np.unique(pairs).size == pairs.size


def test_levels_answer_without_filling_the_array(mf):
    U, I, u, i, r, want = batch("random")
    with _handle(mf, U, I) as m:
        info = mf._lib.OnlineInfo()
        p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        assert m._lib.mfsgd_online_levels(m._handle(), p(u), p(i), u.size, None, C.byref(info)) == OK
        assert info.as_dict() == dict(oc.py_info(want), launches=0)
        out = np.empty(u.size, np.int32)
        assert m._lib.mfsgd_online_levels(m._handle(), p(u), p(i), u.size, p(out), None) == OK
        assert np.array_equal(out, want)


# -- 2. the theorem, on the oracle alone -----------------------------------------------------------------------------
@pytest.mark.parametrize("k", (5, 64))
@pytest.mark.parametrize("name", sorted(BATCHES))
def test_levels_in_ascending_order_give_the_sequential_bits(oracle, name, k):
    U, I, u, i, r, level = batch(name)
    P0, Q0 = oracle.init_factors(U, I, k, SEED)
    P, Q = P0.copy(), Q0.copy()
    oracle.sgd_pass(P, Q, u, i, r, LR, LAM)
    assert not np.array_equal(P, P0) and not np.array_equal(Q, Q0)
    for reverse in (False, True):
        Pl, Ql = P0.copy(), Q0.copy()
        oracle.sgd_pass_ordered(Pl, Ql, u, i, r, oc.level_order(level, reverse), LR, LAM)
        assert np.array_equal(Pl, P) and np.array_equal(Ql, Q), reverse


# -- 3. arguments and state ------------------------------------------------------------------------------------------
def _ptr(a, dtype, ctype):
    """None stands for a NULL pointer."""
    return None if a is None else np.ascontiguousarray(a, dtype).ctypes.data_as(C.POINTER(ctype))


def _apply(m, u, i, r, n, err=False):
    e = np.zeros(max(1, n), np.float32) if err else None
    return m._lib.mfsgd_apply_ratings(m._handle(), _ptr(u, np.int32, C.c_int32), _ptr(i, np.int32, C.c_int32),
                                      _ptr(r, np.float32, C.c_float), n, _ptr(e, np.float32, C.c_float), None)


def _levels(m, u, i, n):
    out = np.zeros(max(1, n), np.int32)
    return m._lib.mfsgd_online_levels(m._handle(), _ptr(u, np.int32, C.c_int32), _ptr(i, np.int32, C.c_int32), n,
                                      _ptr(out, np.int32, C.c_int32), None)


def _err(m):
    return m._lib.mfsgd_last_error(m._h).decode()


U0, I0 = 6, 5
BAD = [
    (dict(u=[0, 1], i=[0, 1], n=-1), "negative"),
    (dict(u=None, i=[0, 1], n=2), "null"),
    (dict(u=[0, 1], i=None, n=2), "null"),
    (dict(u=[0, 1, -1], i=[0, 1, 2], n=3), "rating 2"),
    (dict(u=[0, U0, 1], i=[0, 1, 2], n=3), "rating 1"),
    (dict(u=[0, 1, 2], i=[-1, 1, 2], n=3), "rating 0"),
    (dict(u=[0, 1, 2], i=[0, 1, I0], n=3), "rating 2"),
]


@pytest.fixture
def model(mf):
    with _handle(mf, U0, I0) as m:
        m.init_factors()
        yield m


@pytest.mark.parametrize("kw,word", BAD)
def test_bad_arguments_are_invalid(model, kw, word):
    P0, Q0 = model.get_factors()
    assert _apply(model, kw["u"], kw["i"], [1.0, 2.0, 3.0], kw["n"], err=True) == INVALID_ARG
    msg = _err(model)
    assert msg.startswith("apply_ratings:") and word in msg, msg
    assert _levels(model, kw["u"], kw["i"], kw["n"]) == INVALID_ARG
    msg = _err(model)
    assert msg.startswith("online_levels:") and word in msg, msg
    P, Q = model.get_factors()
    assert np.array_equal(P, P0) and np.array_equal(Q, Q0)


def test_null_ratings_and_null_handle(model):
    assert _apply(model, [0, 1], [0, 1], None, 2) == INVALID_ARG
    assert _err(model).startswith("apply_ratings:") and "null" in _err(model)
    assert model._lib.mfsgd_apply_ratings(None, None, None, None, 0, None, None) == INVALID_ARG
    assert model._lib.mfsgd_online_levels(None, None, None, 0, None, None) == INVALID_ARG


def test_nothing_to_apply_is_ok(model, mf):
    P0, Q0 = model.get_factors()
    info = mf._lib.OnlineInfo(n=-1, pieces=-1, levels=-1, max_width=-1, launches=-1)
    assert model._lib.mfsgd_apply_ratings(model._handle(), None, None, None, 0, None, C.byref(info)) == OK
    assert info.as_dict() == dict(n=0, pieces=0, levels=0, max_width=0, launches=0)
    assert model.partial_fit([], [], [], errors=True).shape == (0,)
    assert model.partial_fit([], [], []) is None
    levels, info = model.online_levels([], [])
    assert levels.shape == (0,) and info == dict(n=0, pieces=0, levels=0, max_width=0, launches=0)
    P, Q = model.get_factors()
    assert np.array_equal(P, P0) and np.array_equal(Q, Q0)


def test_state_errors(mf):
    with _handle(mf, U0, I0) as m:  # factors never initialised
        assert _apply(m, [0], [0], [1.0], 1) == STATE
        assert _err(m).startswith("apply_ratings:") and "not initialised" in _err(m)
        assert _levels(m, [0], [0], 1) == OK  # (the levels need no factors)
    with _handle(mf, U0, I0) as m:  # P alone
        m.init_p_offset(SEED, 0)
        assert _apply(m, [0], [0], [1.0], 1) == STATE
        assert _err(m).startswith("apply_ratings: Q is not initialised")
    with _handle(mf, U0, I0, n_parts=2) as m:  # the handle does not hold Q
        m.init_factors()
        assert _apply(m, [0], [0], [1.0], 1) == STATE
        assert _err(m).startswith("apply_ratings:") and "single-partition" in _err(m)
    with _handle(mf, U0, I0) as m:  # an argument error comes first
        assert _apply(m, [U0], [0], [1.0], 1) == INVALID_ARG


def test_python_shapes_are_checked(model):
    with pytest.raises(ValueError):
        model.partial_fit([0, 1], [0, 1], [1.0])
    with pytest.raises(ValueError):
        model.partial_fit([0, 1], [0], [1.0, 2.0])
    with pytest.raises(ValueError):
        model.online_levels([0, 1], [0])


@pytest.mark.skipif(have_gpu(), reason="checks the no-device error path")
def test_a_valid_call_without_a_device_fails_loudly(model, mf):
    assert _apply(model, [0, 1, 0], [0, 1, 1], [1.0, 2.0, 3.0], 3, err=True) == NO_DEVICE
    with pytest.raises(mf.MfsgdError) as e:
        model.partial_fit([0, 1, 0], [0, 1, 1], [1.0, 2.0, 3.0], errors=True)
    assert e.value.code == NO_DEVICE
    levels, info = model.online_levels([0, 1, 0], [0, 1, 1])  # ... and the levels need none
    assert list(levels) == [0, 0, 1] and info["levels"] == 2 and info["max_width"] == 2
