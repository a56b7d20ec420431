"""Pairwise ranking (BPR) without a GPU (include/mfsgd.h, "pairwise ranking"): lsig through mfsgd_bpr_weights against its
known answers and, bit for bit, against the C restatement of its definition (tests/pairwise_common.py); that it never
increases; mfsgd_triple_levels against the Python restatement; the argument and state checks of the calls in their stated
order, which come before any device work; and that a valid mfsgd_apply_triples without a device fails loudly."""
import ctypes as C

import numpy as np
import pytest

from tests import pairwise_common as pc
from tests.conftest import have_gpu

OK, INVALID_ARG, NO_DEVICE, STATE = 0, -1, -2, -5
LR, LAM, SEED = 0.05, 0.01, 4


# -- 1. lsig ---------------------------------------------------------------------------------------------------------
def test_known_answers(mf):
    x = np.array([a for a, _ in pc.KNOWN], np.float32)
    want = np.array([b for _, b in pc.KNOWN], np.uint32)
    got = mf.bpr_weights(x).view(np.uint32)
    assert [hex(v) for v in got] == [hex(v) for v in want]
    assert [hex(v) for v in pc.c_lsig(x).view(np.uint32)] == [hex(v) for v in want]  # the restatement says the same


def _lsig_inputs():
    rng = np.random.default_rng(1)
    x = rng.uniform(-100.0, 100.0, 1 << 20).astype(np.float32)
    tiny = np.array([0x00000001, 0x00000100, 0x007FFFFF, 0x00800000], np.uint32)  # subnormals and the first normal
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan, 80.0, -80.0, 100.0, -100.0, 3.4e38, -3.4e38], np.float32)
    nans = np.array([0x7FC00000, 0xFFC00000, 0x7F800001, 0xFFFFFFFF, 0x7FC12345], np.uint32).view(np.float32)
    return np.concatenate([x, tiny.view(np.float32), (tiny | np.uint32(0x80000000)).view(np.float32), special, nans,
                           rng.normal(0.0, 1e-3, 4096).astype(np.float32), rng.normal(0.0, 4.0, 1 << 16).astype(np.float32)])


def test_library_and_restatement_agree_bit_for_bit(mf):
    x = _lsig_inputs()
    got, want = mf.bpr_weights(x).view(np.uint32), pc.c_lsig(x).view(np.uint32)
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, [(float(x[b]), hex(got[b]), hex(want[b])) for b in bad[:5]]
    nan = np.isnan(x)
    assert nan.sum() == 6 and (got[nan] == 0x7FC00000).all()  # a NaN stays a NaN, and it is THE quiet NaN
    assert not np.isnan(got.view(np.float32)[~nan]).any()
    g = got.view(np.float32)[~nan]
    assert g.min() > 0.0 and g.max() == 1.0
    # against the function it approximates, in double: the sweep of DESIGN.md found 2.48 ulp at worst
    xs = x[~nan].astype(np.float64).clip(-80.0, 80.0)
    ref = 1.0 / (1.0 + np.exp(xs))
    ulp = np.spacing(ref.astype(np.float32)).astype(np.float64)
    assert (np.abs(g.astype(np.float64) - ref) / ulp).max() < 3.0


def test_weights_never_increase(mf):
    x = np.sort(_lsig_inputs())  # (NaN sorts last)
    x = x[~np.isnan(x)]
    g = mf.bpr_weights(x)
    assert (np.diff(g.astype(np.float64)) <= 0.0).all()
    assert g[0] == 1.0 and g[-1].view(np.uint32) == 0x05BFECBA


def test_weights_arguments(mf):
    lib = mf.load_library()
    f = C.POINTER(C.c_float)
    one = np.zeros(1, np.float32)
    p = one.ctypes.data_as(f)
    assert lib.mfsgd_bpr_weights(None, None, 0) == OK
    assert mf.bpr_weights([]).shape == (0,)
    for args, word in (((p, p, -1), "negative"), ((None, p, 1), "null"), ((p, None, 1), "null")):
        assert lib.mfsgd_bpr_weights(*args) == INVALID_ARG
        msg = lib.mfsgd_last_error(None).decode()
        assert msg.startswith("bpr_weights:") and word in msg, msg
    assert mf.bpr_weights(np.zeros((2, 3), np.float32)).shape == (2, 3)


# -- 2. the levels ---------------------------------------------------------------------------------------------------
BATCHES = {
    "random": pc.random_batch,
    "two_step": pc.two_step_batch,
    "hot_positive": pc.hot_positive_batch,
    "hot_negative": pc.hot_negative_batch,
    "one_user": pc.one_user_batch,
    "cross_role": pc.cross_role_batch,
    "two_pieces": lambda: pc.two_piece_batch(5),
}
_made = {}


def batch(name):
    """(U, I, u, i, j, levels by the restatement): built once, never modified."""
    if name not in _made:
        U, I, u, i, j = BATCHES[name]()
        _made[name] = (U, I, u, i, j, pc.py_levels(u, i, j))
        for a in _made[name][2:]:
            a.setflags(write=False)
    return _made[name]


def _handle(mf, U, I, k=8, **kw):
    return mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED, **kw)


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_levels_equal_the_restatement(mf, name):
    U, I, u, i, j, want = batch(name)
    with _handle(mf, U, I) as m:  # no ratings, no factors, no GPU
        for _ in range(2):  # (the second call finds the handle's scratch as the first left it: all reset)
            got, info = m.triple_levels(u, i, j)
            assert np.array_equal(got, want)
            assert info == dict(pc.py_info(want), launches=0)
        got, info = m.triple_levels(u[:7], i[:7], j[:7])
        assert np.array_equal(got, pc.py_levels(u[:7], i[:7], j[:7])) and info["n"] == min(7, u.size)
        # the pair levels, which share the scratch, are not disturbed by the triples before them
        from tests import online_common as oc

        got, _ = m.online_levels(u[:500], i[:500])
        assert np.array_equal(got, oc.py_levels(u[:500], i[:500]))


def test_the_shapes_the_batches_are_there_for():
    assert list(batch("two_step")[5]) == [0, 1, 0]
    for name, n in (("hot_positive", 600), ("hot_negative", 600), ("one_user", 600), ("cross_role", 300)):
        got = pc.py_info(batch(name)[5])
        assert got["levels"] == n and got["max_width"] == 1, name
    level = batch("two_pieces")[5]
    got = pc.py_info(level)
    assert got["pieces"] == 2 and got["n"] == pc.PIECE + 5 and level[pc.PIECE] == 0 and level[pc.PIECE - 1] > 0


@pytest.mark.parametrize("name", sorted(BATCHES))
def test_no_level_holds_a_row_twice(name):
    U, I, u, i, j, level = batch(name)
    key = (np.arange(u.size, dtype=np.int64) // pc.PIECE) * (int(level.max()) + 1) + level  # (piece, level)
    users = key * U + u
    assert np.unique(users).size == users.size
    items = np.concatenate([key * I + i, key * I + j])  # either position is the same row of Q
    assert np.unique(items).size == items.size


def test_levels_answer_without_filling_the_array(mf):
    U, I, u, i, j, want = batch("random")
    with _handle(mf, U, I) as m:
        info = mf._lib.OnlineInfo()
        p = lambda a: a.ctypes.data_as(C.POINTER(C.c_int32))
        assert m._lib.mfsgd_triple_levels(m._handle(), p(u), p(i), p(j), u.size, None, C.byref(info)) == OK
        assert info.as_dict() == dict(pc.py_info(want), launches=0)
        out = np.empty(u.size, np.int32)
        assert m._lib.mfsgd_triple_levels(m._handle(), p(u), p(i), p(j), u.size, p(out), None) == OK
        assert np.array_equal(out, want)


# -- 3. the theorem, on the restatement alone ------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["random", "two_step", "hot_positive", "cross_role"])
def test_levels_in_ascending_order_give_the_sequential_bits(oracle, name):
    from tests import online_common as oc

    U, I, u, i, j, level = batch(name)
    P0, Q0 = oracle.init_factors(U, I, 5, SEED)
    P, Q, x = pc.c_pass(P0, Q0, u, i, j, LR, LAM)
    assert not np.array_equal(P, P0) and not np.array_equal(Q, Q0)
    for reverse in (False, True):
        order = oc.level_order(level, reverse)
        Pl, Ql, xl = pc.c_pass(P0, Q0, u[order], i[order], j[order], LR, LAM)
        assert Pl.tobytes() == P.tobytes() and Ql.tobytes() == Q.tobytes() and xl.tobytes() == x[order].tobytes(), reverse


# -- 4. arguments and state ------------------------------------------------------------------------------------------
def _ptr(a, dtype, ctype):
    """None stands for a NULL pointer."""
    return None if a is None else np.ascontiguousarray(a, dtype).ctypes.data_as(C.POINTER(ctype))


def _apply(m, u, i, j, n, margins=False):
    x = np.zeros(max(1, n), np.float32) if margins else None
    ip = lambda a: _ptr(a, np.int32, C.c_int32)
    return m._lib.mfsgd_apply_triples(m._handle(), ip(u), ip(i), ip(j), n, _ptr(x, np.float32, C.c_float), None)


def _levels(m, u, i, j, n):
    out = np.zeros(max(1, n), np.int32)
    ip = lambda a: _ptr(a, np.int32, C.c_int32)
    return m._lib.mfsgd_triple_levels(m._handle(), ip(u), ip(i), ip(j), n, ip(out), None)


def _err(m):
    return m._lib.mfsgd_last_error(m._h).decode()


U0, I0 = 6, 5
BAD = [  # in the order the checks are made: each case passes every check before its own
    (dict(u=[0, 1], i=[0, 1], j=[1, 0], n=-1), "negative"),
    (dict(u=None, i=[0, 1], j=[1, 0], n=2), "null"),
    (dict(u=[0, 1], i=None, j=[1, 0], n=2), "null"),
    (dict(u=[0, 1], i=[0, 1], j=None, n=2), "null"),
    (dict(u=[0, 1, -1], i=[0, 1, 2], j=[1, 2, 3], n=3), "triple 2 out of range"),
    (dict(u=[0, U0, 1], i=[0, 1, 2], j=[1, 2, 3], n=3), "triple 1 out of range"),
    (dict(u=[0, 1, 2], i=[-1, 1, 2], j=[1, 2, 3], n=3), "triple 0 out of range"),
    (dict(u=[0, 1, 2], i=[0, 1, I0], j=[1, 2, 3], n=3), "triple 2 out of range"),
    (dict(u=[0, 1, 2], i=[0, 1, 2], j=[1, I0, 3], n=3), "triple 1 out of range"),
    (dict(u=[0, 1, 2], i=[0, 1, 2], j=[1, 2, -1], n=3), "triple 2 out of range"),
    (dict(u=[0, 1, 2], i=[0, 1, 2], j=[1, 1, 3], n=3), "triple 1 has the same"),
    # a null array is reported before a range, a range before i == j, wherever in the list they are
    (dict(u=None, i=[0, I0], j=[0, 0], n=2), "null"),
    (dict(u=[0, 1, U0], i=[1, 1, 2], j=[1, 2, 3], n=3), "triple 2 out of range"),
]


@pytest.fixture
def model(mf):
    with _handle(mf, U0, I0) as m:
        m.init_factors()
        yield m


@pytest.mark.parametrize("kw,word", BAD)
def test_bad_arguments_are_invalid(model, kw, word):
    P0, Q0 = model.get_factors()
    assert _apply(model, kw["u"], kw["i"], kw["j"], kw["n"], margins=True) == INVALID_ARG
    msg = _err(model)
    assert msg.startswith("apply_triples:") and word in msg, msg
    assert _levels(model, kw["u"], kw["i"], kw["j"], kw["n"]) == INVALID_ARG
    msg = _err(model)
    assert msg.startswith("triple_levels:") and word in msg, msg
    P, Q = model.get_factors()
    assert np.array_equal(P, P0) and np.array_equal(Q, Q0)


def test_the_same_item_twice_is_refused_in_python_too(model, mf):
    with pytest.raises(mf.MfsgdError) as e:
        model.partial_fit_pairwise([0, 1], [2, 3], [1, 3])
    assert e.value.code == INVALID_ARG and "triple 1" in str(e.value)
    with pytest.raises(mf.MfsgdError) as e:
        model.triple_levels([0], [4], [4])
    assert e.value.code == INVALID_ARG


def test_null_handle(model):
    assert model._lib.mfsgd_apply_triples(None, None, None, None, 0, None, None) == INVALID_ARG
    assert model._lib.mfsgd_triple_levels(None, None, None, None, 0, None, None) == INVALID_ARG


def test_nothing_to_apply_is_ok(model, mf):
    P0, Q0 = model.get_factors()
    info = mf._lib.OnlineInfo(n=-1, pieces=-1, levels=-1, max_width=-1, launches=-1)
    assert model._lib.mfsgd_apply_triples(model._handle(), None, None, None, 0, None, C.byref(info)) == OK
    assert info.as_dict() == dict(n=0, pieces=0, levels=0, max_width=0, launches=0)
    assert model.partial_fit_pairwise([], [], [], margins=True).shape == (0,)
    assert model.partial_fit_pairwise([], [], []) is None
    x, info = model.partial_fit_pairwise([], [], [], margins=True, info=True)
    assert x.shape == (0,) and info["n"] == 0
    levels, info = model.triple_levels([], [], [])
    assert levels.shape == (0,) and info == dict(n=0, pieces=0, levels=0, max_width=0, launches=0)
    P, Q = model.get_factors()
    assert np.array_equal(P, P0) and np.array_equal(Q, Q0)


def test_state_errors(mf):
    with _handle(mf, U0, I0) as m:  # factors never initialised
        assert _apply(m, [0], [0], [1], 1) == STATE
        assert _err(m).startswith("apply_triples:") and "not initialised" in _err(m)
        assert _apply(m, None, None, None, 0) == STATE  # whatever n is
        assert _levels(m, [0], [0], [1], 1) == OK  # (the levels need no factors)
    with _handle(mf, U0, I0) as m:  # P alone
        m.init_p_offset(SEED, 0)
        assert _apply(m, [0], [0], [1], 1) == STATE
        assert _err(m).startswith("apply_triples: Q is not initialised")
    with _handle(mf, U0, I0, n_parts=2) as m:  # the handle does not hold Q
        m.init_factors()
        assert _apply(m, [0], [0], [1], 1) == STATE
        assert _err(m).startswith("apply_triples:") and "single-partition" in _err(m)
    with _handle(mf, U0, I0) as m:  # an argument error comes first
        assert _apply(m, [U0], [0], [1], 1) == INVALID_ARG
        assert _apply(m, [0], [1], [1], 1) == INVALID_ARG


def test_python_shapes_are_checked(model):
    with pytest.raises(ValueError):
        model.partial_fit_pairwise([0, 1], [0, 1], [1])
    with pytest.raises(ValueError):
        model.partial_fit_pairwise([0, 1], [0], [1, 0])
    with pytest.raises(ValueError):
        model.triple_levels([0, 1], [0, 1], [1])
    with pytest.raises(ValueError):
        model.fit_bpr([0, 1], [0], 1)
    with pytest.raises(ValueError):
        model.fit_bpr([0, 1], [0, 1], -1)


def test_signatures_cover_the_new_names(mf):
    for name in ("mfsgd_triple_levels", "mfsgd_apply_triples", "mfsgd_bpr_weights"):
        assert name in mf._lib.SIGNATURES


@pytest.mark.skipif(have_gpu(), reason="checks the no-device error path")
def test_a_valid_call_without_a_device_fails_loudly(model, mf):
    assert _apply(model, [0, 1, 0], [0, 1, 1], [1, 2, 3], 3, margins=True) == NO_DEVICE
    with pytest.raises(mf.MfsgdError) as e:
        model.partial_fit_pairwise([0, 1, 0], [0, 1, 1], [1, 2, 3], margins=True)
    assert e.value.code == NO_DEVICE
    levels, info = model.triple_levels([0, 1, 0], [0, 1, 1], [1, 2, 3])  # ... and the levels need none
    assert list(levels) == [0, 1, 2] and info["levels"] == 3 and info["max_width"] == 1
