"""WARP, as far as it goes without a GPU: the numpy restatement of the rule (tests/warp_common.py) is what it claims to be on
hand-made score tables; mfsgd_warp_weights against known answers and a float64 cumulative sum; and the two handle calls,
mfsgd_sample_unseen_violating and mfsgd_apply_triples_weighted, check their arguments before any device work, in the order
include/mfsgd.h states, leave their outputs alone when they refuse, and never answer on the CPU."""
import ctypes as C

import numpy as np
import pytest

from tests import implicit_common as IC
from tests import warp_common as WC
from tests.conftest import have_gpu

OK, INVALID_ARG, NO_DEVICE, STATE = 0, -1, -2, -5
U, I, K = 6, 5, 8
I64_MAX = (1 << 63) - 1
UNTOUCHED = -77
PRE = "sample_unseen_violating: "
PREW = "apply_triples_weighted: "


def _f(*x):
    return np.array(x, np.float32)


def _bits(a):
    return np.asarray(a, np.float32).view(np.uint32).tolist()


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_the_rule_on_hand_made_tables():
    nan, inf = np.nan, np.inf
    #                 x[d] = positive's score - candidate's                      margin 1
    x = np.stack([_f(0.5, 3, 3, 3),        # the pick at d = 0
                  _f(3, 2, 1.5, 0.25),     # the pick at d = m - 1
                  _f(3, 2, 1.5, 1.25),     # no pick
                  _f(1, 1, 1, 0.999),      # x == margin is no violation
                  _f(nan, nan, -5, -6),    # a NaN never violates; then the first that does
                  _f(nan, nan, nan, nan),  # nothing but NaNs: no pick
                  _f(-9, 0.5, 0, 0),       # a candidate equal to the positive is passed over, whatever its x
                  _f(2, 0.5, 0.75, 2),     # cnt < pick + 1: rank 1
                  _f(-inf, 0, 0, 0),
                  _f(inf, inf, -0.0, 0)])
    cand = np.tile(np.array([10, 11, 12, 13], np.int32), (x.shape[0], 1))
    pos = np.full(x.shape[0], 3, np.int32)
    pos[6] = 10
    cnt = np.full(x.shape[0], 20, np.int64)
    cnt[7] = 1
    assert WC.first_violating(x, cand, pos, 1.0).tolist() == [0, 3, 4, 3, 2, 4, 1, 1, 0, 2]
    assert WC.first_violating(x, cand, pos, 1.0).dtype == np.int32
    items, draws, margins, ranks = WC.outputs(x, cand, pos, 1.0, cnt)
    assert items.tolist() == [10, 13, -1, 13, 12, -1, 11, 11, 10, 12]
    assert draws.tolist() == [0, 3, 4, 3, 2, 4, 1, 1, 0, 2]
    assert ranks.tolist() == [20, 5, 0, 5, 6, 0, 10, 1, 20, 6]  # max(1, cnt // (d + 1)); 0 without a pick
    want = _bits(_f(0.5, 0.25, 0, 0.999, -5, 0, 0.5, 0.5, -inf, -0.0))
    want[2] = want[5] = WC.NAN_BITS  # no pick
    assert _bits(margins) == want
    assert [a.dtype for a in (items, draws, margins, ranks)] == [np.int32, np.int32, np.float32, np.int32]
    # the margins that are special: 0 takes negative x alone, and -0.0 == +0.0; +Inf takes every number but +Inf; -Inf nothing
    row = _f(0.0, -0.0, inf, nan, -1e-45, -inf)[None]
    c, p = np.arange(6, dtype=np.int32)[None] + 10, np.array([3], np.int32)
    assert WC.first_violating(row, c, p, 0.0).tolist() == [4]
    assert WC.first_violating(row, c, p, -0.0).tolist() == [4]
    assert WC.first_violating(row, c, p, inf).tolist() == [0]
    assert WC.first_violating(row[:, 2:], c[:, 2:], p, inf).tolist() == [2]  # +Inf and NaN do not violate +Inf
    assert WC.first_violating(row, c, p, -inf).tolist() == [6]
    # a user who has seen everything: -1, -1, NaN, 0, whatever the table says
    items, draws, margins, ranks = WC.outputs(x[:1], cand[:1], pos[:1], 1.0, [0])
    assert (items.tolist(), draws.tolist(), _bits(margins), ranks.tolist()) == ([-1], [-1], [WC.NAN_BITS], [0])
    # m = 1: there is one candidate
    assert WC.first_violating(_f(0, 2, nan).reshape(3, 1), np.full((3, 1), 9), np.array([1, 1, 1]), 1.0).tolist() == [0, 1, 1]


def test_the_restated_call_on_a_small_model():
    rng = np.random.default_rng(7)
    n_users, n_items, k = 9, 40, 5
    pu, pi = rng.integers(0, n_users - 1, 150), rng.integers(0, n_items, 150)
    pu, pi = np.concatenate([pu, np.full(n_items, n_users - 1)]), np.concatenate([pi, np.arange(n_items)])  # one has seen all
    lists = IC.lists_of(pu, pi)
    P, Q = rng.standard_normal((n_users, k)).astype(np.float32), rng.standard_normal((n_items, k)).astype(np.float32)
    scorer = lambda u, i: np.einsum("xf,xf->x", P[u], Q[i]).astype(np.float32)
    users = rng.integers(0, n_users, 500).astype(np.int32)
    pos = rng.integers(0, n_items, 500).astype(np.int32)
    for m in (1, 3, 8):
        items, draws, margins, ranks = WC.violating(lists, n_items, users, pos, m, 0.5, 11, 1000, scorer)
        cand = IC.sample(lists, n_items, users, m, 11, 1000)
        full = users == n_users - 1
        assert (items[full] == -1).all() and (draws[full] == -1).all() and (ranks[full] == 0).all()
        assert (margins.view(np.uint32)[items < 0] == WC.NAN_BITS).all()
        x = scorer(users, pos)[:, None] - scorer(np.repeat(users, m), np.where(cand < 0, 0, cand).ravel()).reshape(-1, m)
        viol = (x < np.float32(0.5)) & (cand != pos[:, None])
        hit = np.flatnonzero(items >= 0)
        assert hit.size and (draws[~full & (items < 0)] == m).all() and not viol[~full & (items < 0)].any()
        assert np.array_equal(items[hit], cand[hit, draws[hit]]) and viol[hit, draws[hit]].all()
        assert all(not viol[r, :draws[r]].any() for r in hit)  # the first
        assert np.array_equal(margins[hit], x[hit, draws[hit]])
        cnt = np.array([n_items - len(lists(int(u))) for u in users[hit]])
        assert np.array_equal(ranks[hit], np.maximum(1, cnt // (draws[hit] + 1)))
        assert not np.isin((users[hit].astype(np.int64) << 32) | items[hit], (pu.astype(np.int64) << 32) | pi).any()
    # rows [a, b) of a call are the call on the slices with first + a * m
    whole = WC.violating(lists, n_items, users, pos, 3, 0.5, 11, 1000, scorer)
    part = WC.violating(lists, n_items, users[100:230], pos[100:230], 3, 0.5, 11, 1000 + 100 * 3, scorer)
    for w, p in zip(whole, part):
        assert w[100:230].tobytes() == p.tobytes()


# ---- mfsgd_warp_weights -------------------------------------------------------------------------------------------------------
def test_warp_weights_known_answers(mf):
    w = mf.warp_weights([0, 1, 2, 3, 1, 0])
    assert w.dtype == np.float32 and w.shape == (6,)
    assert _bits(w) == _bits([0.0, 1.0, 1.5, np.float32(1.0 + 0.5 + 1.0 / 3), 1.0, 0.0])
    assert _bits(mf.warp_weights(np.array([[4], [2]]))) == _bits([[np.float32(1.0 + 0.5 + 1.0 / 3 + 0.25)], [1.5]])
    assert mf.warp_weights([]).shape == (0,)
    R = 1 << 20
    want = np.cumsum(1.0 / np.arange(1, R + 1)).astype(np.float32)
    assert mf.warp_weights(np.arange(1, R + 1)).tobytes() == want.tobytes()
    ranks = np.random.default_rng(3).integers(0, R + 1, 5000)  # in any order, 0 among them
    assert mf.warp_weights(ranks).tobytes() == np.concatenate([[np.float32(0)], want])[ranks].tobytes()
    assert mf.warp_weights(ranks).tobytes() == WC.harmonic(ranks).tobytes()
    assert mf.warp_weights([R]).tobytes() == want[-1:].tobytes()  # a large rank alone: the table is the call's own


def test_warp_weights_arguments(mf):
    lib = mf.load_library()
    ip, fp = C.POINTER(C.c_int32), C.POINTER(C.c_float)
    rank, w = np.array([1, 2, -1, 3], np.int32), np.full(4, UNTOUCHED, np.float32)
    assert lib.mfsgd_warp_weights(rank.ctypes.data_as(ip), w.ctypes.data_as(fp), -1) == INVALID_ARG
    assert lib.mfsgd_last_error(None).decode() == "warp_weights: n is negative"
    assert lib.mfsgd_warp_weights(None, w.ctypes.data_as(fp), 4) == INVALID_ARG
    assert lib.mfsgd_last_error(None).decode() == "warp_weights: rank or w is null"
    assert lib.mfsgd_warp_weights(rank.ctypes.data_as(ip), None, 4) == INVALID_ARG
    assert lib.mfsgd_last_error(None).decode() == "warp_weights: rank or w is null"
    assert lib.mfsgd_warp_weights(rank.ctypes.data_as(ip), w.ctypes.data_as(fp), 4) == INVALID_ARG
    assert lib.mfsgd_last_error(None).decode() == "warp_weights: rank 2 is negative"
    assert (w == UNTOUCHED).all()
    assert lib.mfsgd_warp_weights(None, None, 0) == OK
    assert lib.mfsgd_warp_weights(rank.ctypes.data_as(ip), w.ctypes.data_as(fp), 2) == OK and w.tolist() == [1.0, 1.5, UNTOUCHED, UNTOUCHED]
    with pytest.raises(mf.MfsgdError) as e:
        mf.warp_weights([3, -2])
    assert e.value.code == INVALID_ARG and "warp_weights: rank 1 is negative" in str(e.value)


# ---- mfsgd_sample_unseen_violating: the argument checks -----------------------------------------------------------------------
def _i32(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _viol(m, users, pos, n, per_row, margin=1.0, seed=0, first=0, out=True, extra=True):
    """(rc, message, untouched) of one raw call; untouched: every output array is still as it was."""
    uu = None if users is None else np.ascontiguousarray(users, np.int32)
    pp = None if pos is None else np.ascontiguousarray(pos, np.int32)
    items, draws, ranks = (np.full(64, UNTOUCHED, np.int32) for _ in range(3))
    margins = np.full(64, UNTOUCHED, np.float32)
    rc = m._lib.mfsgd_sample_unseen_violating(m._handle(), _i32(uu), _i32(pp), n, per_row, margin, seed, first,
                                              _i32(items) if out else None, _i32(draws) if extra else None,
                                              margins.ctypes.data_as(C.POINTER(C.c_float)) if extra else None,
                                              _i32(ranks) if extra else None)
    untouched = bool((items == UNTOUCHED).all() and (draws == UNTOUCHED).all() and (ranks == UNTOUCHED).all()
                     and (margins == UNTOUCHED).all())
    return rc, m._lib.mfsgd_last_error(m._h).decode(), untouched


@pytest.fixture
def bare(mf):
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        yield m


@pytest.fixture
def ready(bare):
    """An empty index and seeded factors: a valid state that needs no GPU to reach."""
    bare.set_seen([], [])
    bare.init_factors()
    return bare


def test_one_broken_argument_at_a_time(ready):
    m = ready
    for args, msg in ((dict(n=-1), "n is negative"),
                      (dict(per_row=0), "m is below 1"),
                      (dict(per_row=-1), "m is below 1"),
                      (dict(margin=float("nan")), "margin is NaN"),
                      (dict(first=-1), "first is negative"),
                      (dict(first=I64_MAX - 5), "first + n * m exceeds 2^63 - 1"),
                      (dict(n=1 << 62, per_row=2), "first + n * m exceeds 2^63 - 1"),
                      (dict(n=1 << 40, per_row=1 << 30), "first + n * m exceeds 2^63 - 1"),
                      (dict(users=None), "users, pos_items or out_items is null"),
                      (dict(pos=None), "users, pos_items or out_items is null"),
                      (dict(out=False), "users, pos_items or out_items is null"),
                      (dict(users=[0, U]), "row 1 out of range"),
                      (dict(users=[-1, 0]), "row 0 out of range"),
                      (dict(pos=[0, I]), "row 1 out of range"),
                      (dict(pos=[-1, 0]), "row 0 out of range")):
        kw = dict(users=[0, 1], pos=[2, 3], n=2, per_row=3)
        kw.update(args)
        rc, got, untouched = _viol(m, **kw)
        assert (rc, got) == (INVALID_ARG, PRE + msg), args
        assert untouched
    # the largest counter range there is, infinite margins and null optional outputs pass the checks
    want = OK if have_gpu() else NO_DEVICE
    assert _viol(m, [0, 1], [2, 3], 2, 3, first=I64_MAX - 6)[0] == want
    assert _viol(m, [0, 1], [2, 3], 2, 3, margin=float("inf"))[0] == want
    assert _viol(m, [0, 1], [2, 3], 2, 3, margin=float("-inf"))[0] == want
    assert _viol(m, [0, 1], [2, 3], 2, 3, extra=False)[0] == want


def test_the_checks_come_in_the_stated_order(mf, bare):
    m = bare
    nan = float("nan")
    # 1. the arguments before the state: n, then m, then the margin, then first and the overflow, then the null arrays
    assert _viol(m, None, None, -1, 0, margin=nan, first=-1)[1] == PRE + "n is negative"
    assert _viol(m, None, None, 2, 0, margin=nan, first=-1)[1] == PRE + "m is below 1"
    assert _viol(m, None, None, 2, 3, margin=nan, first=-1)[1] == PRE + "margin is NaN"
    assert _viol(m, None, None, 2, 3, first=-1)[1] == PRE + "first is negative"
    assert _viol(m, None, None, 2, 3, first=I64_MAX)[1] == PRE + "first + n * m exceeds 2^63 - 1"
    assert _viol(m, None, None, 1 << 62, 4, first=-1)[1] == PRE + "first is negative"  # (before the overflow)
    assert _viol(m, None, None, 2, 3)[:2] == (INVALID_ARG, PRE + "users, pos_items or out_items is null")
    assert _viol(m, None, None, 0, 3)[:2] == (STATE, PRE + "no seen set")  # (n == 0: null arrays are fine)
    # 2. the state, whatever n is and before the rows: the index, then the factors
    for n in (2, 0):
        assert _viol(m, [0, U], [0, I], n, 3)[:2] == (STATE, PRE + "no seen set")
    m.set_seen([], [])
    for n in (2, 0):
        assert _viol(m, [0, U], [0, I], n, 3)[:2] == (STATE, PRE + "factors not initialised")
    m.init_p_offset(1, 0)  # P alone
    for n in (2, 0):
        rc, msg, untouched = _viol(m, [0, U], [0, I], n, 3)
        assert rc == STATE and msg.startswith(PRE + "Q is not initialised") and untouched
    m.init_factors()
    # 3. n == 0 is fine and reads nothing
    rc, msg, untouched = _viol(m, [0, U], [0, I], 0, 3)
    assert rc == OK and untouched
    assert _viol(m, None, None, 0, 3, out=False, extra=False)[0] == OK
    # 4. then the rows, named: a user or a positive out of range
    for users, pos, row in (([0, U], [0, 0], 1), ([-1, 0], [0, 0], 0), ([0, 1, 2, 1 << 30], [0, 0, 0, 0], 3),
                            ([0, 1, 2], [0, I, -1], 1), ([0, 1, 2], [0, 1, 1 << 30], 2), ([0, U], [I, 0], 0)):
        rc, msg, untouched = _viol(m, users, pos, len(users), 3)
        assert (rc, msg) == (INVALID_ARG, PRE + f"row {row} out of range") and untouched
    # n_parts before the index and the factors: a partitioned handle has neither, and says the former
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as p:
        for n in (2, 0):
            assert _viol(p, [0, U], [0, I], n, 3)[:2] == (STATE, PRE + "single-partition handles only")
        assert _viol(p, None, None, 2, 3)[:2] == (INVALID_ARG, PRE + "users, pos_items or out_items is null")
        assert _viol(p, None, None, 2, 3, margin=nan)[1] == PRE + "margin is NaN"
        assert _viol(p, [0, U], [0, I], 2, 3, first=I64_MAX)[1] == PRE + "first + n * m exceeds 2^63 - 1"
    out = np.zeros(1, np.int32)
    assert mf.load_library().mfsgd_sample_unseen_violating(None, _i32(out), _i32(out), 1, 1, 1.0, 0, 0, _i32(out), None, None,
                                                           None) == INVALID_ARG


def test_nothing_to_do_touches_nothing(ready):
    m = ready
    assert m.sample_unseen_violating([], [], 3).shape == (0,) and m.sample_unseen_violating([], [], 3).dtype == np.int32
    items, draws, margins, ranks = m.sample_unseen_violating([], [], 2, draws=True, margins=True, ranks=True)
    assert (items.shape, draws.dtype, margins.dtype, ranks.dtype) == ((0,), np.int32, np.float32, np.int32)
    assert len(m.sample_unseen_violating([], [], 2, ranks=True)) == 2
    assert m.seen_size() == 0
    with pytest.raises(ValueError):
        m.sample_unseen_violating([0, 1], [1], 2)


@pytest.mark.skipif(have_gpu(), reason="checks the no-device error path")
def test_a_valid_call_needs_the_device_even_for_an_empty_index(ready):
    rc, msg, untouched = _viol(ready, [0, 1], [2, 3], 2, 3)
    assert rc == NO_DEVICE and "no CPU fallback" in msg and untouched
    with pytest.raises(Exception) as e:
        ready.sample_unseen_violating([0, 1], [2, 3], 3)
    assert e.value.code == NO_DEVICE
    with pytest.raises(Exception) as e:  # the first pick is what asks for the device
        ready.fit_warp([0, 1], [1, 2], 1, candidates=2)
    assert e.value.code == NO_DEVICE


def test_fit_warp_refuses_bad_arguments(bare):
    for kw in (dict(candidates=0), dict(candidates=-3), dict(candidates=4, refresh=0), dict(refresh=-1), dict(margin=float("nan"))):
        with pytest.raises(ValueError):
            bare.fit_warp([0, 1], [1, 2], 1, **kw)
    with pytest.raises(ValueError):
        bare.fit_warp([0, 1], [1, 2], -1)
    with pytest.raises(ValueError):
        bare.fit_warp([0, 1], [1], 1)
    assert bare.seen_size() == -1  # refused before anything was done


# ---- mfsgd_apply_triples_weighted: arguments and state ------------------------------------------------------------------------
def _ptr(a, dtype, ctype):
    """None stands for a NULL pointer."""
    return None if a is None else np.ascontiguousarray(a, dtype).ctypes.data_as(C.POINTER(ctype))


def _apply(m, u, i, j, w, n, info=None):
    """(rc, message, untouched) of one raw call that asks for the margins."""
    x = np.full(max(1, n, 8), UNTOUCHED, np.float32)
    ip = lambda a: _ptr(a, np.int32, C.c_int32)
    rc = m._lib.mfsgd_apply_triples_weighted(m._handle(), ip(u), ip(i), ip(j), _ptr(w, np.float32, C.c_float), n,
                                             x.ctypes.data_as(C.POINTER(C.c_float)), None if info is None else C.byref(info))
    return rc, m._lib.mfsgd_last_error(m._h).decode(), bool((x == UNTOUCHED).all())


BAD = [  # in the order the checks are made: each case passes every check before its own
    (dict(u=[0, 1], i=[0, 1], j=[1, 0], w=[1, 1], n=-1), "n is negative"),
    (dict(u=None, i=[0, 1], j=[1, 0], w=[1, 1], n=2), "u, i, j or w is null"),
    (dict(u=[0, 1], i=None, j=[1, 0], w=[1, 1], n=2), "u, i, j or w is null"),
    (dict(u=[0, 1], i=[0, 1], j=None, w=[1, 1], n=2), "u, i, j or w is null"),
    (dict(u=[0, 1], i=[0, 1], j=[1, 0], w=None, n=2), "u, i, j or w is null"),
    (dict(u=[0, 1, -1], i=[0, 1, 2], j=[1, 2, 3], w=[1, 1, 1], n=3), "triple 2 out of range"),
    (dict(u=[0, U, 1], i=[0, 1, 2], j=[1, 2, 3], w=[1, 1, 1], n=3), "triple 1 out of range"),
    (dict(u=[0, 1, 2], i=[-1, 1, 2], j=[1, 2, 3], w=[1, 1, 1], n=3), "triple 0 out of range"),
    (dict(u=[0, 1, 2], i=[0, 1, I], j=[1, 2, 3], w=[1, 1, 1], n=3), "triple 2 out of range"),
    (dict(u=[0, 1, 2], i=[0, 1, 2], j=[1, I, 3], w=[1, 1, 1], n=3), "triple 1 out of range"),
    (dict(u=[0, 1, 2], i=[0, 1, 2], j=[1, 1, 3], w=[1, 1, 1], n=3), "triple 1 has the same positive and negative item"),
    # a null array is reported before a range, a range before i == j, wherever in the list they are
    (dict(u=[0, U], i=[0, I], j=[0, 0], w=None, n=2), "u, i, j or w is null"),
    (dict(u=[0, 1, U], i=[1, 1, 2], j=[1, 2, 3], w=[1, 1, 1], n=3), "triple 2 out of range"),
]


@pytest.mark.parametrize("kw,msg", BAD)
def test_weighted_bad_arguments_are_invalid(ready, kw, msg):
    P0, Q0 = ready.get_factors()
    rc, got, untouched = _apply(ready, **kw)
    assert (rc, got) == (INVALID_ARG, PREW + msg) and untouched
    P, Q = ready.get_factors()
    assert P.tobytes() == P0.tobytes() and Q.tobytes() == Q0.tobytes()


def test_weighted_state_errors_and_nothing_to_apply(mf, bare):
    m = bare
    for n in (1, 0):  # factors never initialised, whatever n is
        rc, msg, _ = _apply(m, [0], [0], [1], [1.0], n)
        assert rc == STATE and msg.startswith(PREW) and "not initialised" in msg
    assert _apply(m, [U], [0], [1], [1.0], 1)[0] == INVALID_ARG  # an argument error comes first
    assert _apply(m, [0], [1], [1], [1.0], 1)[0] == INVALID_ARG
    m.init_p_offset(1, 0)  # P alone
    rc, msg, _ = _apply(m, [0], [0], [1], [1.0], 1)
    assert rc == STATE and msg.startswith(PREW + "Q is not initialised")
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as p:  # the handle does not hold Q
        p.init_factors()
        rc, msg, _ = _apply(p, [0], [0], [1], [1.0], 1)
        assert rc == STATE and msg.startswith(PREW) and "single-partition" in msg
    m.init_factors()
    P0, Q0 = m.get_factors()
    info = mf._lib.OnlineInfo(n=-1, pieces=-1, levels=-1, max_width=-1, launches=-1)
    rc, _, untouched = _apply(m, None, None, None, None, 0, info)
    assert rc == OK and untouched and info.as_dict() == dict(n=0, pieces=0, levels=0, max_width=0, launches=0)
    assert m.partial_fit_pairwise([], [], [], weights=[], margins=True).shape == (0,)
    assert m.partial_fit_pairwise([], [], [], weights=[]) is None
    with pytest.raises(ValueError):
        m.partial_fit_pairwise([0, 1], [0, 1], [1, 0], weights=[1.0])
    P, Q = m.get_factors()
    assert P.tobytes() == P0.tobytes() and Q.tobytes() == Q0.tobytes()
    assert m._lib.mfsgd_apply_triples_weighted(None, None, None, None, None, 0, None, None) == INVALID_ARG


def test_levels_and_info_of_the_weighted_call_are_the_triples(mf, ready):
    """Weights do not enter the levels: what the weighted call counts is what mfsgd_triple_levels counts on the list.  Without
    a GPU the call must refuse, and leave info alone, before it reports anything."""
    u, i, j = [0, 1, 0, 2, 1], [0, 1, 1, 2, 0], [1, 2, 3, 3, 4]
    w = [0.5, -1.0, 2.0, 0.0, 1.0]
    levels, want = ready.triple_levels(u, i, j)
    assert levels.tolist() == [0, 1, 2, 3, 2] and want["levels"] == 4
    info = mf._lib.OnlineInfo(n=-1, pieces=-1, levels=-1, max_width=-1, launches=-1)
    rc, msg, untouched = _apply(ready, u, i, j, w, 5, info)
    if have_gpu():
        got = info.as_dict()
        assert rc == OK and not untouched and got.pop("launches") >= 1 and want.pop("launches") == 0 and got == want
    else:
        assert rc == NO_DEVICE and "no CPU fallback" in msg and untouched and info.n == -1
        with pytest.raises(mf.MfsgdError) as e:
            ready.partial_fit_pairwise(u, i, j, weights=w)
        assert e.value.code == NO_DEVICE


def test_signatures_cover_the_new_names(mf):
    for name in ("mfsgd_sample_unseen_violating", "mfsgd_apply_triples_weighted", "mfsgd_warp_weights"):
        assert name in mf._lib.SIGNATURES
    assert "warp_weights" in mf.__all__
