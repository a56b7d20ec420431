"""Hard negatives, as far as they go without a GPU: the numpy restatement of the pick (tests/hardneg_common.py) is what it
claims to be, mfsgd_sample_unseen_hard checks its arguments before any device work, in the order include/mfsgd.h states,
and never answers on the CPU, and fit_bpr refuses candidates and refresh below 1."""
import ctypes as C

import numpy as np
import pytest

from tests import hardneg_common as HC
from tests import implicit_common as IC
from tests.conftest import have_gpu

OK, INVALID_ARG, NO_DEVICE, STATE = 0, -1, -2, -5
U, I, K = 6, 5, 8
I64_MAX = (1 << 63) - 1
UNTOUCHED = -77
PRE = "sample_unseen_hard: "


# ---- the restatement ------------------------------------------------------------------------------------------------------
def _f(*x):
    return np.array(x, np.float32)


def test_the_pick_on_hand_made_tables():
    nan, inf = np.nan, np.inf
    table = np.stack([_f(1, 3, 2, 3),            # the first of two equal largest
                      _f(-0.0, 0.0, -0.0, 0.0),  # -0.0 == +0.0: the smaller d
                      _f(0.0, -0.0, 0.0, -0.0),
                      _f(nan, -5, nan, -7),      # a NaN loses to every number
                      _f(nan, nan, nan, nan),    # nothing but NaNs: d = 0
                      _f(nan, -inf, nan, -inf),  # ... also to -inf, and then the smaller d
                      _f(-inf, nan, -inf, inf),
                      _f(inf, inf, nan, 1),
                      _f(-3, -2, -1, nan),
                      _f(nan, nan, nan, -inf)])
    assert HC.pick(table).tolist() == [1, 0, 0, 1, 0, 1, 3, 0, 2, 3]
    assert HC.pick(table).dtype == np.int32
    assert HC.pick(_f(nan, 4, nan).reshape(3, 1)).tolist() == [0, 0, 0]  # m = 1: there is one candidate
    # the rule does not depend on the order of examination: the pick of a permuted row is the smallest d among the
    # positions that hold a score equal to the picked one (or, for a row of NaNs, position 0)
    rng = np.random.default_rng(2)
    pool = _f(nan, -inf, inf, -0.0, 0.0, 1, 1, -2, 7, 7)
    for _ in range(300):
        row = pool[rng.integers(0, pool.size, int(rng.integers(1, 9)))]
        d = int(HC.pick(row[None])[0])
        if np.isnan(row).all():
            assert d == 0
        else:
            best = np.nanmax(row)
            assert row[d] == best and not (row[:d] == best).any()


def test_picks_are_the_draws_and_never_seen():
    rng = np.random.default_rng(7)
    n_users, n_items, k = 9, 40, 5
    pu, pi = rng.integers(0, n_users - 1, 150), rng.integers(0, n_items, 150)
    pu, pi = np.concatenate([pu, np.full(n_items, n_users - 1)]), np.concatenate([pi, np.arange(n_items)])  # one has seen all
    lists = IC.lists_of(pu, pi)
    P, Q = rng.standard_normal((n_users, k)).astype(np.float32), rng.standard_normal((n_items, k)).astype(np.float32)
    scorer = lambda u, i: np.einsum("xf,xf->x", P[u], Q[i]).astype(np.float32)
    users = rng.integers(0, n_users, 500).astype(np.int32)
    for m in (1, 3, 8):
        items, scores, draws = HC.hard(lists, n_items, users, m, 11, 1000, scorer)
        cand = IC.sample(lists, n_items, users, m, 11, 1000)
        full = users == n_users - 1
        assert (items[full] == -1).all() and (draws[full] == -1).all() and (scores.view(np.uint32)[full] == HC.NAN_BITS).all()
        rows = np.flatnonzero(~full)
        assert np.array_equal(items[rows], cand[rows, draws[rows]]) and (draws[rows] >= 0).all() and (draws[rows] < m).all()
        assert not np.isin((users[rows].astype(np.int64) << 32) | items[rows], (pu.astype(np.int64) << 32) | pi).any()
        assert np.array_equal(scores[rows], scorer(users[rows], items[rows]))
        assert (scores[rows, None] >= scorer(np.repeat(users[rows], m), cand[rows].ravel()).reshape(-1, m)).all()
        if m == 1:  # m = 1 is the draw
            assert np.array_equal(items, cand[:, 0]) and (draws[rows] == 0).all()
    # rows [a, b) of a call are the call on users[a:b] with first + a * m
    whole = HC.hard(lists, n_items, users, 3, 11, 1000, scorer)
    part = HC.hard(lists, n_items, users[100:230], 3, 11, 1000 + 100 * 3, scorer)
    for w, p in zip(whole, part):
        assert w[100:230].tobytes() == p.tobytes()


# ---- the argument checks -----------------------------------------------------------------------------------------------------
def _i32(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _hard(m, users, n, per_row, seed=0, first=0, out=True, extra=True):
    """(rc, message, untouched) of one raw call; untouched: every output array is still as it was."""
    uu = None if users is None else np.ascontiguousarray(users, np.int32)
    items, draws = np.full(64, UNTOUCHED, np.int32), np.full(64, UNTOUCHED, np.int32)
    scores = np.full(64, UNTOUCHED, np.float32)
    rc = m._lib.mfsgd_sample_unseen_hard(m._handle(), _i32(uu), n, per_row, seed, first, _i32(items) if out else None,
                                         scores.ctypes.data_as(C.POINTER(C.c_float)) if extra else None,
                                         _i32(draws) if extra else None)
    untouched = bool((items == UNTOUCHED).all() and (draws == UNTOUCHED).all() and (scores == UNTOUCHED).all())
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
                      (dict(first=-1), "first is negative"),
                      (dict(first=I64_MAX - 5), "first + n * m exceeds 2^63 - 1"),
                      (dict(n=1 << 62, per_row=2), "first + n * m exceeds 2^63 - 1"),
                      (dict(n=1 << 40, per_row=1 << 30), "first + n * m exceeds 2^63 - 1"),
                      (dict(users=None), "users or out_items is null"),
                      (dict(out=False), "users or out_items is null"),
                      (dict(users=[0, U]), "user 1 out of range"),
                      (dict(users=[-1, 0]), "user 0 out of range")):
        kw = dict(users=[0, 1], n=2, per_row=3)
        kw.update(args)
        rc, got, untouched = _hard(m, **kw)
        assert (rc, got) == (INVALID_ARG, PRE + msg), args
        assert untouched
    # the largest counter range there is passes the checks, and so do null out_scores and out_draw
    want = OK if have_gpu() else NO_DEVICE
    assert _hard(m, [0, 1], 2, 3, first=I64_MAX - 6)[0] == want
    assert _hard(m, [0, 1], 2, 3, extra=False)[0] == want


def test_the_checks_come_in_the_stated_order(mf, bare):
    m = bare
    # 1 - 4. the arguments before the state: n, then m, then first and the overflow, then the null arrays
    assert _hard(m, None, -1, 0, first=-1)[1] == PRE + "n is negative"
    assert _hard(m, None, 2, 0, first=-1)[1] == PRE + "m is below 1"
    assert _hard(m, None, 2, 3, first=-1)[1] == PRE + "first is negative"
    assert _hard(m, None, 2, 3, first=I64_MAX)[1] == PRE + "first + n * m exceeds 2^63 - 1"
    assert _hard(m, None, 1 << 62, 4, first=-1)[1] == PRE + "first is negative"  # (before the overflow)
    assert _hard(m, None, 2, 3)[:2] == (INVALID_ARG, PRE + "users or out_items is null")
    assert _hard(m, None, 0, 3)[:2] == (STATE, PRE + "no seen set")  # (n == 0: null arrays are fine)
    # 5. the state, whatever n is and before the users: the index, then the factors
    for n in (2, 0):
        assert _hard(m, [0, U], n, 3)[:2] == (STATE, PRE + "no seen set")
    m.set_seen([], [])
    for n in (2, 0):
        assert _hard(m, [0, U], n, 3)[:2] == (STATE, PRE + "factors not initialised")
    m.init_p_offset(1, 0)  # P alone
    for n in (2, 0):
        rc, msg, untouched = _hard(m, [0, U], n, 3)
        assert rc == STATE and msg.startswith(PRE + "Q is not initialised") and untouched
    m.init_factors()
    # 6. n == 0 is fine and reads nothing
    rc, msg, untouched = _hard(m, [0, U], 0, 3)
    assert rc == OK and untouched
    assert _hard(m, None, 0, 3, out=False, extra=False)[0] == OK
    # 7. then the users, named by row
    for users, row in (([0, U], 1), ([-1, 0], 0), ([0, 1, 2, 1 << 30], 3)):
        rc, msg, untouched = _hard(m, users, len(users), 3)
        assert (rc, msg) == (INVALID_ARG, PRE + f"user {row} out of range") and untouched
    # n_parts before the index and the factors: a partitioned handle has neither, and says the former
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as p:
        for n in (2, 0):
            assert _hard(p, [0, U], n, 3)[:2] == (STATE, PRE + "single-partition handles only")
        assert _hard(p, None, 2, 3)[:2] == (INVALID_ARG, PRE + "users or out_items is null")
        assert _hard(p, None, 2, 0)[1] == PRE + "m is below 1"
        assert _hard(p, [0, U], 2, 3, first=I64_MAX)[1] == PRE + "first + n * m exceeds 2^63 - 1"
    out = np.zeros(1, np.int32)
    assert mf.load_library().mfsgd_sample_unseen_hard(None, _i32(out), 1, 1, 0, 0, _i32(out), None, None) == INVALID_ARG


def test_nothing_to_do_touches_nothing(ready):
    m = ready
    assert m.sample_unseen_hard([], 3).shape == (0,) and m.sample_unseen_hard([], 3).dtype == np.int32
    items, scores, draws = m.sample_unseen_hard([], 2, scores=True, draws=True)
    assert (items.shape, scores.dtype, draws.dtype) == ((0,), np.float32, np.int32)
    assert len(m.sample_unseen_hard([], 2, draws=True)) == 2
    assert m.seen_size() == 0


@pytest.mark.skipif(have_gpu(), reason="checks the no-device error path")
def test_a_valid_call_needs_the_device_even_for_an_empty_index(ready):
    rc, msg, untouched = _hard(ready, [0, 1], 2, 3)
    assert rc == NO_DEVICE and "no CPU fallback" in msg and untouched
    with pytest.raises(Exception) as e:
        ready.sample_unseen_hard([0, 1], 3)
    assert e.value.code == NO_DEVICE
    with pytest.raises(Exception) as e:  # the first pick is what asks for the device
        ready.fit_bpr([0, 1], [1, 2], 1, candidates=2)
    assert e.value.code == NO_DEVICE


def test_fit_bpr_refuses_candidates_and_refresh_below_one(bare):
    for kw in (dict(candidates=0), dict(candidates=-3), dict(candidates=4, refresh=0), dict(refresh=0), dict(refresh=-1)):
        with pytest.raises(ValueError):
            bare.fit_bpr([0, 1], [1, 2], 1, **kw)
    assert bare.seen_size() == -1  # refused before anything was done
