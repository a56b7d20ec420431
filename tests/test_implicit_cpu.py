"""Negative sampling for implicit feedback, as far as it goes without a GPU: the numpy restatement of the draw
(tests/implicit_common.py) is what it claims to be -- the t-th unseen item, evenly spread -- and mfsgd_sample_unseen checks
its arguments before any device work, in the order include/mfsgd.h states, and never answers on the CPU."""
import ctypes as C

import numpy as np
import pytest

from tests import implicit_common as IC
from tests.conftest import have_gpu

OK, INVALID_ARG, NO_DEVICE, STATE = 0, -1, -2, -5
U, I, K = 6, 5, 8
I64_MAX = (1 << 63) - 1
UNTOUCHED = -77


# ---- the restatement ------------------------------------------------------------------------------------------------------
def test_the_restatement_is_the_t_th_unseen_item():
    rng = np.random.default_rng(5)
    cases = [(1, []), (1, [0]), (7, []), (7, [0]), (7, [6]), (7, [0, 1, 2, 3, 4, 5]), (7, [1, 2, 3, 4, 5, 6]), (7, list(range(7)))]
    for _ in range(200):
        n_items = int(rng.integers(1, 120))
        cases.append((n_items, np.sort(rng.choice(n_items, int(rng.integers(0, n_items + 1)), replace=False))))
    for n_items, S in cases:
        unseen = np.setdiff1d(np.arange(n_items), S)
        assert np.array_equal(IC.unseen_at(S, np.arange(unseen.size)), unseen), (n_items, S)


def test_the_mix_is_the_published_splitmix64():
    # seed 0, counter 0: the first output of splitmix64 seeded with 0, as its reference code gives it
    assert int(IC.mix32(0, np.array([0]))[0]) == 0xE220A8397B1DCDAF >> 32
    assert int(IC.mix32(0, np.array([1]))[0]) == 0x6E789E6AA1B965F4 >> 32
    # a negative seed is its two's complement; the counter wraps
    assert IC.mix32(-1, np.array([0]))[0] == IC.mix32((1 << 64) - 1, np.array([0]))[0]
    assert IC.mix32(3, np.array([(1 << 64) - 1], np.uint64))[0] == (IC.mix32(3 - 0x9E3779B97F4A7C15, np.array([0]))[0])


@pytest.mark.parametrize("seed", [0, 1, -5, 1 << 40])
def test_the_restatement_fills_seven_bins_evenly(seed):
    """cnt = 7 over 70 000 consecutive counters: a bin is binomial(70 000, 1/7), sigma = sqrt(70 000 * 1/7 * 6/7) = 92.6,
    and every bin must lie within 6 sigma of 10 000."""
    n_items, S = 10, np.array([2, 3, 9])
    for first in (0, 1 << 40):
        got = IC.draw(S, n_items, seed, first + np.arange(70_000))
        assert not np.isin(got, S).any() and got.min() >= 0 and got.max() < n_items
        bins = np.bincount(got, minlength=n_items)[np.setdiff1d(np.arange(n_items), S)]
        off = np.abs(bins - 10_000).max()
        print(f"seed {seed} first {first}: bins {bins.tolist()}, at most {off} off")
        assert off <= 6 * np.sqrt(70_000 * (1 / 7) * (6 / 7))


# ---- the argument checks -----------------------------------------------------------------------------------------------------
def _i32(a):
    return None if a is None else a.ctypes.data_as(C.POINTER(C.c_int32))


def _sample(m, users, n, per_row, seed=0, first=0, out=True):
    """(rc, message, out array) of one raw call; the out array starts as UNTOUCHED."""
    uu = None if users is None else np.ascontiguousarray(users, np.int32)
    got = np.full(64, UNTOUCHED, np.int32)
    rc = m._lib.mfsgd_sample_unseen(m._handle(), _i32(uu), n, per_row, seed, first, _i32(got) if out else None)
    return rc, m._lib.mfsgd_last_error(m._h).decode(), got


@pytest.fixture
def bare(mf):
    """Neither factors nor ratings: the call needs neither."""
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        yield m


@pytest.fixture
def indexed(bare):
    bare.set_seen([], [])  # an empty index: a valid state that needs no GPU
    return bare


def test_one_broken_argument_at_a_time(indexed):
    m = indexed
    for args, msg in ((dict(n=-1), "n is negative"),
                      (dict(per_row=-1), "m is negative"),
                      (dict(first=-1), "first is negative"),
                      (dict(first=I64_MAX - 5), "first + n * m exceeds 2^63 - 1"),
                      (dict(n=1 << 62, per_row=2), "first + n * m exceeds 2^63 - 1"),
                      (dict(n=1 << 40, per_row=1 << 30), "first + n * m exceeds 2^63 - 1"),
                      (dict(users=None), "users or out_items is null"),
                      (dict(out=False), "users or out_items is null")):
        kw = dict(users=[0, 1], n=2, per_row=3)
        kw.update(args)
        rc, got, out = _sample(m, **kw)
        assert (rc, got) == (INVALID_ARG, "sample_unseen: " + msg), args
        assert (out == UNTOUCHED).all()
    # the largest counter range there is passes the checks
    assert _sample(m, [0, 1], 2, 3, first=I64_MAX - 6)[0] == (OK if have_gpu() else NO_DEVICE)


def test_the_checks_come_in_the_stated_order(mf, bare):
    m = bare
    # 1. the arguments before the state: negative n or m, then first and the overflow, then the null arrays
    assert _sample(m, None, -1, -1, first=-1)[1] == "sample_unseen: n is negative"
    assert _sample(m, None, 2, -1, first=-1)[1] == "sample_unseen: m is negative"
    assert _sample(m, None, 2, 3, first=-1)[1] == "sample_unseen: first is negative"
    assert _sample(m, None, 2, 3, first=I64_MAX)[1] == "sample_unseen: first + n * m exceeds 2^63 - 1"
    assert _sample(m, None, 1 << 62, 4, first=-1)[1] == "sample_unseen: first is negative"  # (before the overflow)
    assert _sample(m, None, 2, 3)[:2] == (INVALID_ARG, "sample_unseen: users or out_items is null")
    # 3. then the missing index, before the users
    assert _sample(m, [0, U], 2, 3)[:2] == (STATE, "sample_unseen: no seen set")
    for n, per_row in ((0, 3), (2, 0)):  # ... and whatever n * m is, where null arrays are fine
        assert _sample(m, [0, U], n, per_row)[:2] == (STATE, "sample_unseen: no seen set")
        assert _sample(m, None, n, per_row, out=False)[:2] == (STATE, "sample_unseen: no seen set")
    m.set_seen([], [])
    assert _sample(m, [0, U], 0, 3)[0] == OK  # nothing to do comes before the users
    # 4. then the users, named by row
    for users, row in (([0, U], 1), ([-1, 0], 0), ([0, 1, 2, 1 << 30], 3)):
        rc, msg, out = _sample(m, users, len(users), 3)
        assert (rc, msg) == (INVALID_ARG, f"sample_unseen: user {row} out of range")
        assert (out == UNTOUCHED).all()
    # a bad user in the last position of a list longer than one block of the check names that position
    n = 3 * 4096 + 17
    users = np.arange(n, dtype=np.int32) % U
    users[-1] = U
    rc = m._lib.mfsgd_sample_unseen(m._handle(), _i32(users), n, 0, 0, 0, None)
    assert rc == OK  # (m == 0: nothing to do, nothing is read)
    out = np.full(n, UNTOUCHED, np.int32)
    rc = m._lib.mfsgd_sample_unseen(m._handle(), _i32(users), n, 1, 0, 0, _i32(out))
    assert (rc, m._lib.mfsgd_last_error(m._h).decode()) == (INVALID_ARG, f"sample_unseen: user {n - 1} out of range")
    assert (out == UNTOUCHED).all()
    # 2. n_parts before the index: a partitioned handle has none, and says the former
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as p:
        assert _sample(p, [0, U], 2, 3)[:2] == (STATE, "sample_unseen: single-partition handles only")
        assert _sample(p, None, 2, 3)[:2] == (INVALID_ARG, "sample_unseen: users or out_items is null")
        assert _sample(p, [0, U], 0, 3)[:2] == (STATE, "sample_unseen: single-partition handles only")
        assert _sample(p, [0, U], 2, 3, first=I64_MAX)[1] == "sample_unseen: first + n * m exceeds 2^63 - 1"
    assert mf.load_library().mfsgd_sample_unseen(None, _i32(users), 1, 1, 0, 0, _i32(out)) == INVALID_ARG


def test_nothing_to_do_is_ok_and_touches_nothing(indexed):
    m = indexed
    for n, per_row in ((0, 3), (2, 0), (0, 0)):
        rc, msg, out = _sample(m, [0, 1], n, per_row)
        assert rc == OK, msg
        assert (out == UNTOUCHED).all()
        assert _sample(m, None, n, per_row, out=False)[0] == OK  # null arrays are fine then
    assert m.sample_unseen([], 3).shape == (0, 3) and m.sample_unseen([0, 1], 0).shape == (2, 0)
    assert m.sample_unseen([0, 1], 0).dtype == np.int32
    assert m.seen_size() == 0


@pytest.mark.skipif(have_gpu(), reason="checks the no-device error path")
def test_a_valid_call_needs_the_device_even_for_an_empty_index(indexed):
    rc, msg, out = _sample(indexed, [0, 1], 2, 3)
    assert rc == NO_DEVICE and "no CPU fallback" in msg
    assert (out == UNTOUCHED).all()
    with pytest.raises(Exception) as e:
        indexed.sample_unseen([0, 1], 3)
    assert e.value.code == NO_DEVICE
    with pytest.raises(Exception) as e:  # fit_implicit keeps the index it finds and seeds the factors on the host: the
        indexed.fit_implicit([0, 1], [1, 2], 1)  # first draw is what asks for the device
    assert e.value.code == NO_DEVICE
