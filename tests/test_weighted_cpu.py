"""Weighted negatives, as far as they go without a GPU: the numpy restatement of the draw (tests/weighted_common.py) is what
it claims to be -- every unseen item x comes out for exactly w[x] ranks, in ascending order -- popularity_weights computes
what it documents, and the five calls check their arguments before any device work, in the order include/mfsgd.h states."""
import ctypes as C

import numpy as np
import pytest

from tests import implicit_common as IC
from tests import weighted_common as WC
from tests.conftest import have_gpu

OK, INVALID_ARG, NO_DEVICE, STATE = 0, -1, -2, -5
U, I, K = 6, 5, 8
I64_MAX = (1 << 63) - 1
UNTOUCHED = -77


# ---- the restatement ------------------------------------------------------------------------------------------------------
def _cases():
    """(w, S): the corners by hand, then 240 random ones -- n_items <= 24, weights 0 .. 4, s from 0 to n_items."""
    cases = [([1], []), ([1], [0]), ([0], []), ([0, 0, 0], [1]), ([0, 3, 0], []), ([0, 3, 0], [1]), ([2, 0, 0, 5], [0]),
             ([2, 0, 0, 5], [3]), ([4, 4, 4, 4], [0, 1, 2, 3]), ([0, 1, 0, 1, 0], [1]), ([3, 0, 2], [1])]
    rng = np.random.default_rng(11)
    for x in range(240):
        n_items = int(rng.integers(1, 25))
        w = rng.integers(0, 5, n_items)
        if x % 7 == 0:
            w[rng.integers(0, n_items, n_items // 2 + 1)] = 0  # runs of zeros
        s = int(rng.integers(0, n_items + 1)) if x % 5 else (0, n_items)[x % 2]
        cases.append((w, np.sort(rng.choice(n_items, s, replace=False))))
    return [(np.asarray(w, np.int64), np.asarray(S, np.int64)) for w, S in cases]


def test_every_rank_gives_the_unseen_items_repeated_by_weight_in_order():
    cases = _cases()
    assert len(cases) >= 200
    for w, S in cases:
        unseen = np.setdiff1d(np.arange(w.size), S)
        want = np.repeat(unseen, w[unseen])
        cnt = WC.unseen_mass(S, w)
        assert cnt == want.size == int(w.sum() - w[S].sum()), (w, S)
        g = WC.mass_below(S, w)
        assert np.array_equal(g, [int(w[:x].sum() - w[S[S < x]].sum()) for x in S]) and (np.diff(g.astype(np.int64)) >= 0).all()
        assert np.array_equal(WC.weighted_at(S, w, np.arange(cnt)), want), (w, S)
        # every draw is such a rank: unseen, and of positive weight (or -1 when there is no unseen weight)
        got = WC.draw_weighted(S, w, 3, np.arange(50))
        assert (got == -1).all() if cnt == 0 else (np.isin(got, unseen) & (w[got] > 0)).all(), (w, S)


def test_unit_weights_give_the_uniform_rule():
    for w, S in _cases():
        ones = np.ones(w.size, np.int64)
        t = np.arange(w.size - S.size)
        assert WC.unseen_mass(S, ones) == t.size
        assert np.array_equal(WC.weighted_at(S, ones, t), IC.unseen_at(S, t)), S


def test_the_rank_lies_below_the_mass_and_is_the_128_bit_product():
    rng = np.random.default_rng(2)
    z = np.array([0, 1, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, 1 << 63, IC.M64 - 1, IC.M64] +
                 [int(x) for x in rng.integers(0, 1 << 63, 200)] + [int(x) | (1 << 63) for x in rng.integers(0, 1 << 63, 200)],
                 dtype=np.uint64)
    for cnt in (1, 3, (1 << 40) + 7, (1 << 63) - 1):
        t = WC.mulhi64(z, cnt)
        assert t.dtype == np.uint64 and [int(x) for x in t] == [(int(x) * cnt) >> 64 for x in z]
        assert int(t.max()) < cnt and int(WC.mulhi64(WC.mix64(5, np.arange(5000)), cnt).max()) < cnt


def test_the_mix_is_the_published_splitmix64_all_64_bits():
    assert int(WC.mix64(0, 0)) == 0xE220A8397B1DCDAF
    assert int(WC.mix64(0, np.array([1]))[0]) == 0x6E789E6AA1B965F4
    c = np.array([0, 1, 77, 1 << 40, IC.M64], np.uint64)
    for seed in (0, 1, -5, 1 << 40):
        assert np.array_equal(WC.mix64(seed, c) >> np.uint64(32), IC.mix32(seed, c))


def test_sample_weighted_counts_as_the_uniform_sample_does():
    """Row x, draw d: the counter first + x * m + d whatever the order of the users; the mass is the row's user's."""
    w = np.array([3, 0, 1, 4, 0, 2], np.int64)
    lists = IC.lists_of([0, 0, 2, 2, 2], [1, 3, 0, 2, 5])
    users, m, seed, first = np.array([2, 0, 1, 2], np.int32), 3, 9, 1 << 40
    got, mass = WC.sample_weighted(lists, w, users, m, seed, first, mass=True)
    assert got.dtype == np.int32 and got.shape == (4, 3) and mass.tolist() == [4, 6, 10, 4]
    for x, u in enumerate(users):
        assert np.array_equal(got[x], WC.draw_weighted(lists(int(u)), w, seed, first + x * m + np.arange(m)))


# ---- popularity_weights -----------------------------------------------------------------------------------------------------
def test_popularity_weights(mf):
    pw = mf.popularity_weights
    counts = np.array([0, 1, 4, 9, 10_000, 1 << 20], np.int64)
    got = pw(counts, alpha=0.5)
    assert got.dtype == np.uint32 and got.tolist() == [1, 16, 32, 48, 1600, 16 << 10]  # least = 1 lifts the zero
    assert pw(counts, alpha=0.5, least=0).tolist() == [0, 16, 32, 48, 1600, 16 << 10]
    assert pw(counts, alpha=0).tolist() == [16] * 6  # 0 ** 0 = 1: the uniform draw
    assert pw(counts, alpha=1, resolution=3).tolist() == [1, 3, 12, 27, 30_000, 3 << 20]
    assert pw(counts, alpha=1, resolution=1, least=5).tolist() == [5, 5, 5, 9, 10_000, 1 << 20]
    assert pw([7, 8], alpha=1, resolution=0.5, least=0).tolist() == [4, 4]  # rint: halves go to the even neighbour
    want = np.maximum(1, np.rint(16 * np.arange(50, dtype=np.float64) ** 0.75)).astype(np.uint32)
    assert np.array_equal(pw(np.arange(50)), want) and pw([]).shape == (0,)
    assert pw([(1 << 28) - 1], alpha=1).tolist() == [0xFFFFFFF0]  # the largest weight but 15; 16 * 2^28 is one too many
    for bad in (dict(counts=[-1]), dict(counts=[1], alpha=np.nan), dict(counts=[1], alpha=np.inf), dict(counts=[1], alpha=-np.inf),
                dict(counts=[1 << 28], alpha=1), dict(counts=[0], alpha=-1), dict(counts=[1], least=-1),
                dict(counts=[1], least=1 << 32), dict(counts=[[1, 2]])):
        kw = dict(bad)
        with pytest.raises(ValueError):
            pw(kw.pop("counts"), **kw)


# ---- the argument checks -----------------------------------------------------------------------------------------------------
def _ptr(a, t):
    return None if a is None else a.ctypes.data_as(C.POINTER(t))


def _msg(m):
    return m._lib.mfsgd_last_error(m._h).decode()


def _set(m, w, n):
    ww = None if w is None else np.ascontiguousarray(w, np.uint32)
    return m._lib.mfsgd_set_item_weights(m._handle(), _ptr(ww, C.c_uint32), n), _msg(m)


def _sample(m, users, n, per_row, seed=0, first=0, out=True, mass=False):
    """(rc, message, out array, mass array) of one raw call; the arrays start as UNTOUCHED."""
    uu = None if users is None else np.ascontiguousarray(users, np.int32)
    got, ms = np.full(64, UNTOUCHED, np.int32), np.full(64, UNTOUCHED, np.int64)
    rc = m._lib.mfsgd_sample_unseen_weighted(m._handle(), _ptr(uu, C.c_int32), n, per_row, seed, first,
                                             _ptr(got, C.c_int32) if out else None, _ptr(ms, C.c_int64) if mass else None)
    return rc, _msg(m), got, ms


@pytest.fixture
def bare(mf):
    """Neither factors nor ratings: the calls need neither."""
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        yield m


def test_set_item_weights_checks_its_arguments_first(mf, bare):
    m = bare
    w = np.arange(I, dtype=np.uint32)
    assert _set(m, w, -1) == (INVALID_ARG, "set_item_weights: n is negative")
    assert _set(m, None, -1) == (INVALID_ARG, "set_item_weights: n is negative")
    assert _set(m, None, I) == (INVALID_ARG, "set_item_weights: w is null")
    assert _set(m, None, I + 1) == (INVALID_ARG, "set_item_weights: w is null")
    for n in (0, I - 1, I + 1):
        assert _set(m, np.zeros(I + 1, np.uint32), n) == (INVALID_ARG, f"set_item_weights: n is {n}, the model has {I} items")
    assert m.item_weights() is None
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as p:
        assert _set(p, w, I) == (STATE, "set_item_weights: single-partition handles only")
        assert _set(p, None, I)[0] == INVALID_ARG
    assert mf.load_library().mfsgd_set_item_weights(None, _ptr(w, C.c_uint32), I) == INVALID_ARG
    # the wrapper refuses what is no uint32 before the library sees it
    for bad in ([-1, 0, 0, 0, 0], [1 << 32, 0, 0, 0, 0], [0.5] * I, [[1] * I]):
        with pytest.raises(ValueError):
            m.set_item_weights(bad)
    # a valid call needs the device, as set_seen does for n > 0; with one the weights come back as set
    live = mf.debug_device_bytes()
    rc, msg = _set(m, w, I)
    if have_gpu():
        assert rc == OK, msg
        assert m.item_weights().dtype == np.uint32 and np.array_equal(m.item_weights(), w)
        m.set_item_weights([0xFFFFFFFF] * I)
        assert m.item_weights().tolist() == [0xFFFFFFFF] * I
        m.clear_item_weights()
    else:
        assert rc == NO_DEVICE and "no CPU fallback" in msg
    assert m.item_weights() is None and mf.debug_device_bytes() == live


def test_get_clear_and_counts_check_theirs(mf, bare):
    m, lib = bare, bare._lib
    n = C.c_int32(UNTOUCHED)
    w = np.full(I, 7, np.uint32)
    assert lib.mfsgd_get_item_weights(m._handle(), _ptr(w, C.c_uint32), None) == INVALID_ARG
    assert _msg(m) == "get_item_weights: n is null"
    assert lib.mfsgd_get_item_weights(m._handle(), _ptr(w, C.c_uint32), C.byref(n)) == OK
    assert n.value == -1 and (w == 7).all()  # none: nothing is written
    assert lib.mfsgd_clear_item_weights(m._handle()) == OK  # nothing to drop is fine
    counts = np.full(I, UNTOUCHED, np.int64)
    assert lib.mfsgd_seen_item_counts(m._handle(), None) == INVALID_ARG and _msg(m) == "seen_item_counts: counts is null"
    assert lib.mfsgd_seen_item_counts(m._handle(), _ptr(counts, C.c_int64)) == STATE and _msg(m) == "seen_item_counts: no seen set"
    assert (counts == UNTOUCHED).all()
    m.set_seen([], [])  # an empty index: zeros, on the host alone
    assert m.seen_item_counts().dtype == np.int64 and m.seen_item_counts().tolist() == [0] * I
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as p:
        for rc in (lib.mfsgd_get_item_weights(p._handle(), None, C.byref(n)), lib.mfsgd_clear_item_weights(p._handle()),
                   lib.mfsgd_seen_item_counts(p._handle(), _ptr(counts, C.c_int64))):
            assert rc == STATE and _msg(p).endswith("single-partition handles only")
        assert lib.mfsgd_seen_item_counts(p._handle(), None) == INVALID_ARG
    null = mf.load_library()
    assert null.mfsgd_get_item_weights(None, None, C.byref(n)) == INVALID_ARG and null.mfsgd_clear_item_weights(None) == INVALID_ARG
    assert null.mfsgd_seen_item_counts(None, _ptr(counts, C.c_int64)) == INVALID_ARG


def test_the_weighted_draw_one_broken_argument_at_a_time(bare):
    m = bare
    m.set_seen([], [])
    for args, msg in ((dict(n=-1), "n is negative"),
                      (dict(per_row=-1), "m is negative"),
                      (dict(first=-1), "first is negative"),
                      (dict(first=I64_MAX - 5), "first + n * m exceeds 2^63 - 1"),
                      (dict(n=1 << 62, per_row=2), "first + n * m exceeds 2^63 - 1"),
                      (dict(n=1 << 40, per_row=1 << 30), "first + n * m exceeds 2^63 - 1"),
                      (dict(users=None), "users or out_items is null"),
                      (dict(out=False), "users or out_items is null")):
        kw = dict(users=[0, 1], n=2, per_row=3, mass=True)
        kw.update(args)
        rc, got, out, ms = _sample(m, **kw)
        assert (rc, got) == (INVALID_ARG, "sample_unseen_weighted: " + msg), args
        assert (out == UNTOUCHED).all() and (ms == UNTOUCHED).all()


def test_the_weighted_draw_checks_in_the_stated_order(mf, bare):
    m = bare
    call = "sample_unseen_weighted: "
    # 1. the arguments before the state
    assert _sample(m, None, -1, -1, first=-1)[1] == call + "n is negative"
    assert _sample(m, None, 2, -1, first=-1)[1] == call + "m is negative"
    assert _sample(m, None, 2, 3, first=-1)[1] == call + "first is negative"
    assert _sample(m, None, 2, 3, first=I64_MAX)[1] == call + "first + n * m exceeds 2^63 - 1"
    assert _sample(m, None, 1 << 62, 4, first=-1)[1] == call + "first is negative"  # (before the overflow)
    assert _sample(m, None, 2, 3)[:2] == (INVALID_ARG, call + "users or out_items is null")
    # 2. no index, then no weights: both before the users, and whatever n * m is
    assert _sample(m, [0, U], 2, 3)[:2] == (STATE, call + "no seen set")
    assert _sample(m, [0, U], 0, 3)[:2] == (STATE, call + "no seen set")
    m.set_seen([], [])
    assert _sample(m, [0, U], 2, 3)[:2] == (STATE, call + "no item weights")
    assert _sample(m, None, 0, 0, out=False)[:2] == (STATE, call + "no item weights")
    with pytest.raises(mf.MfsgdError) as e:
        m.sample_unseen_weighted([0, 1], 2)
    assert e.value.code == STATE and "no item weights" in str(e.value)
    for fit in (lambda: m.fit_implicit([0, 1], [1, 2], 1, sampling="weighted"), lambda: m.fit_bpr([0, 1], [1, 2], 1, sampling="weighted")):
        with pytest.raises(mf.MfsgdError) as e:  # the first draw is what asks, after the factors were seeded on the host
            fit()
        assert e.value.code == STATE and "no item weights" in str(e.value)
    # n_parts before either
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as p:
        assert _sample(p, [0, U], 2, 3)[:2] == (STATE, call + "single-partition handles only")
        assert _sample(p, None, 2, 3)[:2] == (INVALID_ARG, call + "users or out_items is null")
        assert _sample(p, [0, U], 0, 3)[:2] == (STATE, call + "single-partition handles only")
        assert _sample(p, [0, U], 2, 3, first=I64_MAX)[1] == call + "first + n * m exceeds 2^63 - 1"
    out = np.zeros(4, np.int32)
    assert mf.load_library().mfsgd_sample_unseen_weighted(None, _ptr(out, C.c_int32), 1, 1, 0, 0, _ptr(out, C.c_int32), None) == INVALID_ARG
    if not have_gpu():
        return
    # 3. with weights (they need the device): stale weights, then nothing to do, then the users, named by row
    m.set_item_weights(np.ones(I, np.uint32))
    for n, per_row in ((0, 3), (2, 0), (0, 0)):
        rc, msg, out, ms = _sample(m, [0, 1], n, per_row, mass=True)
        assert rc == OK and (out == UNTOUCHED).all() and (ms == UNTOUCHED).all(), msg
        assert _sample(m, None, n, per_row, out=False)[0] == OK
        assert _sample(m, [0, U], n, per_row)[0] == OK  # nothing to do comes before the users
    for users, row in (([0, U], 1), ([-1, 0], 0), ([0, 1, 2, 1 << 30], 3)):
        rc, msg, out, ms = _sample(m, users, len(users), 3, mass=True)
        assert (rc, msg) == (INVALID_ARG, call + f"user {row} out of range")
        assert (out == UNTOUCHED).all() and (ms == UNTOUCHED).all()
    m.init_factors()
    m.add_items(n=2)
    assert _sample(m, [0, U], 2, 3)[:2] == (STATE, call + f"item weights cover {I} items, the model has {I + 2}")
    assert _sample(m, [0, 1], 0, 3)[0] == STATE


def test_the_keyword_of_the_fits(mf, bare):
    m = bare
    for fit in (m.fit_implicit, m.fit_bpr):
        for bad in ("popular", "", None, "Weighted"):
            with pytest.raises(ValueError):
                fit([0, 1], [1, 2], 1, sampling=bad)
    with pytest.raises(ValueError):
        m.fit_bpr([0, 1], [1, 2], 1, candidates=2, sampling="weighted")
    assert m.seen_size() == -1  # refused before anything was touched


def test_an_empty_index_plus_weights_holds_only_the_prefix(mf, bare):
    """g exists exactly when the handle has weights and an index with pairs: an empty index has none.  Without a device
    the weights cannot be set and nothing is held at all."""
    m = bare
    live = mf.debug_device_bytes()
    m.set_seen([], [])
    if not have_gpu():
        with pytest.raises(mf.MfsgdError) as e:
            m.set_item_weights(np.ones(I, np.uint32))
        assert e.value.code == NO_DEVICE and mf.debug_device_bytes() == live and m.item_weights() is None
        return
    m.set_item_weights(np.ones(I, np.uint32))
    assert mf.debug_device_bytes() == live + 8 * (I + 1)
    m.mark_seen([], [])
    m.set_seen([], [])
    assert mf.debug_device_bytes() == live + 8 * (I + 1) and m.item_weights().tolist() == [1] * I
    m.clear_item_weights()
    assert mf.debug_device_bytes() == live
