"""Weighted picks, as far as they go without a GPU: the restatements of tests/weighted_pick_common.py against exhaustive
enumeration in plain Python integers; the checks of mfsgd_sample_unseen_hard_weighted,
mfsgd_sample_unseen_violating_weighted and mfsgd_fold_in_users_pairwise_weighted before any device work, one broken
argument at a time and in the order include/mfsgd.h states; and the keyword rules of the four Python methods.
Item weights need the device to be set (mfsgd_set_item_weights), so on a machine without one every weighted call of a
handle ends at "no item weights": the checks behind it -- stale weights, the factor state, nothing to do, the ranges --
are checked where a GPU is, and MFSGD_ERR_NO_DEVICE for an otherwise valid call is a state no handle can reach."""
import ctypes as C

import numpy as np
import pytest

from tests import fold_in_pairwise_common as FC
from tests import implicit_common as IC
from tests import weighted_pick_common as WP
from tests.conftest import have_gpu

OK, INVALID_ARG, NO_DEVICE, STATE = 0, -1, -2, -5
U, I, K = 6, 5, 8
I64_MAX = (1 << 63) - 1
UNTOUCHED = -77
HARD, VIOL, FOLD = "sample_unseen_hard_weighted: ", "sample_unseen_violating_weighted: ", "fold_in_pairwise_weighted: "
M64 = (1 << 64) - 1


# ---- the restatements against enumeration ---------------------------------------------------------------------------------------
def _mix(seed, c):
    z = (seed + 0x9E3779B97F4A7C15 * (c + 1)) & M64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def _draw(S, w, seed, c):
    """The weighted draw by walking the unseen items in ascending order: the item whose stretch of the unseen weight holds
    t = (z * cnt) >> 64; -1 when there is no unseen weight."""
    unseen = [x for x in range(len(w)) if x not in set(S)]
    cnt = sum(int(w[x]) for x in unseen)
    if cnt == 0:
        return -1, 0
    t = (_mix(seed, c) * cnt) >> 64
    for x in unseen:
        if t < int(w[x]):
            return x, cnt
        t -= int(w[x])
    raise AssertionError("t is below cnt")


def _best(sc):
    """The hard pick written as a loop over ascending d."""
    best = 0
    for d in range(1, len(sc)):
        if sc[d] > sc[best] or (np.isnan(sc[best]) and not np.isnan(sc[d])):
            best = d
    return best


def _case(seed):
    """Lists, weights with zeros and a score table with ties, NaNs and infinities for I <= 12 items."""
    rng = np.random.default_rng(seed)
    n_items, n_users = int(rng.integers(1, 13)), 7
    w = rng.integers(0, 4, n_items).astype(np.uint32) * rng.integers(1, 1 << 30, n_items).astype(np.uint32)
    sets = [sorted(rng.choice(n_items, int(rng.integers(0, n_items + 1)), replace=False).tolist()) for _ in range(n_users)]
    sets[0], sets[1] = [], list(range(n_items))  # nothing seen; everything seen
    sets[2] = [x for x in range(n_items) if w[x] > 0]  # everything of positive weight seen: unseen items may remain
    table = rng.integers(-2, 3, (n_users, n_items)).astype(np.float32)
    table[rng.random(table.shape) < 0.15] = np.nan
    table[rng.random(table.shape) < 0.05] = np.inf
    table[rng.random(table.shape) < 0.05] = -np.inf
    table[3] = np.nan
    lists = lambda u: np.asarray(sets[u], np.int64)
    scorer = lambda u, i: table[u, i]
    return n_items, n_users, w, sets, lists, table, scorer


@pytest.mark.parametrize("case", range(12))
def test_the_restated_picks_against_enumeration(case):
    n_items, n_users, w, sets, lists, table, scorer = _case(case)
    rng = np.random.default_rng(100 + case)
    users = rng.integers(0, n_users, 40).astype(np.int32)
    pos = rng.integers(0, n_items, users.size).astype(np.int32)
    seed, first = 17 + case, (1 << 40) + case
    for m in (1, 2, 5, 9):
        items, scores, draws, mass = WP.hard(lists, w, users, m, seed, first, scorer)
        for margin in (0.5, -np.inf, np.inf):
            v_items, v_draws, v_margins, v_ranks, v_mass = WP.violating(lists, w, n_items, users, pos, m, margin, seed, first, scorer)
            assert np.array_equal(v_mass, mass)
            for x, u in enumerate(users):
                cand = [_draw(sets[u], w, seed, first + x * m + d) for d in range(m)]
                cnt = cand[0][1]
                assert mass[x] == cnt and all(c[1] == cnt for c in cand)
                if cnt == 0:
                    assert (items[x], draws[x], scores.view(np.uint32)[x]) == (-1, -1, WP.NAN_BITS)
                    assert (v_items[x], v_draws[x], v_margins.view(np.uint32)[x], v_ranks[x]) == (-1, -1, WP.NAN_BITS, 0)
                    continue
                ids = [c[0] for c in cand]
                assert all(w[i] > 0 and i not in sets[u] for i in ids)  # unseen, and never an item that weighs nothing
                d = _best([table[u, i] for i in ids])
                assert (items[x], draws[x]) == (ids[d], d)
                assert scores[x].tobytes() == table[u, ids[d]].tobytes()
                with np.errstate(invalid="ignore"):
                    xs = [np.float32(table[u, pos[x]]) - np.float32(table[u, i]) for i in ids]
                    viol = [d for d in range(m) if ids[d] != pos[x] and xs[d] < np.float32(margin)]
                if not viol:
                    assert (v_items[x], v_draws[x], v_margins.view(np.uint32)[x], v_ranks[x]) == (-1, m, WP.NAN_BITS, 0)
                else:
                    d = viol[0]
                    N = n_items - len(sets[u])  # the unseen COUNT
                    assert (v_items[x], v_draws[x], v_ranks[x]) == (ids[d], d, max(1, N // (d + 1)))
                    assert v_margins[x].tobytes() == np.float32(xs[d]).tobytes()


def test_unit_weights_do_not_give_the_uniform_draw():
    """The header says so: the uniform draw ranks with the 32-bit r, the weighted one with all 64 bits of z."""
    n_items, S = 12, np.array([3, 4, 9], np.int64)
    c = np.arange(400, dtype=np.int64)
    uniform = IC.draw(S, n_items, 5, c)
    weighted = np.array([_draw(S.tolist(), [1] * n_items, 5, int(x))[0] for x in c])
    assert not np.isin(weighted, S).any()
    # a dozen items hide it (the two ranks differ for about cnt in 2^32 counters); a catalogue of 2^31 - 1 does not: with
    # nothing seen and unit weights both draws are their rank t
    cnt = (1 << 31) - 1
    uniform = IC.draw(np.empty(0, np.int64), cnt, 5, c)
    weighted = np.array([(_mix(5, int(x)) * cnt) >> 64 for x in c])
    assert np.array_equal(uniform, [((_mix(5, int(x)) >> 32) * cnt) >> 32 for x in c])
    assert (uniform != weighted).any() and (np.abs(uniform - weighted) <= 1).all()


@pytest.mark.parametrize("m", (1, 3))
def test_the_restated_fold_against_enumeration(oracle, m):
    """The chain of a user step by step in Python: the draws by enumeration, the arithmetic through the restatement's own
    one-step function, which tests/test_fold_in_pairwise_cpu.py pins."""
    rng = np.random.default_rng(m)
    n_items, k, epochs, lr, lam, seed, first = 11, 6, 2, 0.05, 0.01, 9, 1 << 35
    w = np.array([3, 0, 5, 1, 0, 0, 2, 7, 1, 0, 4], np.uint32)
    Q = rng.standard_normal((n_items, k)).astype(np.float32)
    positive = [x for x in range(n_items) if w[x] > 0]
    users = [[2, 7, 2], [], positive, list(range(n_items)), [10, 0, 3, 6]]  # an item twice; none; no unseen weight; all
    row_ptr, items = FC.csr(users)
    init = rng.standard_normal((len(users), k)).astype(np.float32)
    rows, margins, negs = WP.fold(Q, w, row_ptr, items, epochs, m, init, lr, lam, seed, first)
    lib = FC.restatement()
    for x, A in enumerate(users):
        S, o = sorted(set(A)), int(row_ptr[x]) * epochs
        row = init[x].copy()
        for tau in range(len(A) * epochs):
            cand = [_draw(S, w, seed, first + (o + tau) * m + d) for d in range(m)]
            if cand[0][1] == 0:
                assert negs[o + tau] == -1 and margins.view(np.uint32)[o + tau] == WP.NAN_BITS
                continue
            ids = [c[0] for c in cand]
            j = ids[_best([oracle.predict(row[None], Q, np.zeros(1, np.int32), np.array([i], np.int32))[0] for i in ids])]
            xm = lib.fp_step(row.ctypes.data_as(FC._f), Q.ctypes.data_as(FC._f), k, A[tau % len(A)], j, lr, lam)
            assert negs[o + tau] == j and w[j] > 0 and j not in S
            assert np.float32(xm).tobytes() == margins[o + tau].tobytes()
        assert row.tobytes() == rows[x].tobytes()
    assert rows[2].tobytes() == init[2].tobytes() and rows[3].tobytes() == init[3].tobytes()


# ---- the raw calls ---------------------------------------------------------------------------------------------------------------
def _p(a, ctype):
    return None if a is None else a.ctypes.data_as(C.POINTER(ctype))


def _pick(call, m, users, n, per_row, seed=0, first=0, out=True, extra=True, pos=True, margin=1.0):
    """(rc, message, untouched) of one raw call of either pick; untouched: every output array is still as it was."""
    uu = None if users is None else np.ascontiguousarray(users, np.int32)
    pp = None if (users is None or not pos) else np.ascontiguousarray([0] * len(users) if pos is True else pos, np.int32)
    items, draws, ranks = (np.full(64, UNTOUCHED, np.int32) for _ in range(3))
    floats, mass = np.full(64, UNTOUCHED, np.float32), np.full(64, UNTOUCHED, np.int64)
    it = _p(items, C.c_int32) if out else None
    if call == HARD:
        rc = m._lib.mfsgd_sample_unseen_hard_weighted(m._handle(), _p(uu, C.c_int32), n, per_row, seed, first, it,
                                                      _p(floats, C.c_float) if extra else None,
                                                      _p(draws, C.c_int32) if extra else None, _p(mass, C.c_int64) if extra else None)
    else:
        rc = m._lib.mfsgd_sample_unseen_violating_weighted(m._handle(), _p(uu, C.c_int32), _p(pp, C.c_int32), n, per_row, margin, seed,
                                                           first, it, _p(draws, C.c_int32) if extra else None,
                                                           _p(floats, C.c_float) if extra else None,
                                                           _p(ranks, C.c_int32) if extra else None, _p(mass, C.c_int64) if extra else None)
    untouched = all(bool((a == UNTOUCHED).all()) for a in (items, draws, ranks, floats, mass))
    return rc, m._lib.mfsgd_last_error(m._h).decode(), untouched


def _fold(m, row_ptr, items, epochs=1, per_step=1, first=0, rows=True, n_new=None):
    """(rc, message, untouched) of one raw call of the weighted fold-in."""
    rp = None if row_ptr is None else np.ascontiguousarray(row_ptr, np.int64)
    ii = None if items is None else np.ascontiguousarray(items, np.int32)
    n_new = (0 if rp is None else rp.size - 1) if n_new is None else n_new
    out = np.full((8, K), UNTOUCHED, np.float32)
    margins, negs = np.full(256, UNTOUCHED, np.float32), np.full(256, UNTOUCHED, np.int32)
    rc = m._lib.mfsgd_fold_in_users_pairwise_weighted(m._handle(), n_new, _p(rp, C.c_int64), _p(ii, C.c_int32), epochs, per_step, None,
                                                      3, 4, first, _p(out, C.c_float) if rows else None, _p(margins, C.c_float),
                                                      _p(negs, C.c_int32))
    untouched = all(bool((a == UNTOUCHED).all()) for a in (out, margins, negs))
    return rc, m._lib.mfsgd_last_error(m._h).decode(), untouched


@pytest.fixture
def bare(mf):
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        yield m


@pytest.mark.parametrize("call", (HARD, VIOL))
def test_the_picks_one_broken_argument_at_a_time(bare, call):
    m = bare
    m.set_seen([], [])
    m.init_factors()
    null = "users, pos_items or out_items is null" if call == VIOL else "users or out_items is null"
    cases = [(dict(n=-1), "n is negative"),
             (dict(per_row=0), "m is below 1"),
             (dict(per_row=-1), "m is below 1"),
             (dict(first=-1), "first is negative"),
             (dict(first=I64_MAX - 5), "first + n * m exceeds 2^63 - 1"),
             (dict(n=1 << 62, per_row=2), "first + n * m exceeds 2^63 - 1"),
             (dict(n=1 << 40, per_row=1 << 30), "first + n * m exceeds 2^63 - 1"),
             (dict(users=None), null),
             (dict(out=False), null)]
    if call == VIOL:
        cases += [(dict(margin=float("nan")), "margin is NaN"), (dict(pos=False), null)]
    for args, msg in cases:
        kw = dict(users=[0, 1], n=2, per_row=3)
        kw.update(args)
        rc, got, untouched = _pick(call, m, **kw)
        assert (rc, got) == (INVALID_ARG, call + msg), args
        assert untouched
    # a call whose arguments are in order gets as far as the weights, infinite margins included
    for kw in (dict(), dict(extra=False), dict(first=I64_MAX - 6), dict(margin=float("inf")), dict(margin=float("-inf"))):
        assert _pick(call, m, [0, 1], 2, 3, **kw) == (STATE, call + "no item weights", True)


@pytest.mark.parametrize("call", (HARD, VIOL))
def test_the_picks_check_in_the_stated_order(mf, bare, call):
    m = bare
    null = "users, pos_items or out_items is null" if call == VIOL else "users or out_items is null"
    row = "row" if call == VIOL else "user"
    # 1. the arguments before the state: n, m, the margin, first and the overflow, the null arrays
    assert _pick(call, m, None, -1, 0, first=-1, margin=float("nan"))[1] == call + "n is negative"
    assert _pick(call, m, None, 2, 0, first=-1, margin=float("nan"))[1] == call + "m is below 1"
    if call == VIOL:
        assert _pick(call, m, None, 2, 3, first=-1, margin=float("nan"))[1] == call + "margin is NaN"
    assert _pick(call, m, None, 2, 3, first=-1)[1] == call + "first is negative"
    assert _pick(call, m, None, 2, 3, first=I64_MAX)[1] == call + "first + n * m exceeds 2^63 - 1"
    assert _pick(call, m, None, 2, 3)[:2] == (INVALID_ARG, call + null)
    # 2, 3. n_parts, then the index, whatever n is and before the users
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as p:
        for n in (2, 0):
            assert _pick(call, p, [0, U], n, 3)[:2] == (STATE, call + "single-partition handles only")
        assert _pick(call, p, None, 2, 3)[:2] == (INVALID_ARG, call + null)
    for n in (2, 0):
        assert _pick(call, m, [0, U], n, 3)[:2] == (STATE, call + "no seen set")
    assert _pick(call, m, None, 0, 3)[:2] == (STATE, call + "no seen set")  # (n == 0: null arrays are fine)
    # 4. the weights after the index and BEFORE the factor state: this handle has no factors either
    m.set_seen([], [])
    for n in (2, 0):
        assert _pick(call, m, [0, U], n, 3) == (STATE, call + "no item weights", True)
    m.init_factors()
    assert _pick(call, m, [0, U], 2, 3) == (STATE, call + "no item weights", True)
    lib = mf.load_library()
    out = np.zeros(1, np.int32)
    assert lib.mfsgd_sample_unseen_hard_weighted(None, _p(out, C.c_int32), 1, 1, 0, 0, _p(out, C.c_int32), None, None, None) == INVALID_ARG
    assert lib.mfsgd_sample_unseen_violating_weighted(None, _p(out, C.c_int32), _p(out, C.c_int32), 1, 1, 1.0, 0, 0, _p(out, C.c_int32),
                                                      None, None, None, None) == INVALID_ARG
    if not have_gpu():  # weights need the device: nothing behind "no item weights" can be reached
        with pytest.raises(mf.MfsgdError) as e:
            m.set_item_weights(np.ones(I, np.uint32))
        assert e.value.code == NO_DEVICE
        return
    # 5, 6. with weights: the factor state, on a fresh handle; "cover" before it
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as f:
        f.set_seen([], [])
        f.set_item_weights(np.ones(I, np.uint32))
        for n in (2, 0):
            assert _pick(call, f, [0, U], n, 3) == (STATE, call + "factors not initialised", True)
        f.init_p_offset(1, 0)  # P alone
        rc, msg, untouched = _pick(call, f, [0, U], 2, 3)
        assert rc == STATE and msg.startswith(call + "Q is not initialised") and untouched
    m.set_item_weights(np.ones(I, np.uint32))
    # 7. n == 0 is fine and reads nothing
    assert _pick(call, m, [0, U], 0, 3)[::2] == (OK, True)
    assert _pick(call, m, None, 0, 3, out=False, extra=False)[0] == OK
    # 8. then the rows, named
    for users, bad in (([0, U], 1), ([-1, 0], 0), ([0, 1, 2, 1 << 30], 3)):
        assert _pick(call, m, users, len(users), 3) == (INVALID_ARG, call + f"{row} {bad} out of range", True)
    if call == VIOL:
        assert _pick(call, m, [0, 1, 2], 3, 3, pos=[0, I, 0]) == (INVALID_ARG, call + "row 1 out of range", True)
    # 5. stale weights: before the factor state would be asked, and whatever n is
    m.add_items(n=2)
    for n in (2, 0):
        assert _pick(call, m, [0, U], n, 3) == (STATE, call + f"item weights cover {I} items, the model has {I + 2}", True)


def test_the_fold_in_one_broken_argument_at_a_time(bare):
    m = bare
    m.init_factors()
    for kw, msg in ((dict(n_new=-1), "n_new is negative"),
                    (dict(epochs=-1), "epochs is negative"),
                    (dict(per_step=0), "m is below 1"),
                    (dict(first=-1), "first is negative"),
                    (dict(first=I64_MAX - 2), "first + T * epochs * m exceeds 2^63 - 1"),
                    (dict(row_ptr=None, n_new=2), "row_ptr or out_rows is null"),
                    (dict(rows=False), "row_ptr or out_rows is null"),
                    (dict(row_ptr=[1, 2, 3]), "row_ptr[0] is not 0"),
                    (dict(row_ptr=[0, 2, 1], items=[0, 1]), "row_ptr decreases at user 1"),
                    (dict(items=None), "items is null"),
                    (dict(items=[0, 1, I]), "item of positive 2 out of range"),
                    (dict(items=[-1, 1, 2]), "item of positive 0 out of range")):
        args = dict(row_ptr=[0, 2, 3], items=[0, 1, 2])
        args.update(kw)
        assert _fold(m, **args) == (INVALID_ARG, FOLD + msg, True), kw
    assert _fold(m, [0, 2, 3], [0, 1, 2]) == (STATE, FOLD + "no item weights", True)


def test_the_fold_in_checks_in_the_stated_order(mf, bare):
    m = bare
    # the arguments before the state, the state before the weights: this handle has neither factors nor weights
    assert _fold(m, [0, 2, 3], [0, 1, I])[:2] == (INVALID_ARG, FOLD + "item of positive 2 out of range")
    for args in (([0, 2, 3], [0, 1, 2]), ([0], None)):
        assert _fold(m, *args) == (STATE, FOLD + "factors not initialised", True)
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as p:
        assert _fold(p, [0, 2, 3], [0, 1, 2]) == (STATE, FOLD + "single-partition handles only", True)
    m.init_p_offset(1, 0)  # P alone
    rc, msg, untouched = _fold(m, [0, 2, 3], [0, 1, 2])
    assert rc == STATE and msg.startswith(FOLD + "Q is not initialised") and untouched
    m.init_factors()
    # no weights: whatever n_new is; the call needs no index
    assert m.seen_size() == -1
    for args in (([0, 2, 3], [0, 1, 2]), ([0], None)):
        assert _fold(m, *args) == (STATE, FOLD + "no item weights", True)
    assert mf.load_library().mfsgd_fold_in_users_pairwise_weighted(None, 0, None, None, 1, 1, None, 0, 0, 0, None, None, None) == INVALID_ARG
    if not have_gpu():
        return
    m.set_item_weights(np.ones(I, np.uint32))
    assert _fold(m, [0], None)[::2] == (OK, True)  # n_new == 0 touches nothing
    assert m.seen_size() == -1
    m.add_items(n=2)
    for args in (([0, 2, 3], [0, 1, 2]), ([0], None)):
        assert _fold(m, *args) == (STATE, FOLD + f"item weights cover {I} items, the model has {I + 2}", True)


# ---- the keywords of the Python surface ----------------------------------------------------------------------------------------
def test_the_keywords(mf, bare):
    m = bare
    for bad in ("popular", "", None, "Weighted"):
        for call in (lambda: m.sample_unseen_hard([0], 2, sampling=bad),
                     lambda: m.sample_unseen_violating([0], [1], 2, sampling=bad),
                     lambda: m.fit_warp([0, 1], [1, 2], 1, sampling=bad),
                     lambda: m.fit_bpr([0, 1], [1, 2], 1, candidates=2, candidate_sampling=bad),
                     lambda: m.fit_bpr([0, 1], [1, 2], 1, candidate_sampling=bad),
                     lambda: m.fold_in_pairwise([0, 1], [2], 1, sampling=bad)):
            with pytest.raises(ValueError):
                call()
    # mass is the weighted call's alone
    for call in (lambda: m.sample_unseen_hard([0], 2, mass=True), lambda: m.sample_unseen_violating([0], [1], 2, mass=True)):
        with pytest.raises(ValueError):
            call()
    # one candidate is spelled sampling="weighted"; several are spelled candidate_sampling="weighted"
    with pytest.raises(ValueError):
        m.fit_bpr([0, 1], [1, 2], 1, candidate_sampling="weighted")
    with pytest.raises(ValueError):
        m.fit_bpr([0, 1], [1, 2], 1, candidates=2, sampling="weighted")
    # without weights the weighted fits are refused with nothing touched: no index, no factors
    with pytest.raises(ValueError):
        m.fit_bpr([0, 1], [1, 2], 1, candidates=2, candidate_sampling="weighted")
    with pytest.raises(ValueError):
        m.fit_warp([0, 1], [1, 2], 1, sampling="weighted")
    assert m.seen_size() == -1 and not m._initialised and m.item_weights() is None
    # the weighted calls themselves say what is missing
    m.set_seen([], [])
    m.init_factors()
    for call in (lambda: m.sample_unseen_hard([0, 1], 2, sampling="weighted"),
                 lambda: m.sample_unseen_violating([0, 1], [1, 2], 2, sampling="weighted", mass=True),
                 lambda: m.fold_in_pairwise([0, 1], [2], 1, sampling="weighted")):
        with pytest.raises(mf.MfsgdError) as e:
            call()
        assert e.value.code == STATE and "no item weights" in str(e.value)
    # the default is the uniform call: nothing about it moved
    want = OK if have_gpu() else NO_DEVICE
    for call in (lambda: m.sample_unseen_hard([0, 1], 2, sampling="uniform"),
                 lambda: m.sample_unseen_violating([0, 1], [1, 2], 2, sampling="uniform")):
        if want == OK:
            call()
        else:
            with pytest.raises(mf.MfsgdError) as e:
                call()
            assert e.value.code == NO_DEVICE
    assert m.sample_unseen_hard([], 2).shape == (0,)
