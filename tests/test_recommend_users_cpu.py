"""The item-side serving calls (mfsgd_recommend_users and its five kin) check their arguments before any device work, in
recommend_core's order with the words of this side in the messages, so the checks run without a GPU: every refusal, one
broken argument at a time, with its status, its message and its place in the order; the outputs are left untouched.  A
valid call without a device fails with MFSGD_ERR_NO_DEVICE, never with a CPU result."""
import ctypes as C

import numpy as np
import pytest

from tests.conftest import have_gpu

OK, INVALID_ARG, NO_DEVICE, STATE = 0, -1, -2, -5
U, I, K = 6, 5, 8
CANARY_I, CANARY_S = -77, np.float32(123.5)
NAMES = ("mfsgd_recommend_users", "mfsgd_recommend_users_among", "mfsgd_recommend_users_unseen",
         "mfsgd_recommend_users_unseen_among", "mfsgd_recommend_users_rows", "mfsgd_recommend_users_rows_among")


def _ptr(a, dtype, ctype):
    return None if a is None else np.ascontiguousarray(a, dtype).ctypes.data_as(C.POINTER(ctype))


def _i32(a):
    return _ptr(a, np.int32, C.c_int32)


def _call(m, name, first, n, topn, cand=None, excl=None, outs=True):
    """The raw C-ABI call `mfsgd_<name>`: `first` is the items (or the rows), n their count as the call is told it,
    cand = (cand_ptr, cand_users, n_cand) for an _among call, excl = (a, b, n_excl) for a call with pairs; None stands for
    a NULL pointer.  Returns (status, message, outputs untouched)."""
    size = max(1, max(n, 1) * max(topn, 1))
    users, scores = np.full(size, CANARY_I, np.int32), np.full(size, CANARY_S, np.float32)
    args = [_ptr(first, np.float32, C.c_float) if "rows" in name else _i32(first), n, topn]
    if cand is not None:
        args += [_ptr(cand[0], np.int64, C.c_int64), _i32(cand[1]), cand[2]]
    if "unseen" not in name:
        a, b, n_excl = excl if excl is not None else (None, None, 0)
        args += [_i32(a), _i32(b), n_excl]
    args += [_i32(users) if outs else None, _ptr(scores, np.float32, C.c_float) if outs else None]
    rc = getattr(m._lib, "mfsgd_" + name)(m._handle(), *args)
    untouched = bool((users == CANARY_I).all() and (scores == CANARY_S).all())
    return rc, m._lib.mfsgd_last_error(m._h).decode(), untouched


@pytest.fixture
def model(mf):
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        m.init_factors()
        m.set_seen(np.empty(0, np.int32), np.empty(0, np.int32))  # an empty index: no GPU needed
        yield m


def test_the_six_symbols_are_exported_and_bound(mf):
    import subprocess

    from mfsgd_amd import _lib

    exported = subprocess.run(["nm", "-D", "--defined-only", _lib.library_path()], stdout=subprocess.PIPE, text=True,
                              check=True).stdout.split()
    lib = mf.load_library()
    for name in NAMES:
        assert name in exported
        restype, argtypes = _lib.SIGNATURES[name]
        fn = getattr(lib, name)
        assert fn.restype is restype is C.c_int and list(fn.argtypes) == argtypes


ROWS2 = np.ones((2, K), np.float32)
SHARED = (None, [0, 1], 2)


# items [0, 2] (or two rows): one broken argument at a time
@pytest.mark.parametrize("name,first,n,topn,cand,excl,status,message", [
    # the arguments every call has
    ("recommend_users", [0, 2], -1, 3, None, None, INVALID_ARG, "recommend_users: bad argument"),
    ("recommend_users", [0, 2], 2, 0, None, None, INVALID_ARG, "recommend_users: bad argument"),
    ("recommend_users", None, 2, 3, None, None, INVALID_ARG, "recommend_users: bad argument"),
    ("recommend_users", [0, 2], 2, 3, None, ([0], [0], -1), INVALID_ARG, "recommend_users: bad argument"),
    ("recommend_users", [0, 2], 2, 3, None, (None, [0], 1), INVALID_ARG, "recommend_users: bad argument"),
    ("recommend_users", [0, 2], 2, 3, None, ([0], None, 1), INVALID_ARG, "recommend_users: bad argument"),
    ("recommend_users_among", [0, 2], 2, -4, SHARED, None, INVALID_ARG, "recommend_users_among: bad argument"),
    ("recommend_users_unseen", [0, 2], 2, 0, None, None, INVALID_ARG, "recommend_users_unseen: bad argument"),
    ("recommend_users_unseen_among", None, 2, 3, SHARED, None, INVALID_ARG, "recommend_users_unseen_among: bad argument"),
    ("recommend_users_rows", None, 2, 3, None, None, INVALID_ARG, "recommend_users_rows: bad argument"),
    ("recommend_users_rows", ROWS2, -1, 3, None, None, INVALID_ARG, "recommend_users_rows: bad argument"),
    ("recommend_users_rows", ROWS2, 2, 0, None, None, INVALID_ARG, "recommend_users_rows: bad argument"),
    ("recommend_users_rows_among", None, 2, 3, SHARED, None, INVALID_ARG, "recommend_users_rows_among: bad argument"),
    ("recommend_users_rows_among", ROWS2, 2, 0, SHARED, None, INVALID_ARG, "recommend_users_rows_among: bad argument"),
    # topn against the users, not the items
    ("recommend_users", [0, 2], 2, U + 1, None, None, INVALID_ARG, "recommend_users: topn exceeds the number of users"),
    ("recommend_users_among", [0, 2], 2, U + 1, SHARED, None, INVALID_ARG, "recommend_users_among: topn exceeds the number of users"),
    ("recommend_users_unseen", [0, 2], 2, U + 1, None, None, INVALID_ARG, "recommend_users_unseen: topn exceeds the number of users"),
    ("recommend_users_unseen_among", [0, 2], 2, U + 1, SHARED, None, INVALID_ARG,
     "recommend_users_unseen_among: topn exceeds the number of users"),
    ("recommend_users_rows", ROWS2, 2, U + 1, None, None, INVALID_ARG, "recommend_users_rows: topn exceeds the number of users"),
    ("recommend_users_rows_among", ROWS2, 2, U + 1, SHARED, None, INVALID_ARG,
     "recommend_users_rows_among: topn exceeds the number of users"),
    # a requested item: I = 5 is none although it is a user
    ("recommend_users", [0, I], 2, 3, None, None, INVALID_ARG, "recommend_users: item 1 out of range"),
    ("recommend_users", [-1, 2], 2, 3, None, None, INVALID_ARG, "recommend_users: item 0 out of range"),
    ("recommend_users_among", [0, I], 2, 3, SHARED, None, INVALID_ARG, "recommend_users_among: item 1 out of range"),
    ("recommend_users_unseen", [0, I], 2, 3, None, None, INVALID_ARG, "recommend_users_unseen: item 1 out of range"),
    ("recommend_users_unseen_among", [I, 0], 2, 3, SHARED, None, INVALID_ARG, "recommend_users_unseen_among: item 0 out of range"),
    # candidates: users, so I = 5 is one and U = 6 is none
    ("recommend_users_among", [0, 2], 2, 3, (None, [0, 1], -1), None, INVALID_ARG, "recommend_users_among: n_cand is negative"),
    ("recommend_users_among", [0, 2], 2, 3, (None, None, 2), None, INVALID_ARG, "recommend_users_among: cand_users is null"),
    ("recommend_users_among", [0, 2], 2, 3, ([0, 1, 2], None, 2), None, INVALID_ARG, "recommend_users_among: cand_users is null"),
    ("recommend_users_among", [0, 2], 2, 3, ([1, 2, 3], [0, 1, 2], 3), None, INVALID_ARG, "recommend_users_among: cand_ptr[0] is not 0"),
    ("recommend_users_among", [0, 2], 2, 3, ([0, 2, 1], [0, 1, 2], 1), None, INVALID_ARG,
     "recommend_users_among: cand_ptr decreases at row 1"),
    ("recommend_users_among", [0, 2], 2, 3, ([0, 1, 2], [0, 1, 2], 3), None, INVALID_ARG,
     "recommend_users_among: cand_ptr ends at 2, not at n_cand"),
    ("recommend_users_among", [0, 2], 2, 3, (None, [0, I, U, 2], 4), None, INVALID_ARG, "recommend_users_among: candidate 2 out of range"),
    ("recommend_users_among", [0, 2], 2, 3, ([0, 1, 4], [0, 1, 3, -1], 4), None, INVALID_ARG,
     "recommend_users_among: candidate 3 out of range"),
    ("recommend_users_unseen_among", [0, 2], 2, 3, (None, [0, U], 2), None, INVALID_ARG,
     "recommend_users_unseen_among: candidate 1 out of range"),
    ("recommend_users_unseen_among", [0, 2], 2, 3, ([0, 1, 1], [0, 1], 2), None, INVALID_ARG,
     "recommend_users_unseen_among: cand_ptr ends at 1, not at n_cand"),
    ("recommend_users_rows_among", ROWS2, 2, 3, (None, [0, U], 2), None, INVALID_ARG,
     "recommend_users_rows_among: candidate 1 out of range"),
    ("recommend_users_rows_among", ROWS2, 2, 3, ([0, 1, 1], [0, 1], 2), None, INVALID_ARG,
     "recommend_users_rows_among: cand_ptr ends at 1, not at n_cand"),
    # pairs are (user, item): user 5 = I is one, item 5 is none; user 6 = U is none
    ("recommend_users", [0, 2], 2, 3, None, ([0, I], [1, I], 2), INVALID_ARG, "recommend_users: excluded pair 1 out of range"),
    ("recommend_users", [0, 2], 2, 3, None, ([U], [0], 1), INVALID_ARG, "recommend_users: excluded pair 0 out of range"),
    ("recommend_users", [0, 2], 2, 3, None, ([0, 1, -1], [4, 4, 0], 3), INVALID_ARG, "recommend_users: excluded pair 2 out of range"),
    ("recommend_users_among", [0, 2], 2, 3, SHARED, ([U], [0], 1), INVALID_ARG, "recommend_users_among: excluded pair 0 out of range"),
    # ... and for the rows calls (row, user): two rows, so row 2 is none; user 5 is one
    ("recommend_users_rows", ROWS2, 2, 3, None, ([1, 2], [I, 0], 2), INVALID_ARG, "recommend_users_rows: excluded pair 1 out of range"),
    ("recommend_users_rows", ROWS2, 2, 3, None, ([1], [U], 1), INVALID_ARG, "recommend_users_rows: excluded pair 0 out of range"),
    ("recommend_users_rows_among", ROWS2, 2, 3, SHARED, ([2], [0], 1), INVALID_ARG,
     "recommend_users_rows_among: excluded pair 0 out of range"),
])
def test_every_refusal_has_its_status_and_message_and_leaves_the_outputs(model, name, first, n, topn, cand, excl, status, message):
    assert _call(model, name, first, n, topn, cand, excl) == (status, message, True)


def test_null_outputs_are_a_bad_argument(model):
    for name in ("recommend_users", "recommend_users_unseen"):
        assert _call(model, name, [0, 2], 2, 3, outs=False)[:2] == (INVALID_ARG, name + ": bad argument")
    assert _call(model, "recommend_users_rows", ROWS2, 2, 3, outs=False)[:2] == (INVALID_ARG, "recommend_users_rows: bad argument")


def test_checks_run_in_recommend_cores_order(model, mf):
    bad_item, bad_cand, bad_pair = [0, I], (None, [0, U], 2), ([0, U], [1, 1], 2)
    name = "recommend_users_among"
    # everything wrong at once: topn comes before the item, the item before the candidate, the candidate before the pair
    assert _call(model, name, bad_item, 2, U + 1, bad_cand, bad_pair)[1] == name + ": topn exceeds the number of users"
    assert _call(model, name, bad_item, 2, 2, bad_cand, bad_pair)[1] == name + ": item 1 out of range"
    assert _call(model, name, [0, 1], 2, 2, bad_cand, bad_pair)[1] == name + ": candidate 1 out of range"
    assert _call(model, name, [0, 1], 2, 2, ([0, 1, 1], [0, U], 2), bad_pair)[1] == name + ": cand_ptr ends at 1, not at n_cand"
    assert _call(model, name, [0, 1], 2, 2, SHARED, bad_pair)[1] == name + ": excluded pair 1 out of range"
    # "bad argument" comes first of all
    assert _call(model, name, bad_item, 2, 0, bad_cand, bad_pair)[1] == name + ": bad argument"
    # the argument checks come before the factor checks: a handle whose factors were never set
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        assert _call(m, "recommend_users", bad_item, 2, 2)[:2] == (INVALID_ARG, "recommend_users: item 1 out of range")
        assert _call(m, "recommend_users_rows", ROWS2, 2, 2, None, ([2], [0], 1))[:2] == (
            INVALID_ARG, "recommend_users_rows: excluded pair 0 out of range")
        # ... "no seen set" before the remaining argument checks, as for recommend_unseen
        assert _call(m, "recommend_users_unseen", bad_item, 2, U + 1)[:2] == (STATE, "recommend_users_unseen: no seen set")
        assert _call(m, "recommend_users_unseen", bad_item, 2, 0)[:2] == (INVALID_ARG, "recommend_users_unseen: bad argument")
    # ... and the partition check before "no seen set"
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as m:
        assert _call(m, "recommend_users_unseen", bad_item, 2, U + 1)[:2] == (
            STATE, "recommend_users_unseen: single-partition handles only")


def test_the_remaining_neighbours_of_recommend_cores_order(model, mf):
    """Two faults in one call, for the neighbouring pairs the test above leaves out: bad argument / partitions / no seen set /
    topn, the item before the first candidate check, and the candidate checks among themselves."""
    bad_item, bad_pair = [0, I], ([0, U], [1, 1], 2)
    name = "recommend_users_among"
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as m:
        assert _call(m, name, bad_item, 2, 0, SHARED, bad_pair)[:2] == (INVALID_ARG, name + ": bad argument")
        assert _call(m, name, bad_item, 2, U + 1, SHARED, bad_pair)[:2] == (STATE, name + ": single-partition handles only")
        assert _call(m, "recommend_users_unseen_among", bad_item, 2, U + 1, SHARED)[:2] == (
            STATE, "recommend_users_unseen_among: single-partition handles only")
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:  # no index
        unseen = "recommend_users_unseen_among"
        assert _call(m, unseen, bad_item, 2, U + 1, (None, [0, U], -1))[:2] == (STATE, unseen + ": no seen set")
        assert _call(m, unseen, bad_item, -1, U + 1, SHARED)[:2] == (INVALID_ARG, unseen + ": bad argument")
    # the item before the first of the candidate checks
    assert _call(model, name, bad_item, 2, 2, (None, None, -1), bad_pair)[1] == name + ": item 1 out of range"
    # the candidate checks: n_cand, the null array, cand_ptr[0], a decreasing cand_ptr, its end, the range
    assert _call(model, name, [0, 1], 2, 2, (None, None, -1), bad_pair)[1] == name + ": n_cand is negative"
    assert _call(model, name, [0, 1], 2, 2, ([1, 2, 3], None, 3), bad_pair)[1] == name + ": cand_users is null"
    assert _call(model, name, [0, 1], 2, 2, ([1, 3, 2], [0, 1, U], 3), bad_pair)[1] == name + ": cand_ptr[0] is not 0"
    assert _call(model, name, [0, 1], 2, 2, ([0, 2, 1], [0, 1, U], 3), bad_pair)[1] == name + ": cand_ptr decreases at row 1"
    assert _call(model, name, [0, 1], 2, 2, ([0, 1, 2], [0, 1, U], 3), bad_pair)[1] == name + ": cand_ptr ends at 2, not at n_cand"
    assert _call(model, name, [0, 1], 2, 2, ([0, 1, 3], [0, 1, U], 3), bad_pair)[1] == name + ": candidate 2 out of range"


def test_nothing_asked_is_ok(model, mf):
    assert _call(model, "recommend_users", [], 0, 3)[0] == OK
    assert _call(model, "recommend_users", None, 0, 3, outs=False)[0] == OK
    assert _call(model, "recommend_users", None, 0, 3, None, ([1], [1], 1))[0] == OK  # (pairs of items nobody asked about)
    assert _call(model, "recommend_users_among", [], 0, 3, ([0], None, 0))[0] == OK
    assert _call(model, "recommend_users_unseen", [], 0, 3)[0] == OK
    assert _call(model, "recommend_users_unseen_among", [], 0, 3, SHARED)[0] == OK
    assert _call(model, "recommend_users_rows", np.empty((0, K), np.float32), 0, 3)[0] == OK
    assert _call(model, "recommend_users_rows_among", None, 0, 3, ([0], None, 0))[0] == OK
    # ... even of a handle whose factors were never set: n == 0 comes before the state of the factors
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        assert _call(m, "recommend_users", [], 0, 3)[0] == OK
        assert _call(m, "recommend_users_rows", None, 0, 3)[0] == OK


def test_state_errors(mf):
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as m:
        for name in ("recommend_users", "recommend_users_unseen"):
            assert _call(m, name, [0], 1, 2) == (STATE, name + ": single-partition handles only", True)
        for name in ("recommend_users_among", "recommend_users_unseen_among"):
            assert _call(m, name, [0], 1, 2, SHARED) == (STATE, name + ": single-partition handles only", True)
        assert _call(m, "recommend_users_rows", ROWS2, 2, 2) == (STATE, "recommend_users_rows: single-partition handles only", True)
        assert _call(m, "recommend_users_rows_among", ROWS2, 2, 2, SHARED) == (
            STATE, "recommend_users_rows_among: single-partition handles only", True)
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        m.init_factors()  # no index
        assert _call(m, "recommend_users_unseen", [0], 1, 2) == (STATE, "recommend_users_unseen: no seen set", True)
        assert _call(m, "recommend_users_unseen_among", [0], 1, 2, SHARED) == (STATE, "recommend_users_unseen_among: no seen set", True)
        m.set_seen(np.empty(0, np.int32), np.empty(0, np.int32))
        m.clear_seen()
        assert _call(m, "recommend_users_unseen", [0], 1, 2)[:2] == (STATE, "recommend_users_unseen: no seen set")
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:  # factors never set
        assert _call(m, "recommend_users_rows", ROWS2, 2, 2) == (STATE, "recommend_users_rows: factors not initialised", True)
        assert _call(m, "recommend_users_rows_among", ROWS2, 2, 2, SHARED) == (
            STATE, "recommend_users_rows_among: factors not initialised", True)
        # the items' call reports it exactly as mfsgd_recommend_excluding does, whatever that is on this machine
        uu, out_i, out_s = np.zeros(1, np.int32), np.empty(2, np.int32), np.empty(2, np.float32)
        want = m._lib.mfsgd_recommend_excluding(m._handle(), _i32(uu), 1, 2, None, None, 0, _i32(out_i),
                                                _ptr(out_s, np.float32, C.c_float))
        want_msg = m._lib.mfsgd_last_error(m._h).decode()
        rc, msg, untouched = _call(m, "recommend_users", [0], 1, 2)
        assert want != OK and rc == want and untouched and msg == want_msg.replace("recommend:", "recommend_users:", 1)
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:  # P alone: no Q to take the items' rows from
        m.init_p_offset(1, 0)
        for name, first, cand in (("recommend_users", [0], None), ("recommend_users_among", [0], SHARED),
                                  ("recommend_users_rows", ROWS2[:1], None)):
            rc, msg, untouched = _call(m, name, first, 1, 2, cand)
            assert rc == STATE and untouched and msg.startswith(name + ": Q is not initialised")


def test_valid_call_without_device_fails_loudly(model, mf):
    """... and with one it is answered: the same calls, so this test asks the same of both machines."""
    want = OK if have_gpu() else NO_DEVICE
    assert _call(model, "recommend_users", [0, 2, 2], 3, 3)[0] == want
    assert _call(model, "recommend_users", [0, 2], 2, U, None, ([0, 5], [4, 0], 2))[0] == want
    assert _call(model, "recommend_users_among", [0, 2], 2, 3, ([0, 0, 2], [5, 0], 2), ([0], [4], 1))[0] == want
    assert _call(model, "recommend_users_unseen", [0, 2], 2, 3)[0] == want
    assert _call(model, "recommend_users_unseen_among", [0, 2], 2, 3, SHARED)[0] == want
    assert _call(model, "recommend_users_rows", ROWS2, 2, 3, None, ([1], [5], 1))[0] == want
    assert _call(model, "recommend_users_rows_among", ROWS2, 2, 3, SHARED)[0] == want
    for cand in (None, [1, 2], ([0, 1, 2], [3, 4]), [[1], []]):
        for call in (lambda: model.recommend_users([0, 2], 3, candidates=cand),
                     lambda: model.recommend_users([0, 2], 3, exclude="seen", candidates=cand),
                     lambda: model.recommend_users_rows(ROWS2, 3, exclude=([0], [1]), candidates=cand)):
            if have_gpu():
                users, scores = call()
                assert users.shape == scores.shape == (2, 3)
            else:
                with pytest.raises(mf.MfsgdError) as e:
                    call()
                assert e.value.code == NO_DEVICE


def test_python_shapes_are_checked(model):
    with pytest.raises(ValueError):
        model.recommend_users([0, 2], 2, candidates=np.zeros((2, 2), np.int32))
    with pytest.raises(ValueError):
        model.recommend_users([0, 2], 2, candidates=[[0, 1]])  # one list for two rows
    with pytest.raises(ValueError):
        model.recommend_users_rows(np.ones((2, K + 1), np.float32), 2)
    with pytest.raises(ValueError):
        model.recommend_users_rows(ROWS2, 2, exclude=([0, 1], [0]))


def test_appended_users_are_candidates_and_the_reserve_beyond_them_is_not(mf):
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        m.init_factors()  # host staging: no device yet
        m.reserve(users=U + 8)
        assert m.add_users(n=3) == U
        name = "recommend_users_among"
        bad_pair = ([U + 3], [0], 1)  # reported only once every candidate has passed
        assert _call(m, name, [0], 1, 2, (None, [U, U + 2, 0], 3), bad_pair)[:2] == (INVALID_ARG, name + ": excluded pair 0 out of range")
        # the new count is the first index that is none, however much room was reserved
        assert _call(m, name, [0], 1, 2, (None, [U, U + 3], 2))[:2] == (INVALID_ARG, name + ": candidate 1 out of range")
        assert _call(m, name, [0], 1, U + 3, (None, [U], 1), bad_pair)[1] == name + ": excluded pair 0 out of range"
        assert _call(m, name, [0], 1, U + 4, (None, [U], 1))[1] == name + ": topn exceeds the number of users"
