"""mfsgd_fold_in_solve and mfsgd_gram without a GPU: every argument screen, in its order, before any device work; a
valid call without a device is MFSGD_ERR_NO_DEVICE.  And the C restatement of the rule (tests/solve_common.py), which the
GPU tests compare with bit for bit, against an fp64 solve, with its refusals, the empty-list rule and ALS on top."""
import ctypes as C

import numpy as np
import pytest

from tests import solve_common as sc
from tests.conftest import have_gpu

OK, INVALID_ARG, NO_DEVICE, STATE = 0, -1, -2, -5
U, I, K = 6, 5, 8
USERS, ITEMS = 0, 1
SENTINEL = np.float32(-77.0)


def _ptr(a, dtype, ctype):
    """None stands for a NULL pointer."""
    return None if a is None else np.ascontiguousarray(a, dtype).ctypes.data_as(C.POINTER(ctype))


def _solve(m, side, n_new, row_ptr, ids, b, a=None, alpha=0.0, ridge=0.0, rpe=0.05, out=True, status=True):
    """(return code, message, rows, status) of one raw call; the outputs start as sentinels."""
    rows = np.full((max(1, n_new), K), SENTINEL, np.float32) if out else None
    st = np.full(max(1, n_new), -7, np.int32) if status else None
    rp = None if row_ptr is None else np.ascontiguousarray(row_ptr, np.int64)
    rc = m._lib.mfsgd_fold_in_solve(m._handle(), side, n_new, _ptr(rp, np.int64, C.c_int64), _ptr(ids, np.int32, C.c_int32),
                                    _ptr(a, np.float32, C.c_float), _ptr(b, np.float32, C.c_float), alpha, ridge, rpe,
                                    None if rows is None else rows.ctypes.data_as(C.POINTER(C.c_float)),
                                    None if st is None else st.ctypes.data_as(C.POINTER(C.c_int32)))
    return rc, m._lib.mfsgd_last_error(m._h).decode(), rows, st


def _untouched(rows, st):
    return (rows is None or (rows == SENTINEL).all()) and (st is None or (st == -7).all())


PRE = "fold_in_solve: "
TWO = dict(ids=[0, 1], b=[1, 2])


def test_every_screen_in_its_order(mf):
    """One case per screen, and for each neighbouring pair of the order a call with both faults: the earlier one is
    reported.  Nothing is written to the outputs of a refused call."""
    def refused(m, code, msg, *args, **kw):
        rc, got, rows, st = _solve(m, *args, **kw)
        assert (rc, got) == (code, PRE + msg), (rc, got)
        assert _untouched(rows, st)

    side_msg = "side is neither MFSGD_SIDE_USERS nor MFSGD_SIDE_ITEMS"
    null_msg = "row_ptr or out_rows is null"
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:  # factors never set: every screen comes before the state
        refused(m, INVALID_ARG, side_msg, 2, 2, [0, 1, 2], **TWO)
        refused(m, INVALID_ARG, side_msg, -1, -1, [0], [], [])                      # ... before n_new
        refused(m, INVALID_ARG, "n_new is negative", USERS, -1, [0], [], [])
        refused(m, INVALID_ARG, "n_new is negative", USERS, -1, None, [], [])       # ... before the null row_ptr
        refused(m, INVALID_ARG, null_msg, USERS, 2, None, **TWO)
        refused(m, INVALID_ARG, null_msg, USERS, 2, [1, 1, 2], out=False, **TWO)    # ... before row_ptr[0]
        refused(m, INVALID_ARG, "row_ptr[0] is not 0", USERS, 2, [1, 1, 2], **TWO)
        refused(m, INVALID_ARG, "row_ptr[0] is not 0", USERS, 2, [1, 3, 2], **TWO)  # ... before a decreasing row_ptr
        refused(m, INVALID_ARG, "row_ptr decreases at row 1", USERS, 3, [0, 2, 1, 3], [0, 1, 2], [1, 2, 3])
        refused(m, INVALID_ARG, "row_ptr decreases at row 1", USERS, 3, [0, 2, 1, 3], None, [1, 2, 3])  # ... before the null ids
        refused(m, INVALID_ARG, "ids or b is null", USERS, 2, [0, 1, 2], None, [1, 2])
        refused(m, INVALID_ARG, "ids or b is null", USERS, 2, [0, 1, 2], [0, 1], None)
        refused(m, INVALID_ARG, "ids or b is null", USERS, 2, [0, 1, 3], [0, I, 1], None)               # ... before the range
        # the fixed side of new users is the items, that of new items the users
        refused(m, INVALID_ARG, "id of entry 1 out of range", USERS, 2, [0, 1, 3], [0, I, 1], [1, 2, 3])
        refused(m, INVALID_ARG, "id of entry 2 out of range", USERS, 2, [0, 1, 3], [0, 1, -1], [1, 2, 3])
        refused(m, INVALID_ARG, "id of entry 2 out of range", ITEMS, 2, [0, 1, 3], [0, I, U], [1, 2, 3])
        refused(m, INVALID_ARG, "id of entry 1 out of range", USERS, 2, [0, 1, 3], [0, I, 1], [1, 2, 3], alpha=np.nan)  # ... before the numbers
        for bad in (np.nan, np.inf, -np.inf):
            for kw in (dict(alpha=bad), dict(ridge=bad), dict(rpe=bad)):
                refused(m, INVALID_ARG, "alpha, ridge or ridge_per_entry is not finite", USERS, 2, [0, 1, 2], **TWO, **kw)
        # ... and only then the state, whatever n_new is
        refused(m, STATE, "factors not initialised", USERS, 2, [0, 1, 2], **TWO)
        refused(m, STATE, "factors not initialised", USERS, 0, None, None, None)
        refused(m, INVALID_ARG, "alpha, ridge or ridge_per_entry is not finite", USERS, 0, None, None, None, ridge=np.nan)
        m.init_p_offset(1, 0)  # P alone
        rc, msg, rows, st = _solve(m, ITEMS, 2, [0, 1, 2], **TWO)
        assert rc == STATE and msg.startswith(PRE + "Q is not initialised") and _untouched(rows, st)
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as m:
        refused(m, STATE, "single-partition handles only", USERS, 2, [0, 1, 2], **TWO)
        refused(m, INVALID_ARG, null_msg, USERS, 2, None, **TWO)
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        m.init_factors()
        rc, _, rows, st = _solve(m, USERS, 0, None, None, None, out=False, status=False)
        assert rc == OK
        rc, _, rows, st = _solve(m, ITEMS, 0, [5], [99], None)  # nobody to fold in: nothing is read or written
        assert rc == OK and _untouched(rows, st)
        assert m._lib.mfsgd_fold_in_solve(None, USERS, 0, None, None, None, None, 0.0, 0.0, 0.0, None, None) == INVALID_ARG


def test_the_gram_screens(mf):
    out = np.full((K, K), SENTINEL, np.float32)

    def go(m, side, o=out):
        rc = m._lib.mfsgd_gram(m._handle(), side, None if o is None else o.ctypes.data_as(C.POINTER(C.c_float)))
        return rc, m._lib.mfsgd_last_error(m._h).decode()

    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        assert go(m, 2, None) == (INVALID_ARG, "gram: side is neither MFSGD_SIDE_USERS nor MFSGD_SIDE_ITEMS")
        assert go(m, USERS, None) == (INVALID_ARG, "gram: out is null")
        assert go(m, USERS) == (STATE, "gram: factors not initialised")
        with pytest.raises(ValueError):
            m.gram("rows")
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as m:
        assert go(m, ITEMS) == (STATE, "gram: single-partition handles only")
    assert (out == SENTINEL).all()


def test_python_shapes_are_checked(mf):
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        m.init_factors()
        with pytest.raises(ValueError):
            m.fold_in_exact([0, 1, 2], [0, 1, 2], [1.0, 2.0])                        # items and ratings differ
        with pytest.raises(ValueError):
            m.fold_in_exact([0, 1, 3], [0, 1], [1.0, 2.0])                           # row_ptr ends elsewhere
        with pytest.raises(ValueError):
            m.fold_in_exact([0, 1, 2], [0, 1], [1.0, 2.0], weights=[1.0])            # weights differ
        with pytest.raises(ValueError):
            m.fold_in_items_implicit([[0, 1, 2]], [0, 1], [1.0, 2.0], 0.1)           # row_ptr not 1-d
        assert m.fold_in_exact([0], [], []).shape == (0, K)
        rows, st = m.fold_in_implicit([0], [], [], 0.1, status=True)
        assert rows.shape == (0, K) and st.shape == (0,)


@pytest.mark.skipif(have_gpu(), reason="checks the no-device error path")
def test_valid_calls_without_device_fail_loudly(mf):
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        m.init_factors()
        assert _solve(m, USERS, 3, [0, 2, 2, 3], [0, 4, 0], [1, 2, 3])[0] == NO_DEVICE
        assert _solve(m, ITEMS, 2, [0, 0, 0], None, None)[0] == NO_DEVICE
        for call in (lambda: m.fold_in_exact([0, 2, 3], [0, 4, 0], [1.0, 2.0, 3.0]), lambda: m.gram("items"),
                     lambda: m.fold_in_items_implicit([0, 2, 3], [0, 5, 0], [1.0, 2.0, 3.0], 0.1),
                     lambda: m.fit_als([0, 1], [0, 1], [1.0, 2.0], 1)):
            with pytest.raises(mf.MfsgdError) as e:
                call()
            assert e.value.code == NO_DEVICE


# -- the restatement itself ------------------------------------------------------------------------------------------

def _fp64_rows(F, row_ptr, ids, a, b, alpha, ridge, rpe):
    F64 = F.astype(np.float64)
    k = F.shape[1]
    alpha, ridge, rpe = (float(np.float32(v)) for v in (alpha, ridge, rpe))  # the numbers the call gets
    G = F64.T @ F64
    out = np.zeros((row_ptr.size - 1, k))
    for x in range(row_ptr.size - 1):
        s = slice(row_ptr[x], row_ptr[x + 1])
        if s.stop == s.start:
            continue
        f = F64[ids[s]]
        aa = np.ones(f.shape[0]) if a is None else a[s].astype(np.float64)
        A = (f * aa[:, None]).T @ f + alpha * G + (rpe * f.shape[0] + ridge) * np.eye(k)
        out[x] = np.linalg.solve(A, f.T @ b[s].astype(np.float64))
    return out


def _rel_err(got, want):
    live = np.abs(want).max(axis=1) > 0
    return float((np.abs(got[live] - want[live]).max(axis=1) / np.abs(want[live]).max(axis=1)).max())


# The largest relative max-norm error of a solved row against the fp64 solve, over every k of K_ALL, the plain, the
# weighted and the implicit form, as observed with gcc 13 / glibc 2.39 on x86-64; the restatement is deterministic (fmaf,
# sqrtf and / are correctly rounded), so the factor of 2 only absorbs another libm or compiler.
# The largest are k = 1 (one quotient of two sums, the upper one cancelling) and the implicit form at k = 256 (G of
# 300 rows is close to singular there, 1.96e-5); in between the error is 0.7e-6 to 4.2e-6.
OBSERVED_REL_ERR = 1.981e-5
REL_ERR_BOUND = 2 * OBSERVED_REL_ERR


@pytest.mark.parametrize("k", sc.K_ALL)
def test_the_restatement_solves_the_gpu_inputs_and_agrees_with_fp64(k):
    c = sc.case(k)
    worst = 0.0
    for name, (got, st), want in (
            ("exact", sc.exact(c["F"], c["row_ptr"], c["ids"], c["r"], sc.LAM_EXACT),
             _fp64_rows(c["F"], c["row_ptr"], c["ids"], None, c["r"], 0.0, 0.0, sc.LAM_EXACT)),
            ("weighted", sc.exact(c["F"], c["row_ptr"], c["ids"], c["r"], sc.LAM_EXACT, c["w"]),
             _fp64_rows(c["F"], c["row_ptr"], c["ids"], c["w"], c["w"] * c["r"], 0.0, 0.0, sc.LAM_EXACT)),
            ("implicit", sc.implicit(c["F"], c["row_ptr"], c["ids"], c["c"], sc.LAM_IMPLICIT),
             _fp64_rows(c["F"], c["row_ptr"], c["ids"], c["c"] - np.float32(1.0), c["c"], 1.0, sc.LAM_IMPLICIT, 0.0))):
        assert not st.any(), f"{name} k={k}: the restatement refuses rows {np.flatnonzero(st)}"
        assert np.isfinite(got).all()
        empty = np.diff(c["row_ptr"]) == 0
        assert empty.sum() >= 2 and not got[empty].any() and not np.signbit(got[empty]).any()
        err = _rel_err(got, want)
        print(f"k={k} {name}: relative max-norm error {err:.3e}")
        worst = max(worst, err)
    assert worst <= REL_ERR_BOUND


def test_the_gram_restatement_against_fp64():
    rng = np.random.default_rng(3)
    for n, k in ((1, 3), (257, 12), (1000, 64), (65537, 8)):
        F = sc.fixed_side(n, k, rng)
        G = sc.gram(F)
        want = F.astype(np.float64).T @ F.astype(np.float64)
        assert np.array_equal(G, G.T)
        # a chain of n fmas: n * 2^-24 relative to sum |f_p f_q|, which the product of the norms bounds
        scale = np.sqrt(np.outer(np.diag(want), np.diag(want)))
        assert (np.abs(G - want) <= n * 2.0 ** -24 * scale + 1e-45).all()


def _nan_row(x):
    return x.view(np.uint32).tolist() == [0x7FC00000] * x.size


def test_the_expected_refusals():
    rng = np.random.default_rng(8)
    for k in (16, 64, 100, 256):
        F = sc.fixed_side(300, k, rng)
        ids = rng.integers(0, 300, 5).astype(np.int32)
        r = rng.uniform(0.5, 5.0, 5).astype(np.float32)
        rows, st = sc.call(F, [0, 5], ids, None, r)         # rank 5 and no ridge
        assert st[0] in (6, 7) and _nan_row(rows[0]), (k, st)
    F = sc.fixed_side(300, 256, rng)
    ids = rng.integers(0, 300, 400).astype(np.int32)
    rows, st = sc.call(F, [0, 400], ids, None, rng.uniform(0.5, 5.0, 400).astype(np.float32))
    assert 200 <= st[0] <= 256 and _nan_row(rows[0]), st   # 400 entries name fewer than 256 distinct rows' worth of rank
    # an empty list as a full solve (not the empty-list shortcut): the first pivot is +0.0f
    A, rhs = sc.system(F, np.empty(0, np.int32), None, np.empty(0, np.float32))
    assert not A.any() and not rhs.any()
    x, status = sc.solve(A, rhs)
    assert status == 1 and _nan_row(x)
    # a NaN pivot is reported, never solved through
    A, rhs = sc.system(F[:, :4].copy(), [0, 1, 2, 3, 4, 5], None, np.ones(6, np.float32), ridge=1.0)
    A[2, 2] = np.nan
    x, status = sc.solve(A, rhs)
    assert status == 3 and _nan_row(x)


def test_the_empty_list_rule():
    rng = np.random.default_rng(1)
    F = sc.fixed_side(20, 8, rng)
    # no ridge at all: a solve would be refused at pivot 1, the rule says zeros and status 0
    rows, st = sc.call(F, [0, 0, 9, 9], rng.integers(0, 20, 9), None, np.ones(9, np.float32), ridge_per_entry=0.05)
    assert st.tolist() == [0, 0, 0]
    assert rows[[0, 2]].view(np.uint32).tolist() == [[0] * 8] * 2 and rows[1].any()
    rows, st = sc.implicit(F, [0, 0], np.empty(0, np.int32), np.empty(0, np.float32), 0.1)
    assert st.tolist() == [0] and rows.view(np.uint32).tolist() == [[0] * 8]


# The smallest fall of the objective over the six half-sweeps below, relative to the objective before it; fp32 rounding
# of the factors moves the objective by about 1e-7 of itself.
# Observed: ALS 0.345, 0.643, 0.401, 0.184, 0.128, 0.092; iALS 0.698, 0.612, 0.386, 0.104, 0.058, 0.039.
SMALLEST_FALL_OBSERVED = 0.039


def test_als_on_the_restatement_falls_at_every_half_sweep():
    u, i, r, c, P0, Q0 = sc.als_case()
    for name, values, fold, objective in (
            ("als", r, lambda F, ptr, ids, v: sc.exact(F, ptr, ids, v, sc.ALS_LAM),
             lambda P, Q: sc.als_objective(P, Q, u, i, r, sc.ALS_LAM)),
            ("ials", c, lambda F, ptr, ids, v: sc.implicit(F, ptr, ids, v, sc.LAM_IMPLICIT),
             lambda P, Q: sc.ials_objective(P, Q, u, i, c, sc.LAM_IMPLICIT, 1.0))):
        P, Q, obj = sc.als_loop(P0, Q0, u, i, values, 3, fold, objective)
        obj = np.concatenate([[objective(P0, Q0)], obj])
        falls = (obj[:-1] - obj[1:]) / obj[:-1]
        print(name, "objective", obj, "relative falls", falls)
        assert np.isfinite(P).all() and np.isfinite(Q).all()
        assert (falls > 1e-4).all(), falls   # far above rounding
