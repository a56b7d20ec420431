"""The arithmetic contract (fp32, round to nearest even, SUBNORMALS KEPT, the sign of a zero as
IEEE gives it) at the edges of fp32, on every path that computes with the factors: training through each loop form of
the epoch kernel, whoever computes lr * r (host packer, device packer, the re-bake), predict, RMSE and fold-in.

The reference is the oracle replaying the order the handle exports, from factors the test sets.  Factors compare bit for
bit (tobytes: -0.0 is not +0.0), RMSE to 1e-9 relative with NO absolute term -- the values are around 1e-39.  What keeps
each comparison from being vacuous (the inputs really are subnormal, the oracle's result moves and differs from a
flushed run's, real -0.0 dots occur) is asserted on the oracle's side only: tests/edge_inputs.py, and without a GPU in
tests/test_contract_edges_cpu.py."""
import numpy as np
import pytest

from tests import edge_inputs as E
from tests.test_gpu_parity import _same_schedule

pytestmark = pytest.mark.gpu

EPOCHS = 2


def _sign_only(a, b):
    """For a failure message: do two arrays differ in nothing but the sign of zeros?"""
    return bool(np.array_equal(a, b))


def _train_from(mf, oracle, fam, U, I, k, u, i, P0, Q0, r, seen=None, **kw):
    """set_ratings, set_factors(P0, Q0), fit(EPOCHS) against the oracle over the exported order; returns
    (schedule_info, debug_schedule).  seen: {order: the oracle's result} of the runs of one test on the same inputs
    (the oracle spends about a second on 12 000 subnormal ratings at k = 256: one replay per distinct order)."""
    assert E.host_keeps_subnormals()
    with mf.MatrixFactorizationSGD(U, I, k, E.LR, E.LAM, 11, **kw) as m:
        m.set_ratings(u, i, r)
        m.set_factors(P0, Q0)
        rm = m.fit(EPOCHS)
        P, Q = m.get_factors()
        order, cell_ptr = m.order()
        info = m.schedule_info()
        sched = m.debug_schedule()
        rm_again = m.rmse()
    assert oracle.check_block_schedule(u, i, U, I, order, cell_ptr, info["rounds"], info["blocks"]) == 0
    seen = {} if seen is None else seen
    if order.tobytes() not in seen:
        seen[order.tobytes()] = E.oracle_train_from(oracle, P0, Q0, u, i, r, order, EPOCHS)
        if len(seen) == 1:
            E.check_training(oracle, fam, P0, Q0, u, i, r, order, EPOCHS, seen[order.tobytes()])
    Po, Qo, rmo = seen[order.tobytes()]
    print(f"{fam} k={k}: rmse {rm.tolist()} oracle {rmo.tolist()}; subnormal entries of the oracle's P "
          f"{E.is_subnormal(Po).mean():.2f}, Q {E.is_subnormal(Qo).mean():.2f}")
    for name, got, want in (("P", P, Po), ("Q", Q, Qo)):
        assert got.tobytes() == want.tobytes(), (
            f"{name} differs in {(E.bits(got) != E.bits(want)).mean():.3f} of its entries"
            f" (only in the sign of zeros: {_sign_only(got, want)})")
    np.testing.assert_allclose(rm, rmo, rtol=1e-9, atol=0)
    np.testing.assert_allclose(rm_again, rmo[-1], rtol=1e-9, atol=0)
    return info, sched


def _solo_steps(sched):
    return int((sched[2][:, 0] >> 16).sum())


# ---- A2: training through every loop form ---------------------------------------------------------------------------------
@pytest.mark.parametrize("case", E.training_cases(), ids=lambda c: c[0])
def test_training_keeps_subnormals_and_signed_zeros(mf, oracle, case):
    from mfsgd_amd import _lib

    name, fam, make, args, k = case
    U, I, u, i, kw = make(*args)
    P0, Q0, r = E.family(fam, U, I, k, u.size)
    if make is E.hot_item_set:  # run loops, solo runs (chain wave + helper wave) and their one-wave forms
        seen = {}
        for flags in (0, _lib.FLAG_ROUND_LAUNCH, _lib.FLAG_NO_SOLO):
            _, sched = _train_from(mf, oracle, fam, U, I, k, u, i, P0, Q0, r, seen=seen, flags=flags, **kw)
            assert (_solo_steps(sched) == 0) == (flags == _lib.FLAG_NO_SOLO), (flags, _solo_steps(sched))
        return
    info, _ = _train_from(mf, oracle, fam, U, I, k, u, i, P0, Q0, r, **kw)
    if make is E.chunked_set:
        assert info["split_cells"] >= 1
    if make is E.hot_user_set:
        assert info["swapped"] == 1


# ---- A3: whoever computes lr * r ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("form", ["general", "solo"])
def test_subnormal_lr_times_r_is_the_same_word_whoever_computes_it(mf, form):
    """Host packer, device packer and the device re-bake on subnormal ratings: lr * r is a subnormal (at lr = 1e-3 often
    within a few units of the smallest one, so that rounding decides it), and every build holds the same words."""
    from mfsgd_amd import _lib
    from tests.test_hyper_cpu import assert_same, snapshot

    k = 64
    U, I, u, i, kw = E.general_set(k) if form == "general" else E.hot_item_set(k, 2)
    _, _, r = E.family("p_subnormal", U, I, k, u.size)
    lr2, lam2 = 1e-3, 0.02
    prod = np.float32(lr2) * r  # (numpy's fp32 product: one rounding, subnormals kept)
    assert E.host_keeps_subnormals() and E.is_subnormal(r).all()
    assert E.is_subnormal(prod).mean() >= 0.9 and (prod < np.float32(1e-42)).sum() >= 100
    assert (prod.astype(np.float64) != r.astype(np.float64) * float(np.float32(lr2))).mean() >= 0.5  # rounded
    _same_schedule(mf, U, I, k, u, i, r, **kw)
    made = []
    for lr, lam in ((E.LR, E.LAM), (lr2, lam2)):
        m = mf.MatrixFactorizationSGD(U, I, k, lr, lam, 5, flags=_lib.FLAG_DEVICE_INGEST, **kw)
        made.append(m)
        m.set_ratings(u, i, r)
    m, f = made
    try:
        if form == "solo":
            assert _solo_steps(f.debug_schedule()) > 0
        packed = m.schedule_info()["device_ingest"] == 2 and f.schedule_info()["device_ingest"] == 2
        assert packed, "the device packer must have taken this set"
        # the words a fresh handle holds are the oracle-side products: every lr2 * r is among its entries' third words
        words = np.unique(f.debug_schedule()[3][:, 2])
        assert np.isin(E.bits(prod), words).all()
        m.set_hyper(lr2, lam2)
        assert_same(snapshot(m), snapshot(f), "device re-bake of subnormal lr * r")
    finally:
        m.close()
        f.close()


# ---- A4: predict, RMSE, fold-in -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k,fam", E.predict_cases())
def test_predict_and_rmse_every_width_at_the_edges(mf, oracle, k, fam):
    P, Q, u, i, r = E.predict_inputs(k, fam)
    want = oracle.predict(P, Q, u, i)
    E.check_predictions(fam, want)
    assert E.host_keeps_subnormals()
    with mf.MatrixFactorizationSGD(P.shape[0], Q.shape[0], k, E.LR, E.LAM, 1) as m:
        m.set_factors(P, Q)
        got = m.predict(u, i)
        m.set_ratings(u, i, r)
        rmse = m.rmse()
    assert got.tobytes() == want.tobytes(), f"{(E.bits(got) != E.bits(want)).sum()} of {want.size} predictions differ"
    ref = oracle.rmse(P, Q, u, i, r)
    assert ref != 0
    np.testing.assert_allclose(rmse, ref, rtol=1e-9, atol=0)


@pytest.mark.parametrize("fam", E.FOLD_IN_FAMILIES)
@pytest.mark.parametrize("k", E.FOLD_IN_K)
def test_fold_in_keeps_subnormals(mf, oracle, k, fam):
    from tests.test_fold_in_gpu import fold_in_ref

    Q, row_ptr, items, ratings, init = E.fold_in_inputs(k, fam)
    want = fold_in_ref(oracle, Q, row_ptr, items, ratings, 3, init, E.LR, E.LAM)
    assert E.host_keeps_subnormals() and np.isfinite(want).all()
    with mf.MatrixFactorizationSGD(4, Q.shape[0], k, E.LR, E.LAM, 1) as m:
        m.set_factors(np.zeros((4, k), np.float32), Q)
        got = m.fold_in(row_ptr, items, ratings, 3, init=init)
    assert got.tobytes() == want.tobytes(), f"{(E.bits(got) != E.bits(want)).mean():.3f} of the entries differ"


# ---- A5: overflow ---------------------------------------------------------------------------------------------------------
def _assert_same_but_for_the_nans(name, got, want):
    nan = np.isnan(want)
    assert np.array_equal(np.isnan(got), nan), f"{name}: {(np.isnan(got) != nan).sum()} entries are NaN on one side only"
    assert got[~nan].tobytes() == want[~nan].tobytes(), f"{name}: entries that are not NaN differ"


@pytest.mark.parametrize("where", ["anywhere", "last_in_the_order"])
def test_overflow_goes_to_infinity_and_nan_where_the_oracle_does(mf, oracle, where):
    """1 % of the ratings at +-3e38: rows go to +-inf and then to NaN.  Which entries are NaN, and every bit of the
    others (infinities included), are the contract; the sign and payload of a NaN are not (x86 and the GPU differ).
    NaN spreads through every row it meets: with the large ratings anywhere, all of P and Q is NaN within the first
    epoch (on the oracle, in natural order as well), which compares masks and nothing else.  So the second case puts them
    at the end of the order the handle exports -- the order depends on (u, i) only, which is asserted -- and compares after
    each epoch: after the first the oracle holds finite, infinite and NaN entries side by side."""
    k = 64
    U, I, u, i, _ = E.general_set(k)
    rng = np.random.default_rng(5)
    r = (rng.random(u.size) * 4 + 1).astype(np.float32)
    n_big = u.size // 100
    huge = np.where(rng.random(n_big) < 0.5, np.float32(3e38), np.float32(-3e38))
    with mf.MatrixFactorizationSGD(U, I, k, E.LR, E.LAM, 11) as m:
        m.set_ratings(u, i, r)
        order, _ = m.order()
        r[rng.choice(u.size, n_big, replace=False) if where == "anywhere" else order[-n_big:]] = huge
        m.set_ratings(u, i, r)
        assert np.array_equal(m.order()[0], order)
        m.init_factors()
        got = []
        for _ in range(EPOCHS):
            rm = m.fit(1)
            got.append(m.get_factors() + (rm[0],))
    Po, Qo = oracle.init_factors(U, I, k, 11)
    seen_finite = seen_inf = seen_nan = False
    was_finite = True
    for epoch, (P, Q, rm) in enumerate(got):
        oracle.sgd_pass_ordered(Po, Qo, u, i, r, order, E.LR, E.LAM)
        rmo = oracle.rmse(Po, Qo, u, i, r)
        print(f"{where}, epoch {epoch + 1}: NaN P {np.isnan(Po).mean():.3f} Q {np.isnan(Qo).mean():.3f}; inf P "
              f"{np.isinf(Po).mean():.3f} Q {np.isinf(Qo).mean():.3f}; rmse {rm} oracle {rmo}")
        _assert_same_but_for_the_nans("P", P, Po)
        _assert_same_but_for_the_nans("Q", Q, Qo)
        assert np.isfinite(rm) == np.isfinite(rmo)
        if np.isfinite(rmo):
            assert was_finite
            np.testing.assert_allclose(rm, rmo, rtol=1e-9, atol=0)
        was_finite = bool(np.isfinite(rmo))
        both = np.concatenate([Po.ravel(), Qo.ravel()])
        mixed = np.isfinite(both).any() and np.isinf(both).any() and np.isnan(both).any()
        seen_finite, seen_inf, seen_nan = seen_finite or mixed, seen_inf or mixed, seen_nan or np.isnan(both).any()
    assert seen_nan and not was_finite
    if where == "last_in_the_order":
        assert seen_finite and seen_inf, "no epoch left finite, infinite and NaN entries side by side"
