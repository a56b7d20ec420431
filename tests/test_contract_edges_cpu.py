"""The conditions that keep tests/test_contract_edges_gpu.py from being vacuous, on the oracle alone (no GPU): for every
parametrisation that module uses, the inputs are what their family says (non-zero subnormals, -0.0 rows), the oracle
keeps subnormals (its result moves, and differs from the result of the same problem with the subnormal inputs flushed
to zero), the predictions are subnormal or signed zeros, and the RMSE is not zero.  The GPU module asserts the same on
the order its handle exports; here the order is the natural one."""
import numpy as np
import pytest

from tests import edge_inputs as E

EPOCHS = 2


def test_this_process_keeps_subnormals():
    assert E.host_keeps_subnormals()


@pytest.mark.parametrize("case", E.training_cases(), ids=lambda c: c[0])
def test_training_inputs_are_not_vacuous(oracle, case):
    _, fam, make, args, k = case
    U, I, u, i, _ = make(*args)
    P0, Q0, r = E.family(fam, U, I, k, u.size)
    trained = E.oracle_train_from(oracle, P0, Q0, u, i, r, None, EPOCHS)
    E.check_training(oracle, fam, P0, Q0, u, i, r, None, EPOCHS, trained)


@pytest.mark.parametrize("k,fam", E.predict_cases())
def test_predict_inputs_are_not_vacuous(oracle, k, fam):
    P, Q, u, i, r = E.predict_inputs(k, fam)
    want = oracle.predict(P, Q, u, i)
    if fam != "ordinary":
        E.check_inputs(fam, P, Q, r)
    E.check_predictions(fam, want)
    if fam in ("p_subnormal", "q_subnormal"):  # products of a subnormal and a normal of about 1 / sqrt(k)
        assert (want != 0).all() and E.is_subnormal(want).mean() >= 0.9
    assert oracle.rmse(P, Q, u, i, r) != 0


@pytest.mark.parametrize("fam", E.FOLD_IN_FAMILIES)
@pytest.mark.parametrize("k", E.FOLD_IN_K)
def test_fold_in_inputs_are_not_vacuous(oracle, k, fam):
    from tests.test_fold_in_gpu import fold_in_ref

    Q, row_ptr, items, ratings, init = E.fold_in_inputs(k, fam)
    E.check_inputs(fam, init, Q, ratings)
    want = fold_in_ref(oracle, Q, row_ptr, items, ratings, 3, init, E.LR, E.LAM)
    assert np.isfinite(want).all()
    rated = np.diff(row_ptr) > 0
    assert (E.bits(want[rated]) != E.bits(init[rated])).mean() >= 0.5
    if fam == "p_subnormal":  # the rows are the subnormal side: they move by s * Q, which a flushed s would not give
        zi, zq, zr = E.flushed(fam, init, Q, ratings)
        flush = fold_in_ref(oracle, zq, row_ptr, items, zr, 3, zi, E.LR, E.LAM)
        assert (E.bits(want[rated]) != E.bits(flush[rated])).mean() >= 0.5


@pytest.mark.parametrize("k", [4, 64])
def test_edge_scores_are_what_they_claim(oracle, k):
    for kind in E.SCORE_KINDS:
        P, Q, user = E.edge_score_factors(kind, k)
        E.check_edge_scores(kind, E.all_scores(oracle, P, Q, user))


# ---- tests/test_chain_specials_gpu.py: NaN and Inf through the chain waves, apply_ratings and fold-in --------------------
def _order_of(mf, U, I, k, u, i, kw):
    """The order a handle exports (the host scheduler runs without a GPU)."""
    with mf.MatrixFactorizationSGD(U, I, k, E.LR, E.LAM, 11, **kw) as m:
        m.set_ratings(u, i, np.ones(u.size, np.float32))
        return m.order()[0], m.schedule_info(), m.debug_schedule()


def _states(oracle, P, Q, u, i, r, order):
    out = []
    for _ in range(EPOCHS):
        oracle.sgd_pass_ordered(P, Q, u, i, r, order, E.LR, E.LAM)
        out.append((P.copy(), Q.copy(), oracle.rmse(P, Q, u, i, r)))
    return out


@pytest.mark.parametrize("k,W,where", [(k, W, where) for k, W in E.SOLO_KW + (("lone", 2),) for where in E.NAN_PLACES
                                       if k != "lone" or where != "rating_last_step_of_an_odd_run"])  # (its runs are even)
def test_nan_cases_are_not_vacuous(mf, oracle, k, W, where):
    """One all-ones NaN late in the order: after the first epoch between 0.05 % and 60 % of the oracle's entries are NaN
    (Q[hot item]: see E.check_nan_case), and the place really is a step of a solo run of the hot item."""
    item = E.HOT_ITEM
    if k == "lone":
        U, I, k, u, i, r0, kw = E.lone_problem()
        item = E.LONE_ITEM
    else:
        U, I, u, i, kw = E.odd_run_set(mf, k, W) if where == "rating_last_step_of_an_odd_run" else E.hot_item_set(k, W)
        r0 = E.ordinary_ratings(u.size)
    P0, Q0 = E.ordinary_factors(U, I, k)
    P, Q, r, n, step = E.place_nan(where, mf, k, U, I, u, i, kw, P0, Q0, r0, item=item)
    assert (E.bits(P) == 0xFFFFFFFF).sum() + (E.bits(Q) == 0xFFFFFFFF).sum() + (E.bits(r) == 0xFFFFFFFF).sum() == 1
    assert float(np.float32(E.LR) * E.ALL_ONES_NAN) != float(np.float32(E.LR) * E.ALL_ONES_NAN)  # NaN, whatever its payload
    if where.startswith("rating"):
        assert 0 <= step < n and (step % 2 == 1) == (where == "rating_odd_step") and n >= 12
        assert (where != "rating_last_step_of_an_odd_run") or (n % 2 == 1 and step == n - 1)
    order, _, sched = _order_of(mf, U, I, k, u, i, kw)
    assert (sched[0][:, 5] & 1).sum() == (E.LONE_PROBLEM_CELLS if item == E.LONE_ITEM else E.LONE_CELLS[k])
    E.check_nan_case(where, _states(oracle, P, Q, u, i, r, order))


@pytest.mark.parametrize("name,where", E.overflow_cases())
def test_overflow_cases_are_not_vacuous(mf, oracle, name, where):
    make, k, hot = E.OVERFLOW_SETS[name]
    U, I, u, i, kw = make()
    order, info, sched = _order_of(mf, U, I, k, u, i, kw)
    E.check_overflow_set(name, info, sched)
    r = E.overflow_ratings(where, u, i, order, hot)
    assert (np.abs(r) > 1e38).sum() == (20 if where == "on_the_hot_item" else u.size // 100)
    P, Q = oracle.init_factors(U, I, k, 11)
    E.check_overflow_case(where, _states(oracle, P, Q, u, i, r, order))


@pytest.mark.parametrize("batch,kind,k", E.ONLINE_SPECIALS)
def test_online_specials_are_not_vacuous(oracle, batch, kind, k):
    from tests.test_online_gpu import SEED, _oracle_apply

    U, I, u, i, r, at = E.online_special_batch(batch, kind)
    P0, Q0 = oracle.init_factors(U, I, k, SEED)
    P, Q, err = _oracle_apply(oracle, P0, Q0, u, i, r)
    E.check_online_special(kind, at, err, P, Q)


@pytest.mark.parametrize("k", E.FOLD_IN_K)
def test_fold_in_specials_are_not_vacuous(oracle, k):
    from tests.test_fold_in_gpu import fold_in_ref

    Q, row_ptr, items, ratings, init = E.fold_in_specials(k)
    E.check_fold_in_specials(fold_in_ref(oracle, Q, row_ptr, items, ratings, 3, init, E.LR, E.LAM))
