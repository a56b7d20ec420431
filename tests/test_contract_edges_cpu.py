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
