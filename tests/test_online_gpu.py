"""Online updates on the device (csrc/online.hip, mfsgd_apply_ratings): P, Q and the pre-update errors against the
oracle's sequential loop, bit for bit, for every lane-group size and for the level shapes that reach each launch path --
one wide level, runs of narrow ones, a hot row inside a wide batch, widths at the boundary between the two, two pieces;
and that a live handle stays whole: its schedules, cached graphs, rating identity, held-out set and device memory."""
import numpy as np
import pytest

from tests import online_common as oc

pytestmark = pytest.mark.gpu

LR, LAM, SEED = 0.01, 0.05, 4
ALL_K = (1, 3, 4, 5, 8, 12, 16, 17, 32, 33, 64, 65, 128, 129, 256)


def _group_lanes(k):
    """L: lanes per rating, the power of two that holds k floats in chunks of four."""
    L = 1
    while 4 * L < k:
        L *= 2
    return L


def _oracle_apply(oracle, P, Q, u, i, r, lr=LR, lam=LAM, errors=True):
    """The sequential loop on copies of P and Q: (P, Q, err), err by the oracle's own update, one rating at a time."""
    P, Q = P.copy(), Q.copy()
    if not errors:
        oracle.sgd_pass(P, Q, u, i, r, lr, lam)
        return P, Q, None
    err = np.empty(u.size, np.float32)
    for j in range(u.size):
        err[j] = oracle.sgd_update(P[u[j]], Q[i[j]], float(r[j]), lr, lam)
    return P, Q, err


def _check(mf, oracle, U, I, k, u, i, r):
    """partial_fit on a freshly seeded model against the oracle from the same seed; returns the call's info."""
    P0, Q0 = oracle.init_factors(U, I, k, SEED)
    P, Q, err = _oracle_apply(oracle, P0, Q0, u, i, r)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as m:
        m.init_factors()
        got_err, info = m.partial_fit(u, i, r, errors=True, info=True)
        gP, gQ = m.get_factors()
    assert np.array_equal(gP, P) and np.array_equal(gQ, Q)
    assert np.array_equal(got_err, err)
    want = oc.py_info(oc.py_levels(u, i))
    assert {x: info[x] for x in want} == want
    return info


@pytest.mark.parametrize("k", ALL_K)
def test_every_lane_group_size(mf, oracle, k):
    U, I, u, i, r = oc.random_batch()
    info = _check(mf, oracle, U, I, k, u, i, r)
    assert 1 <= info["launches"] <= info["levels"]


@pytest.mark.parametrize("k", (64, 5))
def test_one_wide_level_is_one_launch(mf, oracle, k):
    U, I, u, i, r = oc.distinct_batch()
    info = _check(mf, oracle, U, I, k, u, i, r)
    assert info["levels"] == 1 and info["max_width"] == 5000 and info["launches"] == 1


@pytest.mark.parametrize("k", (64, 5))
@pytest.mark.parametrize("make", (oc.one_item_batch, oc.one_user_batch, oc.same_pair_batch), ids=("one_item", "one_user", "same_pair"))
def test_a_chain_is_walked_by_one_workgroup(mf, oracle, make, k):
    U, I, u, i, r = make()
    info = _check(mf, oracle, U, I, k, u, i, r)
    assert info["levels"] == u.size and info["max_width"] == 1 and info["launches"] <= 2


@pytest.mark.parametrize("k", (64, 5))
def test_a_hot_item_inside_a_wide_batch(mf, oracle, k):
    U, I, u, i, r = oc.hot_item_batch()
    info = _check(mf, oracle, U, I, k, u, i, r)
    assert info["levels"] >= 300 and 1 < info["launches"] < info["levels"]


@pytest.mark.parametrize("k", (64, 5, 256, 1))
def test_widths_at_the_boundary_between_narrow_and_wide(mf, oracle, k):
    """Levels of exactly one workgroup pass, one rating more, and one rating, in succession; then every narrow width."""
    G = 256 // _group_lanes(k)
    widths = oc.boundary_widths(G)
    U, I, u, i, r = oc.widths_batch(widths)
    assert list(np.bincount(oc.py_levels(u, i))) == widths
    info = _check(mf, oracle, U, I, k, u, i, r)
    # wide levels: the G + 1 ones, a launch each; the narrow ones between them: one launch per run
    assert info["launches"] == 5 and info["max_width"] == G + 1


def test_two_pieces(mf, oracle):
    U, I, u, i, r = oc.two_piece_batch(4097)
    k = 8
    P0, Q0 = oracle.init_factors(U, I, k, SEED)
    P, Q, _ = _oracle_apply(oracle, P0, Q0, u, i, r, errors=False)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as m:
        m.init_factors()
        err, info = m.partial_fit(u, i, r, errors=True, info=True)
        gP, gQ = m.get_factors()
    assert info["pieces"] == 2 and info["n"] == oc.PIECE + 4097
    assert np.array_equal(gP, P) and np.array_equal(gQ, Q)
    # the errors of the second piece's ratings, by the oracle from the factors after the first piece
    P1, Q1, _ = _oracle_apply(oracle, P0, Q0, u[:oc.PIECE], i[:oc.PIECE], r[:oc.PIECE], errors=False)
    _, _, tail = _oracle_apply(oracle, P1, Q1, u[oc.PIECE:], i[oc.PIECE:], r[oc.PIECE:])
    assert np.array_equal(err[oc.PIECE:], tail) and np.isfinite(err).all()


@pytest.mark.parametrize("name", ("solo_k64_w2", "hot_user"))
def test_a_live_handle_stays_whole(mf, oracle, name):
    """set_ratings, fit(1), partial_fit(batch), fit(1): the stored set, its schedule and its graphs serve the second
    epoch as they served the first, on the updated rows."""
    from tests.test_hyper_cpu import PROBLEMS, SEED as MODEL_SEED, fresh

    U, I, u, i, r = PROBLEMS[name][0]()
    k = PROBLEMS[name][1]
    rng = np.random.default_rng(31)
    n = 2000
    bu, bi = rng.integers(0, U, n).astype(np.int32), rng.integers(0, I, n).astype(np.int32)
    br = (rng.integers(1, 11, n) * 0.5).astype(np.float32)
    with fresh(mf, name, LR, LAM) as m:
        assert m.schedule_info()["swapped"] == (1 if name == "hot_user" else 0)
        m.init_factors()
        order = m.order()[0]
        m.fit(1, rmse=False)
        before = m.debug_counters()
        info = m.partial_fit(bu, bi, br, info=True)
        assert info["n"] == n and info["launches"] >= 1
        assert m.debug_counters() == before  # schedule builds, cached graphs, the launch path
        assert np.array_equal(m.order()[0], order)
        m.fit(1, rmse=False)
        gP, gQ = m.get_factors()
        m.set_ratings(u, i, r)  # the same triples are still recognised
        assert m.debug_counters()["schedule_builds"] == before["schedule_builds"] == 1
    P, Q = oracle.init_factors(U, I, k, MODEL_SEED)
    oracle.sgd_pass_ordered(P, Q, u, i, r, order, LR, LAM)
    oracle.sgd_pass(P, Q, bu, bi, br, LR, LAM)
    oracle.sgd_pass_ordered(P, Q, u, i, r, order, LR, LAM)
    assert np.array_equal(gP, P) and np.array_equal(gQ, Q)


def test_no_stored_ratings_are_needed(mf, oracle):
    U, I, u, i, r = oc.random_batch()
    k = 20
    rng = np.random.default_rng(2)
    P0 = rng.standard_normal((U, k)).astype(np.float32) * 0.3
    Q0 = rng.standard_normal((I, k)).astype(np.float32) * 0.3
    P, Q, err = _oracle_apply(oracle, P0, Q0, u, i, r)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as m:
        m.set_factors(P0, Q0)
        got = m.partial_fit(u, i, r, errors=True)
        gP, gQ = m.get_factors()
        pu, pi = np.repeat(np.arange(U, dtype=np.int32), I), np.tile(np.arange(I, dtype=np.int32), U)
        pred = m.predict(pu, pi)
    assert np.array_equal(gP, P) and np.array_equal(gQ, Q) and np.array_equal(got, err)
    assert np.array_equal(pred, oracle.predict(P, Q, pu, pi))


def test_the_current_hyper_parameters_are_used(mf, oracle):
    U, I, u, i, r = oc.random_batch()
    k, lr2, lam2 = 16, 0.03, 0.002
    P0, Q0 = oracle.init_factors(U, I, k, SEED)
    lr32, lam32 = float(np.float32(lr2)), float(np.float32(lam2))
    P, Q, err = _oracle_apply(oracle, P0, Q0, u, i, r, lr32, lam32)
    Pold, _, _ = _oracle_apply(oracle, P0, Q0, u, i, r, errors=False)
    assert not np.array_equal(P, Pold)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as m:
        m.init_factors()
        m.set_hyper(lr2, lam2)
        got = m.partial_fit(u, i, r, errors=True)
        gP, gQ = m.get_factors()
    assert np.array_equal(gP, P) and np.array_equal(gQ, Q) and np.array_equal(got, err)


def test_the_held_out_set_sees_the_updated_rows(mf, oracle):
    U, I, u, i, r = oc.random_batch()
    k = 64
    hu, hi, hr = oc.random_batch(seed=77, n=1000)[2:]
    P0, Q0 = oracle.init_factors(U, I, k, SEED)
    P, Q, _ = _oracle_apply(oracle, P0, Q0, u, i, r, errors=False)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as m:
        m.init_factors()
        m.set_validation(hu, hi, hr)
        first = m.validation_rmse()  # (the set is on the device from here on)
        np.testing.assert_allclose(first, oracle.rmse(P0, Q0, hu, hi, hr), rtol=1e-9, atol=1e-12)
        m.partial_fit(u, i, r)
        assert m.validation_size() == 1000
        # the bar of tests/test_validation_gpu.py for this call against the oracle: the order of the fp64 sum differs
        np.testing.assert_allclose(m.validation_rmse(), oracle.rmse(P, Q, hu, hi, hr), rtol=1e-9, atol=1e-12)
        assert m.validation_rmse() != first


def test_no_device_memory_is_kept(mf):
    U, I, u, i, r = oc.random_batch()
    start = mf.debug_device_bytes()
    with mf.MatrixFactorizationSGD(U, I, 64, LR, LAM, SEED) as m:
        m.init_factors()
        m.predict([0], [0])  # the handle is on the device
        before = mf.debug_device_bytes()
        assert before > start
        m.partial_fit(u, i, r, errors=True)
        assert mf.debug_device_bytes() == before
        m.partial_fit(u, i, r)
        assert mf.debug_device_bytes() == before
        with pytest.raises(mf.MfsgdError) as e:
            m.partial_fit([0, U], [0, 0], [1.0, 1.0])
        assert e.value.code == -1 and mf.debug_device_bytes() == before
    assert mf.debug_device_bytes() == start
