"""Held-out validation on the device: the streaming SSE kernel over arbitrary pairs (csrc/validate.hip) against the
oracle for every lane-group size and at the pair counts where its launch changes shape; the determinism its header
promises; the pieces of mfsgd_rmse_pairs; mfsgd_train_early_stop against a replay of its rule on the oracle, down to
the bits of the factors it leaves; and that none of it keeps device memory or touches the model."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

U, I, SEED = 37, 29, 11
K_OF_L = {1: 1, 2: 5, 4: 9, 8: 20, 16: 64, 32: 100, 64: 256}  # one k per lane-group size
COUNTS = (1, 63, 257, 100_003)  # one group; a ragged wave; a ragged workgroup; many strides over the partials
PIECE = 1 << 20  # pairs per upload of mfsgd_rmse_pairs (include/mfsgd.h)
RTOL, ATOL = 1e-9, 1e-12  # the bar of device fp64 RMSE against the oracle (tests/test_hyper_gpu.py): the order of the sum differs


def _flags(name):
    from mfsgd_amd import _lib

    return 0 if name == "default" else getattr(_lib, name)


def _bits(x):
    return np.float64(x).tobytes()


def _pairs(n, rng=None):
    """n pairs drawn with replacement (duplicates occur), (U - 1, I - 1) among them and, from two pairs on, (0, 0)."""
    rng = rng or np.random.default_rng(1000 + n)
    u, i = rng.integers(0, U, n).astype(np.int32), rng.integers(0, I, n).astype(np.int32)
    r = (rng.integers(1, 11, n) * 0.5).astype(np.float32)
    u[0], i[0] = U - 1, I - 1
    if n > 1:
        u[-1], i[-1] = 0, 0
    return u, i, r


@pytest.fixture(scope="module")
def trained(mf):
    """Per k: a model of U x I after one trained epoch, and its factors.  Built on demand, closed with the module."""
    made = {}

    def get(k):
        if k not in made:
            rng = np.random.default_rng(k)
            key = rng.choice(U * I, 400, replace=False)
            m = mf.MatrixFactorizationSGD(U, I, k, 0.02, 0.01, SEED)
            m.set_ratings(key // I, key % I, (rng.integers(1, 11, key.size) * 0.5).astype(np.float32))
            m.init_factors()
            m.fit(1, rmse=False)
            made[k] = (m,) + m.get_factors()
        return made[k]

    yield get
    for m, _, _ in made.values():
        m.close()


# -- 1. the SSE against the oracle ----------------------------------------------------------------------------------
@pytest.mark.parametrize("n", COUNTS)
@pytest.mark.parametrize("L", sorted(K_OF_L))
def test_sse_matches_the_oracle(trained, oracle, L, n):
    m, P, Q = trained(K_OF_L[L])
    assert m.kp == 4 * L
    u, i, r = _pairs(n)
    want_rmse, want_sse = oracle.rmse(P, Q, u, i, r), oracle.sse(P, Q, u, i, r)
    m.set_validation(u, i, r)
    assert m.validation_size() == n
    kept = m.validation_rmse(sse=True)
    given = m.rmse_on(u, i, r, sse=True)
    print(f"L={L} n={n}: rmse {kept[0]!r} oracle {want_rmse!r} rel {abs(kept[0] - want_rmse) / want_rmse:.3e}")
    for got in (kept, given):
        np.testing.assert_allclose(got[0], want_rmse, rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(got[1], want_sse, rtol=RTOL, atol=ATOL)
    assert _bits(kept[0]) == _bits(given[0]) and _bits(kept[1]) == _bits(given[1]), "the kept set and the given pairs are one launch"
    assert m.validation_rmse() == kept[0]


@pytest.mark.parametrize("L", (1, 16, 64))
def test_empty_set_and_nan(trained, L):
    m, _, _ = trained(K_OF_L[L])
    m.set_validation([], [], [])
    assert m.validation_rmse(sse=True) == (0.0, 0.0)
    assert m.rmse_on([], [], []) == 0.0
    for n, at in ((1, 0), (300, 0), (300, 171), (300, 299)):  # (pair 0 is also what the groups past the end compute on)
        u, i, r = _pairs(n)
        r[at] = np.nan
        m.set_validation(u, i, r)
        assert np.isnan(m.validation_rmse()) and np.isnan(m.rmse_on(u, i, r)), (n, at)
    u, i, r = _pairs(300)
    r[171] = np.inf
    assert np.isinf(m.rmse_on(u, i, r))


def test_swapped_roles_give_the_same_answers(mf, oracle):
    """A schedule that exchanged the roles hands the kernels (Q, P); the held-out pairs are still (user, item)."""
    from tests.test_hyper_cpu import PROBLEMS, fresh

    with fresh(mf, "hot_user", 0.01, 0.05) as m:
        assert m.schedule_info()["swapped"] == 1
        Uh, Ih = m.users, m.items
        m.init_factors()
        m.fit(1, rmse=False)
        P, Q = m.get_factors()
        rng = np.random.default_rng(2)
        u, i = rng.integers(0, Uh, 5000).astype(np.int32), rng.integers(0, Ih, 5000).astype(np.int32)
        u[0], i[0] = Uh - 1, 0  # (in range only when read as (user, item): U < I here)
        i[1], u[1] = Ih - 1, 0
        r = rng.random(5000, dtype=np.float32)
        assert Uh < Ih and PROBLEMS["hot_user"][3] == "swapped"
        m.set_validation(u, i, r)
        np.testing.assert_allclose(m.validation_rmse(), oracle.rmse(P, Q, u, i, r), rtol=RTOL, atol=ATOL)
        np.testing.assert_allclose(m.rmse_on(u, i, r), oracle.rmse(P, Q, u, i, r), rtol=RTOL, atol=ATOL)


# -- 2. determinism -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", (16, 32))
def test_same_bits_whatever_the_handle(mf, trained, L):
    from mfsgd_amd import _lib

    k = K_OF_L[L]
    m, P, Q = trained(k)
    u, i, r = _pairs(100_003)
    m.set_validation(u, i, r)
    first = m.validation_rmse(sse=True)
    assert [_bits(x) for x in m.validation_rmse(sse=True)] == [_bits(x) for x in first]
    assert [_bits(x) for x in m.rmse_on(u, i, r, sse=True)] == [_bits(x) for x in first]
    for kw in (dict(blocks=1, waves=1), dict(blocks=3, waves=4, flags=_lib.FLAG_ROUND_LAUNCH), dict(blocks=2, waves=8, flags=_lib.FLAG_NO_GRAPH)):
        with mf.MatrixFactorizationSGD(U, I, k, 0.5, 0.25, 99, **kw) as other:
            other.set_factors(P, Q)
            other.set_validation(u, i, r)
            assert [_bits(x) for x in other.validation_rmse(sse=True)] == [_bits(x) for x in first], kw
            assert [_bits(x) for x in other.rmse_on(u, i, r, sse=True)] == [_bits(x) for x in first], kw


# -- 3. the pieces of mfsgd_rmse_pairs ----------------------------------------------------------------------------------
def test_pieces_add_up_in_order(mf, oracle):
    Ub, Ib, k, n = 2000, 1500, 8, 2_500_000
    rng = np.random.default_rng(8)
    P, Q = (rng.random((Ub, k), np.float32) - 0.5), (rng.random((Ib, k), np.float32) - 0.5)
    u, i = rng.integers(0, Ub, n).astype(np.int32), rng.integers(0, Ib, n).astype(np.int32)
    r = rng.random(n, dtype=np.float32)
    assert PIECE < n < 3 * PIECE and n % PIECE
    with mf.MatrixFactorizationSGD(Ub, Ib, k, 0.01, 0.0, 1) as m:
        m.set_factors(P, Q)
        rm, sse = m.rmse_on(u, i, r, sse=True)
        total = None
        for j0 in range(0, n, PIECE):
            s = m.rmse_on(u[j0:j0 + PIECE], i[j0:j0 + PIECE], r[j0:j0 + PIECE], sse=True)[1]
            total = s if total is None else total + s  # fp64, in order
        assert _bits(sse) == _bits(total)
        assert _bits(rm) == _bits(np.sqrt(np.float64(total) / np.float64(n)))
        # exactly one piece is still the kept set's launch
        m.set_validation(u[:PIECE], i[:PIECE], r[:PIECE])
        assert _bits(m.validation_rmse(sse=True)[1]) == _bits(m.rmse_on(u[:PIECE], i[:PIECE], r[:PIECE], sse=True)[1])
    np.testing.assert_allclose(sse, oracle.sse(P, Q, u, i, r), rtol=RTOL, atol=ATOL)


# -- 4. early stopping against the oracle's replay of the rule -------------------------------------------------------------
ES_U, ES_I, ES_TRAIN, ES_HELD, ES_LR, ES_EPOCHS, ES_SEED, ES_MARGIN = 300, 200, 6000, 1500, 0.05, 25, 3, 1e-6
ES_DECAY = (ES_LR * 0.97 ** np.arange(ES_EPOCHS)).astype(np.float32)


def _es_problem():
    """Distinct pairs with ratings of a rank-4 signal plus noise, in half stars: (training triples, held-out triples)."""
    rng = np.random.default_rng(4)
    a, b = rng.standard_normal((ES_U, 4)), rng.standard_normal((ES_I, 4))
    key = rng.choice(ES_U * ES_I, ES_TRAIN + ES_HELD, replace=False)
    u, i = (key // ES_I).astype(np.int32), (key % ES_I).astype(np.int32)
    noise = rng.standard_normal(key.size)
    r = np.clip(np.round(2 * (3 + 0.5 * (a[u] * b[i]).sum(1) + 0.5 * noise)) / 2, 0.5, 5).astype(np.float32)
    return (u[:ES_TRAIN], i[:ES_TRAIN], r[:ES_TRAIN]), (u[ES_TRAIN:], i[ES_TRAIN:], r[ES_TRAIN:])


def _rule(val, patience, min_delta):
    """The rule of include/mfsgd.h over a whole curve: (epochs_run, best_epoch, smallest margin of a decision)."""
    best, best_epoch, bad, margin = np.inf, -1, 0, np.inf
    for e, v in enumerate(val):
        margin = min(margin, abs(v - (best - min_delta)))
        if v < best - min_delta:
            best, best_epoch, bad = v, e, 0
        else:
            bad += 1
            if bad >= patience:
                return e + 1, best_epoch, margin
    return len(val), best_epoch, margin


_es_cache = {}


def _es_reference(oracle, k, order, decay):
    """The oracle over all ES_EPOCHS epochs in the order the handle exports: the held-out and training curves and the
    factors after every epoch.  Computed once per (k, order, rates), never modified."""
    key = (k, order.tobytes(), decay)
    if key not in _es_cache:
        train, held = _es_problem()
        P, Q = oracle.init_factors(ES_U, ES_I, k, ES_SEED)
        val, trn, factors = [], [], []
        for e in range(ES_EPOCHS):
            oracle.sgd_pass_ordered(P, Q, *train, order, float(ES_DECAY[e]) if decay else ES_LR, 0.0)
            val.append(oracle.rmse(P, Q, *held))
            trn.append(oracle.rmse(P, Q, *train))
            factors.append((P.copy(), Q.copy()))
        _es_cache[key] = (np.array(val), np.array(trn), factors)
    return _es_cache[key]


def _es_model(mf, k, flag):
    train, held = _es_problem()
    m = mf.MatrixFactorizationSGD(ES_U, ES_I, k, ES_LR, 0.0, ES_SEED, blocks=2, waves=2, flags=_flags(flag))
    m.set_ratings(*train)
    m.set_validation(*held)
    m.init_factors()
    return m


def _es_expect(oracle, m, k, patience, min_delta, decay=False):
    """What the reference says the call must do; the conditions on the reference alone are asserted here, first."""
    val, trn, factors = _es_reference(oracle, k, m.order()[0], decay)
    ran, best, margin = _rule(val, patience, min_delta)
    assert margin > ES_MARGIN, f"a decision within {margin:.2e}: change the seed of the problem"
    assert 0 < best < ran - 1 < ES_EPOCHS - 1, (ran, best)
    return val, trn, factors, ran, best


@pytest.mark.parametrize("restore", [True, False])
@pytest.mark.parametrize("min_delta", [0.0, 0.01])
@pytest.mark.parametrize("flag", ["default", "FLAG_ROUND_LAUNCH"])
@pytest.mark.parametrize("k", [64, 100])
def test_early_stopping_replays_on_the_oracle(mf, oracle, k, flag, min_delta, restore):
    with _es_model(mf, k, flag) as m:
        val, trn, factors, ran, best = _es_expect(oracle, m, k, 3, min_delta)
        if min_delta > 0:  # the larger threshold stops earlier, at another best epoch
            ran0, best0, _ = _rule(val, 3, 0.0)
            assert ran < ran0 and best < best0
        res = m.fit_early_stopping(ES_EPOCHS, patience=3, min_delta=min_delta, restore_best=restore, train_rmse=restore)
        P, Q = m.get_factors()
        after = m.validation_rmse()
    print(f"k={k} {flag} min_delta={min_delta}: ran {res['epochs_run']} best {res['best_epoch']} (oracle {ran}, {best}); "
          f"max rel {np.abs(res['val_rmse'] / val[:res['epochs_run']] - 1).max():.3e}")
    assert (res["epochs_run"], res["best_epoch"]) == (ran, best)
    assert res["val_rmse"].shape == (ran,)
    np.testing.assert_allclose(res["val_rmse"], val[:ran], rtol=RTOL)
    if restore:
        np.testing.assert_allclose(res["train_rmse"], trn[:ran], rtol=RTOL)
    else:
        assert res["train_rmse"] is None
    Po, Qo = factors[best if restore else ran - 1]
    assert np.array_equal(P, Po), f"P differs: max abs {np.abs(P - Po).max()}"
    assert np.array_equal(Q, Qo), f"Q differs: max abs {np.abs(Q - Qo).max()}"
    assert _bits(after) == _bits(res["val_rmse"][best if restore else ran - 1]), "the factors left are the ones that were measured"


@pytest.mark.parametrize("flag", ["default", "FLAG_ROUND_LAUNCH"])
def test_early_stopping_under_a_decaying_rate(mf, oracle, flag):
    k = 64
    with _es_model(mf, k, flag) as m:
        val, trn, factors, ran, best = _es_expect(oracle, m, k, 3, 0.0, decay=True)
        res = m.fit_early_stopping(ES_EPOCHS, patience=3, lr=ES_DECAY, train_rmse=True)
        assert (res["epochs_run"], res["best_epoch"]) == (ran, best)
        assert m.hyper() == (float(ES_DECAY[ran - 1]), 0.0) == (m.lr, m.lam)
        np.testing.assert_allclose(res["val_rmse"], val[:ran], rtol=RTOL)
        np.testing.assert_allclose(res["train_rmse"], trn[:ran], rtol=RTOL)
        P, Q = m.get_factors()
        assert np.array_equal(P, factors[best][0]) and np.array_equal(Q, factors[best][1])
        # the call can be made again: it goes on from the restored factors, at the rates given
        more = m.fit_early_stopping(1, lr=[ES_LR], lam=[0.0])
        assert more["epochs_run"] == 1 and more["best_epoch"] == 0 and m.hyper() == (float(np.float32(ES_LR)), 0.0)


def test_early_stopping_that_never_improves(mf):
    """A NaN curve: nothing ever compares below +inf, so the call stops after `patience` epochs with best_epoch -1 and
    the factors as trained (nothing is restored), and epochs beyond are untouched."""
    train, held = _es_problem()
    with mf.MatrixFactorizationSGD(ES_U, ES_I, 64, ES_LR, 0.0, ES_SEED, blocks=2, waves=2) as m, \
            mf.MatrixFactorizationSGD(ES_U, ES_I, 64, ES_LR, 0.0, ES_SEED, blocks=2, waves=2) as ref:
        r = held[2].copy()
        r[700] = np.nan
        for x in (m, ref):
            x.set_ratings(*train)
            x.init_factors()
        m.set_validation(held[0], held[1], r)
        res = m.fit_early_stopping(10, patience=2)
        assert res["epochs_run"] == 2 and res["best_epoch"] == -1 and np.isnan(res["val_rmse"]).all()
        ref.fit(2, rmse=False)
        for a, b in zip(m.get_factors(), ref.get_factors()):
            assert np.array_equal(a, b)


# -- 5. memory ----------------------------------------------------------------------------------------------------------
def test_nothing_is_kept_on_the_device(mf):
    train, held = _es_problem()
    start = mf.debug_device_bytes()
    m = mf.MatrixFactorizationSGD(ES_U, ES_I, 64, ES_LR, 0.0, ES_SEED, blocks=2, waves=2)
    m.set_ratings(*train)
    m.init_factors()
    m.fit(1, rmse=False)
    before = mf.debug_device_bytes()
    m.rmse_on(*held)
    assert mf.debug_device_bytes() == before
    m.set_validation(*held)
    assert mf.debug_device_bytes() == before, "the set is the host's until it is measured"
    m.validation_rmse()
    with_set = mf.debug_device_bytes()
    assert with_set > before
    for restore in (True, False):
        m.fit_early_stopping(4, patience=1, restore_best=restore)
        assert mf.debug_device_bytes() == with_set, restore
    m.set_validation(held[0][:10], held[1][:10], held[2][:10])  # a replaced set takes the old one's memory with it
    assert mf.debug_device_bytes() == before
    m.validation_rmse()
    m.set_validation([], [], [])
    assert mf.debug_device_bytes() == before
    m.set_validation(*held)
    m.validation_rmse()
    assert mf.debug_device_bytes() == with_set
    m.close()  # ... while it still holds a set
    assert mf.debug_device_bytes() == start


# -- 6. the model is not touched ----------------------------------------------------------------------------------------------
def test_measuring_leaves_the_model_alone(mf, oracle):
    train, held = _es_problem()
    k = 64
    with _es_model(mf, k, "default") as m:
        m.fit(1, rmse=False)
        P, Q = m.get_factors()
        order, cell_ptr = m.order()
        m.validation_rmse()
        m.rmse_on(*held)
        m.rmse_on(*train)
        P2, Q2 = m.get_factors()
        order2, cell_ptr2 = m.order()
        assert np.array_equal(P, P2) and np.array_equal(Q, Q2)
        assert np.array_equal(order, order2) and np.array_equal(cell_ptr, cell_ptr2)
        rm = m.fit(2)
        P3, Q3 = m.get_factors()
    val, trn, factors = _es_reference(oracle, k, order, False)
    assert np.array_equal(P3, factors[2][0]) and np.array_equal(Q3, factors[2][1])
    np.testing.assert_allclose(rm, trn[1:3], rtol=RTOL, atol=ATOL)
