"""The held-out set of a handle and the calls that measure it, as far as they go without a GPU: every argument and
state error has its code and its message prefix and comes before any device is asked for; the set is host-only until
it is measured (size round-trips, empty arrays clear it, it survives set_ratings and set_hyper); the calls that do
nothing succeed without a device; and a valid measuring call without a GPU is MFSGD_ERR_NO_DEVICE, never a CPU result."""
import ctypes as C

import numpy as np
import pytest

from tests.conftest import have_gpu

INVALID, NO_DEVICE, STATE = -1, -2, -5
U, I, K = 9, 7, 5


def _model(mf, **kw):
    return mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, **kw)


def _raises(mf, code, prefix, call):
    with pytest.raises(mf.MfsgdError) as ei:
        call()
    assert ei.value.code == code, ei.value
    assert f": {prefix}: " in str(ei.value), ei.value


def _ready(m):
    """Ratings, factors and a held-out set: everything a measuring call needs but the device."""
    m.set_ratings([0, 1, 2, 8], [0, 1, 2, 6], [1.0, 2.0, 3.0, 4.0])
    m.init_factors()
    m.set_validation([3, 8], [4, 6], [2.5, 3.5])


def _early_stop(m, max_epochs=3, patience=2, min_delta=0.0, lr=None, lam=None, val=True, ran=True, best=True):
    """mfsgd_train_early_stop with any of its pointers left out."""
    f32 = lambda a: None if a is None else np.asarray(a, np.float32)
    lr, lam = f32(lr), f32(lam)
    out = np.zeros(max(max_epochs, 1), np.float64)
    e, b = C.c_int32(-7), C.c_int32(-7)
    p = lambda a, t: None if a is None else a.ctypes.data_as(C.POINTER(t))
    m._check(m._lib.mfsgd_train_early_stop(m._handle(), max_epochs, patience, min_delta, 1, p(lr, C.c_float), p(lam, C.c_float),
                                           p(out, C.c_double) if val else None, None, C.byref(e) if ran else None,
                                           C.byref(b) if best else None))
    return e.value, b.value


def test_pair_lists_are_checked(mf):
    with _model(mf) as m:
        m.init_factors()
        for prefix, call in (("set_validation", m.set_validation), ("rmse_pairs", m.rmse_on)):
            _raises(mf, INVALID, prefix, lambda: call([0, U], [0, 1], [1.0, 2.0]))   # user out of range
            _raises(mf, INVALID, prefix, lambda: call([0, -1], [0, 1], [1.0, 2.0]))
            _raises(mf, INVALID, prefix, lambda: call([0, 1], [0, I], [1.0, 2.0]))   # item out of range
            _raises(mf, INVALID, prefix, lambda: call([0, 1], [-1, 1], [1.0, 2.0]))
        i32, f32, f64 = C.POINTER(C.c_int32), C.POINTER(C.c_float), C.POINTER(C.c_double)
        a, r = np.zeros(2, np.int32), np.ones(2, np.float32)
        pa, pr = a.ctypes.data_as(i32), r.ctypes.data_as(f32)
        rm = C.c_double()
        lib, h = m._lib, m._handle()
        _raises(mf, INVALID, "set_validation", lambda: m._check(lib.mfsgd_set_validation(h, pa, pa, pr, -1)))
        _raises(mf, INVALID, "rmse_pairs", lambda: m._check(lib.mfsgd_rmse_pairs(h, pa, pa, pr, -1, C.byref(rm), None)))
        for args in ((None, pa, pr), (pa, None, pr), (pa, pa, None)):
            _raises(mf, INVALID, "set_validation", lambda: m._check(lib.mfsgd_set_validation(h, *args, 2)))
            _raises(mf, INVALID, "rmse_pairs", lambda: m._check(lib.mfsgd_rmse_pairs(h, *args, 2, C.byref(rm), None)))
        _raises(mf, INVALID, "rmse_pairs", lambda: m._check(lib.mfsgd_rmse_pairs(h, pa, pa, pr, 2, None, None)))
        _raises(mf, INVALID, "validation_rmse", lambda: m._check(lib.mfsgd_validation_rmse(h, None, None)))
        _raises(mf, INVALID, "validation_size", lambda: m._check(lib.mfsgd_validation_size(h, None)))
        assert m.validation_size() == 0, "a rejected set must not replace anything"


def test_early_stop_arguments_are_checked(mf):
    with _model(mf) as m:
        _ready(m)
        nan = float("nan")
        _raises(mf, INVALID, "early_stop", lambda: _early_stop(m, max_epochs=-1))
        _raises(mf, INVALID, "early_stop", lambda: _early_stop(m, patience=0))
        _raises(mf, INVALID, "early_stop", lambda: _early_stop(m, patience=-3))
        _raises(mf, INVALID, "early_stop", lambda: _early_stop(m, min_delta=nan))
        _raises(mf, INVALID, "early_stop", lambda: _early_stop(m, min_delta=-1e-9))
        _raises(mf, INVALID, "early_stop", lambda: _early_stop(m, lr=[0.01, nan, 0.01]))
        _raises(mf, INVALID, "early_stop", lambda: _early_stop(m, lam=[0.0, 0.0, nan]))
        _raises(mf, INVALID, "early_stop", lambda: _early_stop(m, val=False))
        _raises(mf, INVALID, "early_stop", lambda: _early_stop(m, ran=False))
        _raises(mf, INVALID, "early_stop", lambda: _early_stop(m, best=False))
        _raises(mf, INVALID, "early_stop", lambda: _early_stop(m, max_epochs=0, ran=False))  # ... even when nothing would run
        with pytest.raises(ValueError):
            m.fit_early_stopping(3, lr=[0.01, 0.02])
        assert m.hyper() == (float(np.float32(0.01)), float(np.float32(0.05))), "a rejected call changes nothing"


def test_the_set_is_host_only_and_survives(mf):
    rng = np.random.default_rng(0)
    n = 1000
    u, i, r = rng.integers(0, U, n), rng.integers(0, I, n), rng.random(n, dtype=np.float32)
    with _model(mf) as m:
        assert m.validation_size() == 0
        m.set_validation(u, i, r)
        assert m.validation_size() == n
        m.set_validation(u[:10], i[:10], r[:10])  # replaces
        assert m.validation_size() == 10
        m.set_ratings(u, i, r)
        m.set_hyper(0.02, 0.0)
        m.init_factors()
        m.set_factors(*m.get_factors())
        assert m.validation_size() == 10
        m.set_validation([], [], [])
        assert m.validation_size() == 0
        # n == 0 with null pointers clears as well
        m.set_validation(u, i, r)
        m._check(m._lib.mfsgd_set_validation(m._handle(), None, None, None, 0))
        assert m.validation_size() == 0
        if not have_gpu():
            assert mf.debug_device_bytes() == 0


def test_state_errors(mf):
    with _model(mf, n_parts=2) as m:
        m.set_ratings([0, 1], [0, 1], [1.0, 2.0])
        m.init_p_offset(1, 0)
        _raises(mf, STATE, "set_validation", lambda: m.set_validation([0], [0], [1.0]))
        _raises(mf, STATE, "validation_rmse", m.validation_rmse)
        _raises(mf, STATE, "rmse_pairs", lambda: m.rmse_on([0], [0], [1.0]))
        _raises(mf, STATE, "early_stop", lambda: _early_stop(m))
        assert _early_stop(m, max_epochs=0) == (0, -1)
    with _model(mf) as m:  # factors never initialised
        m.set_ratings([0, 1], [0, 1], [1.0, 2.0])
        m.set_validation([0], [0], [1.0])
        _raises(mf, STATE, "validation_rmse", m.validation_rmse)
        _raises(mf, STATE, "rmse_pairs", lambda: m.rmse_on([0], [0], [1.0]))
        _raises(mf, STATE, "early_stop", lambda: _early_stop(m))
    with _model(mf) as m:  # no ratings
        m.init_factors()
        m.set_validation([0], [0], [1.0])
        _raises(mf, STATE, "early_stop", lambda: _early_stop(m))
    with _model(mf) as m:  # no validation set
        m.set_ratings([0, 1], [0, 1], [1.0, 2.0])
        m.init_factors()
        _raises(mf, STATE, "early_stop", lambda: _early_stop(m))
        m.set_validation([0], [0], [1.0])
        m.set_validation([], [], [])  # ... or a cleared one
        _raises(mf, STATE, "early_stop", lambda: _early_stop(m))


def test_calls_that_do_nothing_need_no_device(mf):
    with _model(mf) as m:
        _ready(m)
        P, Q = m.get_factors()
        assert _early_stop(m, max_epochs=0) == (0, -1)
        res = m.fit_early_stopping(0)
        assert res["epochs_run"] == 0 and res["best_epoch"] == -1 and res["val_rmse"].size == 0 and res["train_rmse"] is None
        assert m.rmse_on([], [], []) == 0.0 and m.rmse_on([], [], [], sse=True) == (0.0, 0.0)
        rm = C.c_double(-1.0)
        m._check(m._lib.mfsgd_rmse_pairs(m._handle(), None, None, None, 0, C.byref(rm), None))
        assert rm.value == 0.0
        m.set_validation([], [], [])
        assert m.validation_rmse() == 0.0 and m.validation_rmse(sse=True) == (0.0, 0.0)  # an empty set, like mfsgd_rmse
        for a, b in zip((P, Q), m.get_factors()):
            assert np.array_equal(a, b)


def test_measuring_without_a_device_fails_loudly(mf):
    with _model(mf) as m:
        _ready(m)
        calls = (m.validation_rmse, lambda: m.rmse_on([0, 1], [0, 1], [1.0, 2.0]), lambda: m.fit_early_stopping(2),
                 lambda: m.fit_early_stopping(2, restore_best=False, train_rmse=True))
        if have_gpu():
            for call in calls:
                call()  # (the values are tests/test_validation_gpu.py's business)
            return
        for call in calls:
            with pytest.raises(mf.MfsgdError) as ei:
                call()
            assert ei.value.code == NO_DEVICE, ei.value  # never a CPU result
        assert m.validation_size() == 2
