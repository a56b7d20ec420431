"""mfsgd_recommend_excluding checks its arguments before any device work, so that these checks run without a GPU;
a valid call without a device fails with MFSGD_ERR_NO_DEVICE, never with a CPU result."""
import ctypes as C

import numpy as np
import pytest

from tests.conftest import have_gpu

INVALID_ARG, NO_DEVICE = -1, -2
U, I = 6, 5


def _call(m, users, topn, eu, ei, n_excl):
    """The raw C-ABI call: None stands for a NULL pointer."""
    def ptr(a):
        return None if a is None else np.ascontiguousarray(a, np.int32).ctypes.data_as(C.POINTER(C.c_int32))

    uu = np.ascontiguousarray(users, np.int32)
    items = np.empty(max(1, uu.size * topn), np.int32)
    scores = np.empty(max(1, uu.size * topn), np.float32)
    return m._lib.mfsgd_recommend_excluding(m._handle(), ptr(uu), uu.size, topn, ptr(eu), ptr(ei), n_excl,
                                            ptr(items), scores.ctypes.data_as(C.POINTER(C.c_float)))


@pytest.fixture
def model(mf):
    with mf.MatrixFactorizationSGD(U, I, 8, 0.01, 0.05, 1) as m:
        m.init_factors()
        yield m


@pytest.mark.parametrize("eu,ei,n_excl", [
    ([0], [1], -1),           # negative count
    (None, [1], 1),           # NULL user array
    ([0], None, 1),           # NULL item array
    (None, None, 2),          # both NULL
    ([0, -1], [1, 1], 2),     # user below range
    ([0, U], [1, 1], 2),      # user above range
    ([0, 1], [1, -1], 2),     # item below range
    ([0, 1], [1, I], 2),      # item above range
    ([5, U + 7], [0, 0], 2),  # out of range even though that user is not requested
])
def test_bad_exclusions_are_invalid_arguments(model, eu, ei, n_excl):
    assert _call(model, [0, 2], 3, eu, ei, n_excl) == INVALID_ARG
    assert "recommend" in model._lib.mfsgd_last_error(model._h).decode()


def test_python_exclude_shapes_are_checked(model):
    with pytest.raises(ValueError):
        model.recommend([0], 2, exclude=([0, 1], [1]))


@pytest.mark.skipif(have_gpu(), reason="checks the no-device error path")
@pytest.mark.parametrize("eu,ei,n_excl", [([0, 3, 0], [1, 4, 1], 3), (None, None, 0)])
def test_valid_call_without_device_fails_loudly(model, mf, eu, ei, n_excl):
    assert _call(model, [0, 2], 3, eu, ei, n_excl) == NO_DEVICE
    with pytest.raises(mf.MfsgdError) as ei_:
        model.recommend([0, 2], 3, exclude=([0, 3], [1, 4]))
    assert ei_.value.code == NO_DEVICE
