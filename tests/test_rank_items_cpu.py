"""The host side of the ranking calls: mfsgd_ranking_metrics_from_ranks against the same formulas in numpy fp64, and
the argument checks of mfsgd_rank_items / mfsgd_rank_items_rows / mfsgd_evaluate_ranking, which come before any
device work and therefore run without a GPU.  A valid call without a device fails with MFSGD_ERR_NO_DEVICE, never
with a CPU result."""
import ctypes as C

import numpy as np
import pytest

from tests.conftest import have_gpu

INVALID_ARG, NO_DEVICE = -1, -2
U, I, K = 6, 5, 8
FIELDS = ("hit_rate", "precision", "recall", "ndcg", "mrr")
# the metrics are sums of at most a few thousand fp64 terms in [0, 1], divided once: n * 2^-53 is far below this
ATOL = 1e-12


def _metrics_ref(users, ranks, topn):
    """The header's formulas, per user, in fp64."""
    users, ranks = np.asarray(users, np.int64), np.asarray(ranks, np.int64)
    out = dict(n_pairs=users.size, n_users=0, **{f: 0.0 for f in FIELDS})
    per = {f: [] for f in FIELDS}
    for u in np.unique(users):
        r = np.sort(ranks[users == u])
        hits = r[r < topn]
        per["hit_rate"].append(float(hits.size > 0))
        per["precision"].append(hits.size / topn)
        per["recall"].append(hits.size / r.size)
        idcg = np.sum(1.0 / np.log2(np.arange(min(r.size, topn), dtype=np.float64) + 2.0))
        per["ndcg"].append(np.sum(1.0 / np.log2(hits.astype(np.float64) + 2.0)) / idcg)
        per["mrr"].append(1.0 / (r[0] + 1.0))
        out["n_users"] += 1
    for f in FIELDS:
        out[f] = float(np.mean(per[f])) if per[f] else 0.0
    return out


def _assert_metrics(got, want):
    assert got["n_pairs"] == want["n_pairs"] and got["n_users"] == want["n_users"]
    for f in FIELDS:
        assert abs(got[f] - want[f]) <= ATOL, (f, got[f], want[f])


def test_metrics_of_the_worked_example(mf):
    got = mf.ranking_metrics([0, 0, 2], [0, 4, 5], 3)
    want = dict(n_pairs=3, n_users=2, hit_rate=0.5, precision=1.0 / 6.0, recall=0.25,
                ndcg=0.5 / (1.0 + 1.0 / np.log2(3.0)), mrr=(1.0 + 1.0 / 6.0) / 2.0)
    _assert_metrics(got, want)
    _assert_metrics(got, _metrics_ref([0, 0, 2], [0, 4, 5], 3))
    assert abs(got["ndcg"] - 0.30657359) < 1e-8


@pytest.mark.parametrize("topn", [1, 10, 500])
def test_metrics_match_numpy_on_random_pairs(mf, topn):
    rng = np.random.default_rng(topn)
    users = rng.integers(0, 300, 2000).astype(np.int32)
    ranks = rng.integers(0, 1500, 2000).astype(np.int32)
    ranks[rng.integers(0, 2000, 300)] = rng.integers(0, 12, 300)  # enough hits at the small cut-offs
    got = mf.ranking_metrics(users, ranks, topn)
    _assert_metrics(got, _metrics_ref(users, ranks, topn))
    assert got["n_users"] == np.unique(users).size
    # the order of the pairs does not matter
    perm = rng.permutation(2000)
    assert mf.ranking_metrics(users[perm], ranks[perm], topn) == got


def test_metrics_of_no_pairs_are_zero(mf):
    got = mf.ranking_metrics([], [], 10)
    assert got == dict(n_pairs=0, n_users=0, hit_rate=0.0, precision=0.0, recall=0.0, ndcg=0.0, mrr=0.0)


def _ptr(a, dtype=np.int32, ctype=C.c_int32):
    """None stands for a NULL pointer."""
    return None if a is None else np.ascontiguousarray(a, dtype).ctypes.data_as(C.POINTER(ctype))


def _metrics_call(mf, users, ranks, n, topn, with_out=True):
    from mfsgd_amd import _lib

    lib = mf.load_library()
    out = _lib.RankingMetrics()
    rc = lib.mfsgd_ranking_metrics_from_ranks(_ptr(users), _ptr(ranks), n, topn, C.byref(out) if with_out else None)
    return rc, lib.mfsgd_last_error(None).decode()


@pytest.mark.parametrize("users,ranks,n,topn,with_out", [
    ([0, 1], [0, 1], -1, 3, True),    # negative n
    (None, [0, 1], 2, 3, True),       # NULL users
    ([0, 1], None, 2, 3, True),       # NULL ranks
    ([0, 1], [0, 1], 2, 3, False),    # NULL out
    ([0, 1], [0, 1], 2, 0, True),     # topn = 0
    ([0, 1], [0, 1], 2, -4, True),
    ([0, 1], [3, -1], 2, 3, True),    # a negative rank
])
def test_bad_metrics_arguments(mf, users, ranks, n, topn, with_out):
    rc, msg = _metrics_call(mf, users, ranks, n, topn, with_out)
    assert rc == INVALID_ARG
    assert msg.startswith("ranking_metrics: ")


@pytest.fixture
def model(mf):
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:
        m.init_factors()
        yield m


def _rank_call(m, users, items, n, eu, ei, n_excl, with_out=True):
    out = np.zeros(max(1, abs(n)), np.int32)
    return m._lib.mfsgd_rank_items(m._handle(), _ptr(users), _ptr(items), n, _ptr(eu), _ptr(ei), n_excl,
                                   _ptr(out) if with_out else None)


def _rows_call(m, rows, n_rows, row, items, n, er, ei, n_excl, with_out=True):
    out = np.zeros(max(1, abs(n)), np.int32)
    return m._lib.mfsgd_rank_items_rows(m._handle(), _ptr(rows, np.float32, C.c_float), n_rows, _ptr(row), _ptr(items), n,
                                        _ptr(er), _ptr(ei), n_excl, _ptr(out) if with_out else None)


def _eval_call(m, users, items, n, topn, eu, ei, n_excl, with_out=True):
    from mfsgd_amd import _lib

    out = _lib.RankingMetrics()
    ranks = np.zeros(max(1, abs(n)), np.int32)
    return m._lib.mfsgd_evaluate_ranking(m._handle(), _ptr(users), _ptr(items), n, topn, _ptr(eu), _ptr(ei), n_excl,
                                         C.byref(out) if with_out else None, _ptr(ranks))


BAD_PAIRS = [
    # users, items, n, excl_u, excl_i, n_excl, out_rank given
    ([0, 2], [1, 1], -1, [0], [1], 1, True),          # negative n
    ([0, 2], [1, 1], 2, [0], [1], -1, True),          # negative n_excl
    (None, [1, 1], 2, [0], [1], 1, True),             # each NULL pointer
    ([0, 2], None, 2, [0], [1], 1, True),
    ([0, 2], [1, 1], 2, None, [1], 1, True),
    ([0, 2], [1, 1], 2, [0], None, 1, True),
    ([0, 2], [1, 1], 2, [0], [1], 1, False),
    ([0, -1], [1, 1], 2, [0], [1], 1, True),          # pair list: user below / above, item below / above
    ([0, U], [1, 1], 2, [0], [1], 1, True),
    ([0, 2], [1, -1], 2, [0], [1], 1, True),
    ([0, 2], [1, I], 2, [0], [1], 1, True),
    ([0, 2], [1, 1], 2, [0, -1], [1, 1], 2, True),    # exclusion list: the same
    ([0, 2], [1, 1], 2, [0, U], [1, 1], 2, True),
    ([0, 2], [1, 1], 2, [0, 2], [1, -1], 2, True),
    ([0, 2], [1, 1], 2, [0, 2], [1, I], 2, True),
    ([0, 2], [1, 1], 2, [5, U + 7], [0, 0], 2, True),  # out of range even though nobody asked about that user
]


@pytest.mark.parametrize("users,items,n,eu,ei,n_excl,with_out", BAD_PAIRS)
def test_bad_rank_arguments_are_invalid_arguments(model, users, items, n, eu, ei, n_excl, with_out):
    def message():
        return model._lib.mfsgd_last_error(model._h).decode()

    assert _rank_call(model, users, items, n, eu, ei, n_excl, with_out) == INVALID_ARG
    assert message().startswith("rank_items: ")
    # the same with a row matrix of the call's own
    rows = np.ones((U, K), np.float32)
    assert _rows_call(model, rows, U, users, items, n, eu, ei, n_excl, with_out) == INVALID_ARG
    assert message().startswith("rank_items: ")
    if with_out:  # (evaluate_ranking may be given no rank array)
        assert _eval_call(model, users, items, n, 3, eu, ei, n_excl) == INVALID_ARG
        assert message().startswith("rank_items: ")


def test_more_bad_arguments(model):
    def message():
        return model._lib.mfsgd_last_error(model._h).decode()

    rows = np.ones((3, K), np.float32)
    assert _rows_call(model, None, 3, [0], [1], 1, None, None, 0) == INVALID_ARG      # NULL row matrix
    assert message().startswith("rank_items: ")
    assert _rows_call(model, rows, -3, [0], [1], 1, None, None, 0) == INVALID_ARG     # negative n_rows
    assert message().startswith("rank_items: ")
    assert _rows_call(model, rows, 3, [3], [1], 1, None, None, 0) == INVALID_ARG      # a row P has, the matrix has not
    assert _rows_call(model, rows, 3, [0], [1], 1, [3], [1], 1) == INVALID_ARG
    assert message().startswith("rank_items: ")
    for topn in (0, -2):
        assert _eval_call(model, [0, 2], [1, 1], 2, topn, None, None, 0) == INVALID_ARG
        assert message().startswith("rank_items: ") or message().startswith("ranking_metrics: ")
    assert _eval_call(model, [0, 2], [1, 1], 2, 3, None, None, 0, with_out=False) == INVALID_ARG  # NULL metrics struct
    assert message().startswith("rank_items: ")


def test_no_pairs_is_ok_and_touches_nothing(model, mf):
    before = mf.debug_device_bytes()
    assert _rank_call(model, None, None, 0, None, None, 0, with_out=False) == 0
    assert _rank_call(model, None, None, 0, [0, 3], [1, 4], 2, with_out=False) == 0
    assert model.rank_items([], []).shape == (0,)
    res = model.evaluate_ranking([], [], 10)
    assert res["ranks"].shape == (0,) and res["n_pairs"] == 0 and res["ndcg"] == 0.0
    assert mf.debug_device_bytes() == before


def test_states_that_cannot_rank(mf):
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1) as m:   # factors never initialised
        assert _rank_call(m, [0], [1], 1, None, None, 0) == -5
        assert _rank_call(m, None, None, 0, None, None, 0, with_out=False) == 0  # (no pairs: nothing is needed)
        assert m._lib.mfsgd_last_error(m._h).decode().startswith("rank_items: ")
    with mf.MatrixFactorizationSGD(U, I, K, 0.01, 0.05, 1, n_parts=2) as m:
        m.init_factors()
        assert _rank_call(m, [0], [1], 1, None, None, 0) == -5
        assert _eval_call(m, [0], [1], 1, 3, None, None, 0) == -5
        assert _rows_call(m, np.ones((2, K), np.float32), 2, [0], [1], 1, None, None, 0) == -5


def test_python_shapes_are_checked(model, mf):
    with pytest.raises(ValueError):
        model.rank_items([0, 1], [1])
    with pytest.raises(ValueError):
        model.rank_items([0], [1], exclude=([0, 1], [1]))
    with pytest.raises(ValueError):
        model.rank_items([[0, 1]], [[1, 2]])
    with pytest.raises(ValueError):
        model.evaluate_ranking([0, 1], [1], 3)
    with pytest.raises(ValueError):
        model.evaluate_ranking([0], [1], 3, exclude=([0], [1, 2]))
    with pytest.raises(ValueError):
        model.rank_items_rows(np.ones((2, K + 1), np.float32), [0], [1])
    with pytest.raises(ValueError):
        model.rank_items_rows(np.ones((2, K), np.float32), [0, 1], [1])
    with pytest.raises(ValueError):
        model.rank_items_rows(np.ones((2, K), np.float32), [0], [1], exclude=([0, 1], [1]))
    with pytest.raises(ValueError):
        mf.ranking_metrics([0, 1], [1], 3)


@pytest.mark.skipif(have_gpu(), reason="checks the no-device error path")
def test_valid_call_without_device_fails_loudly(model, mf):
    assert _rank_call(model, [0, 2, 0], [1, 4, 1], 3, [0, 3, 0], [1, 4, 1], 3) == NO_DEVICE
    assert _rank_call(model, [0, 2], [1, 4], 2, None, None, 0) == NO_DEVICE
    assert _eval_call(model, [0, 2], [1, 4], 2, 3, [0, 3], [1, 4], 2) == NO_DEVICE
    assert _rows_call(model, np.ones((3, K), np.float32), 3, [0, 2], [1, 4], 2, None, None, 0) == NO_DEVICE
    for call in (lambda: model.rank_items([0, 2], [1, 4], exclude=([0, 3], [1, 4])),
                 lambda: model.evaluate_ranking([0, 2], [1, 4], 3),
                 lambda: model.rank_items_rows(np.ones((3, K), np.float32), [0, 2], [1, 4])):
        with pytest.raises(mf.MfsgdError) as e:
            call()
        assert e.value.code == NO_DEVICE
