"""mfsgd_set_hyper, mfsgd_train_schedule and mfsgd_train_bold_driver on the device: training through a change of lr
and lambda equals the oracle run at those values epoch by epoch, bit for bit, on every launch path (a stale graph or a
stale lr / c kernel argument would show); the device re-bake (csrc/rehyper.hip) writes the bytes a fresh handle holds,
on the packer's own buffers and on the adopted ones; fold-in and DSGD partitions follow; no device memory is kept."""
import numpy as np
import pytest

from tests.test_hyper_cpu import PAIRS, PROBLEMS, SEED, assert_same, fresh, snapshot

pytestmark = pytest.mark.gpu

STAGES = (((0.01, 0.05), 2), ((0.006, 0.02), 2), ((0.02, 0.0), 1))  # ((lr, lambda), epochs)


def _flags(name):
    from mfsgd_amd import _lib

    return 0 if name == "default" else getattr(_lib, name)


def _problem(name):
    make, k, kw, _ = PROBLEMS[name]
    return (k, kw) + make()


_oracle_cache = {}


def _oracle_stages(oracle, name, order):
    """Factors and RMSEs of the oracle over STAGES, in the order the handle exports: computed once per (problem, order)."""
    key = (name, order.tobytes())
    if key not in _oracle_cache:
        k, kw, U, I, u, i, r = _problem(name)
        P, Q = oracle.init_factors(U, I, k, SEED)
        rm = []
        for (lr, lam), epochs in STAGES:
            for _ in range(epochs):
                oracle.sgd_pass_ordered(P, Q, u, i, r, order, lr, lam)
                rm.append(oracle.rmse(P, Q, u, i, r))
        _oracle_cache[key] = (P, Q, np.array(rm))
    return _oracle_cache[key]


@pytest.mark.parametrize("flag", ["default", "FLAG_ROUND_LAUNCH", "FLAG_NO_GRAPH", "FLAG_HOST_INGEST", "FLAG_DEVICE_INGEST"])
@pytest.mark.parametrize("name", ["solo_k64_w2", "solo_k128_w4", "run_k32_w2", "chunked_k256"])
def test_parity_through_a_change_of_values(mf, oracle, name, flag):
    (lr0, lam0), _ = STAGES[0]
    with fresh(mf, name, lr0, lam0, flags=_flags(flag)) as m:
        if flag == "FLAG_DEVICE_INGEST":
            assert m.schedule_info()["device_ingest"] == 2, "the entries must exist on the device only"
        m.init_factors()
        rm = []
        for (lr, lam), epochs in STAGES:
            m.set_hyper(lr, lam)
            rm += list(m.fit(epochs))
        P, Q = m.get_factors()
        order = m.order()[0]
        again = m.rmse()
    Po, Qo, rmo = _oracle_stages(oracle, name, order)
    assert np.array_equal(P, Po), f"P differs: max abs {np.abs(P - Po).max()}"
    assert np.array_equal(Q, Qo), f"Q differs: max abs {np.abs(Q - Qo).max()}"
    np.testing.assert_allclose(rm, rmo, rtol=1e-9, atol=1e-12)
    assert abs(again - rm[-1]) <= 1e-12


@pytest.mark.parametrize("trained", [False, True])
@pytest.mark.parametrize("pair", range(len(PAIRS)))
def test_device_rebake_is_the_fresh_schedule_byte_for_byte(mf, pair, trained):
    """trained False: the buffers are still the device packer's; True: the part has adopted them."""
    _device_rebake(mf, "solo_k64_w2", pair, trained)


@pytest.mark.parametrize("trained", [False, True])
@pytest.mark.parametrize("pair", range(len(PAIRS)))
def test_device_rebake_of_nan_ratings_is_the_fresh_schedule_byte_for_byte(mf, pair, trained):
    """The same on the set whose ratings hold all-ones NaNs, in solo records and in step entries: device packer, device
    re-bake and (the snapshot of the host copy) the host re-bake write the quiet NaN for lr * r at every lr, 0 included;
    and training through such a schedule returns."""
    from tests.test_hyper_cpu import check_kind

    with fresh(mf, "solo_nan_k64_w2", *PAIRS[pair][0]) as m:
        check_kind(m, "solo_nan")
    _device_rebake(mf, "solo_nan_k64_w2", pair, trained)


def _device_rebake(mf, name, pair, trained):
    from mfsgd_amd import _lib

    (lr0, lam0), (lr1, lam1) = PAIRS[pair]
    with fresh(mf, name, lr1, lam1, flags=_lib.FLAG_DEVICE_INGEST) as f, \
            fresh(mf, name, lr0, lam0, flags=_lib.FLAG_DEVICE_INGEST) as m:
        assert m.schedule_info()["device_ingest"] == 2 and f.schedule_info()["device_ingest"] == 2
        if trained:
            for x in (f, m):
                x.init_factors()
                x.fit(1, rmse=False)
        m.set_hyper(lr1, lam1)
        assert_same(snapshot(m), snapshot(f), "device re-bake")
        m.set_hyper(lr0, lam0)  # ... and a host copy that exists by now is kept in step with the device's
        m.set_hyper(lr1, lam1)
        assert_same(snapshot(m), snapshot(f), "device re-bake with a host copy")


def test_fit_schedule_equals_the_manual_loop(mf):
    name = "solo_k64_w2"
    a, b, c = (0.01, 0.05), (0.006, 0.02), (0.02, 0.0)
    sched = [a, b, b, c]
    with fresh(mf, name, 0.03, 0.01) as m, fresh(mf, name, 0.03, 0.01) as ref:
        for x in (m, ref):
            x.init_factors()
        rm = m.fit_schedule([p[0] for p in sched], [p[1] for p in sched])
        want = []
        for lr, lam in sched:
            ref.set_hyper(lr, lam)
            want += list(ref.fit(1))
        assert np.array_equal(rm, np.array(want))
        for x, y in zip(m.get_factors(), ref.get_factors()):
            assert np.array_equal(x, y)
        assert m.hyper() == (float(np.float32(c[0])), float(np.float32(c[1]))) == (m.lr, m.lam)
        # lam None: the current lambda throughout; no RMSE asked for: none computed
        assert m.fit_schedule([0.01, 0.005], rmse=False) is None
        assert m.hyper() == (float(np.float32(0.005)), float(np.float32(c[1])))
        # a long schedule of distinct rates does not pile up graphs
        m.fit_schedule(np.linspace(0.01, 0.001, 40), rmse=False)
        assert m.debug_counters()["graphs"] <= 32


@pytest.mark.parametrize("rmse", [True, False])
def test_fit_equals_a_constant_schedule(mf, rmse):
    """mfsgd_train and mfsgd_train_schedule with the handle's own lr throughout run one loop: the same factors and the
    same RMSE values, bit for bit, with and without RMSE output."""
    name, epochs = "solo_k64_w2", 3
    with fresh(mf, name, 0.01, 0.05) as m, fresh(mf, name, 0.01, 0.05) as s:
        for x in (m, s):
            x.init_factors()
        a = m.fit(epochs, rmse=rmse)
        b = s.fit_schedule([s.hyper()[0]] * epochs, rmse=rmse)
        if rmse:
            assert len(a) == len(b) == epochs
            np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
        else:
            assert a is None and b is None
        for x, y in zip(m.get_factors(), s.get_factors()):
            np.testing.assert_array_equal(x, y)
        assert m.hyper() == s.hyper()


def test_bold_driver_follows_its_rule(mf, oracle):
    name, lr0, lam, up, down, epochs = "solo_k64_w2", 0.01, 0.05, 2.0, 0.5, 7
    k, kw, U, I, u, i, r = _problem(name)
    with fresh(mf, name, lr0, lam) as m:
        order = m.order()[0]  # (needs no device)
        # the oracle's own trajectory: it must take both branches, each decision with a margin far above the 1e-9 by
        # which the device's fp64 RMSE may differ
        P, Q = oracle.init_factors(U, I, k, SEED)
        lr, prev, lrs, rmo, grew = np.float32(lr0), oracle.rmse(P, Q, u, i, r), [], [], []
        for _ in range(epochs):
            oracle.sgd_pass_ordered(P, Q, u, i, r, order, float(lr), lam)
            rm = oracle.rmse(P, Q, u, i, r)
            assert abs(rm - prev) > 1e-3 * prev, "a decision too close to call: choose other values"
            lrs.append(lr)
            rmo.append(rm)
            grew.append(rm < prev)
            lr = lr * np.float32(up) if rm < prev else lr * np.float32(down)
            prev = rm
        assert any(grew) and not all(grew), "the run must show a growth and a cut"
        m.init_factors()
        rm0 = m.rmse()
        used, got = m.fit_bold_driver(epochs, up, down)
        Pg, Qg = m.get_factors()
        # the rule, re-derived in float32 from what the call itself reported
        assert used.dtype == np.float32 and used[0] == np.float32(lr0)
        p, branches = rm0, set()
        for e in range(epochs):
            nxt = used[e] * np.float32(up) if got[e] < p else used[e] * np.float32(down)
            branches.add(bool(got[e] < p))
            p = got[e]
            assert nxt == (used[e + 1] if e + 1 < epochs else np.float32(m.hyper()[0])), e
        assert branches == {True, False}
        assert np.array_equal(used, np.array(lrs, np.float32))
        np.testing.assert_allclose(got, rmo, rtol=1e-9, atol=1e-12)
        assert np.array_equal(Pg, P) and np.array_equal(Qg, Q)
        assert m.lr == m.hyper()[0] == float(lr)


def test_fold_in_uses_the_new_values(mf, oracle):
    from tests.test_fold_in_gpu import fold_in_ref

    name, lr1, lam1 = "solo_k64_w2", 0.006, 0.02
    k, kw, U, I, u, i, r = _problem(name)
    rng = np.random.default_rng(5)
    lens = rng.integers(0, 40, 20)
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    items = rng.integers(0, I, int(row_ptr[-1])).astype(np.int32)
    ratings = rng.uniform(0.5, 5.0, items.size).astype(np.float32)
    R0 = (rng.random((20, k), np.float32) - 0.5) * 0.2
    with fresh(mf, name, 0.01, 0.05) as m:
        m.init_factors()
        m.set_hyper(lr1, lam1)
        got = m.fold_in(row_ptr, items, ratings, 3, init=R0)
        _, Q = m.get_factors()
    assert np.array_equal(got, fold_in_ref(oracle, Q, row_ptr, items, ratings, 3, R0, lr1, lam1))


def test_dsgd_partitions_follow(mf, oracle):
    """A handle with n_parts = 2 driven by the Python DSGD driver (dsgd.DSGD over HipBackend, one rank holding both
    item partitions and training them one after the other on caller-owned blocks): one epoch, set_hyper, one epoch."""
    import torch

    from mfsgd_amd.dsgd import DSGD, HipBackend, TorchDistRing, assemble_q
    from tests.dsgd_common import SEED as DSEED, rank_workload

    G, k, U, I, nnz = 2, 64, 300, 211, 6000
    stages = ((0.01, 0.05), (0.006, 0.02))
    dev = torch.device("cuda", 0)
    u, i, r = rank_workload(0, U, I, nnz)
    Ps, Qs = oracle.init_factors(U, I, k, DSEED)
    with mf.MatrixFactorizationSGD(U, I, k, *stages[0], DSEED, n_parts=G) as t:
        t.set_ratings(u, i, r)
        t.init_p_offset(DSEED, 0)
        d = DSGD(HipBackend(t, dev), TorchDistRing(None, 0, 1), 0, 1, I, t.kp, DSEED, U, nnz, parts_per_rank=G)
        for lr, lam in stages:
            d.b.synchronize()  # (nothing of a partition in flight when the values change)
            t.set_hyper(lr, lam)
            d.epoch()
            for part in range(G):
                oracle.sgd_pass_ordered(Ps, Qs, u, i, r, t.order(part)[0], lr, lam)
        d.b.synchronize()
        P = t.get_factors()[0]
        Q = assemble_q(d.home_blocks(), I, k, G)
        sse = d.sse()
    assert np.array_equal(P, Ps) and np.array_equal(Q, Qs)
    np.testing.assert_allclose(sse, oracle.sse(Ps, Qs, u, i, r), rtol=1e-9)


@pytest.mark.parametrize("flag", ["default", "FLAG_DEVICE_INGEST"])
def test_set_hyper_keeps_no_device_memory(mf, flag):
    start = mf.debug_device_bytes()
    m = fresh(mf, "solo_k64_w2", 0.01, 0.05, flags=_flags(flag))
    before = mf.debug_device_bytes()
    m.set_hyper(0.006, 0.02)  # (with FLAG_DEVICE_INGEST: the packer's buffers, descriptors uploaded for the call only)
    assert mf.debug_device_bytes() == before
    m.init_factors()
    m.fit(1, rmse=False)
    before = mf.debug_device_bytes()
    m.set_hyper(0.02, 0.0)
    assert mf.debug_device_bytes() == before
    m.close()
    assert mf.debug_device_bytes() == start
