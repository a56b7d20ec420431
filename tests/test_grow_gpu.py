"""Growing a live model on the device (csrc/grow.hip, mfsgd_append_users / mfsgd_append_items / mfsgd_reserve_rows):
rows appended in place and by reallocation, and everything that reads the grown model afterwards -- training over the
kept schedule, the cached training graphs, online updates, serving, the cold-start flow fold-in -> append -> recommend,
device memory -- against numpy and the CPU oracle, bit for bit."""
import numpy as np
import pytest

from tests.test_validation_gpu import ATOL, RTOL   # the bar of a device fp64 RMSE against the oracle's

pytestmark = pytest.mark.gpu

LR, LAM = 0.02, 0.03
INVALID = -1
QUIET_NAN = 0x7FC00000


def _bits(a, b, what=""):
    a, b = np.ascontiguousarray(a, np.float32), np.ascontiguousarray(b, np.float32)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    bad = np.flatnonzero(a.view(np.uint32).ravel() != b.view(np.uint32).ravel())
    assert bad.size == 0, f"{what}: {bad.size} of {a.size} words differ, first at {bad[:4]}"


def _ratings(rng, U, I, n):
    """n distinct (u, i) pairs with ratings 0.5 .. 5."""
    key = rng.choice(U * I, min(n, U * I), replace=False)
    return (key // I).astype(np.int32), (key % I).astype(np.int32), (rng.integers(1, 11, key.size) * 0.5).astype(np.float32)


def _rows(rng, n, k, nan_at=None):
    rows = rng.standard_normal((n, k)).astype(np.float32)
    want = rows.copy()
    if nan_at is not None:
        rows.view(np.uint32)[nan_at] = 0x7FFFFFFF
        want.view(np.uint32)[nan_at] = QUIET_NAN
    return rows, want


# ---- append on the device, both paths ----------------------------------------------------------------------------------
@pytest.mark.parametrize("reserve", [False, True], ids=["realloc", "in_place"])
@pytest.mark.parametrize("n_new", [1, 257])
@pytest.mark.parametrize("old", [5, 1000])
@pytest.mark.parametrize("k", [1, 3, 33, 64, 200, 256])
def test_append_on_the_device(mf, oracle, k, old, n_new, reserve):
    rng = np.random.default_rng(1000 * k + old + n_new)
    U = I = old
    u, i, r = _ratings(rng, U, I, 400)
    new_p, want_p = _rows(rng, n_new, k, nan_at=(n_new - 1, k - 1))
    new_q, want_q = _rows(rng, n_new, k, nan_at=(0, 0))
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 7) as m:
        m.train(u, i, r, 1)                         # the factors are on the device, trained
        P0, Q0 = m.get_factors()
        if reserve:
            m.reserve(users=U + 300, items=I + 300)   # (a reallocation of its own: the old rows must survive it)
            assert m.capacity() == (U + 300, I + 300)
        live = mf.debug_device_bytes()
        assert m.add_users(new_p) == U and m.add_items(new_q) == I
        assert (m.users, m.items) == (U + n_new, I + n_new)
        if reserve:
            assert mf.debug_device_bytes() == live and m.capacity() == (U + 300, I + 300)
        else:
            assert m.capacity() == (U + n_new, I + n_new)
            assert mf.debug_device_bytes() == live + 2 * 4 * n_new * m.kp
        P1, Q1 = m.get_factors()
        _bits(P1, np.vstack([P0, want_p]), "P")
        _bits(Q1, np.vstack([Q0, want_q]), "Q")
        assert m.add_users(n=3, seed=5) == U + n_new     # seeded rows, drawn in place
        P2, _ = m.get_factors()
    _bits(P2[:U + n_new], P1, "P after the seeded append")
    _bits(P2[U + n_new:], oracle.init_factors(3, 0, k, 5)[0], "seeded rows")


# ---- training after growth ----------------------------------------------------------------------------------------------
def _grow_and_train(mf, oracle, k, flags, reserve):
    rng = np.random.default_rng(31 + k)
    U, I, seed = 40, 30, 7
    u, i, r = _ratings(rng, U, I, 600)
    new_p, _ = _rows(rng, 5, k)
    P, Q = oracle.init_factors(U, I, k, seed)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, seed, flags=flags) as m:
        if reserve:
            m.reserve(users=U + 5, items=I + 3)
        m.set_ratings(u, i, r)
        m.init_factors()
        m.fit(1)
        order, cells = m.order()
        graphs0 = m.debug_counters()["graphs"]
        assert m.add_users(new_p) == U
        graphs_mid = [m.debug_counters()["graphs"]]   # cached now: between each append and the next fit
        assert m.add_items(n=3, seed=99) == I
        graphs_mid.append(m.debug_counters()["graphs"])
        rm = m.fit(2)
        graphs1 = m.debug_counters()["graphs"]
        order1, cells1 = m.order()
        got_p, got_q = m.get_factors()
        got_rmse = m.rmse()
    assert np.array_equal(order, order1) and np.array_equal(cells, cells1)
    oracle.sgd_pass_ordered(P, Q, u, i, r, order, LR, LAM)
    new_q = oracle.init_factors(3, 0, k, 99)[0]
    P, Q = np.vstack([P, new_p]), np.vstack([Q, new_q])
    ref = []
    for _ in range(2):
        oracle.sgd_pass_ordered(P, Q, u, i, r, order, LR, LAM)
        ref.append(oracle.rmse(P, Q, u, i, r))
    _bits(got_p, P, "P")
    _bits(got_q, Q, "Q")
    _bits(got_p[U:], new_p, "appended users")      # no ratings: not touched
    _bits(got_q[I:], new_q, "appended items")
    np.testing.assert_allclose(rm, ref, rtol=RTOL, atol=ATOL)
    np.testing.assert_allclose(got_rmse, ref[-1], rtol=RTOL, atol=ATOL)
    return graphs0, graphs_mid, graphs1


@pytest.mark.parametrize("round_launch", [False, True])
@pytest.mark.parametrize("k", [8, 33])
def test_training_after_growth_follows_the_kept_order(mf, oracle, k, round_launch):
    from mfsgd_amd import _lib

    _grow_and_train(mf, oracle, k, _lib.FLAG_ROUND_LAUNCH if round_launch else 0, reserve=False)


def test_an_append_inside_the_capacity_keeps_the_training_graphs(mf, oracle):
    """The counter is the number of graphs cached NOW, so it is read between the append and the next fit: a handle that
    dropped its graphs on an append would show 0 there, and 1 again behind the fit, which captures."""
    before, mid, after = _grow_and_train(mf, oracle, 33, 0, reserve=True)
    assert before >= 1 and mid == [before, before] and after == before, (before, mid, after)


def test_a_reallocating_append_drops_the_graphs_and_the_next_fit_captures_again(mf, oracle):
    before, mid, after = _grow_and_train(mf, oracle, 33, 0, reserve=False)
    assert before >= 1 and mid == [0, 0] and after >= 1, (before, mid, after)


def test_reserve_drops_the_graphs_only_when_it_reallocates(mf):
    rng = np.random.default_rng(41)
    U, I, k = 40, 30, 33
    u, i, r = _ratings(rng, U, I, 600)
    graphs = lambda m: m.debug_counters()["graphs"]
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 7) as m:
        m.train(u, i, r, 1)
        g = graphs(m)
        assert g >= 1
        m.reserve(users=U, items=I - 5)            # at or below the capacity: nothing moves
        assert graphs(m) == g
        m.reserve(users=U + 10)                    # P moves
        assert graphs(m) == 0
        m.fit(1)
        assert graphs(m) == g
        m.reserve(users=U + 4, items=0)            # inside what is reserved
        m.add_users(n=10)
        assert graphs(m) == g
        m.reserve(items=I + 1)                     # Q moves
        assert graphs(m) == 0
        m.fit(1)
        assert graphs(m) == g


# ---- early stopping on a handle whose capacity exceeds its count ---------------------------------------------------------
def test_early_stop_restores_the_best_epoch_inside_a_reserve(mf, oracle):
    """The snapshot is of the rows P and Q have, not of their capacity: with room reserved and rows appended into it, the
    factors after a restore are the oracle's after best_epoch + 1 epochs, the appended rows as they went in."""
    rng = np.random.default_rng(43)
    U, I, k, lr, lam = 40, 30, 8, 0.03, 0.0
    u, i, r = _ratings(rng, U, I, 300)               # ratings at random: the held-out error turns up after a few epochs
    vu, vi, vr = _ratings(rng, U, I, 200)
    new_p, new_q = _rows(rng, 3, k)[0], _rows(rng, 2, k)[0]
    with mf.MatrixFactorizationSGD(U, I, k, lr, lam, 7) as m:
        m.reserve(users=U + 50, items=I + 20)
        m.set_ratings(u, i, r)
        m.init_factors()
        m.set_validation(vu, vi, vr)
        m.fit(1)                                     # (on the device, a graph cached)
        assert m.add_users(new_p) == U and m.add_items(new_q) == I
        assert m.capacity() == (U + 50, I + 20)
        res = m.fit_early_stopping(40, patience=2, restore_best=True)
        got_p, got_q = m.get_factors()
        order, _ = m.order()
    best, ran = res["best_epoch"], res["epochs_run"]
    assert 0 <= best < ran - 1, res                  # something was restored
    P, Q = oracle.init_factors(U, I, k, 7)
    oracle.sgd_pass_ordered(P, Q, u, i, r, order, lr, lam)
    P, Q = np.vstack([P, new_p]), np.vstack([Q, new_q])
    val = []
    for e in range(ran):
        oracle.sgd_pass_ordered(P, Q, u, i, r, order, lr, lam)
        val.append(oracle.rmse(P, Q, vu, vi, vr))
        if e == best:
            best_p, best_q = P.copy(), Q.copy()
    np.testing.assert_allclose(res["val_rmse"], val, rtol=RTOL, atol=ATOL)
    _bits(got_p, best_p, "P")
    _bits(got_q, best_q, "Q")


# ---- online updates after growth --------------------------------------------------------------------------------------
def test_online_updates_reach_the_new_rows(mf, oracle):
    rng = np.random.default_rng(17)
    U, I, k, n = 25, 20, 12, 300
    P0 = (rng.standard_normal((U, k)) * 0.3).astype(np.float32)
    Q0 = (rng.standard_normal((I, k)) * 0.3).astype(np.float32)
    new_p, new_q = 0.3 * _rows(rng, 4, k)[0], 0.3 * _rows(rng, 3, k)[0]
    uu = rng.integers(0, U + 4, n).astype(np.int32)
    ii = rng.integers(0, I + 3, n).astype(np.int32)
    rr = (rng.integers(1, 11, n) * 0.5).astype(np.float32)
    uu[:4], ii[:4] = [U, 0, U + 3, 1], [0, I, I + 2, 1]      # new with old, old with new, new with new, old with old
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 3) as m:
        m.set_factors(P0, Q0)
        m.predict([0], [0])                                   # on the device
        with pytest.raises(mf.MfsgdError) as e:
            m.partial_fit(uu, ii, rr)
        assert e.value.code == INVALID and "apply_ratings: rating 0 out of range" in str(e.value)
        P1, Q1 = m.get_factors()
        _bits(P1, P0, "P after the refused list")
        _bits(Q1, Q0, "Q after the refused list")
        m.add_users(new_p)
        m.add_items(new_q)
        err = m.partial_fit(uu, ii, rr, errors=True)
        got_p, got_q = m.get_factors()
    P, Q = np.vstack([P0, new_p]), np.vstack([Q0, new_q])
    want = np.empty(n, np.float32)
    for j in range(n):
        want[j] = oracle.sgd_update(P[uu[j]], Q[ii[j]], float(rr[j]), LR, LAM)
    assert np.isfinite(P).all() and np.isfinite(Q).all()
    _bits(got_p, P, "P")
    _bits(got_q, Q, "Q")
    _bits(err, want, "errors")


# ---- serving after growth -----------------------------------------------------------------------------------------------
def test_serving_sees_the_new_rows(mf, oracle):
    rng = np.random.default_rng(23)
    U, I, k = 50, 40, 33
    P0 = rng.standard_normal((U, k)).astype(np.float32)
    Q0 = rng.standard_normal((I, k)).astype(np.float32)
    new_p, _ = _rows(rng, 2, k)
    new_q = np.vstack([10.0 * P0[7], rng.standard_normal(k)]).astype(np.float32)   # item I: 10 x user 7's row
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 3) as m:
        m.set_factors(P0, Q0)
        m.predict([0], [0])
        m.add_users(new_p)
        m.add_items(new_q)
        P, Q = np.vstack([P0, new_p]), np.vstack([Q0, new_q])
        got = m.predict([U + 1, U, 0], [I + 1, 3, I])
        _bits(got, oracle.predict(P, Q, [U + 1, U, 0], [I + 1, 3, I]), "predict")
        items, scores = m.recommend([7, U + 1], 3)
        assert items[0, 0] == I
        all_items, all_scores = m.recommend([U], I + 2)        # topn = the new number of items
        assert sorted(all_items[0].tolist()) == list(range(I + 2))
        sc = oracle.predict(P, Q, np.full(I + 2, U, np.int32), np.arange(I + 2, dtype=np.int32))
        _bits(all_scores[0], sc[all_items[0]], "scores of the new user")
        assert (np.diff(all_scores[0].astype(np.float64)) <= 0).all()
        with pytest.raises(mf.MfsgdError):
            m.recommend([U], I + 3)
        m.add_items((3.0 * Q[4])[None, :])                     # a scaled copy of item 4: its nearest neighbour
        sim, _ = m.similar_items([4], 1)
        assert sim[0, 0] == I + 2
        norms = m.row_inv_norms("items")
        assert norms.shape == (I + 3,) and np.isfinite(norms).all() and (norms > 0).all()
        assert m.row_inv_norms("users").shape == (U + 2,)
        ranks = m.rank_items([7], [I])
        assert ranks.tolist() == [0]


# ---- end-to-end cold start ----------------------------------------------------------------------------------------------
def test_cold_start_fold_in_append_recommend(mf):
    rng = np.random.default_rng(29)
    U, I, k = 60, 50, 16
    A = rng.standard_normal((U, 3)).astype(np.float32)
    B = rng.standard_normal((I, 3)).astype(np.float32)
    u, i, _ = _ratings(rng, U, I, 1500)
    r = (np.einsum("ij,ij->i", A[u], B[i]) + 3.0).astype(np.float32)
    with mf.MatrixFactorizationSGD(U, I, k, 0.02, 0.01, 7) as m:
        m.reserve(users=U + 8, items=I + 8)
        m.train(u, i, r, 30)
        # a new item that users 0 .. 19 rate 50: once folded in and appended it tops their recommendations
        fans = np.arange(20, dtype=np.int32)
        q_rows = m.fold_in_items([0, fans.size], fans, np.full(fans.size, 50.0, np.float32), 40)
        assert m.add_items(q_rows) == I
        items, _ = m.recommend(fans, 1)
        assert (items[:, 0] == I).sum() >= 15, items[:, 0]
        # two new users: in the model their recommendations are those of their folded rows
        row_ptr = np.array([0, 12, 30], np.int64)
        their_items = rng.integers(0, I, 30).astype(np.int32)
        their_ratings = (rng.integers(1, 11, 30) * 0.5).astype(np.float32)
        p_rows = m.fold_in(row_ptr, their_items, their_ratings, 10)
        want_i, want_s = m.recommend_rows(p_rows, 5)
        first = m.add_users(p_rows)
        assert first == U
        got_i, got_s = m.recommend([first, first + 1], 5)
        assert np.array_equal(got_i, want_i)
        _bits(got_s, want_s, "scores")
        m.partial_fit([first], [I], [4.0])                     # and the next rating of the new user applies
        assert m.fit(1).shape == (1,)


# ---- device memory ------------------------------------------------------------------------------------------------------
def test_device_memory_of_a_grown_handle(mf):
    rng = np.random.default_rng(37)
    U, I, k, nu, ni = 200, 150, 33, 57, 31
    u, i, r = _ratings(rng, U, I, 3000)
    new_p, _ = _rows(rng, nu, k)
    new_q, _ = _rows(rng, ni, k)
    live0 = mf.debug_device_bytes()
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 7) as m:
        m.train(u, i, r, 1)
        sizes = m.debug_schedule()
        m.add_users(new_p)
        m.add_items(new_q)
        P, Q = m.get_factors()
        m.fit(1)
        grown = mf.debug_device_bytes() - live0
        m.reserve(users=U + nu + 100)
        assert mf.debug_device_bytes() - live0 == grown + 4 * 100 * m.kp
        in_cap = mf.debug_device_bytes()
        m.add_users(n=100)
        assert mf.debug_device_bytes() == in_cap
    assert mf.debug_device_bytes() == live0
    with mf.MatrixFactorizationSGD(U + nu, I + ni, k, LR, LAM, 7) as fresh:
        fresh.set_ratings(u, i, r)
        fresh.set_factors(P, Q)
        fresh.fit(1)
        # (the comparison needs schedules of one size: new rows have no ratings, and at this shape the cut is the same)
        assert [a.shape for a in fresh.debug_schedule()] == [a.shape for a in sizes]
        assert mf.debug_device_bytes() - live0 == grown
    assert mf.debug_device_bytes() == live0


# ---- sequences ------------------------------------------------------------------------------------------------------------
class _Model:
    """What a single-partition handle with one fixed rating set is, in numpy and the oracle."""

    def __init__(self, oracle, U, I, k, seed, u, i, r, order):
        self.o, self.k = oracle, k
        self.P, self.Q = oracle.init_factors(U, I, k, seed)
        self.u, self.i, self.r, self.order = u, i, r, order
        self.lr, self.lam = LR, LAM
        self.res = [0, 0]

    def counts(self):
        return self.P.shape[0], self.Q.shape[0]

    def capacity(self):
        return tuple(max(c, x) for c, x in zip(self.counts(), self.res))

    def fit(self):
        self.o.sgd_pass_ordered(self.P, self.Q, self.u, self.i, self.r, self.order, self.lr, self.lam)
        return self.o.rmse(self.P, self.Q, self.u, self.i, self.r)

    def add(self, side, rows):
        if side == 0:
            self.P = np.vstack([self.P, rows])
        else:
            self.Q = np.vstack([self.Q, rows])

    def partial_fit(self, uu, ii, rr):
        return np.array([self.o.sgd_update(self.P[a], self.Q[b], float(c), self.lr, self.lam) for a, b, c in zip(uu, ii, rr)],
                        np.float32)


@pytest.mark.parametrize("seed", [1, 2, 3])
def test_sequences_of_growth_training_and_updates(mf, oracle, seed):
    rng = np.random.default_rng(seed)
    U = I = 30
    k = 12
    u, i, r = _ratings(rng, U, I, 400)
    done = {}
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 7) as m:
        m.set_ratings(u, i, r)
        m.init_factors()
        model = _Model(oracle, U, I, k, 7, u, i, r, m.order()[0])
        ops = ["fit", "add_users", "add_items", "partial_fit", "set_hyper", "reserve"]
        steps = ops + list(rng.choice(ops, 16))               # every op at least once
        rng.shuffle(steps)
        for step, op in enumerate(steps):
            nu, ni = model.counts()
            if op == "fit":
                np.testing.assert_allclose(m.fit(1), [model.fit()], rtol=RTOL, atol=ATOL)
            elif op in ("add_users", "add_items"):
                side = 0 if op == "add_users" else 1
                n = int(rng.integers(0, 5))
                add = m.add_users if side == 0 else m.add_items
                if rng.random() < 0.5:
                    rows, _ = _rows(rng, n, k)
                    assert add(rows) == (nu, ni)[side]
                else:
                    s = int(rng.integers(0, 1000))
                    assert add(n=n, seed=s) == (nu, ni)[side]
                    rows = oracle.init_factors(n, 0, k, s)[0] if n else np.empty((0, k), np.float32)
                model.add(side, rows)
            elif op == "partial_fit":
                n = int(rng.integers(1, 40))
                uu, ii = rng.integers(0, nu, n).astype(np.int32), rng.integers(0, ni, n).astype(np.int32)
                rr = (rng.integers(1, 11, n) * 0.5).astype(np.float32)
                _bits(m.partial_fit(uu, ii, rr, errors=True), model.partial_fit(uu, ii, rr), f"step {step}: errors")
            elif op == "set_hyper":
                m.set_hyper(float(rng.uniform(0.005, 0.03)), float(rng.uniform(0.0, 0.05)))
                model.lr, model.lam = m.lr, m.lam
            else:
                want = [int(nu + rng.integers(-3, 10)), int(ni + rng.integers(-3, 10))]
                want[int(rng.integers(0, 2))] = 0
                m.reserve(users=want[0], items=want[1])
                model.res = [max(a, b) for a, b in zip(model.res, want)]
            done[op] = done.get(op, 0) + 1
            got_p, got_q = m.get_factors()
            _bits(got_p, model.P, f"step {step} ({op}): P")
            _bits(got_q, model.Q, f"step {step} ({op}): Q")
            assert (m.users, m.items) == model.counts() and m.capacity() == model.capacity(), (step, op)
            assert np.array_equal(m.order()[0], model.order)
        assert m.debug_counters()["schedule_builds"] == 1
    assert all(done.get(op, 0) >= 1 for op in ops), done
