"""Growing a live model on host staging: add_users / add_items (mfsgd_append_users / mfsgd_append_items), reserve and
capacity (mfsgd_reserve_rows / mfsgd_get_capacity).  No GPU: the factors stay where set_factors put them, the calls
that are host-only (set_ratings, order, online_levels, save / load) see the grown sizes."""
import numpy as np
import pytest

LR, LAM = 0.01, 0.05
INVALID, STATE = -1, -5
INT32_MAX = 2**31 - 1
QUIET_NAN = 0x7FC00000


def _model(mf, U, I, k, rng, **kw):
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    m = mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 7, **kw)
    m.set_factors(P, Q)
    return m, P, Q


def _dims(m):
    import ctypes as C

    u, i, k = C.c_int32(), C.c_int32(), C.c_int32()
    assert m._lib.mfsgd_get_dims(m._h, C.byref(u), C.byref(i), C.byref(k)) == 0
    return u.value, i.value, k.value


def _raises(mf, code, prefix, call):
    with pytest.raises(mf.MfsgdError) as e:
        call()
    assert e.value.code == code, str(e.value)
    assert f": {prefix}" in str(e.value), str(e.value)


@pytest.mark.parametrize("k", [1, 3, 33, 64, 200, 256])
def test_append_on_host_staging(mf, oracle, k):
    rng = np.random.default_rng(k)
    U, I = 6, 5
    m, P, Q = _model(mf, U, I, k, rng)
    with m:
        new_p = rng.standard_normal((3, k)).astype(np.float32)
        new_q = rng.standard_normal((4, k)).astype(np.float32)
        new_p.view(np.uint32)[1, k - 1] = 0x7FFFFFFF   # a NaN with a payload
        new_q.view(np.uint32)[0, 0] = 0xFFFFFFFF
        assert m.add_users(new_p) == U
        assert (m.users, m.items) == (U + 3, I) and _dims(m) == (U + 3, I, k)
        assert m.add_items(new_q) == I
        assert _dims(m) == (U + 3, I + 4, k) and m.capacity() == (U + 3, I + 4)
        want_p, want_q = np.vstack([P, new_p]), np.vstack([Q, new_q])
        want_p.view(np.uint32)[U + 1, k - 1] = QUIET_NAN
        want_q.view(np.uint32)[I, 0] = QUIET_NAN
        got_p, got_q = m.get_factors()
        assert got_p.tobytes() == want_p.tobytes() and got_q.tobytes() == want_q.tobytes()
        # seeded rows: fold-in's default start
        assert m.add_users(n=5, seed=99) == U + 3
        assert m.add_items(n=2) == I + 4          # the model's seed
        got_p, got_q = m.get_factors()
        assert got_p[:U + 3].tobytes() == want_p.tobytes() and got_q[:I + 4].tobytes() == want_q.tobytes()
        assert np.array_equal(got_p[U + 3:], oracle.init_factors(5, 0, k, 99)[0])
        assert np.array_equal(got_q[I + 4:], oracle.init_factors(2, 0, k, 7)[0])


def test_zero_row_append_changes_nothing(mf):
    rng = np.random.default_rng(1)
    m, P, Q = _model(mf, 4, 3, 5, rng)
    with m:
        assert m.add_users(np.empty((0, 5), np.float32)) == 4
        assert m.add_items(n=0) == 3
        assert _dims(m) == (4, 3, 5) and m.capacity() == (4, 3)
        got_p, got_q = m.get_factors()
        assert got_p.tobytes() == P.tobytes() and got_q.tobytes() == Q.tobytes()


def test_errors(mf):
    import ctypes as C

    rng = np.random.default_rng(2)
    k = 4
    m, P, Q = _model(mf, 4, 3, k, rng)
    with m:
        rows = np.zeros((2, k), np.float32)
        for call, name in ((m._lib.mfsgd_append_users, "append_users: "), (m._lib.mfsgd_append_items, "append_items: ")):
            first = C.c_int32(-7)
            assert call(m._h, -1, None, 0, C.byref(first)) == INVALID
            assert m._lib.mfsgd_last_error(m._h).decode().startswith(name) and first.value == -7
            assert call(m._h, INT32_MAX - 2, None, 0, C.byref(first)) == INVALID   # 4 or 3 rows + this: beyond INT32_MAX
            assert m._lib.mfsgd_last_error(m._h).decode().startswith(name) and first.value == -7
        _raises(mf, INVALID, "reserve_rows: ", lambda: m.reserve(users=-1))
        _raises(mf, INVALID, "reserve_rows: ", lambda: m.reserve(items=-5))
        assert _dims(m) == (4, 3, k) and m.capacity() == (4, 3)
        assert m.get_factors()[0].tobytes() == P.tobytes()
    with mf.MatrixFactorizationSGD(6, 5, k, LR, LAM, 1, n_parts=2) as m2:
        m2.init_factors()
        _raises(mf, STATE, "append_users: ", lambda: m2.add_users(rows))
        _raises(mf, STATE, "append_items: ", lambda: m2.add_items(n=1))
        _raises(mf, STATE, "reserve_rows: ", lambda: m2.reserve(users=10))
        _raises(mf, INVALID, "append_users: ", lambda: m2.add_users(n=-1))     # the argument comes before the state
        assert m2.capacity() == (6, 5)
    with mf.MatrixFactorizationSGD(6, 5, k, LR, LAM, 1) as m3:     # factors never set
        _raises(mf, STATE, "append_users: ", lambda: m3.add_users(rows))
        _raises(mf, STATE, "append_items: ", lambda: m3.add_items(rows))
        assert _dims(m3) == (6, 5, k)
    with mf.MatrixFactorizationSGD(6, 5, k, LR, LAM, 1) as m4:     # P alone: no Q
        m4.init_p_offset(3, 0)
        _raises(mf, STATE, "append_users: ", lambda: m4.add_users(rows))
        _raises(mf, STATE, "append_items: ", lambda: m4.add_items(rows))
        assert _dims(m4) == (6, 5, k)
    with pytest.raises(ValueError):
        m.add_users()
    with pytest.raises(ValueError):
        m.add_users(rows, n=2)


def test_ratings_identity_and_order_survive_an_append(mf):
    rng = np.random.default_rng(3)
    U, I, k, n = 20, 15, 8, 200
    u = rng.integers(0, U, n).astype(np.int32)
    i = rng.integers(0, I, n).astype(np.int32)
    r = rng.uniform(1, 5, n).astype(np.float32)
    m, _, _ = _model(mf, U, I, k, rng)
    with m:
        m.set_ratings(u, i, r)
        builds = m.debug_counters()["schedule_builds"]
        order0, cells0 = m.order()
        info0 = m.schedule_info()
        m.add_users(n=3)
        m.add_items(n=2)
        m.set_ratings(u, i, r)                     # the same triples: still recognised
        assert m.debug_counters()["schedule_builds"] == builds
        order1, cells1 = m.order()
        assert np.array_equal(order0, order1) and np.array_equal(cells0, cells1)
        assert m.schedule_info() == info0
        u2, i2 = u.copy(), i.copy()
        u2[5], i2[9] = U + 2, I + 1                # the new indices in a rating set of their own
        m.set_ratings(u2, i2, r)
        assert m.debug_counters()["schedule_builds"] == builds + 1
        assert m.schedule_info()["nnz"] == n
    m, _, _ = _model(mf, U, I, k, rng)
    with m:
        _raises(mf, INVALID, "set_ratings: ", lambda: m.set_ratings(u2, i2, r))


def test_online_levels_follow_the_counts(mf):
    rng = np.random.default_rng(4)
    U, I = 7, 6
    m, _, _ = _model(mf, U, I, 4, rng)
    with m:
        levels, _ = m.online_levels([0, 0, 1], [1, 2, 2])     # (allocates the per-row scratch at the old sizes)
        assert levels.tolist() == [0, 1, 2]
        _raises(mf, INVALID, "online_levels: ", lambda: m.online_levels([U], [0]))
        _raises(mf, INVALID, "online_levels: ", lambda: m.online_levels([0], [I]))
        m.add_users(n=2)
        m.add_items(n=1)
        levels, info = m.online_levels([U + 1, 0, U + 1, 3], [I, I, 2, 2])
        assert levels.tolist() == [0, 1, 1, 2] and info["levels"] == 3
        levels, _ = m.online_levels([U + 1, 0], [0, I])      # the scratch came back all zero
        assert levels.tolist() == [0, 0]
        _raises(mf, INVALID, "online_levels: ", lambda: m.online_levels([U + 2], [0]))


def test_reserve(mf):
    rng = np.random.default_rng(5)
    k = 6
    with mf.MatrixFactorizationSGD(10, 8, k, LR, LAM, 1) as m:
        assert m.capacity() == (10, 8)
        m.reserve(users=50)                        # before any factors: a number
        assert m.capacity() == (50, 8)
        m.set_factors(rng.standard_normal((10, k)).astype(np.float32), rng.standard_normal((8, k)).astype(np.float32))
        assert m.capacity() == (50, 8)
        m.reserve(users=20, items=0)               # never shrinks; 0 leaves a side alone
        assert m.capacity() == (50, 8)
        m.reserve(items=9)
        assert m.capacity() == (50, 9)
        assert m.add_items(n=3) == 8               # beyond the reserve: the capacity follows the count
        assert m.capacity() == (50, 11)
        assert m.add_users(n=40) == 10
        assert m.capacity() == (50, 11) and (m.users, m.items) == (50, 11)
        m.add_users(n=1)
        assert m.capacity() == (51, 11)
        m.reserve()
        assert m.capacity() == (51, 11)


def test_save_and_load_of_a_grown_model(mf, tmp_path):
    rng = np.random.default_rng(6)
    k = 5
    m, P, Q = _model(mf, 9, 4, k, rng)
    path = tmp_path / "grown.mfsgdf"
    with m:
        m.add_users(rng.standard_normal((2, k)).astype(np.float32))
        m.add_items(n=3, seed=5)
        want_p, want_q = m.get_factors()
        m.save_factors(path)
    with mf.MatrixFactorizationSGD(11, 7, k, LR, LAM, 1) as fresh:
        fresh.load_factors(path)
        got_p, got_q = fresh.get_factors()
    assert got_p.tobytes() == want_p.tobytes() and got_q.tobytes() == want_q.tobytes()
    assert got_p[:9].tobytes() == P.tobytes() and got_q[:4].tobytes() == Q.tobytes()
    with mf.MatrixFactorizationSGD(9, 4, k, LR, LAM, 1) as old:     # the file has the grown sizes
        with pytest.raises(mf.MfsgdError):
            old.load_factors(path)
