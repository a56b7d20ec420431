"""similar_items / similar_users / similar_rows / row_inv_norms against numpy on the oracle's dot (include/mfsgd.h,
"similar items and users"):
    n2 = dot(x, x);  rn = n2 > 0 ? 1 / sqrt(n2) : 0;  cos(a, b) = (dot(a, b) * rn(a)) * rn(b)       (fp32 throughout)
the query's own index dropped (not for similar_rows), np.lexsort((index, -score)), cut at topn, padded with -1 / NaN.
Indices compare exactly and scores bit for bit; the tolerance is zero.  Shapes: three tiles of the fused kernel; the last
fused topn and the first of the sort path; a side as small as topn; every kind of lane-group width; P instead of Q."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LR, LAM = 0.01, 0.05
ZERO_ROWS = (50, 51, 52, 53)
TINY_ROW = 60  # entries 1e-20: n2 is subnormal
PLANTED_QUERIES = (3, 10, 20, 41, 50, 77)  # the row, its duplicate, its double, its negative, a zero row, an ordinary one


def _matrix(n, k, seed):
    """n x k: a third of the rows copies of row 3 (a tie group that straddles every selection threshold), and for
    n > 100 the planted rows: exact ties of row 3 by duplication and by powers of two, its negative (sorts last), zero
    rows (one entry -0.0), and a row whose squared norm is subnormal."""
    rng = np.random.default_rng(seed)
    M = rng.standard_normal((n, k)).astype(np.float32)
    M[rng.integers(0, n, n // 3)] = M[3 % n]
    if n > 100:
        M[10] = M[3]
        M[20] = np.float32(2) * M[3]
        M[30] = np.float32(0.25) * M[3]
        M[41] = -M[3]
        M[ZERO_ROWS[0]:ZERO_ROWS[-1] + 1] = 0.0
        M[ZERO_ROWS[2], 0] = -0.0
        M[TINY_ROW] = np.float32(1e-20)
    return M


def _rn(oracle, M):
    idx = np.arange(M.shape[0], dtype=np.int32)
    n2 = oracle.predict(M, M, idx, idx)  # dot(M[j], M[j]) for every j
    assert n2[0] == np.float32(oracle.dot(M[0], M[0])) and n2[-1] == np.float32(oracle.dot(M[-1], M[-1]))
    with np.errstate(divide="ignore"):
        return np.where(n2 > 0, np.float32(1) / np.sqrt(n2, dtype=np.float32), np.float32(0)).astype(np.float32)


def _expected(oracle, A, ra, queries, M, rn, topn, drop_self):
    """Rows queries[...] of A (inverse norms ra) against every row of M (inverse norms rn)."""
    n = M.shape[0]
    cand = np.arange(n, dtype=np.int32)
    index = np.full((len(queries), topn), -1, np.int32)
    scores = np.full((len(queries), topn), np.nan, np.float32)
    for row, a in enumerate(queries):
        d = oracle.predict(A, M, np.full(n, a, np.int32), cand)
        s = ((d * ra[a]).astype(np.float32) * rn).astype(np.float32)
        assert d.dtype == np.float32 and s.dtype == np.float32
        keep = cand != a if drop_self else np.ones(n, bool)
        c = cand[keep]
        order = c[np.lexsort((c, -s[keep]))][:topn]
        index[row, :order.size] = order
        scores[row, :order.size] = s[order]
    return index, scores


def _same(got, want):
    (gi, gs), (wi, ws) = got, want
    np.testing.assert_array_equal(gi, wi)
    pad = wi < 0
    assert np.isnan(gs[pad]).all()
    np.testing.assert_array_equal(gs[~pad].view(np.uint32), ws[~pad].view(np.uint32))


def _queries(n):
    q = [0, n - 1, n // 6, n // 2, n - n // 6, n // 2] + list(PLANTED_QUERIES) + [TINY_ROW]
    return np.array([x for x in q if x < n], np.int32)


def _check_side(m, oracle, M, side, topn, queries):
    """similar_items or similar_users of the queries, similar_rows of the same rows, and the side's inverse norms."""
    rn = _rn(oracle, M)
    np.testing.assert_array_equal(m.row_inv_norms(side).view(np.uint32), rn.view(np.uint32))
    by_index = m.similar_items if side == "items" else m.similar_users
    got = by_index(queries, topn)
    _same(got, _expected(oracle, M, rn, queries, M, rn, topn, True))
    for row, a in enumerate(queries):
        assert a not in got[0][row]
    R = np.ascontiguousarray(M[queries])
    _same(m.similar_rows(R, topn, side=side),
          _expected(oracle, R, _rn(oracle, R), np.arange(len(queries)), M, rn, topn, False))
    return rn


def _planted_properties(m, M, topn):
    """What the contract promises of the planted rows, stated on the output itself."""
    idx, sc = m.similar_items(np.array([3, 20, 41, 50], np.int32), topn)
    # the duplicate, the double and the quarter of row 3 tie exactly with every other copy of it: index order decides
    copies = np.flatnonzero((M == M[3]).all(axis=1) | (M == 2 * M[3]).all(axis=1) | (M == M[3] / 4).all(axis=1))
    for row, a in ((0, 3), (1, 20)):
        np.testing.assert_array_equal(idx[row], copies[copies != a][:topn])
        assert (sc[row].view(np.uint32) == sc[row, 0].view(np.uint32)).all()
    assert sc[0].tobytes() == sc[1].tobytes()  # scaling the query by two changes no bit
    assert 3 not in idx[2][:min(topn, 5)] and (sc[2] <= 1.0000002).all()
    np.testing.assert_array_equal(idx[3], [x for x in range(topn + 1) if x != 50][:topn])  # a zero query: smallest indices
    assert (sc[3] == 0).all()
    zi, zs = m.similar_rows(np.zeros((1, M.shape[1]), np.float32), topn)
    np.testing.assert_array_equal(zi[0], np.arange(topn))
    assert (zs == 0).all()


def test_three_tiles_fused(mf, oracle):
    I, k, topn = 30000, 64, 10  # three tiles of 14336
    Q = _matrix(I, k, 1)
    P = np.random.default_rng(2).standard_normal((8, k)).astype(np.float32)
    with mf.MatrixFactorizationSGD(8, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        _check_side(m, oracle, Q, "items", topn, _queries(I))
        _planted_properties(m, Q, topn)
        # the negative of row 3 sorts last: it ends the ranking of the whole catalogue
        idx, sc = m.similar_rows(Q[3:4], I)
        assert idx[0, -1] == 41 and sc[0, -1] < -0.99


@pytest.mark.parametrize("topn", [128, 129])  # the last fused topn, the first of the sort path
def test_fused_sort_boundary(mf, oracle, topn):
    I, k = 700, 8
    Q = _matrix(I, k, 3)
    P = np.random.default_rng(4).standard_normal((8, k)).astype(np.float32)
    with mf.MatrixFactorizationSGD(8, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        _check_side(m, oracle, Q, "items", topn, _queries(I))
        _planted_properties(m, Q, topn)


def test_padding_and_the_topn_bound(mf, oracle):
    I, k = 5, 16
    Q = _matrix(I, k, 5)
    P = np.random.default_rng(6).standard_normal((3, k)).astype(np.float32)
    q = np.array([4, 0, 2, 0], np.int32)
    with mf.MatrixFactorizationSGD(3, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        rn = _rn(oracle, Q)
        full = m.similar_items(q, 4)
        _same(full, _expected(oracle, Q, rn, q, Q, rn, 4, True))
        assert (full[0] >= 0).all()
        padded = m.similar_items(q, 5)
        _same(padded, _expected(oracle, Q, rn, q, Q, rn, 5, True))
        assert (padded[0][:, :4] >= 0).all() and (padded[0][:, 4] == -1).all() and np.isnan(padded[1][:, 4]).all()
        rows = m.similar_rows(Q[q], 5)  # nothing excluded: no padding
        _same(rows, _expected(oracle, Q[q], _rn(oracle, Q[q]), np.arange(4), Q, rn, 5, False))
        assert (rows[0] >= 0).all()
        for call in (lambda: m.similar_items(q, 6), lambda: m.similar_rows(Q[q], 6), lambda: m.similar_users([0], 4)):
            with pytest.raises(mf.MfsgdError) as err:
                call()
            assert err.value.code == -1
        _same(m.similar_users([0, 2], 3), _expected(oracle, P, _rn(oracle, P), [0, 2], P, _rn(oracle, P), 3, True))


@pytest.mark.parametrize("k", [1, 5, 17, 256])  # L = 1; zero padding inside a chunk; an odd count of chunks; L = 64
def test_lane_group_widths(mf, oracle, k):
    I, topn = 300, 10
    Q = _matrix(I, k, 7 + k)
    P = _matrix(200, k, 70 + k)
    with mf.MatrixFactorizationSGD(200, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        _check_side(m, oracle, Q, "items", topn, _queries(I))
        _check_side(m, oracle, P, "users", 129, _queries(200))  # ... and the sort path's kernels at this width


def test_user_side(mf, oracle):
    U, I, k, topn = 700, 40, 32, 10  # U != I: the wrong matrix or the wrong size shows
    P, Q = _matrix(U, k, 8), _matrix(I, k, 9)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        _check_side(m, oracle, P, "users", topn, _queries(U))
        _check_side(m, oracle, Q, "items", topn, _queries(I))
        _check_side(m, oracle, P, "users", 129, _queries(U))
        # a vector from the other side's space: folded-in users against items is the same call
        _same(m.similar_rows(P[:5], topn, side="items"),
              _expected(oracle, P[:5], _rn(oracle, P[:5]), np.arange(5), Q, _rn(oracle, Q), topn, False))
        with pytest.raises(mf.MfsgdError):
            m.similar_items([I], 3)
        with pytest.raises(mf.MfsgdError):
            m.similar_rows(P[:5], I + 1, side="items")


def test_no_stale_state(mf, oracle):
    I, k, topn = 700, 8, 10
    q = _queries(I)
    Q1, Q2 = _matrix(I, k, 10), _matrix(I, k, 11)
    P = np.random.default_rng(12).standard_normal((8, k)).astype(np.float32)
    with mf.MatrixFactorizationSGD(8, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q1)
        rn = _rn(oracle, Q1)
        _same(m.similar_items(q, topn), _expected(oracle, Q1, rn, q, Q1, rn, topn, True))
        m.set_factors(P, Q2)
        rn = _rn(oracle, Q2)
        _same(m.similar_items(q, topn), _expected(oracle, Q2, rn, q, Q2, rn, topn, True))
    w = mf.synth.workload("cfg1_ml100k", scale=0.2)
    with mf.MatrixFactorizationSGD(w["U"], w["I"], w["k"], LR, LAM, 7) as m:
        m.train(w["u"], w["i"], w["r"], 1)
        P, Q = m.get_factors()
        for M, side, size in ((Q, "items", w["I"]), (P, "users", w["U"])):
            q = np.array([0, size - 1, size // 2, 3], np.int32)
            _check_side(m, oracle, M, side, topn, q)


@pytest.mark.parametrize("topn", [10, 129])
def test_no_side_effects(mf, topn):
    U, I, k = 300, 700, 8
    P, Q = _matrix(U, k, 13), _matrix(I, k, 14)
    q = _queries(U)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        m.predict([0], [0])  # the factors are on the device from here on
        P0, Q0 = m.get_factors()
        before = mf.debug_device_bytes()
        calls = (lambda: m.similar_items(q, topn), lambda: m.similar_users(q, topn),
                 lambda: m.similar_rows(P[q], topn, side="items"), lambda: m.similar_rows(Q[q], topn, side="users"),
                 lambda: (m.row_inv_norms("items"), m.row_inv_norms("users")))
        for call in calls:
            first = call()
            assert mf.debug_device_bytes() == before
            again = call()
            assert mf.debug_device_bytes() == before
            for a, b in zip(first, again):
                assert a.tobytes() == b.tobytes()
        P1, Q1 = m.get_factors()
        assert P0.tobytes() == P1.tobytes() and Q0.tobytes() == Q1.tobytes()
