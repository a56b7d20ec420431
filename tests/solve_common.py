"""What the least-squares fold-in tests share (tests/test_fold_in_solve_cpu.py, tests/test_fold_in_solve_gpu.py): a C
restatement of the rule in include/mfsgd.h ("least-squares fold-in") -- the Gram matrix with its tiles, the system of a
row, Cholesky with the two substitutions, and a whole call over CSR -- written from that text, and the list generators.
The restatement works on dense n x k matrices; it is left-looking where the library's kernel is right-looking."""
import ctypes as C

import numpy as np

from tests import restatement

K_ALL = [1, 3, 8, 12, 16, 33, 64, 100, 128, 200, 256]
N_FIXED = 300       # rows of the fixed side in the per-k cases
LAM_EXACT = 0.05    # ridge_per_entry of the exact cases
LAM_IMPLICIT = 0.1  # ridge of the implicit cases (alpha = 1, confidences in [1, 41])

_SOURCE = r"""
#include <math.h>
#include <stdint.h>
#include <string.h>

/* G = gram(F), F dense n x k; tmp: k * k floats. */
void rs_gram(const float* F, int64_t n, int32_t k, float* G, float* tmp) {
    const int64_t T = 256 * ((n + 65535) / 65536);
    for (int64_t t = 0; t * T < n; ++t) {
        const int64_t r1 = (t + 1) * T < n ? (t + 1) * T : n;
        for (int32_t p = 0; p < k; ++p)
            for (int32_t q = 0; q <= p; ++q) {
                float g = 0.0f;
                for (int64_t r = t * T; r < r1; ++r) g = fmaf(F[r * k + p], F[r * k + q], g);
                tmp[p * k + q] = g;
            }
        for (int32_t p = 0; p < k; ++p)
            for (int32_t q = 0; q <= p; ++q) G[p * k + q] = t == 0 ? tmp[p * k + q] : G[p * k + q] + tmp[p * k + q];
    }
    for (int32_t p = 0; p < k; ++p)
        for (int32_t q = 0; q < p; ++q) G[q * k + p] = G[p * k + q];
}

/* The system of one row: A (k x k, lower triangle written) and rhs.  a and G nullable (G is read where alpha != 0). */
void rs_system(const float* F, int32_t k, const int32_t* ids, const float* a, const float* b, int64_t len, float alpha,
               const float* G, float ridge, float ridge_per_entry, float* A, float* rhs) {
    for (int32_t p = 0; p < k; ++p) {
        for (int32_t q = 0; q <= p; ++q) {
            float s = 0.0f;
            for (int64_t j = 0; j < len; ++j) {
                const float* f = F + (int64_t)ids[j] * k;
                const float t = a ? a[j] * f[p] : f[p];
                s = fmaf(t, f[q], s);
            }
            if (alpha != 0.0f) s = fmaf(alpha, G[p * k + q], s);
            A[p * k + q] = s;
        }
        float r = 0.0f;
        for (int64_t j = 0; j < len; ++j) r = fmaf(b[j], F[(int64_t)ids[j] * k + p], r);
        rhs[p] = r;
    }
    const float dg = fmaf(ridge_per_entry, (float)len, ridge);
    for (int32_t p = 0; p < k; ++p) A[p * k + p] = A[p * k + p] + dg;
}

/* Cholesky by columns in place (A's lower triangle becomes L), then the two substitutions.  Returns the status; on a
 * refusal x is k times 0x7FC00000.  work: 2 * k floats. */
int32_t rs_solve(int32_t k, float* A, const float* rhs, float* x, float* work) {
    float *inv = work, *y = work + k;
    for (int32_t j = 0; j < k; ++j) {
        float s = A[j * k + j];
        for (int32_t t = 0; t < j; ++t) s = fmaf(-A[j * k + t], A[j * k + t], s);
        if (!(s > 0.0f)) {
            const uint32_t nan = 0x7FC00000u;
            for (int32_t f = 0; f < k; ++f) memcpy(x + f, &nan, 4);
            return j + 1;
        }
        const float d = sqrtf(s);
        inv[j] = 1.0f / d;
        for (int32_t i = j + 1; i < k; ++i) {
            float v = A[i * k + j];
            for (int32_t t = 0; t < j; ++t) v = fmaf(-A[i * k + t], A[j * k + t], v);
            A[i * k + j] = v * inv[j];
        }
    }
    for (int32_t i = 0; i < k; ++i) {
        float s = rhs[i];
        for (int32_t t = 0; t < i; ++t) s = fmaf(-A[i * k + t], y[t], s);
        y[i] = s * inv[i];
    }
    for (int32_t i = k - 1; i >= 0; --i) {
        float s = y[i];
        for (int32_t t = k - 1; t > i; --t) s = fmaf(-A[t * k + i], x[t], s);
        x[i] = s * inv[i];
    }
    return 0;
}

/* A whole call: n_new lists in CSR form against F (n x k).  work: 3 * k * k + 3 * k floats. */
void rs_call(const float* F, int64_t n, int32_t k, int32_t n_new, const int64_t* row_ptr, const int32_t* ids, const float* a,
             const float* b, float alpha, float ridge, float ridge_per_entry, float* out_rows, int32_t* out_status, float* work) {
    float *G = work, *tmp = G + k * k, *A = tmp + k * k, *rhs = A + k * k, *w2 = rhs + k;
    if (alpha != 0.0f) rs_gram(F, n, k, G, tmp);
    for (int32_t x = 0; x < n_new; ++x) {
        const int64_t j0 = row_ptr[x], len = row_ptr[x + 1] - j0;
        if (len == 0) {
            for (int32_t f = 0; f < k; ++f) out_rows[(int64_t)x * k + f] = 0.0f;
            out_status[x] = 0;
            continue;
        }
        rs_system(F, k, ids + j0, a ? a + j0 : 0, b + j0, len, alpha, G, ridge, ridge_per_entry, A, rhs);
        out_status[x] = rs_solve(k, A, rhs, out_rows + (int64_t)x * k, w2);
    }
}
"""

_f32p, _i32p, _i64p = C.POINTER(C.c_float), C.POINTER(C.c_int32), C.POINTER(C.c_int64)


def _lib():
    return restatement.build("solve", _SOURCE, {
        "rs_gram": (None, [_f32p, C.c_int64, C.c_int32, _f32p, _f32p]),
        "rs_system": (None, [_f32p, C.c_int32, _i32p, _f32p, _f32p, C.c_int64, C.c_float, _f32p, C.c_float, C.c_float, _f32p, _f32p]),
        "rs_solve": (C.c_int32, [C.c_int32, _f32p, _f32p, _f32p, _f32p]),
        "rs_call": (None, [_f32p, C.c_int64, C.c_int32, C.c_int32, _i64p, _i32p, _f32p, _f32p, C.c_float, C.c_float, C.c_float,
                           _f32p, _i32p, _f32p]),
    })


def _p(a, t):
    return None if a is None else a.ctypes.data_as(t)


def _f32(a):
    return None if a is None else np.ascontiguousarray(a, np.float32)


def gram(F):
    F = _f32(F)
    n, k = F.shape
    G, tmp = np.zeros((k, k), np.float32), np.zeros((k, k), np.float32)
    _lib().rs_gram(_p(F, _f32p), n, k, _p(G, _f32p), _p(tmp, _f32p))
    return G


def system(F, ids, a, b, alpha=0.0, G=None, ridge=0.0, ridge_per_entry=0.0):
    """(A, rhs) of one row; A's lower triangle is the system's, the upper is zero."""
    F, a, b, G = _f32(F), _f32(a), _f32(b), _f32(G)
    ids = np.ascontiguousarray(ids, np.int32)
    k = F.shape[1]
    A, rhs = np.zeros((k, k), np.float32), np.zeros(k, np.float32)
    _lib().rs_system(_p(F, _f32p), k, _p(ids, _i32p), _p(a, _f32p), _p(b, _f32p), ids.size, alpha, _p(G, _f32p), ridge,
                     ridge_per_entry, _p(A, _f32p), _p(rhs, _f32p))
    return A, rhs


def solve(A, rhs):
    """(x, status) of the rule's Cholesky solve of the system whose lower triangle is A's."""
    A, rhs = _f32(A).copy(), _f32(rhs)
    k = rhs.size
    x, work = np.zeros(k, np.float32), np.zeros(2 * k, np.float32)
    st = _lib().rs_solve(k, _p(A, _f32p), _p(rhs, _f32p), _p(x, _f32p), _p(work, _f32p))
    return x, st


def call(F, row_ptr, ids, a, b, alpha=0.0, ridge=0.0, ridge_per_entry=0.0):
    """(rows, status) of a whole mfsgd_fold_in_solve call against the dense fixed side F."""
    F, a, b = _f32(F), _f32(a), _f32(b)
    row_ptr, ids = np.ascontiguousarray(row_ptr, np.int64), np.ascontiguousarray(ids, np.int32)
    n, k = F.shape
    n_new = row_ptr.size - 1
    rows, st = np.zeros((n_new, k), np.float32), np.zeros(n_new, np.int32)
    work = np.zeros(3 * k * k + 3 * k, np.float32)
    _lib().rs_call(_p(F, _f32p), n, k, n_new, _p(row_ptr, _i64p), _p(ids, _i32p), _p(a, _f32p), _p(b, _f32p), alpha, ridge,
                   ridge_per_entry, _p(rows, _f32p), _p(st, _i32p), _p(work, _f32p))
    return rows, st


def exact(F, row_ptr, ids, r, lam, w=None):
    """fold_in_exact / fold_in_items_exact by the restatement."""
    r = _f32(r)
    return call(F, row_ptr, ids, _f32(w), r if w is None else _f32(w) * r, 0.0, 0.0, lam)


def implicit(F, row_ptr, ids, c, lam, unobserved=1.0):
    """fold_in_implicit / fold_in_items_implicit by the restatement."""
    c = _f32(c)
    return call(F, row_ptr, ids, c - np.float32(unobserved), c, unobserved, lam, 0.0)


def fixed_side(n, k, rng):
    """Rows N(0, 0.25 / k)."""
    return (rng.standard_normal((n, k)) * (0.5 / np.sqrt(k))).astype(np.float32)


def mixed_lists(n_fixed, k, rng):
    """(row_ptr, ids): 150 rows up to k = 64 and 24 above, of lengths 0, 1, below k, k, above k and a few hundred,
    shuffled so that neighbours differ widely; one row names an id twice, adjacent and not adjacent."""
    n = 150 if k <= 64 else 24
    lens = np.concatenate([[0, 0, 1, 1, max(k - 1, 1), k, k + 1, 2 * k + 3, 17],
                           rng.integers(1, max(k, 2), (n - 9) // 3), rng.integers(k, 3 * k + 2, (n - 9) // 3),
                           rng.integers(100, 400, n - 9 - 2 * ((n - 9) // 3))])
    rng.shuffle(lens)
    at = int(np.flatnonzero(lens == 17)[0])
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    ids = rng.integers(0, n_fixed, int(row_ptr[-1])).astype(np.int32)
    ids[row_ptr[at] + 5] = ids[row_ptr[at] + 2]   # the same id twice in one list, not adjacent
    ids[row_ptr[at] + 9] = ids[row_ptr[at] + 8]   # ... and adjacent
    return row_ptr, ids


def case(k):
    """The per-k inputs of the CPU and GPU tests: the fixed side, the lists, ratings in [0.5, 5], weights in [0.5, 2]
    and confidences in [1, 41]."""
    rng = np.random.default_rng(4000 + k)
    F = fixed_side(N_FIXED, k, rng)
    row_ptr, ids = mixed_lists(N_FIXED, k, rng)
    r = rng.uniform(0.5, 5.0, ids.size).astype(np.float32)
    w = rng.uniform(0.5, 2.0, ids.size).astype(np.float32)
    c = rng.uniform(1.0, 41.0, ids.size).astype(np.float32)
    return dict(F=F, row_ptr=row_ptr, ids=ids, r=r, w=w, c=c)


def reversed_rows(row_ptr, *arrays):
    """The same lists with the rows in the opposite order: (row_ptr, arrays...)."""
    n = row_ptr.size - 1
    pieces = [slice(row_ptr[x], row_ptr[x + 1]) for x in range(n)][::-1]
    rev_ptr = np.concatenate([[0], np.cumsum(np.diff(row_ptr)[::-1])]).astype(np.int64)
    return (rev_ptr,) + tuple(np.concatenate([a[s] for s in pieces]) for a in arrays)


# ALS at the shape both tests use
ALS_U, ALS_I, ALS_K, ALS_N, ALS_LAM, ALS_SEED = 60, 40, 8, 600, 0.05, 11


def als_case():
    """(u, i, r, c, P0, Q0): about 600 ratings of a rank-3 ground truth plus noise, confidences, and seeded factors."""
    rng = np.random.default_rng(ALS_SEED)
    u = rng.integers(0, ALS_U, ALS_N).astype(np.int32)
    i = rng.integers(0, ALS_I, ALS_N).astype(np.int32)
    A, B = rng.standard_normal((ALS_U, 3)), rng.standard_normal((ALS_I, 3))
    r = (np.einsum("ij,ij->i", A[u], B[i]) + 3.0 + 0.1 * rng.standard_normal(ALS_N)).astype(np.float32)
    c = rng.uniform(1.0, 41.0, ALS_N).astype(np.float32)
    P0 = fixed_side(ALS_U, ALS_K, rng)
    Q0 = fixed_side(ALS_I, ALS_K, rng)
    return u, i, r, c, P0, Q0


def _csr(keys, n):
    order = np.argsort(keys, kind="stable")
    return np.concatenate([[0], np.cumsum(np.bincount(keys, minlength=n))]).astype(np.int64), order


def als_objective(P, Q, u, i, r, lam):
    P, Q = P.astype(np.float64), Q.astype(np.float64)
    e = r.astype(np.float64) - np.einsum("ij,ij->i", P[u], Q[i])
    nu, ni = np.bincount(u, minlength=P.shape[0]), np.bincount(i, minlength=Q.shape[0])
    return float(e @ e) + lam * float(nu @ (P * P).sum(1)) + lam * float(ni @ (Q * Q).sum(1))


def ials_objective(P, Q, u, i, c, lam, unobserved):
    P, Q = P.astype(np.float64), Q.astype(np.float64)
    s = np.einsum("ij,ij->i", P[u], Q[i])
    rest = float(((P.T @ P) * (Q.T @ Q)).sum()) - float(s @ s)
    return float(c.astype(np.float64) @ ((1.0 - s) ** 2)) + unobserved * rest + lam * (float((P * P).sum()) + float((Q * Q).sum()))


def als_loop(P, Q, u, i, values, sweeps, fold, objective):
    """The alternation over the restatement: fold(F, row_ptr, ids, values) -> (rows, status).  Returns (P, Q, the
    objective after each half-sweep)."""
    ptr_u, by_u = _csr(u, P.shape[0])
    ptr_i, by_i = _csr(i, Q.shape[0])
    out = []
    for _ in range(sweeps):
        P, st = fold(Q, ptr_u, i[by_u], values[by_u])
        assert not st.any()
        out.append(objective(P, Q))
        Q, st = fold(P, ptr_i, u[by_i], values[by_i])
        assert not st.any()
        out.append(objective(P, Q))
    return P, Q, np.array(out)
