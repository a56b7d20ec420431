"""What the WARP tests share (tests/test_warp_cpu.py, tests/test_warp_gpu.py), restated from include/mfsgd.h: the rule of
mfsgd_sample_unseen_violating in numpy, on top of tests/implicit_common.sample for the candidates and a scorer that is
passed in; the harmonic weight of mfsgd_warp_weights; the sequential loop of mfsgd_apply_triples_weighted in C over the
oracle's canonical dot (compiled as tests/pairwise_common.py compiles its own); and fit_warp as the loop it is documented
as.  Everything the device is compared with is compared byte for byte."""
import ctypes as C

import numpy as np

from tests import implicit_common as IC
from tests.restatement import build

NAN_BITS = 0x7FC00000  # the margin of a row without a pick


# ---- the rule ---------------------------------------------------------------------------------------------------------------
def first_violating(x, cand, pos, margin):
    """d per row of a float32 table x[n, m] (x[r, d] = the positive's score minus candidate d's): the smallest d with
    cand[r, d] != pos[r] and x[r, d] < margin as floats -- a NaN never is, x == margin is not -- and m where there is none."""
    x = np.asarray(x, np.float32)
    assert x.ndim == 2 and x.shape == np.shape(cand)
    with np.errstate(invalid="ignore"):
        viol = (np.asarray(cand) != np.asarray(pos)[:, None]) & (x < np.float32(margin))
    d = np.where(viol.any(axis=1), np.argmax(viol, axis=1), x.shape[1])
    return d.astype(np.int32)


def outputs(x, cand, pos, margin, cnt):
    """(items, draws, margins, ranks) of the rule for rows whose users have cnt[r] unseen items; cnt[r] == 0: nothing to draw."""
    x, cand, cnt = np.asarray(x, np.float32), np.asarray(cand, np.int32), np.asarray(cnt, np.int64)
    n, m = x.shape
    d = first_violating(x, cand, pos, margin)
    hit = (d < m) & (cnt > 0)
    rows, at = np.arange(n), np.minimum(d, m - 1)
    items = np.where(hit, cand[rows, at], -1).astype(np.int32)
    margins = np.where(hit, x[rows, at], np.float32(0)).astype(np.float32)
    margins.view(np.uint32)[~hit] = NAN_BITS
    ranks = np.where(hit, np.maximum(1, cnt // (d.astype(np.int64) + 1)), 0).astype(np.int32)
    draws = np.where(cnt > 0, d, -1).astype(np.int32)
    return items, draws, margins, ranks


def violating(lists, n_items, users, pos, m, margin, seed, first, scorer):
    """(items int32[n], draws int32[n], margins float32[n], ranks int32[n]) that sample_unseen_violating(users, pos, m,
    margin, seed, first, draws=True, margins=True, ranks=True) must return when user u's list is lists(u) and scorer(u, i)
    gives float32 dot(P[u[x]], Q[i[x]]) for int32 arrays u, i."""
    users, pos = np.asarray(users, np.int32), np.asarray(pos, np.int32)
    n = users.size
    cand = IC.sample(lists, n_items, users, m, seed, first)
    full = cand[:, 0] < 0 if n else np.zeros(0, bool)  # a row is -1 throughout or not at all
    assert ((cand < 0) == full[:, None]).all()
    cnt = np.array([0 if f else n_items - len(lists(int(u))) for u, f in zip(users, full)], np.int64)
    assert ((cnt == 0) == full).all()
    sp = scorer(users, pos)
    sc = scorer(np.repeat(users, m), np.where(cand < 0, 0, cand).ravel().astype(np.int32)).reshape(n, m)
    assert sp.dtype == np.float32 and sc.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        x = sp[:, None] - sc  # one fp32 subtraction
    return outputs(x, cand, pos, margin, cnt)


# ---- the weight -------------------------------------------------------------------------------------------------------------
def harmonic(rank):
    """float32 L(rank): L(0) = 0, L(r) = 1/1 + ... + 1/r in float64, ascending, rounded once."""
    rank = np.asarray(rank, np.int64)
    top = int(rank.max()) if rank.size else 0
    table = np.zeros(top + 1, np.float64)
    table[1:] = np.cumsum(1.0 / np.arange(1, top + 1, dtype=np.float64))  # (cumsum adds in ascending order, one by one)
    return table[rank].astype(np.float32)


# ---- the weighted loop, in C --------------------------------------------------------------------------------------------------
C_SOURCE = r"""
#include <math.h>
#include <stdint.h>

float mfo_dot(const float* p, const float* q, int32_t k);

/* the sequential loop of mfsgd_apply_triples_weighted: P, Q dense (k floats a row); margin nullable */
void ww_pass(float* P, float* Q, int32_t k, const int32_t* u, const int32_t* i, const int32_t* j, const float* w, int64_t n,
             float lr, float lambda, float* margin) {
    const float c = 1.0f - lr * lambda;
    for (int64_t t = 0; t < n; ++t) {
        float* p = P + (int64_t)u[t] * k;
        float* qi = Q + (int64_t)i[t] * k;
        float* qj = Q + (int64_t)j[t] * k;
        const float di = mfo_dot(p, qi, k);
        const float dj = mfo_dot(p, qj, k);
        const float x = di - dj;
        const float s = lr * w[t];
        if (margin) margin[t] = x;
        for (int32_t f = 0; f < k; ++f) {
            const float pf = p[f], a = qi[f], b = qj[f];
            const float diff = a - b;
            const float cp = c * pf, ca = c * a, cb = c * b;
            p[f] = fmaf(s, diff, cp);
            qi[f] = fmaf(s, pf, ca);
            qj[f] = fmaf(-s, pf, cb);
        }
    }
}
"""

_f = C.POINTER(C.c_float)
_i = C.POINTER(C.c_int32)


def restatement():
    """The compiled restatement (tests/restatement.py builds it, once per process)."""
    return build("warp", C_SOURCE, {"ww_pass": (None, [_f, _f, C.c_int32, _i, _i, _i, _f, C.c_int64, C.c_float, C.c_float, _f])})


def canon_weights(w):
    """The weights as the call takes them in: every NaN is 0x7FC00000."""
    w = np.ascontiguousarray(w, np.float32).copy()
    w.view(np.uint32)[np.isnan(w)] = NAN_BITS
    return w


def c_pass(P, Q, u, i, j, w, lr, lam):
    """The weighted sequential loop on copies of the dense P and Q: (P, Q, margins)."""
    P, Q = np.ascontiguousarray(P, np.float32).copy(), np.ascontiguousarray(Q, np.float32).copy()
    u, i, j = (np.ascontiguousarray(a, np.int32) for a in (u, i, j))
    w = canon_weights(w)
    assert u.shape == i.shape == j.shape == w.shape and not (i == j).any() and P.shape[1] == Q.shape[1]
    assert u.size == 0 or (0 <= u.min() and u.max() < P.shape[0] and 0 <= min(i.min(), j.min()) and max(i.max(), j.max()) < Q.shape[0])
    x = np.empty(u.size, np.float32)
    restatement().ww_pass(P.ctypes.data_as(_f), Q.ctypes.data_as(_f), P.shape[1], u.ctypes.data_as(_i), i.ctypes.data_as(_i),
                          j.ctypes.data_as(_i), w.ctypes.data_as(_f), u.size, lr, lam, x.ctypes.data_as(_f))
    return P, Q, x


# ---- fit_warp ---------------------------------------------------------------------------------------------------------------
def fit_warp(oracle, P, Q, lists, u, i, epochs, lr, lam, *, candidates, margin, refresh=None, seed=0, first_epoch=0):
    """fit_warp as include/mfsgd.h's calls say it runs, from the dense factors P, Q: (P, Q, dict(violating, trials))."""
    u, i = np.asarray(u, np.int32), np.asarray(i, np.int32)
    n, m, n_items = u.size, int(candidates), Q.shape[0]
    step = max(n, 1) if refresh is None else int(refresh)
    violating_, trials = np.zeros(epochs), np.zeros(epochs)
    P, Q = P.copy(), Q.copy()
    for e in range(epochs):
        hits = draws = 0
        for a in range(0, n, step):
            bu, bi = u[a:a + step], i[a:a + step]
            J, d, _, rk = violating(lists, n_items, bu, bi, m, margin, seed, ((first_epoch + e) * n + a) * m,
                                    lambda uu, ii: oracle.predict(P, Q, uu, ii))
            keep = J >= 0
            P, Q, _ = c_pass(P, Q, bu[keep], bi[keep], J[keep], harmonic(rk[keep]), lr, lam)
            hits += int(keep.sum())
            draws += int(d[keep].sum()) + int(keep.sum())
        violating_[e] = hits / n if n else 0.0
        trials[e] = draws / hits if hits else 0.0
    return P, Q, dict(violating=violating_, trials=trials)
