"""What the pairwise (BPR) tests share (tests/test_pairwise_cpu.py, tests/test_pairwise_gpu.py): the three-way dependency
levels restated in Python, the batches that reach each shape of a level list, and a small C restatement of the arithmetic
of DESIGN.md section 3 ("Pairwise ranking") -- lsig and the sequential triple loop over dense rows -- written from that
text, compiled here with the host compiler at -O2 -ffp-contract=off and linked to the oracle for its canonical dot."""
import ctypes as C

import numpy as np

from tests import online_common as oc
from tests.restatement import build

PIECE = oc.PIECE  # triples per piece (include/mfsgd.h, "pairwise ranking")

KNOWN = [  # x, bits of lsig(x): the table of DESIGN.md
    (0.0, 0x3F000000), (1.0, 0x3E89B2B1), (-1.0, 0x3F3B26A8), (0.5, 0x3EC14D03), (-7.25, 0x3F7FD17E),
    (30.0, 0x29D2B707), (80.0, 0x05BFECBA), (np.inf, 0x05BFECBA), (-80.0, 0x3F800000), (-np.inf, 0x3F800000),
]


# ---- the levels -------------------------------------------------------------------------------------------------------------
def py_levels(u, i, j):
    """level[x] as include/mfsgd.h defines it, piece by piece: an item is one row whichever position it stands in."""
    level = np.zeros(len(u), np.int32)
    for x0 in range(0, len(u), PIECE):
        last_u, last_i = {}, {}
        for x in range(x0, min(x0 + PIECE, len(u))):
            a, b, c = int(u[x]), int(i[x]), int(j[x])
            level[x] = 1 + max(last_u.get(a, -1), last_i.get(b, -1), last_i.get(c, -1))
            last_u[a] = last_i[b] = last_i[c] = level[x]
    return level


py_info = oc.py_info


def _other_item(rng, i, I):
    """For every i[x] an item of 0 .. I - 1 that is not i[x], uniformly."""
    return ((i + rng.integers(1, I, i.size)) % I).astype(np.int32)


def random_batch(U=37, I=29, n=3000, seed=5):
    rng = np.random.default_rng(seed)
    u, i = rng.integers(0, U, n).astype(np.int32), rng.integers(0, I, n).astype(np.int32)
    return U, I, u, i, _other_item(rng, i, I)


def hot_positive_batch(n=600, seed=7):
    """n users prefer item 3 to n different items: n levels of width 1."""
    rng = np.random.default_rng(seed)
    return n, n + 4, rng.permutation(n).astype(np.int32), np.full(n, 3, np.int32), (4 + rng.permutation(n)).astype(np.int32)


def hot_negative_batch(n=600, seed=8):
    U, I, u, i, j = hot_positive_batch(n, seed)
    return U, I, u, j, i


def one_user_batch(n=600, seed=9):
    """One user, 2 n different items: the user row carries the chain."""
    rng = np.random.default_rng(seed)
    items = rng.permutation(2 * n).astype(np.int32)
    return 3, 2 * n, np.full(n, 1, np.int32), items[:n].copy(), items[n:].copy()


def cross_role_batch(n=300):
    """Item x + 1 is the negative of triple x and the positive of triple x + 1; every triple has a user of its own, so
    the only dependence is through an item that changes its position: n levels of width 1."""
    x = np.arange(n, dtype=np.int32)
    return n, n + 1, x.copy(), x.copy(), x + 1


def two_step_batch():
    """Item 2 is i in the first triple and j in the next; the third shares nothing with either."""
    return 4, 6, np.array([0, 1, 2], np.int32), np.array([2, 4, 0], np.int32), np.array([3, 2, 1], np.int32)


def hot_in_wide_batch(U=4096, I=4096, n=12000, seed=11):
    """A wide random batch in which every 40th positive is item 7."""
    rng = np.random.default_rng(seed)
    u, i = rng.integers(0, U, n).astype(np.int32), rng.integers(0, I, n).astype(np.int32)
    i[::40] = 7
    return U, I, u, i, _other_item(rng, i, I)


def two_piece_batch(extra, seed=10, U=3001, I=3001):
    n = PIECE + extra
    rng = np.random.default_rng(seed)
    u, i = rng.integers(0, U, n).astype(np.int32), rng.integers(0, I, n).astype(np.int32)
    return U, I, u, i, _other_item(rng, i, I)


def widths_batch(widths):
    """online_common.widths_batch carried over to triples: its (user, item) pairs are the (user, positive) pairs, and
    every triple gets a negative nobody else names, so the levels are exactly those widths."""
    U, I, u, i, _ = oc.widths_batch(widths)
    j = (I + np.arange(u.size)).astype(np.int32)
    return U, I + u.size, u, i, j


# ---- the arithmetic, in C ---------------------------------------------------------------------------------------------------
C_SOURCE = r"""
#include <math.h>
#include <stdint.h>
#include <string.h>

float mfo_dot(const float* p, const float* q, int32_t k);

static float from_bits(uint32_t b) { float f; memcpy(&f, &b, 4); return f; }

static float lsig(float x) {
    if (isnan(x)) return from_bits(0x7FC00000u);
    float t = x > 80.0f ? 80.0f : (x < -80.0f ? -80.0f : x);
    float n = rintf(t * from_bits(0x3FB8AA3Bu));
    float r = fmaf(n, -0.693359375f, t);
    r = fmaf(n, 2.12194440e-4f, r);
    float q = 1.9875691500e-4f;
    q = fmaf(q, r, 1.3981999507e-3f);
    q = fmaf(q, r, 8.3334519073e-3f);
    q = fmaf(q, r, 4.1665795894e-2f);
    q = fmaf(q, r, 1.6666665459e-1f);
    q = fmaf(q, r, 5.0000001201e-1f);
    float rr = r * r;
    float e = fmaf(q, rr, r);
    e = e + 1.0f;
    float y = e * from_bits((uint32_t)((int32_t)n + 127) << 23);
    float d = 1.0f + y;
    return 1.0f / d;
}

void pw_lsig(const float* x, float* g, int64_t n) {
    for (int64_t a = 0; a < n; ++a) g[a] = lsig(x[a]);
}

/* the sequential loop: P, Q dense (k floats a row); margin nullable */
void pw_pass(float* P, float* Q, int32_t k, const int32_t* u, const int32_t* i, const int32_t* j, int64_t n, float lr,
             float lambda, float* margin) {
    const float c = 1.0f - lr * lambda;
    for (int64_t t = 0; t < n; ++t) {
        float* p = P + (int64_t)u[t] * k;
        float* qi = Q + (int64_t)i[t] * k;
        float* qj = Q + (int64_t)j[t] * k;
        const float di = mfo_dot(p, qi, k);
        const float dj = mfo_dot(p, qj, k);
        const float x = di - dj;
        const float g = lsig(x);
        const float s = lr * g;
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
    return build("pairwise", C_SOURCE, {"pw_lsig": (None, [_f, _f, C.c_int64]),
                                          "pw_pass": (None, [_f, _f, C.c_int32, _i, _i, _i, C.c_int64, C.c_float, C.c_float, _f])})


def c_lsig(x):
    x = np.ascontiguousarray(x, np.float32)
    g = np.empty(x.shape, np.float32)
    restatement().pw_lsig(x.ctypes.data_as(_f), g.ctypes.data_as(_f), x.size)
    return g


def c_pass(P, Q, u, i, j, lr, lam):
    """The sequential loop on copies of the dense P and Q: (P, Q, margins)."""
    P, Q = np.ascontiguousarray(P, np.float32).copy(), np.ascontiguousarray(Q, np.float32).copy()
    u, i, j = (np.ascontiguousarray(a, np.int32) for a in (u, i, j))
    assert u.shape == i.shape == j.shape and not (i == j).any() and P.shape[1] == Q.shape[1]
    assert u.size == 0 or (0 <= u.min() and u.max() < P.shape[0] and 0 <= min(i.min(), j.min()) and max(i.max(), j.max()) < Q.shape[0])
    x = np.empty(u.size, np.float32)
    restatement().pw_pass(P.ctypes.data_as(_f), Q.ctypes.data_as(_f), P.shape[1], u.ctypes.data_as(_i), i.ctypes.data_as(_i),
                          j.ctypes.data_as(_i), u.size, lr, lam, x.ctypes.data_as(_f))
    return P, Q, x
