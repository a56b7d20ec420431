"""What the pairwise fold-in tests share (tests/test_fold_in_pairwise_cpu.py, tests/test_fold_in_pairwise_gpu.py): the rule
of mfsgd_fold_in_users_pairwise (include/mfsgd.h) restated.  The draws are tests/implicit_common.draw, the pick is
tests/hardneg_common.pick, and the arithmetic of a step is a small C restatement written from the header's text -- the
canonical dot is the oracle's mfo_dot, lsig is the text tests/pairwise_common.py compiles -- built the way that module
builds its own: the host compiler at -O2 -ffp-contract=off, linked to the oracle."""
import ctypes as C

import numpy as np

from tests import hardneg_common as HC
from tests import implicit_common as IC
from tests import pairwise_common as PC
from tests.restatement import build

NAN_BITS = HC.NAN_BITS  # the margin of a step that was not taken

# from_bits and lsig, character for character what tests/pairwise_common.py compiles
_LSIG_TEXT = PC.C_SOURCE[PC.C_SOURCE.index("static float from_bits"):PC.C_SOURCE.index("void pw_lsig")]

C_SOURCE = r"""
#include <math.h>
#include <stdint.h>
#include <string.h>

float mfo_dot(const float* p, const float* q, int32_t k);

""" + _LSIG_TEXT + r"""
/* score(d) = dot(row, Q[cand[d]]); Q dense (k floats a row) */
void fp_scores(const float* row, const float* Q, int32_t k, const int32_t* cand, int32_t m, float* out) {
    for (int32_t d = 0; d < m; ++d) out[d] = mfo_dot(row, Q + (int64_t)cand[d] * k, k);
}

/* one step on the row against Q[i] and Q[j]: the margin before it */
float fp_step(float* row, const float* Q, int32_t k, int32_t i, int32_t j, float lr, float lambda) {
    const float* qi = Q + (int64_t)i * k;
    const float* qj = Q + (int64_t)j * k;
    const float c = 1.0f - lr * lambda;
    const float di = mfo_dot(row, qi, k);
    const float dj = mfo_dot(row, qj, k);
    const float xm = di - dj;
    const float g = lsig(xm);
    const float sz = lr * g;
    for (int32_t f = 0; f < k; ++f) {
        const float diff = qi[f] - qj[f];
        const float cr = c * row[f];
        row[f] = fmaf(sz, diff, cr);
    }
    return xm;
}

/* n steps with given negatives (m == 1: the draw is the negative) */
void fp_chain(float* row, const float* Q, int32_t k, const int32_t* pos, const int32_t* neg, int64_t n, float lr, float lambda,
              float* margin) {
    for (int64_t t = 0; t < n; ++t) margin[t] = fp_step(row, Q, k, pos[t], neg[t], lr, lambda);
}
"""

_f = C.POINTER(C.c_float)
_i = C.POINTER(C.c_int32)


def restatement():
    """The compiled restatement (tests/restatement.py builds it, once per process)."""
    return build("fold_in_pairwise", C_SOURCE, {
        "fp_scores": (None, [_f, _f, C.c_int32, _i, C.c_int32, _f]),
        "fp_step": (C.c_float, [_f, _f, C.c_int32, C.c_int32, C.c_int32, C.c_float, C.c_float]),
        "fp_chain": (None, [_f, _f, C.c_int32, _i, _i, C.c_int64, C.c_float, C.c_float, _f])})


def chain(row, Q, pos, neg, lr, lam):
    """(row, margins) after the steps (pos[t], neg[t]) on a copy of `row`, the negatives given."""
    row, Q = np.ascontiguousarray(row, np.float32).copy(), np.ascontiguousarray(Q, np.float32)
    pos, neg = np.ascontiguousarray(pos, np.int32), np.ascontiguousarray(neg, np.int32)
    assert row.ndim == 1 and Q.shape[1] == row.size and pos.shape == neg.shape
    xm = np.empty(pos.size, np.float32)
    restatement().fp_chain(row.ctypes.data_as(_f), Q.ctypes.data_as(_f), row.size, pos.ctypes.data_as(_i), neg.ctypes.data_as(_i),
                           pos.size, lr, lam, xm.ctypes.data_as(_f))
    return row, xm


def counters(row_ptr, x, epochs, m, first=0):
    """c_d of every step of user x: int64 [len * epochs, m]."""
    steps = int(row_ptr[x + 1] - row_ptr[x]) * epochs
    tau = int(row_ptr[x]) * epochs + np.arange(steps, dtype=np.int64)
    return int(first) + tau[:, None] * m + np.arange(m, dtype=np.int64)


def fold(Q, row_ptr, items, epochs, m, init, lr, lam, draw_seed=0, first=0):
    """(rows, margins, negatives) that fold_in_pairwise(row_ptr, items, epochs, candidates=m, init=init, draw_seed=...,
    first=...) must return against the dense Q, bit for bit."""
    lib = restatement()
    Q = np.ascontiguousarray(Q, np.float32)
    n_items, k = Q.shape
    row_ptr, items = np.asarray(row_ptr, np.int64), np.ascontiguousarray(items, np.int32)
    rows = np.ascontiguousarray(init, np.float32).copy()
    total = int(row_ptr[-1]) * epochs
    margins, negs = np.empty(total, np.float32), np.full(total, -1, np.int32)
    margins.view(np.uint32)[:] = NAN_BITS
    sc = np.empty(m, np.float32)
    for x in range(row_ptr.size - 1):
        A = items[row_ptr[x]:row_ptr[x + 1]]
        S = np.unique(A)
        steps, o = A.size * epochs, int(row_ptr[x]) * epochs
        if S.size == n_items or steps == 0:
            continue
        cand = np.ascontiguousarray(IC.draw(S, n_items, draw_seed, counters(row_ptr, x, epochs, m, first)))
        pos = np.tile(A, epochs)
        if m == 1:
            rows[x], margins[o:o + steps] = chain(rows[x], Q, pos, cand[:, 0], lr, lam)
            negs[o:o + steps] = cand[:, 0]
            continue
        row = rows[x]  # (a view: the steps write the row in place)
        for tau in range(steps):
            lib.fp_scores(row.ctypes.data_as(_f), Q.ctypes.data_as(_f), k, cand[tau].ctypes.data_as(_i), m, sc.ctypes.data_as(_f))
            j = int(cand[tau, int(HC.pick(sc[None])[0])])
            margins[o + tau] = lib.fp_step(row.ctypes.data_as(_f), Q.ctypes.data_as(_f), k, int(pos[tau]), j, lr, lam)
            negs[o + tau] = j
    return rows, margins, negs


def csr(lists):
    """(row_ptr int64, items int32) of a list of lists."""
    row_ptr = np.concatenate([[0], np.cumsum([len(a) for a in lists])]).astype(np.int64)
    items = np.concatenate([np.asarray(a, np.int32) for a in lists] + [np.empty(0, np.int32)]).astype(np.int32)
    return row_ptr, items


def same_bits(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()
