"""What the weighted-pick tests share (tests/test_weighted_picks_cpu.py, tests/test_weighted_picks_gpu.py): the rules of
mfsgd_sample_unseen_hard_weighted, mfsgd_sample_unseen_violating_weighted and mfsgd_fold_in_users_pairwise_weighted
(include/mfsgd.h) restated, composed from what the tests of their parts already have and of nothing new: the candidates
are tests/weighted_common.sample_weighted, the hard pick is tests/hardneg_common.pick, the violating outputs are
tests/warp_common.outputs, and the fold is the chain of tests/fold_in_pairwise_common.py with the weighted candidates in
the place of the uniform ones.  Everything the device is compared with is compared byte for byte."""
import numpy as np

from tests import fold_in_pairwise_common as FC
from tests import hardneg_common as HC
from tests import warp_common as WC
from tests import weighted_common as WM

NAN_BITS = HC.NAN_BITS


def _scores(scorer, users, cand):
    n, m = cand.shape
    sc = scorer(np.repeat(users, m), np.where(cand < 0, 0, cand).ravel().astype(np.int32)).reshape(n, m)
    assert sc.dtype == np.float32
    return sc


def _candidates(lists, w, users, m, seed, first):
    """(cand int32[n, m], mass int64[n]): a row is -1 throughout exactly where its unseen weight is 0."""
    cand, mass = WM.sample_weighted(lists, w, users, m, seed, first, mass=True)
    assert ((cand < 0) == (mass == 0)[:, None]).all()
    return cand, mass


def hard(lists, w, users, m, seed, first, scorer):
    """(items int32[n], scores float32[n], draws int32[n], mass int64[n]) that sample_unseen_hard(users, m, seed, first,
    scores=True, draws=True, sampling="weighted", mass=True) must return when user u's list is lists(u), the weights are w
    and scorer(u, i) gives float32 dot(P[u[x]], Q[i[x]]) for int32 arrays u, i."""
    users = np.asarray(users, np.int32)
    cand, mass = _candidates(lists, w, users, m, seed, first)
    sc = _scores(scorer, users, cand)
    d = HC.pick(sc)
    rows, none = np.arange(users.size), mass == 0
    items, scores = cand[rows, d].copy(), sc[rows, d].copy()
    items[none], d[none] = -1, -1
    scores.view(np.uint32)[none] = NAN_BITS
    return items, scores, d, mass


def violating(lists, w, n_items, users, pos, m, margin, seed, first, scorer):
    """(items, draws, margins, ranks, mass) that sample_unseen_violating(users, pos, m, margin, seed, first, draws=True,
    margins=True, ranks=True, sampling="weighted", mass=True) must return.  The rank scales by the unseen item COUNT of
    the rows that have unseen weight; the rows that have none are warp_common's "nothing to draw"."""
    users, pos = np.asarray(users, np.int32), np.asarray(pos, np.int32)
    cand, mass = _candidates(lists, w, users, m, seed, first)
    cnt = np.array([n_items - len(lists(int(u))) if ms > 0 else 0 for u, ms in zip(users, mass)], np.int64)
    sp, sc = scorer(users, pos), _scores(scorer, users, cand)
    assert sp.dtype == np.float32
    with np.errstate(invalid="ignore", over="ignore"):
        x = sp[:, None] - sc  # one fp32 subtraction
    return WC.outputs(x, cand, pos, margin, cnt) + (mass,)


def fold(Q, w, row_ptr, items, epochs, m, init, lr, lam, draw_seed=0, first=0):
    """(rows, margins, negatives) that fold_in_pairwise(row_ptr, items, epochs, candidates=m, init=init, draw_seed=...,
    first=..., sampling="weighted") must return against the dense Q under the weights w: fold_in_pairwise_common.fold with
    the weighted draw, and no step for a user whose unseen weight is 0."""
    lib = FC.restatement()
    Q = np.ascontiguousarray(Q, np.float32)
    k = Q.shape[1]
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
        if WM.unseen_mass(S, w) == 0 or steps == 0:
            continue
        cand = np.ascontiguousarray(WM.draw_weighted(S, w, draw_seed, FC.counters(row_ptr, x, epochs, m, first)))
        pos = np.tile(A, epochs)
        if m == 1:
            rows[x], margins[o:o + steps] = FC.chain(rows[x], Q, pos, cand[:, 0], lr, lam)
            negs[o:o + steps] = cand[:, 0]
            continue
        row = rows[x]  # (a view: the steps write the row in place)
        for tau in range(steps):
            lib.fp_scores(row.ctypes.data_as(FC._f), Q.ctypes.data_as(FC._f), k, cand[tau].ctypes.data_as(FC._i), m,
                          sc.ctypes.data_as(FC._f))
            j = int(cand[tau, int(HC.pick(sc[None])[0])])
            margins[o + tau] = lib.fp_step(row.ctypes.data_as(FC._f), Q.ctypes.data_as(FC._f), k, int(pos[tau]), j, lr, lam)
            negs[o + tau] = j
    return rows, margins, negs


def same(got, want, names, what=""):
    """Every array of `got` is `want`'s, byte for byte; the message names the first rows that differ."""
    assert len(got) == len(want) == len(names), what
    for g, w, name in zip(got, want, names):
        assert g.dtype == w.dtype and g.shape == w.shape, (what, name, g.dtype, w.dtype, g.shape, w.shape)
        if g.tobytes() != w.tobytes():
            bits = np.uint64 if g.dtype.itemsize == 8 else np.uint32
            bad = np.flatnonzero((g.view(bits) != w.view(bits)).reshape(g.shape[0], -1).any(axis=1))
            raise AssertionError(f"{what}: {bad.size} {name} differ, first at rows {bad[:5]}: {g[bad[:5]]} instead of {w[bad[:5]]}")
