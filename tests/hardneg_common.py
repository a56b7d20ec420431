"""The pick of mfsgd_sample_unseen_hard (include/mfsgd.h) restated in numpy, on top of tests/implicit_common.sample for the
candidates and a scorer that is passed in: what tests/test_hardneg_cpu.py checks on its own and tests/test_hardneg_gpu.py
compares the device with, byte for byte."""
import numpy as np

from tests import implicit_common as IC

NAN_BITS = 0x7FC00000  # the score of a row whose user has seen everything


def pick(scores):
    """d per row of a float32 table [n, m], m >= 1: the largest non-NaN score, equal scores (-0.0 == +0.0) to the smaller d,
    a NaN loses to every non-NaN, and 0 where the whole row is NaN."""
    s = np.asarray(scores, np.float32)
    nan = np.isnan(s)
    d = np.argmax(np.where(nan, -np.inf, s), axis=1)  # the first of the largest, NaNs standing in as -inf ...
    rows = np.arange(s.shape[0])
    lost = nan[rows, d] & ~nan.all(axis=1)  # ... which a NaN may win only against numbers that are -inf themselves
    d[lost] = np.argmax(~nan[lost], axis=1)
    return d.astype(np.int32)


def hard(lists, n_items, users, m, seed, first, scorer):
    """(items int32[n], scores float32[n], draws int32[n]) that sample_unseen_hard(users, m, seed, first) must return when
    user u's list is lists(u) and scorer(u, i) gives float32 dot(P[u[x]], Q[i[x]]) for int32 arrays u, i."""
    users = np.asarray(users, np.int32)
    n = users.size
    cand = IC.sample(lists, n_items, users, m, seed, first)
    full = cand[:, 0] < 0  # a row is -1 throughout or not at all
    assert ((cand < 0) == full[:, None]).all()
    sc = scorer(np.repeat(users, m), np.where(cand < 0, 0, cand).ravel().astype(np.int32)).reshape(n, m)
    assert sc.dtype == np.float32
    d = pick(sc)
    rows = np.arange(n)
    items, scores = cand[rows, d].copy(), sc[rows, d].copy()
    items[full], d[full] = -1, -1
    scores.view(np.uint32)[full] = NAN_BITS
    return items, scores, d
