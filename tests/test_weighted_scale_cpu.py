"""The planted index of tests/scale_index.py without a device: that it has the shape the device tests rely on, and that
the two-search restatement of the weighted draw (tests/weighted_common.py) is the draw's definition -- enumerate, accumulate,
look up -- on lists of 66 000 entries and a prefix of 70 002, where both searches run to depth 17."""
import numpy as np

from tests import scale_index as SI
from tests import weighted_common as WC


def test_the_planted_index_crosses_every_boundary():
    p = SI.planted()
    w, off = p.w, p.off
    length = np.diff(off)
    assert p.N == off[-1] == p.keys.size and p.eu.size > p.N  # (duplicates among the pairs handed in)
    assert p.N > SI.FIRST_PASS + (1 << 16)  # the second pass of the grid-stride kernels is more than a sliver
    assert SI.I > 1 << 16 and SI.I & (SI.I - 1) != 0
    # the lists
    assert length[SI.WHALE] == SI.WHALE_ITEMS > 1 << 16
    assert length[SI.EVERY] == SI.I
    assert off[SI.EVERY] >= SI.FIRST_PASS  # wholly beyond the first pass
    assert off[SI.WHALE] < SI.FIRST_PASS < off[SI.WHALE + 1]  # ... and the whale's list lies across its end
    assert off[SI.ONE_LEFT + 1] < SI.FIRST_PASS  # the early special users are wholly inside it
    assert (length[SI.EMPTY] == 0).all() and (length[np.setdiff1d(np.arange(SI.U), SI.EMPTY)] > 0).all()
    assert length[0] == 0 and length[SI.U - 1] == 0 and length[1400:1420].sum() == 0  # ties in off: start, middle, end
    assert length[SI.WHALE + 1] == 0  # ... and right behind the longest list
    late = np.flatnonzero((off[:-1] >= SI.FIRST_PASS) & (length > 0))
    assert late.size > 40 and np.isin(SI.EVERY, late) and (late > SI.EVERY).any()  # plain users behind it too
    # the weights
    assert w.dtype == np.uint32 and 0.25 < (w == 0).mean() < 0.4 and 0.01 < (w == SI.BIG).mean() < 0.05
    assert w[0] == 0 and w[-1] == 0 and (w[SI.RUN[0]:SI.RUN[1]] == 0).all() and w[SI.RUN[0] - 1] > 0 and w[SI.RUN[1]] > 0
    beside = p.lists(SI.BESIDE)
    assert np.isin([SI.RUN[0] - 1, SI.RUN[0] + 4, SI.RUN[1]], beside).all()  # seen beside and under the run
    # the masses
    mass = p.row_mass()
    assert mass.max() == p.W > 1 << 40 and (mass[SI.EMPTY] == p.W).all()
    assert mass[SI.EVERY] == 0 and mass[SI.ZERO_LEFT] == 0 and mass[SI.ONE_LEFT] == w[SI.LEFT] == 3
    assert length[SI.ZERO_LEFT] < SI.I and not np.isin(SI.LEFT, p.lists(SI.ONE_LEFT))
    assert 1 << 36 < mass[SI.WHALE] < p.W  # 4 001 unseen items, heavy ones among them
    assert np.median(mass) > 1 << 40  # the plain users: nearly all of W
    C = WC.prefix(w)
    assert int((C[p.lists(SI.WHALE)[1:]] - C[p.lists(SI.WHALE)[:-1]]).max()) > 1 << 32  # prefix differences past 32 bits
    assert int(np.sum(w[p.ki].astype(np.uint64), dtype=np.uint64)) > 1 << 46  # the scan of the pairs' weights is wide
    # the histogram
    counts = np.bincount(p.ki, minlength=SI.I)
    assert counts.sum() == p.N > SI.FIRST_PASS and counts[SI.HOT] > 0.9 * SI.U and counts.min() >= 1


def test_the_two_search_restatement_is_the_definition_at_depth_17():
    p = SI.planted()
    rng = np.random.default_rng(1)
    others = rng.choice(np.setdiff1d(np.arange(SI.U), SI.SPECIAL), 120, replace=False)
    users = np.concatenate([SI.SPECIAL, others, [SI.WHALE, SI.ONE_LEFT]]).astype(np.int32)  # two of them twice
    for m, seed, first in ((1, 0, 0), (5, -5, (1 << 40) + 3)):
        got, mass = SI.sample_enumerated(p, users, m, seed, first)
        want, cnt = WC.sample_weighted(p.lists, p.w, users, m, seed, first, mass=True)
        assert np.array_equal(got, want) and np.array_equal(mass, cnt), m
        assert (got[np.isin(users, (SI.EVERY, SI.ZERO_LEFT))] == -1).all() and (got[users == SI.ONE_LEFT] == SI.LEFT).all()
        rest = ~np.isin(users, (SI.EVERY, SI.ZERO_LEFT))
        assert (got[rest] >= 0).all() and (p.w[got[rest]] > 0).all()
    # the whale at many counters: the draws land all over its 4 001 unseen items, before the first and behind the last
    S = p.lists(SI.WHALE)
    c = np.arange(20000, dtype=np.uint64)
    got, cnt = SI.enumerate_draws(S, p.w, 9, c)
    assert np.array_equal(got, WC.draw_weighted(S, p.w, 9, c)) and cnt == WC.unseen_mass(S, p.w)
    assert not np.isin(got, S).any() and np.unique(got).size > 50
    assert WC.mulhi64(WC.mix64(9, c), cnt).max() > 1 << 36  # ranks that need more than 32 bits
