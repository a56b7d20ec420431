"""Pairwise ranking (BPR) on the device (csrc/pairwise.hip, mfsgd_apply_triples): P, Q and the pre-update margins against
the C restatement of the sequential loop (tests/pairwise_common.py), byte for byte, for the lane-group sizes and the level
shapes that reach each launch path; infinite margins and a NaN factor; that a live handle stays whole; fit_bpr against the
sequence of calls it is documented as; and a planted one-class problem that it learns."""
import numpy as np
import pytest

from tests import pairwise_common as pc

pytestmark = pytest.mark.gpu

LR, LAM, SEED = 0.05, 0.01, 4


def _group_lanes(k):
    """L: lanes per triple, the power of two that holds k floats in chunks of four."""
    L = 1
    while 4 * L < k:
        L *= 2
    return L


def _same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if got.tobytes() != want.tobytes():
        bad = np.flatnonzero(got.view(np.uint32).ravel() != want.view(np.uint32).ravel())
        raise AssertionError(f"{what}: {bad.size} words differ, first at {bad[:5]}: "
                             f"{got.ravel()[bad[:5]]} instead of {want.ravel()[bad[:5]]}")


def _check(mf, oracle, U, I, k, u, i, j, after=None):
    """partial_fit_pairwise on a freshly seeded model against the restatement from the same seed; returns the call's
    info.  after(m, P, Q): more checks on the live handle, given the factors the restatement reached."""
    P0, Q0 = oracle.init_factors(U, I, k, SEED)
    P, Q, x = pc.c_pass(P0, Q0, u, i, j, LR, LAM)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as m:
        m.init_factors()
        got_x, info = m.partial_fit_pairwise(u, i, j, margins=True, info=True)
        gP, gQ = m.get_factors()
        _same(gP, P, "P"), _same(gQ, Q, "Q"), _same(got_x, x, "margins")
        if after:
            after(m, P, Q)
    want = pc.py_info(pc.py_levels(u, i, j))
    assert {a: info[a] for a in want} == want
    return info


# ---- 1. every lane-group shape ------------------------------------------------------------------------------------------------
# L = 1; pad columns at L = 2; L = 4 without; L = 8 with a lane of padding only; L = 16; L = 32 (the permlane level of the
# dot) with pad columns and without; one group per wave
@pytest.mark.parametrize("k", (1, 6, 16, 20, 64, 100, 128, 256))
def test_lane_group_sizes(mf, oracle, k):
    U, I, u, i, j = pc.random_batch()

    def then_train(m, P, Q):
        """One epoch over a small rating set on the updated rows: a pad column that stopped being +0.0 shows here."""
        rng = np.random.default_rng(3)
        ru, ri = rng.integers(0, U, 400).astype(np.int32), rng.integers(0, I, 400).astype(np.int32)
        rr = (rng.integers(1, 11, 400) * 0.5).astype(np.float32)
        m.set_ratings(ru, ri, rr)
        m.fit(1, rmse=False)
        oracle.sgd_pass_ordered(P, Q, ru, ri, rr, m.order()[0], LR, LAM)
        gP, gQ = m.get_factors()
        _same(gP, P, "P after fit(1)"), _same(gQ, Q, "Q after fit(1)")

    info = _check(mf, oracle, U, I, k, u, i, j, after=then_train if k in (6, 20, 100) else None)
    assert 1 <= info["launches"] <= info["levels"]


# ---- 2. the level shapes ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", (64, 6, 256, 1))
def test_widths_at_the_boundary_between_narrow_and_wide(mf, oracle, k):
    """Levels of exactly one workgroup pass, one triple more, and one triple, in succession; then every narrow width."""
    G = 256 // _group_lanes(k)
    from tests import online_common as oc

    widths = oc.boundary_widths(G)
    U, I, u, i, j = pc.widths_batch(widths)
    assert list(np.bincount(pc.py_levels(u, i, j))) == widths
    info = _check(mf, oracle, U, I, k, u, i, j)
    assert info["launches"] == 5 and info["max_width"] == G + 1


@pytest.mark.parametrize("k", (64, 6))
@pytest.mark.parametrize("make", (pc.hot_positive_batch, pc.hot_negative_batch, pc.cross_role_batch, pc.one_user_batch),
                         ids=("hot_positive", "hot_negative", "cross_role", "one_user"))
def test_a_chain_is_walked_by_one_workgroup(mf, oracle, make, k):
    U, I, u, i, j = make()
    info = _check(mf, oracle, U, I, k, u, i, j)
    assert info["levels"] == u.size and info["max_width"] == 1 and info["launches"] == 1


@pytest.mark.parametrize("k", (64, 6))
def test_a_hot_positive_inside_a_wide_batch(mf, oracle, k):
    U, I, u, i, j = pc.hot_in_wide_batch()
    info = _check(mf, oracle, U, I, k, u, i, j)
    assert info["levels"] >= 300 and 1 < info["launches"] < info["levels"]


def test_two_pieces(mf, oracle):
    U, I, u, i, j = pc.two_piece_batch(5)
    info = _check(mf, oracle, U, I, 8, u, i, j)
    assert info["pieces"] == 2 and info["n"] == pc.PIECE + 5


# ---- 3. specials ----------------------------------------------------------------------------------------------------------------
def _special_factors(k, rng):
    """8 users, 8 items: the first four triples below have the margins 100, -100, +Inf and -Inf."""
    P = (rng.standard_normal((8, k)) * 0.3).astype(np.float32)
    Q = (rng.standard_normal((8, k)) * 0.3).astype(np.float32)
    P[:4], Q[:6] = 0.0, 0.0
    P[0, 0], Q[0, 0] = 10.0, 10.0      # (0, 0, 1): x = 100 - 0
    P[1, 0], Q[2, 0] = 10.0, 10.0      # (1, 1, 2): x = 0 - 100
    P[2, 0], Q[3, 0] = 3e38, 3e38      # (2, 3, 4): x = +Inf - 0
    P[3, 0], Q[5, 0] = 3e38, 3e38      # (3, 4, 5): x = 0 - Inf
    return P, Q


SPECIAL = (np.array([0, 1, 2, 3], np.int32), np.array([0, 1, 3, 4], np.int32), np.array([1, 2, 4, 5], np.int32))


@pytest.mark.parametrize("k", (6, 9, 64, 65))  # 9 and 65: the last lane of a group (L = 4), the last 15 (L = 32) hold padding only
def test_saturated_and_infinite_margins(mf, k):
    rng = np.random.default_rng(k)
    P0, Q0 = _special_factors(k, rng)
    tail = 200
    u = np.concatenate([SPECIAL[0], rng.integers(0, 8, tail)]).astype(np.int32)
    i = np.concatenate([SPECIAL[1], rng.integers(0, 8, tail)]).astype(np.int32)
    j = np.concatenate([SPECIAL[2], (i[4:] + rng.integers(1, 8, tail)) % 8]).astype(np.int32)
    P, Q, x = pc.c_pass(P0, Q0, u, i, j, LR, LAM)
    assert list(x[:4]) == [100.0, -100.0, np.inf, -np.inf]
    with mf.MatrixFactorizationSGD(8, 8, k, LR, LAM, SEED) as m:
        m.set_factors(P0, Q0)
        got = m.partial_fit_pairwise(u[:4], i[:4], j[:4], margins=True)  # the four on their own: no NaN anywhere
        P4, Q4, x4 = pc.c_pass(P0, Q0, u[:4], i[:4], j[:4], LR, LAM)
        gP, gQ = m.get_factors()
        assert not np.isnan(P4).any() and not np.isnan(Q4).any()
        _same(got, x4, "margins"), _same(gP, P4, "P"), _same(gQ, Q4, "Q")
        m.set_factors(P0, Q0)
        got = m.partial_fit_pairwise(u, i, j, margins=True)  # ... and with what follows from them (Inf - Inf is NaN)
        gP, gQ = m.get_factors()
    for g, w, what in ((got, x, "margins"), (gP, P, "P"), (gQ, Q, "Q")):
        assert np.array_equal(np.isnan(g), np.isnan(w)), what
        assert np.array_equal(g.view(np.uint32)[~np.isnan(w)], w.view(np.uint32)[~np.isnan(w)]), what


def _nan_alike(got, want, what):
    """NaN payloads and signs are not part of the contract: which entries are NaN is, and every other bit."""
    assert got.dtype == want.dtype and got.shape == want.shape, what
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    assert np.array_equal(got.view(np.uint32)[~np.isnan(want)], want.view(np.uint32)[~np.isnan(want)]), what


@pytest.mark.parametrize("k", (6, 9, 64, 65))  # 9 and 65: lanes that hold padding only (L = 4, L = 32)
def test_a_nan_factor(mf, oracle, k):
    """NaN payloads and signs are not part of the contract: which entries are NaN is, and every other bit.  After the
    batch with the NaN steps a second one goes over the three rows of a NaN step and over rows still finite, and every
    pair is predicted, against the sequential loop: the state after a NaN step goes on working.  (A NaN step makes every
    real column of its rows NaN, so this cannot tell whether a pad column took the NaN too; the infinite steps of
    tests/test_warp_gpu.py can.)"""
    U, I, u, i, j = pc.random_batch(n=80)
    P0, Q0 = oracle.init_factors(U, I, k, SEED)
    P0[5, k // 2], Q0[7, 0] = np.nan, np.nan
    P, Q, x = pc.c_pass(P0, Q0, u, i, j, LR, LAM)
    assert np.isnan(x).any() and not np.isnan(x).all() and not np.isnan(P).all()
    # The second batch, in this order:
    #   three finite steps: users still finite, all on the two items still finite (the batch left no more than a few);
    #   the triple t of a NaN step once more: its three rows are NaN already;
    #   `again`: those of the batch's first 20 triples that name neither finite item, so more NaN steps, which leave the
    #   two finite items finite and the last predict with numbers to compare.
    t = int(np.flatnonzero(np.isnan(x))[0])
    assert np.isnan(P[u[t]]).all() and np.isnan(Q[i[t]]).all() and np.isnan(Q[j[t]]).all()
    fu, fi = np.flatnonzero(~np.isnan(P).any(axis=1)), np.flatnonzero(~np.isnan(Q).any(axis=1))
    assert fu.size >= 3 and fi.size >= 2
    again = np.flatnonzero(~np.isin(i[:20], fi) & ~np.isin(j[:20], fi))
    assert again.size >= 10
    u2 = np.concatenate([fu[:3], [u[t]], u[again]]).astype(np.int32)
    i2 = np.concatenate([np.full(3, fi[0]), [i[t]], i[again]]).astype(np.int32)
    j2 = np.concatenate([np.full(3, fi[1]), [j[t]], j[again]]).astype(np.int32)
    P2, Q2, x2 = pc.c_pass(P, Q, u2, i2, j2, LR, LAM)
    assert np.isnan(x2[3]) and not np.isnan(x2[:3]).any()
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as m:
        m.set_factors(P0, Q0)
        got = m.partial_fit_pairwise(u, i, j, margins=True)
        gP, gQ = m.get_factors()
        pu, pi = np.repeat(np.arange(U, dtype=np.int32), I), np.tile(np.arange(I, dtype=np.int32), U)
        pred = m.predict(pu, pi)  # the pad columns stayed +0.0: a row without a NaN column has finite dots
        got2 = m.partial_fit_pairwise(u2, i2, j2, margins=True)
        gP2, gQ2 = m.get_factors()
        pred2 = m.predict(pu, pi)
    for g, w, what in ((got, x, "margins"), (gP, P, "P"), (gQ, Q, "Q"), (pred, oracle.predict(P, Q, pu, pi), "predict"),
                       (got2, x2, "margins of the second batch"), (gP2, P2, "P after it"), (gQ2, Q2, "Q after it"),
                       (pred2, oracle.predict(P2, Q2, pu, pi), "predict after it")):
        _nan_alike(g, w, what)
    assert not np.isnan(pred2).all() and np.isnan(pred2).any()


# ---- 4. a live handle stays whole -----------------------------------------------------------------------------------------------
def test_side_effects(mf, oracle):
    U, I, u, i, j = pc.random_batch()
    k = 16
    rng = np.random.default_rng(8)
    ru, ri = rng.integers(0, U, 900).astype(np.int32), rng.integers(0, I, 900).astype(np.int32)
    rr = (rng.integers(1, 11, 900) * 0.5).astype(np.float32)
    start = mf.debug_device_bytes()
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as m:
        m.reserve(items=I + 8)
        m.init_factors()
        m.set_ratings(ru, ri, rr)
        m.set_seen(ru, ri)
        m.fit(1, rmse=False)
        seen, order = m.seen_size(), m.order()[0]
        first = m.rmse()
        bytes_before, counters = mf.debug_device_bytes(), m.debug_counters()
        assert bytes_before > start
        P0, Q0 = m.get_factors()
        m.partial_fit_pairwise(u, i, j)
        assert mf.debug_device_bytes() == bytes_before
        x = m.partial_fit_pairwise(u, i, j, margins=True)
        assert mf.debug_device_bytes() == bytes_before
        with pytest.raises(mf.MfsgdError) as e:
            m.partial_fit_pairwise([0, U], [0, 0], [1, 1])
        assert e.value.code == -1 and mf.debug_device_bytes() == bytes_before
        assert m.debug_counters() == counters  # schedule builds, cached graphs, the launch path
        assert m.seen_size() == seen and np.array_equal(m.order()[0], order)
        P1, Q1, _ = pc.c_pass(P0, Q0, u, i, j, LR, LAM)
        P, Q, want_x = pc.c_pass(P1, Q1, u, i, j, LR, LAM)
        gP, gQ = m.get_factors()
        _same(gP, P, "P"), _same(gQ, Q, "Q"), _same(x, want_x, "margins")
        assert np.isfinite(m.rmse()) and m.rmse() != first  # the stored set is still there, and sees the updated rows
        m.set_ratings(ru, ri, rr)  # the same triples are still recognised
        assert m.debug_counters()["schedule_builds"] == counters["schedule_builds"] == 1
        # new items inside the reserved capacity: valid as i and as j at once
        with pytest.raises(mf.MfsgdError):
            m.partial_fit_pairwise([0], [I], [0])
        m.add_items(n=4, seed=99)
        P0, Q0 = m.get_factors()
        assert Q0.shape[0] == I + 4
        nu = np.array([1, 2, 1, 3], np.int32)
        ni = np.array([I, 0, I + 3, I + 2], np.int32)
        nj = np.array([3, I + 1, I, I + 3], np.int32)
        levels, _ = m.triple_levels(nu, ni, nj)
        assert np.array_equal(levels, pc.py_levels(nu, ni, nj))
        x = m.partial_fit_pairwise(nu, ni, nj, margins=True)
        P, Q, want_x = pc.c_pass(P0, Q0, nu, ni, nj, LR, LAM)
        gP, gQ = m.get_factors()
        _same(gP, P, "P"), _same(gQ, Q, "Q"), _same(x, want_x, "margins")
    assert mf.debug_device_bytes() == start


def test_the_current_hyper_parameters_are_used(mf, oracle):
    U, I, u, i, j = pc.random_batch()
    k, lr2, lam2 = 16, 0.03, 0.002
    P0, Q0 = oracle.init_factors(U, I, k, SEED)
    P, Q, x = pc.c_pass(P0, Q0, u, i, j, float(np.float32(lr2)), float(np.float32(lam2)))
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED) as m:
        m.init_factors()
        m.set_hyper(lr2, lam2)
        got = m.partial_fit_pairwise(u, i, j, margins=True)
        gP, gQ = m.get_factors()
    _same(gP, P, "P"), _same(gQ, Q, "Q"), _same(got, x, "margins")


# ---- 5. fit_bpr is the sequence it is documented as -----------------------------------------------------------------------------
def _bits(m):
    P, Q = m.get_factors()
    return P.tobytes(), Q.tobytes()


@pytest.mark.parametrize("held", (False, True))
def test_fit_bpr_is_its_documented_sequence(mf, held):
    U, I, k, epochs, seed, full = 60, 50, 8, 3, 21, 17
    rng = np.random.default_rng(5)
    pu, pi = rng.integers(0, U, 400).astype(np.int32), rng.integers(0, I, 400).astype(np.int32)  # duplicates among them
    pu, pi = np.concatenate([pu, np.full(I, full)]).astype(np.int32), np.concatenate([pi, np.arange(I)]).astype(np.int32)
    order = rng.permutation(pu.size)
    pu, pi = pu[order], pi[order]
    n = pu.size
    hu, hi = rng.integers(0, U, 200).astype(np.int32), rng.integers(0, I, 200).astype(np.int32)
    fresh = ~np.isin((hu.astype(np.int64) << 32) | hi, (pu.astype(np.int64) << 32) | pi)
    hu, hi = hu[fresh], hi[fresh]
    new = lambda: mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED)
    with new() as a, new() as b, new() as c:
        if held:  # the index also holds the held-out pairs: every handle gets it first
            for h in (a, b, c):
                h.set_seen(np.concatenate([pu, hu]), np.concatenate([pi, hi]))
            size = a.seen_size()
        stats = a.fit_bpr(pu, pi, epochs, seed=seed)
        assert sorted(stats) == ["auc", "loss"] and all(v.shape == (epochs,) and v.dtype == np.float64 for v in stats.values())
        assert a.debug_counters()["schedule_builds"] == 0  # no rating set was made
        if held:
            assert a.seen_size() == size
        else:  # a handle without an index got one: the distinct positives
            assert a.seen_size() == np.unique((pu.astype(np.int64) << 32) | pi).size
            b.set_seen(pu, pi)
        # the same steps written out
        b.init_factors()
        for e in range(epochs):
            J = b.sample_unseen(pu, 1, seed, first=e * n)[:, 0]
            assert (J[pu == full] == -1).all() and (J[pu != full] >= 0).all()
            if held:
                assert not np.isin((pu.astype(np.int64) << 32) | J, (hu.astype(np.int64) << 32) | hi).any()
            keep = J >= 0
            x = b.partial_fit_pairwise(pu[keep], pi[keep], J[keep], margins=True).astype(np.float64)
            assert x.size == n - (pu == full).sum()
            np.testing.assert_allclose(stats["loss"][e], np.log1p(np.exp(-x)).mean(), rtol=1e-12)
            assert stats["auc"][e] == (x > 0).mean()
        assert _bits(a) == _bits(b)
        # two epochs and then the third: the same bits
        first = c.fit_bpr(pu, pi, 2, seed=seed)
        last = c.fit_bpr(pu, pi, 1, seed=seed, first_epoch=2)
        for name in ("loss", "auc"):
            assert np.concatenate([first[name], last[name]]).tobytes() == stats[name].tobytes()
        assert _bits(a) == _bits(c)
        assert c.fit_bpr(pu, pi, 1, seed=seed, first_epoch=3, stats=False) is None
        assert c.fit_bpr(pu, pi, 0, seed=seed)["loss"].shape == (0,)


# ---- 6. it learns ---------------------------------------------------------------------------------------------------------------
def test_bpr_learns_a_planted_one_class_problem(mf):
    """The planted problem of tests/test_implicit_gpu.py: 600 users, 400 items in 20 groups of 20; a user's 12 positives
    lie in the user's group, 11 to train on and 1 held out (and kept in the seen-item index, so never drawn); k = 16,
    lambda = 0.01, lr = 0.05, 20 epochs of fit_bpr on the positives in the order given.  A plain sequential BPR in numpy
    with uniform unseen negatives on exactly this data had a held-out hit rate at 10 of 0.045 untrained and 1.0 after 20
    epochs (at lr 0.05 and 0.1, shuffled and not).  The library's draws differ, so the bounds are wide, as in the
    implicit test: untrained below 0.1, trained above 0.5.
    Measured on an MI355X: untrained 0.02, after fit_bpr 1.0 (mean loss 0.695 in the first epoch, 0.067 in the last)."""
    U, I, G, k, lr, lam, seed = 600, 400, 20, 16, 0.05, 0.01, 3
    rng = np.random.default_rng(0)
    per = I // G
    its = np.stack([(u % G) * per + rng.choice(per, 12, replace=False) for u in range(U)]).astype(np.int32)
    hu, hi = np.arange(U, dtype=np.int32), its[:, 0].copy()
    pu, pi = np.repeat(hu, 11), its[:, 1:].ravel().copy()
    with mf.MatrixFactorizationSGD(U, I, k, lr, lam, seed) as h:
        h.set_seen(np.concatenate([pu, hu]), np.concatenate([pi, hi]))  # held-out positives are never negatives
        h.init_factors()
        untrained = h.evaluate_ranking(hu, hi, 10, exclude="seen")["hit_rate"]
        stats = h.fit_bpr(pu, pi, 20, seed=seed)
        trained = h.evaluate_ranking(hu, hi, 10, exclude="seen")["hit_rate"]
    print("held-out hit rate at 10: untrained", round(untrained, 4), "after fit_bpr", round(trained, 4))
    print("loss per epoch:", np.round(stats["loss"], 4).tolist(), "auc:", np.round(stats["auc"], 4).tolist())
    assert untrained < 0.1
    assert trained > 0.5
    assert stats["loss"][-1] < stats["loss"][0] and stats["auc"][-1] > stats["auc"][0]
