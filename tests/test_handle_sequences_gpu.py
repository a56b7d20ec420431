"""Seeded sequences of about seventy calls on one live handle, each call compared with the model of tests/handle_model.py
(the oracle and numpy) before the next is made: training in every flavour, lr and lambda changed on schedules the device
packed and on schedules the host packed, before and after the first compute call, rating sets that are kept, rebuilt in
recycled allocations and dropped by a failed call, factors seeded, set, loaded and seeded without Q, users and items
appended in place and by reallocation, room reserved, online updates, fold-in of users and of items with the rows
appended, top-N among candidates, the held-out set, the seen-item index (set, merged, cleared, read back after every
call that must leave it alone or move its tables, served from with exclude="seen"), serving and the getters -- for every
launch path (flags) and four
geometries (the C++ step; solo runs with a lone-tile mailbox; the padded L = 32; exchanged roles, where the hot row is a
user's and the kernels receive (Q, P)).  get_factors is drawn like any other op and never added after one: it
synchronises, and would hide a missing wait (the one exception reads back an appended NaN).  One scripted life per launch
path reaches the deep combinations whatever the draw does.  The last test sums what all cases did and asserts that they
did not pass by doing nothing."""
import time

import numpy as np
import pytest

from tests import handle_model as hm

pytestmark = pytest.mark.gpu

_results = {}


@pytest.mark.parametrize("seed", hm.GPU_SEEDS)
@pytest.mark.parametrize("geometry", sorted(hm.GEOMETRIES))
@pytest.mark.parametrize("flag", hm.GPU_FLAGS)
def test_sequence(mf, oracle, flag, geometry, seed):
    cfg = hm.gpu_config(flag, geometry)
    _geometry_is_what_it_is_for(mf, cfg)
    res = hm.run_sequence(mf, oracle, hm.gpu_seed(flag, geometry, seed), hm.GPU_OPS, cfg)
    _results[(flag, geometry, seed)] = res
    print(f"{flag} {geometry} seed {seed}: {res['seconds']:.2f} s, {res['errors']} of {res['n_ops']} ops an error code")


def _geometry_is_what_it_is_for(mf, cfg):
    """The set is there for its lone-tile cells, as in test_lone_tile_mailbox_hand_off, and, with the roles exchanged,
    for a schedule that hands the training kernels (Q, P)."""
    if cfg.get("blocks", 0) > 0:
        full = dict(dict(blocks=0, waves=0, lr=0.02, lam=0.03, seed=7), **cfg)
        triples = hm.rating_sets(cfg["U"], cfg["I"], bool(cfg.get("swap_roles")))["A"]
        ref = hm.reference_schedule(mf, full, triples, hm._digest(*triples), full["lr"], full["lam"])
        n_lone = int((ref["sched"][0][:, 5] & 1).sum())
        assert n_lone >= cfg["blocks"] and n_lone % cfg["blocks"] == 0, n_lone
        assert ref["info"]["swapped"] == (1 if cfg.get("swap_roles") else 0), ref["info"]


# early stopping: the held-out RMSE falls by 0.1 to 0.2 an epoch, less than min_delta, so only epoch 0 counts as an
# improvement, two bad epochs end the call, and the snapshot of epoch 0 comes back; the rate changes on the way
LIFE_LR, LIFE_MIN_DELTA = (0.011, 0.011, 0.03, 0.03, 0.03, 0.03), 0.5


@pytest.mark.parametrize("geometry", ["k64_b16_w2", "k100_b12_w2", "k64_b12_w2_hot_user"])
@pytest.mark.parametrize("flag", ["default", "FLAG_ROUND_LAUNCH", "FLAG_NO_GRAPH", "FLAG_DEVICE_INGEST"])
def test_a_grown_model_through_a_whole_life(mf, oracle, flag, geometry):
    """The deep combinations, scripted: fit; reserve; users appended in place; an online batch with the hot row 200 times
    and the new user; fit over the kept schedule and graph; items appended beyond the capacity (Q moves); other values
    re-baked into the kept schedule; fit; a rating set that names the appended rows, built at the grown sizes; a held-out
    set with pairs on appended rows; early stopping that restores a snapshot of the grown model.  The factors are the
    oracle's bit for bit over the exported orders, and the cached graphs and the schedule builds are counted at every step.
    The seen-item index goes along: set from the ratings before the growth (no graph goes), the appended users and items
    marked after it, read back whole at the end, and the three serving calls with exclude="seen" answered for the grown,
    restored model by the oracle."""
    cfg = dict(dict(blocks=0, waves=0, lr=0.02, lam=0.03, seed=7), **hm.gpu_config(flag, geometry))
    _geometry_is_what_it_is_for(mf, cfg)
    U, I, k, swap = cfg["U"], cfg["I"], cfg["k"], bool(cfg.get("swap_roles"))
    one = 0 if flag == "FLAG_NO_GRAPH" else 1  # graphs cached behind an epoch
    rng = np.random.default_rng(5)
    A = hm.rating_sets(U, I, swap)["A"]
    order_a = hm.reference_order(mf, oracle, cfg, A, hm._digest(*A))[0]
    new_p = (rng.standard_normal((4, k)) * 0.1).astype(np.float32)
    new_q = (rng.standard_normal((25, k)) * 0.1).astype(np.float32)
    U1, I1 = U + 7, I + 25
    # the online batch: the hot row 200 times, the new user on the hot row and elsewhere, one pair twice
    other = rng.integers(0, I if swap else U, 200).astype(np.int32)
    hot = np.full(200, hm.HOT, np.int32)
    bu, bi = (hot, other) if swap else (other, hot)
    bu = np.concatenate([bu, [U, U, U + 3, U]]).astype(np.int32)
    bi = np.concatenate([bi, [hm.HOT, 3, 4, 3]]).astype(np.int32)
    br = (rng.integers(1, 11, bu.size) * 0.5).astype(np.float32)
    C = hm.grown_set(rng, A, U, I, U1, I1)
    grown = dict(cfg, U=U1, I=I1)  # (the reference handle of set C has the grown sizes)
    order_c = hm.reference_order(mf, oracle, grown, C, hm._digest(*C))[0]
    assert hm.reference_schedule(mf, grown, C, hm._digest(*C), cfg["lr"], cfg["lam"])["info"]["swapped"] == (1 if swap else 0)
    vu, vi = rng.integers(0, U1, 300).astype(np.int32), rng.integers(0, I1, 300).astype(np.int32)
    vu[::5], vi[2::5] = rng.integers(U, U1, 60), rng.integers(I, I1, 60)
    vr = (rng.integers(1, 11, 300) * 0.5).astype(np.float32)
    lrs = np.array(LIFE_LR, np.float32)
    # the index: the ratings before the growth; after it pairs of appended users and of appended items, one pair twice
    mu = np.concatenate([rng.integers(U, U1, 40), rng.integers(0, U1, 40), [U, U]]).astype(np.int32)
    mi = np.concatenate([rng.integers(0, I1, 40), rng.integers(I, I1, 40), [I1 - 1, I1 - 1]]).astype(np.int32)
    su, si = np.concatenate([A[0], mu]), np.concatenate([A[1], mi])
    users = np.array([0, U, U1 - 1, hm.HOT, U], np.int32)       # old and appended users, one twice
    hu = np.concatenate([mu[:6], A[0][:6], [U1 - 1, 3]]).astype(np.int32)  # held-out pairs, some of them seen
    hi = np.concatenate([mi[:6], A[1][:6], [I1 - 1, I]]).astype(np.int32)
    t0 = time.perf_counter()
    with mf.MatrixFactorizationSGD(U, I, k, cfg["lr"], cfg["lam"], 7, blocks=cfg["blocks"], waves=cfg["waves"], flags=cfg["flags"]) as m:
        def counters(graphs, builds, what):
            got = m.debug_counters()
            assert (got["graphs"], got["schedule_builds"]) == (graphs, builds), (what, got)

        m.set_ratings(*A)
        m.init_factors()
        m.fit(2, rmse=False)
        counters(one, 1, "fit")
        m.set_seen(A[0], A[1])                        # the index and the model do not touch each other
        counters(one, 1, "set_seen")
        m.reserve(users=U + 10)                       # P moves: the graph holds its old address
        counters(0, 1, "reserve")
        assert m.capacity() == (U + 10, I)
        assert m.add_users(new_p) == U                # in place
        counters(0, 1, "add_users")
        err = m.partial_fit(bu, bi, br, errors=True)
        counters(0, 1, "partial_fit")
        rm5 = m.fit(1)
        counters(one, 1, "fit behind the online batch")
        assert m.add_users(n=3, seed=11) == U + 4     # in place again, with a graph cached this time: it stays
        counters(one, 1, "add_users with a graph cached")
        assert m.capacity() == (U + 10, I)
        assert m.add_items(new_q) == I                # beyond the capacity: Q moves
        counters(0, 1, "add_items")
        assert m.capacity() == (U + 10, I1) and (m.users, m.items) == (U1, I1)
        m.mark_seen(mu, mi)                           # the appended rows are valid, and their lists start empty
        counters(0, 1, "mark_seen")
        m.set_hyper(0.011, 0.02)                      # re-baked into the kept schedule
        counters(0, 1, "set_hyper")
        rm8 = m.fit(1)
        counters(one, 1, "fit at the other values")
        m.set_ratings(*C)
        counters(0, 2, "set C")
        m.set_validation(vu, vi, vr)
        res = m.fit_early_stopping(len(lrs), patience=2, min_delta=LIFE_MIN_DELTA, restore_best=True, lr=lrs)
        counters(one, 2, "early stopping")
        got = m.get_factors()
        order_kept = m.order()[0]
        unseen = (m.recommend(users, 6, exclude="seen"), m.rank_items(hu, hi, exclude="seen"),
                  m.evaluate_ranking(hu, hi, 5, exclude="seen"))
        counters(one, 2, "the calls against the index")
        index = m.seen(np.arange(U1, dtype=np.int32))
        assert m.seen_size() == index[1].size
    seconds = time.perf_counter() - t0
    P, Q = oracle.init_factors(U, I, k, 7)
    lr, lam = cfg["lr"], cfg["lam"]
    for _ in range(2):
        oracle.sgd_pass_ordered(P, Q, *A, order_a, lr, lam)
    P = np.vstack([P, new_p])
    want = np.array([oracle.sgd_update(P[a], Q[b], float(c), lr, lam) for a, b, c in zip(bu, bi, br)], np.float32)
    hm._same_bits(err, want, "errors of the online batch")
    oracle.sgd_pass_ordered(P, Q, *A, order_a, lr, lam)
    np.testing.assert_allclose(rm5, [oracle.rmse(P, Q, *A)], rtol=hm.RTOL, atol=hm.ATOL)
    P = np.vstack([P, oracle.init_factors(3, 0, k, 11)[0]])
    Q = np.vstack([Q, new_q])
    lr, lam = float(np.float32(0.011)), float(np.float32(0.02))
    oracle.sgd_pass_ordered(P, Q, *A, order_a, lr, lam)
    np.testing.assert_allclose(rm8, [oracle.rmse(P, Q, *A)], rtol=hm.RTOL, atol=hm.ATOL)
    assert np.array_equal(order_kept, order_c)
    ran, best = res["epochs_run"], res["best_epoch"]
    moved = (P[U:].copy(), Q[I:].copy())
    for e in range(ran):
        oracle.sgd_pass_ordered(P, Q, *C, order_c, float(lrs[e]), lam)
        np.testing.assert_allclose(res["val_rmse"][e], oracle.rmse(P, Q, vu, vi, vr), rtol=hm.RTOL, atol=hm.ATOL)
        if e == best:
            best_p, best_q = P.copy(), Q.copy()
    print(f"{flag} {geometry}: {seconds:.2f} s; early stopping ran {ran} epochs, best {best}, held-out RMSE {res['val_rmse']}")
    assert (ran, best) == (3, 0), res                 # the rule of the header: the snapshot of epoch 0 was restored
    hm._same_bits(got[0], best_p, "P")
    hm._same_bits(got[1], best_q, "Q")
    assert not np.array_equal(best_p[U:], moved[0]) and not np.array_equal(best_q[I:], moved[1])  # set C trained the new rows
    # the index kept every list through reserve, both appends, two rating sets and the training, and serves the final model
    keys = np.unique((su.astype(np.int64) << 32) | si)
    assert np.array_equal(index[0], np.searchsorted(keys >> 32, np.arange(U1 + 1))), "the index's offsets"
    assert np.array_equal(index[1], (keys & 0xFFFFFFFF).astype(np.int32)), "the index's items"
    assert (np.diff(index[0])[U:] > 0).any()  # (appended users have lists of their own by now)
    hm.same_topn(unseen[0], hm.recommend_ref(oracle, best_p, best_q, users, 6, su, si))
    ranks = hm.ranks_ref(oracle, best_p, best_q, hu, hi, su, si)
    assert np.array_equal(unseen[1], ranks) and np.array_equal(unseen[2]["ranks"], ranks), (unseen[1], ranks)
    assert not np.array_equal(ranks, hm.ranks_ref(oracle, best_p, best_q, hu, hi, su[:0], si[:0]))  # (the index matters)
    hm.same_metrics(unseen[2], hm.metrics_ref(hu, ranks, 5))


def test_fallback_to_round_launches_in_the_middle_of_a_life(mf, oracle):
    """fit; a persistent launch that finds itself not resident (test_persistent_kernel_not_resident_falls_back_to_round_
    launches) and is made up for by round launches; other values; another rating set (a new partition, probed again):
    the factors are the oracle's bit for bit all the way."""
    U, I, k, lr, lam, seed, blocks = 2000, 1500, 64, 0.02, 0.03, 7, 64  # the shape at which that test's launch is not resident
    cfg = dict(U=U, I=I, k=k, blocks=blocks, waves=2, flags=0, lr=lr, lam=lam, seed=seed)
    rng = np.random.default_rng(88)
    key = rng.choice(U * I, 120000 + 60001, replace=False)
    u, i, r = (key // I).astype(np.int32), (key % I).astype(np.int32), (rng.random(key.size) * 4 + 1).astype(np.float32)
    A, B = (u[:120000], i[:120000], r[:120000]), (u[120000:], i[120000:], r[120000:])
    order_a = hm.reference_order(mf, oracle, cfg, A, hm._digest(*A))[0]
    order_b = hm.reference_order(mf, oracle, cfg, B, hm._digest(*B))[0]
    P, Q = oracle.init_factors(U, I, k, seed)
    with mf.MatrixFactorizationSGD(U, I, k, lr, lam, seed, blocks=blocks, waves=2) as m:
        m.set_ratings(*A)
        m.init_factors()
        m.fit(1, rmse=False)
        persistent = m.debug_counters()["persistent_parts"] == 1
        m.debug_occupy(600)
        m.fit(2, rmse=False)
        after_occupy = m.debug_counters()
        m.set_hyper(0.011, 0.0)
        rm = m.fit(1)
        m.set_ratings(*B)
        rm_b = m.fit(1)
        after_b = m.debug_counters()
        got = m.get_factors()
    for _ in range(3):
        oracle.sgd_pass_ordered(P, Q, *A, order_a, lr, lam)
    oracle.sgd_pass_ordered(P, Q, *A, order_a, float(np.float32(0.011)), 0.0)
    np.testing.assert_allclose(rm, [oracle.rmse(P, Q, *A)], rtol=hm.RTOL, atol=hm.ATOL)
    oracle.sgd_pass_ordered(P, Q, *B, order_b, float(np.float32(0.011)), 0.0)
    np.testing.assert_allclose(rm_b, [oracle.rmse(P, Q, *B)], rtol=hm.RTOL, atol=hm.ATOL)
    hm._same_bits(got[0], P, "P")
    hm._same_bits(got[1], Q, "Q")
    print(f"persistent kernel in use: {persistent}; counters after the occupied launch {after_occupy}, after set B {after_b}")
    if persistent:  # (a box on which the persistent kernel is never used has only the factors to show)
        assert after_occupy["not_resident"] >= 1 and after_occupy["persistent_parts"] == 0, after_occupy
        assert after_b["persistent_parts"] == 1, after_b


def test_the_sequences_together_covered_what_they_are_for():
    """Over all cases: every op kind succeeded at least ten times, every error the model can answer with occurred, rating
    sets were kept and rebuilt at equal length, lr and lambda changed on a device-packed schedule before and after its
    first compute call and on a host-packed one, a lone-tile schedule was trained, the schedule getters ran before and
    after the first compute call of a schedule, every fact of growth and online updates (handle_model.GROWTH_FACTS) and
    of the seen-item index (handle_model.SEEN_FACTS) happened, and at most 35 % of all ops ended in an error code."""
    want = len(hm.GPU_FLAGS) * len(hm.GEOMETRIES) * len(hm.GPU_SEEDS)
    assert len(_results) == want, f"{len(_results)} of {want} cases ran before this one: run the whole module"
    total = hm.check_coverage(_results.values())
    slowest = max(_results, key=lambda key: _results[key]["seconds"])
    print(f"{total['ops']} ops, {total['errors']} error codes ({100 * total['errors'] / total['ops']:.1f} %); slowest case "
          f"{slowest}: {_results[slowest]['seconds']:.2f} s")
    print(sorted(total["counts"].items()))
    print(sorted(total["facts"].items()))
