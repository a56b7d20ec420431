"""Seeded sequences of about forty calls on one live handle, each call compared with the model of tests/handle_model.py
(the oracle and numpy) before the next is made: training in every flavour, lr and lambda changed on schedules the device
packed and on schedules the host packed, before and after the first compute call, rating sets that are kept, rebuilt in
recycled allocations and dropped by a failed call, factors seeded, set, loaded and seeded without Q, the held-out set,
serving and the getters -- for every launch path (flags) and three geometries (the C++ step; solo runs with a lone-tile
mailbox; the padded L = 32).  get_factors is drawn like any other op and never added after one: it synchronises, and would
hide a missing wait.  The last test sums what all cases did and asserts that they did not pass by doing nothing."""
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
    if cfg.get("blocks", 0) > 0:  # the set is there for its lone-tile cells, as in test_lone_tile_mailbox_hand_off
        full = dict(dict(blocks=0, waves=0, lr=0.02, lam=0.03, seed=7), **cfg)
        triples = hm.rating_sets(cfg["U"], cfg["I"])["A"]
        ref = hm.reference_schedule(mf, full, triples, hm._digest(*triples), full["lr"], full["lam"])
        n_lone = int((ref["sched"][0][:, 5] & 1).sum())
        assert n_lone >= cfg["blocks"] and n_lone % cfg["blocks"] == 0, n_lone
    res = hm.run_sequence(mf, oracle, hm.gpu_seed(flag, geometry, seed), hm.GPU_OPS, cfg)
    _results[(flag, geometry, seed)] = res
    print(f"{flag} {geometry} seed {seed}: {res['seconds']:.2f} s, {res['errors']} of {res['n_ops']} ops an error code")


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
    after the first compute call of a schedule, and at most 35 % of all ops ended in an error code."""
    want = len(hm.GPU_FLAGS) * len(hm.GEOMETRIES) * len(hm.GPU_SEEDS)
    assert len(_results) == want, f"{len(_results)} of {want} cases ran before this one: run the whole module"
    total = hm.check_coverage(_results.values())
    slowest = max(_results, key=lambda key: _results[key]["seconds"])
    print(f"{total['ops']} ops, {total['errors']} error codes ({100 * total['errors'] / total['ops']:.1f} %); slowest case "
          f"{slowest}: {_results[slowest]['seconds']:.2f} s")
    print(sorted(total["counts"].items()))
    print(sorted(total["facts"].items()))
