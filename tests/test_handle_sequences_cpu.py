"""Seeded sequences of calls on one live handle against the model of tests/handle_model.py, as far as they go without a
GPU: ratings (kept, rebuilt, dropped by a failed call), lr and lambda re-baked into a schedule any number of times, factors
seeded on the host, set, saved, loaded and seeded without Q, rows appended to the host staging, room reserved, empty
batches of online updates, the held-out set, the seen-item index as far as the host keeps it (an empty index, seen_size,
get_seen of an empty index or of no users, "no seen set" in front of every other state error, a refused set_seen /
mark_seen) and every getter, each compared with the model after the call; the calls
that need a device are MFSGD_ERR_NO_DEVICE and change nothing.  (On a machine that has a
GPU the same sequences run with it, and the few compute calls they draw are compared with the oracle.)
Also here: the driver's self-test (a model with one rule wrong must be reported), and the dry run of the GPU module's
cases, which shows that the op weights meet that module's coverage conditions by the model alone."""
import numpy as np
import pytest

from tests import handle_model as hm
from tests.conftest import have_gpu

HOST_SEEDS = range(20)
HOST_OPS = 40
HOST_SHAPE = dict(U=120, I=40, profile="host")


def _config(k, flag):
    return dict(HOST_SHAPE, k=k, flags=hm.flag_value(flag))


@pytest.mark.parametrize("flag", ["default", "FLAG_HOST_INGEST"])
@pytest.mark.parametrize("k", [5, 64])
def test_host_sequences(mf, oracle, k, flag):
    counts, facts = {}, {}
    for seed in HOST_SEEDS:
        seed += 100 * k + (50 if flag == "default" else 0)  # other sequences for every configuration
        res = hm.run_sequence(mf, oracle, seed, HOST_OPS, _config(k, flag), device=have_gpu())
        for key, n in res["counts"].items():
            counts[key] = counts.get(key, 0) + n
        for key, n in res["facts"].items():
            facts[key] = facts.get(key, 0) + n
    print(f"k={k} {flag}: {sorted(counts.items())}\n{sorted(facts.items())}")
    # what the host path is there to cover has happened, successfully, in these twenty lives
    for kind in ("set_ratings", "set_hyper", "set_factors", "init_factors", "init_p_offset", "get_factors", "set_validation",
                 "clear_validation", "save_load", "order", "debug_schedule", "schedule_info", "hyper", "debug_counters",
                 "add_users", "add_items", "reserve", "set_seen", "mark_seen", "clear_seen", "seen_size"):
        assert counts.get((kind, "ok"), 0) >= 5, (kind, counts)
    assert facts.get("partial_fit_of_no_ratings", 0) >= 5, facts  # (n = 0 needs no device)
    assert counts.get(("set_ratings", "INVALID_ARG"), 0) >= 1
    for fact in ("set_ratings_reuse", "set_ratings_rebuild_of_equal_length", "set_ratings_build_of_the_set_a_failed_call_dropped",
                 "set_hyper_before_any_ratings", "set_hyper_on_a_host_packed_schedule", "set_hyper_same_bits",
                 "set_ratings_reuse_after_growth", "init_factors_after_growth", "stale_factor_file_refused"):
        assert facts.get(fact, 0) >= 1, (fact, facts)
    # the index on the host: refused for a bad pair, empty, read back on the host, and "no seen set" before the factors
    for kind in ("set_seen", "mark_seen"):
        assert counts.get((kind, "INVALID_ARG"), 0) >= 1, (kind, counts)
    for kind in ("get_seen", "recommend_unseen", "rank_unseen", "evaluate_unseen"):
        assert counts.get((kind, "STATE"), 0) >= 1, (kind, counts)
    for fact in ("set_seen_of_no_pairs", "mark_seen_of_no_pairs", "get_seen_answered_on_the_host",
                 "unseen_refused_for_no_seen_set_without_factors"):
        assert facts.get(fact, 0) >= 1, (fact, facts)
    if not have_gpu():
        assert any(outcome == "NO_DEVICE" for _, outcome in counts), "no call that needs a device was drawn"
        for kind in ("set_seen", "mark_seen", "recommend_unseen"):  # (pairs, or an empty index and factors, but no device)
            assert counts.get((kind, "NO_DEVICE"), 0) >= 1, (kind, counts)
        assert mf.debug_device_bytes() == 0


def test_schedule_after_many_changes_of_values_is_the_fresh_one(mf):
    """debug_schedule() after any number of set_hyper calls equals a fresh handle's at the final values (the sequences
    draw this too; here it is the whole test)."""
    cfg = dict(_config(64, "default"), blocks=0, waves=0, seed=7, lr=0.02, lam=0.03)
    triples = hm.rating_sets(cfg["U"], cfg["I"])["A"]
    rng = np.random.default_rng(5)
    with mf.MatrixFactorizationSGD(cfg["U"], cfg["I"], 64, 0.02, 0.03, 7) as m:
        m.set_ratings(*triples)
        for n in (1, 2, 5):
            for _ in range(n):
                lr, lam = np.float32(rng.uniform(0.001, 0.05)), np.float32(rng.uniform(0, 0.1) * rng.integers(2))
                m.set_hyper(lr, lam)
            want = hm.reference_schedule(mf, cfg, triples, hm._digest(*triples), lr, lam)
            info = m.schedule_info()
            info.pop("build_seconds")
            assert info == want["info"]
            for x, y in zip(m.debug_schedule(), want["sched"]):
                assert np.array_equal(x, y)


def _caught(mf, oracle, wrong):
    caught = []
    for seed in HOST_SEEDS:
        try:
            hm.run_sequence(mf, oracle, seed, HOST_OPS, _config(5, "default"), device=have_gpu(), wrong=wrong)
        except hm.SequenceMismatch as e:
            text = str(e)
            assert "ops so far:" in text and f"seed {seed}" in text and "(seed=" in text, text
            caught.append(seed)
    print(f"{wrong}: reported for seeds {caught}")
    return caught


@pytest.mark.parametrize("wrong", ["hyper_before_ratings", "failed_set_ratings_keeps", "reseed_forgets_growth",
                                   "append_forgets_the_ratings"])
def test_the_driver_reports_a_model_with_one_wrong_rule(mf, oracle, wrong):
    """The comparison has teeth: a model that believes `set_hyper before set_ratings does not change lr`, `a failed
    set_ratings keeps the old schedule`, `init_factors seeds the sizes the handle was created with` or `the same triples
    after an append are built again` disagrees with the library on the same seeds the correct model passes."""
    assert len(_caught(mf, oracle, wrong)) >= 3


def test_the_driver_reports_a_model_whose_set_factors_clears_the_index(mf, oracle):
    """... and so does one that believes `set_factors drops the seen-item index`: seen_size() after the call says otherwise,
    also for the empty index a machine without a GPU keeps."""
    assert len(_caught(mf, oracle, "set_factors_clears_the_index")) >= 1


def test_the_driver_reports_a_model_whose_new_users_inherit_a_list(mf, oracle):
    """... and one that believes `append_users gives the new users the last user's list`.  That takes an index that holds
    pairs, so a device: without one every list is empty, the wrong rule and the right one say the same, and no seed may
    be reported at all."""
    caught = _caught(mf, oracle, "append_users_gives_new_users_the_last_list")
    if have_gpu():
        assert len(caught) >= 1
    else:
        assert caught == []


def test_a_failure_lists_every_op_so_far(mf, oracle):
    with pytest.raises(hm.SequenceMismatch) as ei:
        hm.run_sequence(mf, oracle, 0, HOST_OPS, _config(5, "default"), device=not have_gpu())  # the wrong expectation of a device
    lines = str(ei.value).split("ops so far:\n")[1].splitlines()
    assert len(lines) >= 1 and all(line.split()[0] == str(n) for n, line in enumerate(lines)), lines


def test_the_op_weights_meet_the_gpu_modules_conditions_by_the_model_alone():
    """The GPU module's cases in a dry run (no library, no oracle): the draw depends only on the seed and the model's
    abstract state, so these are the ops and outcomes of the real runs, and the coverage conditions hold for them."""
    cases = [(flag, geo, seed) for flag in hm.GPU_FLAGS for geo in sorted(hm.GEOMETRIES) for seed in hm.GPU_SEEDS]
    results = [hm.run_sequence(None, None, hm.gpu_seed(flag, geo, seed), hm.GPU_OPS, hm.gpu_config(flag, geo), dry=True)
               for flag, geo, seed in cases]
    total = hm.check_coverage(results)
    for geometry in hm.GEOMETRIES:  # every geometry runs both kernels of csrc/online.hip at least once
        for fact in ("partial_fit_with_a_wide_level", "partial_fit_with_a_narrow_level"):
            assert sum(res["facts"][fact] for (_, geo, _), res in zip(cases, results) if geo == geometry) >= 1, (geometry, fact)
    print(f"{total['ops']} ops, {total['errors']} errors ({100 * total['errors'] / total['ops']:.1f} %)")
    print(sorted(total["counts"].items()))
    print(sorted(total["facts"].items()))
