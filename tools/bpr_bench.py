"""What a pairwise (BPR) epoch costs ("Pairwise ranking (BPR)").

cfg2_ml20m (138 K users, 27 K items, k = 64); its 20 M pairs, shuffled once, are the positives and the seen-item index.
Wall times through the C-ABI from Python (host arrays in and out), each the median of RUNS rounds after a warm-up round:

    one fit_bpr epoch                        the steps of trainer.fit_bpr timed one by one: the draws (one per positive,
                                             download included), the host's look for users without negatives, and
                                             partial_fit_pairwise with margins -- of which triple_levels, timed on its own,
                                             is the host's levelling pass (the counting sort by level is a second pass of
                                             the same length); the rest is that sort, the uploads (16 bytes a triple), the
                                             launches and the margins coming down
    partial_fit of as many ratings           the same (user, item) pairs as ratings, errors asked for: the two-row update
                                             of the same machinery, for scale

with the levels, the widest level and the launches of both.  Stops if fit_bpr itself does not reproduce the bits of the
steps timed here.  Prints one JSON line with all of it.

    python tools/bpr_bench.py [WORKLOAD] [SCALE]
"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import mfsgd_amd as mf  # noqa: E402

RUNS = 2


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


def median(times):
    return round(float(np.median(times[1:])), 3), [round(t, 3) for t in times[1:]]  # the first is the warm-up


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "cfg2_ml20m"
    scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    w = mf.synth.workload(name, scale)
    U, I, k = int(w["U"]), int(w["I"]), int(w["k"])
    order = np.random.default_rng(0).permutation(len(w["u"]))
    u, i = np.ascontiguousarray(w["u"], np.int32)[order], np.ascontiguousarray(w["i"], np.int32)[order]
    n = u.size
    res = dict(workload=name, scale=scale, users=U, items=I, k=k, positives=int(n), pieces=int(-(-n // (1 << 20))))
    with mf.MatrixFactorizationSGD(U, I, k, 0.01, 0.05, 3, host_threads=16) as m:
        t0 = time.perf_counter()
        m.set_seen(u, i)
        res["set_seen_ms"] = round(ms(t0), 3)
        m.init_factors()
        # the two-row update of the same pairs, for scale (the parent's kernel, in this process)
        ones = np.ones(n, np.float32)
        times = []
        for run in range(RUNS + 1):
            t0 = time.perf_counter()
            _, info = m.partial_fit(u, i, ones, errors=True, info=True)
            times.append(ms(t0))
        res["ratings_apply_ms"], res["ratings_apply_runs_ms"] = median(times)
        res["ratings_levels"], res["ratings_max_width"], res["ratings_launches"] = info["levels"], info["max_width"], info["launches"]
        res["ratings_ms_per_piece"] = round(res["ratings_apply_ms"] / res["pieces"], 3)
        # the epochs of fit_bpr, step by step
        m.init_factors()
        level = mf.debug_device_bytes()
        J = np.empty((n, 1), np.int32)
        steps = dict(sample=[], host=[], levels=[], apply=[], epoch=[])
        for e in range(RUNS + 1):
            t_epoch = t0 = time.perf_counter()
            m._sample_unseen_into(u, 1, 0, e * n, J)
            steps["sample"].append(ms(t0))
            t0 = time.perf_counter()
            assert J.min() >= 0  # (nobody has seen everything: nothing to filter)
            steps["host"].append(ms(t0))
            t0 = time.perf_counter()
            x, info = m.partial_fit_pairwise(u, i, J[:, 0], margins=True, info=True)
            steps["apply"].append(ms(t0))
            steps["epoch"].append(ms(t_epoch))
            t0 = time.perf_counter()
            m.triple_levels(u, i, J[:, 0])  # (outside the epoch: partial_fit_pairwise has made this pass itself)
            steps["levels"].append(ms(t0))
            assert mf.debug_device_bytes() == level
        for step, times in steps.items():
            res[f"epoch_{step}_ms"], res[f"epoch_{step}_runs_ms"] = median(times)
        res["triples_levels"], res["triples_max_width"], res["triples_launches"] = info["levels"], info["max_width"], info["launches"]
        res["triples_ms_per_piece"] = round(res["epoch_apply_ms"] / res["pieces"], 3)
        res["apply_beyond_levels_ms"] = round(res["epoch_apply_ms"] - res["epoch_levels_ms"], 3)
        res["us_per_launch_all_in"] = round(res["apply_beyond_levels_ms"] * 1e3 / max(1, info["launches"]), 3)
        res["triples_over_ratings"] = round(res["epoch_apply_ms"] / res["ratings_apply_ms"], 3)
        x = x.astype(np.float64)
        res["last_epoch_loss"], res["last_epoch_auc"] = round(float(np.logaddexp(0.0, -x).mean()), 6), round(float((x > 0).mean()), 6)
        P, Q = m.get_factors()
    with mf.MatrixFactorizationSGD(U, I, k, 0.01, 0.05, 3, host_threads=16) as m2:
        t0 = time.perf_counter()
        m2.fit_bpr(u, i, RUNS + 1)
        res["fit_bpr_ms_per_epoch"] = round(ms(t0) / (RUNS + 1), 3)  # (its set_seen and the cold epoch included)
        P2, Q2 = m2.get_factors()
    if not (np.array_equal(P.view(np.uint32), P2.view(np.uint32)) and np.array_equal(Q.view(np.uint32), Q2.view(np.uint32))):
        sys.exit("fit_bpr differs from the steps timed here")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
