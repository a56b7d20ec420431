"""What weighted negative sampling costs beside the uniform draw ("Weighted negatives").

cfg2_ml20m (138 K users, 27 K items); its 20 M pairs are the seen-item index, the item weights are
set_popularity_weights() of it.  Wall times through the C-ABI from Python (host arrays in and out), each the median of 3
rounds after a warm-up round, all on one handle in one run:

    sample_unseen_weighted(u, m) and sample_unseen(u, m) for m = 1, 4, 16, one row per pair, into an output array that
                                             has been written before (what the fits do), the download included
    set_item_weights                         the prefix going up and the unseen-mass table of the 20 M pairs
    mark_seen of 2^10 pairs the index lacks  with weights and without: the difference is the rebuild of the table

and, as a fact about the two samplers, the share of one epoch's negatives (m = 4) that falls on the 1 % most popular
items.  Prints one JSON line with all of it.

    python tools/weighted_bench.py [WORKLOAD] [SCALE]
"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import mfsgd_amd as mf  # noqa: E402

RUNS = 3
BATCH = 1 << 10


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


def median(times):
    return round(float(np.median(times[1:])), 3), [round(t, 3) for t in times[1:]]  # the first is the warm-up


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "cfg2_ml20m"
    scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    w = mf.synth.workload(name, scale)
    U, I = int(w["U"]), int(w["I"])
    u, i = np.ascontiguousarray(w["u"], np.int32), np.ascontiguousarray(w["i"], np.int32)
    n = u.size
    res = dict(workload=name, scale=scale, users=U, items=I, rows=int(n))
    # pairs the index lacks, for the mark_seen rounds: 2 x (RUNS + 1) batches
    rng = np.random.default_rng(1)
    fu, fi = rng.integers(0, U, 64 * BATCH).astype(np.int32), rng.integers(0, I, 64 * BATCH).astype(np.int32)
    keys = np.unique((fu.astype(np.int64) << 32) | fi)
    keys = rng.permutation(keys[~np.isin(keys, (u.astype(np.int64) << 32) | i)])[:2 * (RUNS + 1) * BATCH]
    assert keys.size == 2 * (RUNS + 1) * BATCH
    fu, fi = (keys >> 32).astype(np.int32), (keys & 0xFFFFFFFF).astype(np.int32)
    with mf.MatrixFactorizationSGD(U, I, 8, 0.01, 0.05, 3) as m:
        t0 = time.perf_counter()
        m.set_seen(u, i)
        res["set_seen_ms"] = round(ms(t0), 3)
        res["distinct_pairs"] = m.seen_size()
        t0 = time.perf_counter()
        counts = m.seen_item_counts()
        res["seen_item_counts_ms"] = round(ms(t0), 3)
        weights = mf.popularity_weights(counts)
        res["weight_sum"], res["weight_max"], res["weight_zero_items"] = int(weights.sum()), int(weights.max()), int((weights == 0).sum())
        times = []
        for run in range(RUNS + 1):
            t0 = time.perf_counter()
            m.set_item_weights(weights)
            times.append(ms(t0))
        res["set_item_weights_ms"], res["set_item_weights_runs_ms"] = median(times)
        level = mf.debug_device_bytes()
        top = np.argsort(-counts, kind="stable")[:max(1, I // 100)]  # the 1 % most popular items
        is_top = np.zeros(I, bool)
        is_top[top] = True
        for per_row in (1, 4, 16):
            out = np.zeros((n, per_row), np.int32)
            for kind, draw in (("uniform", m._sample_unseen_into), ("weighted", m._sample_weighted_into)):
                times = []
                for run in range(RUNS + 1):
                    t0 = time.perf_counter()
                    draw(u, per_row, run, 0, out)
                    times.append(ms(t0))
                assert out.min() >= 0 and out.max() < I and mf.debug_device_bytes() == level
                med, runs = median(times)
                res[f"{kind}_m{per_row}_ms"], res[f"{kind}_m{per_row}_runs_ms"] = med, runs
                res[f"{kind}_m{per_row}_draws_per_s"] = round(n * per_row / (med * 1e-3))
                if per_row == 4:
                    res[f"{kind}_top1pct_share"] = round(float(is_top[out].mean()), 4)
            res[f"weighted_over_uniform_m{per_row}"] = round(res[f"weighted_m{per_row}_ms"] / res[f"uniform_m{per_row}_ms"], 3)
            del out
        res["top1pct_items"] = int(top.size)
        res["top1pct_share_of_pairs"] = round(float(counts[top].sum() / counts.sum()), 4)
        # mark_seen of fresh pairs: with the weights (the table is rebuilt), then without
        for kind, base in (("with_weights", 0), ("without_weights", RUNS + 1)):
            if kind == "without_weights":
                m.clear_item_weights()
            times = []
            for run in range(RUNS + 1):
                a = (base + run) * BATCH
                before = m.seen_size()
                t0 = time.perf_counter()
                m.mark_seen(fu[a:a + BATCH], fi[a:a + BATCH])
                times.append(ms(t0))
                assert m.seen_size() == before + BATCH
            res[f"mark_seen_{kind}_ms"], res[f"mark_seen_{kind}_runs_ms"] = median(times)
        res["mass_rebuild_ms"] = round(res["mark_seen_with_weights_ms"] - res["mark_seen_without_weights_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
