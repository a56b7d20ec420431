"""What negative sampling and an implicit-feedback epoch cost ("Implicit feedback").

cfg2_ml20m (138 K users, 27 K items, k = 64); its 20 M pairs are the positives and the seen-item index.  Wall times through
the C-ABI from Python (host arrays in and out), each the median of 3 rounds after a warm-up round:

    sample_unseen(u, m) for m = 1, 4, 16     one row per positive: draws per second, the download included
    one fit_implicit epoch, negatives = 4    the steps of trainer.fit_implicit timed one by one: the draws (download
                                             included, into the tail of the epoch's rating set, which is laid out once),
                                             the host's look for users without negatives, set_ratings of the 5 n triples
                                             (a new schedule every epoch), fit(1)

and, for scale, set_ratings and fit(1) of the positives alone.  Stops if fit_implicit itself does not reproduce the bits
of the steps timed here.  Prints one JSON line with all of it.

    python tools/implicit_bench.py [WORKLOAD] [SCALE]
"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import mfsgd_amd as mf  # noqa: E402

RUNS = 3
NEGATIVES = 4


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


def median(times):
    return round(float(np.median(times[1:])), 3), [round(t, 3) for t in times[1:]]  # the first is the warm-up


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "cfg2_ml20m"
    scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    w = mf.synth.workload(name, scale)
    U, I, k = int(w["U"]), int(w["I"]), int(w["k"])
    u, i = np.ascontiguousarray(w["u"], np.int32), np.ascontiguousarray(w["i"], np.int32)
    n = u.size
    res = dict(workload=name, scale=scale, users=U, items=I, k=k, positives=int(n), negatives=NEGATIVES)
    with mf.MatrixFactorizationSGD(U, I, k, 0.01, 0.05, 3, host_threads=16) as m:
        t0 = time.perf_counter()
        m.set_seen(u, i)
        res["set_seen_ms"] = round(ms(t0), 3)
        res["distinct_pairs"] = m.seen_size()
        level = mf.debug_device_bytes()
        for per_row in (1, 4, 16):
            times = []
            for run in range(RUNS + 1):
                t0 = time.perf_counter()
                drawn = m.sample_unseen(u, per_row, seed=run)
                times.append(ms(t0))
            assert drawn.min() >= 0 and drawn.max() < I and mf.debug_device_bytes() == level
            med, runs = median(times)
            res[f"sample_m{per_row}_ms"], res[f"sample_m{per_row}_runs_ms"] = med, runs
            res[f"sample_m{per_row}_draws_per_s"] = round(n * per_row / (med * 1e-3))
            del drawn
        # the positives alone, for scale
        ones = np.ones(n, np.float32)
        m.init_factors()
        steps = dict(set_ratings=[], fit=[])
        for run in range(RUNS + 1):
            ones[0] = 1.0 + run  # (another set every time: the same triples again would keep the schedule)
            t0 = time.perf_counter()
            m.set_ratings(u, i, ones)
            steps["set_ratings"].append(ms(t0))
            t0 = time.perf_counter()
            m.fit(1, rmse=False)
            steps["fit"].append(ms(t0))
        for step, times in steps.items():
            res[f"positives_{step}_ms"], res[f"positives_{step}_runs_ms"] = median(times)
        # the epochs of fit_implicit, step by step
        ones[0] = 1.0
        m.init_factors()
        t0 = time.perf_counter()
        set_u, set_i = np.concatenate([u, np.repeat(u, NEGATIVES)]), np.concatenate([i, np.empty(n * NEGATIVES, np.int32)])
        set_r = np.concatenate([ones, np.zeros(n * NEGATIVES, np.float32)])
        res["layout_once_ms"] = round(ms(t0), 3)
        steps = dict(sample=[], host=[], set_ratings=[], fit=[], epoch=[])
        for e in range(RUNS + 1):
            t_epoch = t0 = time.perf_counter()
            m._sample_unseen_into(u, NEGATIVES, 0, e * n * NEGATIVES, set_i[n:])
            steps["sample"].append(ms(t0))
            t0 = time.perf_counter()
            assert set_i[n:].min() >= 0  # (nobody has seen everything: nothing to filter)
            steps["host"].append(ms(t0))
            t0 = time.perf_counter()
            m.set_ratings(set_u, set_i, set_r)
            steps["set_ratings"].append(ms(t0))
            t0 = time.perf_counter()
            m.fit(1, rmse=False)
            steps["fit"].append(ms(t0))
            steps["epoch"].append(ms(t_epoch))
        for step, times in steps.items():
            res[f"epoch_{step}_ms"], res[f"epoch_{step}_runs_ms"] = median(times)
        res["epoch_sample_share"] = round(res["epoch_sample_ms"] / res["epoch_epoch_ms"], 4)
        res["schedule_builds"] = int(m.debug_counters()["schedule_builds"])
        P, Q = m.get_factors()
    with mf.MatrixFactorizationSGD(U, I, k, 0.01, 0.05, 3, host_threads=16) as m2:
        t0 = time.perf_counter()
        m2.fit_implicit(u, i, RUNS + 1, NEGATIVES, rmse=False)
        res["fit_implicit_ms_per_epoch"] = round(ms(t0) / (RUNS + 1), 3)  # (its set_seen and the cold epoch included)
        P2, Q2 = m2.get_factors()
    if not (np.array_equal(P.view(np.uint32), P2.view(np.uint32)) and np.array_equal(Q.view(np.uint32), Q2.view(np.uint32))):
        sys.exit("fit_implicit differs from the steps timed here")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
