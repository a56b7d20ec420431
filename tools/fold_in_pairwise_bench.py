"""What the pairwise fold-in costs beside the squared-loss fold-in ("Pairwise fold-in").

A Q of the MovieLens-20M shape (26 744 items, k = 64, seeded); 10 000 new users with 20 positives each, 10 epochs.
Wall times through the C-ABI from Python (host arrays in and out), each the median of RUNS calls after a warm-up call:

    fold_in_pairwise, candidates = 1 and 10    the rows alone, and with margins and negatives coming down as well
    fold_in of the same lists, ratings 1.0     the yardstick: one gathered row a step, no draw, no lsig -- in the same process

Prints one JSON line with all of it.  With `kernel` as the first argument it only makes one warm and one measured call of
each of the three and prints what a step gathers: the run to put under a kernel trace, which gives the kernels' own time.
Run it under a time limit:

    timeout 300 python tools/fold_in_pairwise_bench.py [kernel] [USERS] [POSITIVES] [EPOCHS]
"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import mfsgd_amd as mf  # noqa: E402

RUNS = 3
MS = (1, 10)
ITEMS, K = 26744, 64


def median(times):
    return round(float(np.median(times[1:])), 3), [round(t, 3) for t in times[1:]]  # the first is the warm-up


def timed(call, runs):
    times = []
    for _ in range(runs + 1):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return times


def main():
    args = sys.argv[1:]
    kernel_only = bool(args) and args[0] == "kernel"
    args = [int(a) for a in (args[1:] if kernel_only else args)]
    users, positives, epochs = (args + [10000, 20, 10][len(args):])[:3]
    rng = np.random.default_rng(0)
    Q = (rng.standard_normal((ITEMS, K)) * (0.5 / np.sqrt(K))).astype(np.float32)
    items = rng.integers(0, ITEMS, users * positives).astype(np.int32)  # (an item twice in a list is two steps)
    row_ptr = np.arange(users + 1, dtype=np.int64) * positives
    ones = np.ones(items.size, np.float32)
    steps = users * positives * epochs
    res = dict(items=ITEMS, k=K, users=users, positives=positives, epochs=epochs, steps=steps)
    with mf.MatrixFactorizationSGD(4, ITEMS, K, 0.05, 0.01, 3) as m:
        m.set_factors(np.zeros((4, K), np.float32), Q)
        m.fold_in(row_ptr[:2], items[:positives], ones[:positives], 1)  # (the factors go to the device here, once)
        level = mf.debug_device_bytes()
        calls = [("fold_in", lambda: m.fold_in(row_ptr, items, ones, epochs))]
        for cand in MS:
            calls.append((f"pairwise_m{cand}", lambda c=cand: m.fold_in_pairwise(row_ptr, items, epochs, candidates=c)))
            if not kernel_only:
                calls.append((f"pairwise_m{cand}_with_outputs",
                              lambda c=cand: m.fold_in_pairwise(row_ptr, items, epochs, candidates=c, margins=True, negatives=True)))
        for name, call in calls:
            times = timed(call, 1 if kernel_only else RUNS)
            res[f"{name}_ms"], res[f"{name}_runs_ms"] = median(times)
        assert mf.debug_device_bytes() == level
        if not kernel_only:
            for cand in MS:
                res[f"pairwise_m{cand}_over_fold_in"] = round(res[f"pairwise_m{cand}_ms"] / res["fold_in_ms"], 3)
        res["gathered_rows_per_step"] = {"fold_in": 1, **{f"pairwise_m{c}": 1 + c for c in MS}}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
