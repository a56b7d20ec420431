"""What the least-squares fold-in costs beside the SGD fold-in ("Fold-in by least squares").

A Q of the MovieLens-20M shape (26 744 items, seeded) at k = 64 and at k = 128; 4096 new users with 100 ratings each.
Wall times through the C-ABI from Python (host arrays in and out; every call ends in a device synchronise), each the
median of RUNS calls after a warm-up call, the two alternating in one process:

    fold_in_exact                 the solve: one pass over each list, one k x k system per user
    fold_in at 20 epochs          the yardstick: the SGD chain, whose code this feature does not touch
    fold_in_implicit              the same lists as confidences: the solve plus one Gram matrix of Q per call

and the largest element-wise distance between the rows of the first two (the chain at 20 epochs has not converged: the
distance says how far it still is from its fixed point, not how wrong either is).  Prints one JSON line per k.
Run it under a time limit:

    timeout 300 python tools/fold_solve_bench.py [USERS] [RATINGS] [EPOCHS]
"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import mfsgd_amd as mf  # noqa: E402

RUNS = 5
ITEMS = 26744
LR, LAM = 0.01, 0.05


def main():
    args = [int(a) for a in sys.argv[1:]]
    users, ratings, epochs = (args + [4096, 100, 20][len(args):])[:3]
    for k in (64, 128):
        rng = np.random.default_rng(k)
        Q = (rng.standard_normal((ITEMS, k)) * (0.5 / np.sqrt(k))).astype(np.float32)
        items = rng.integers(0, ITEMS, users * ratings).astype(np.int32)
        r = rng.uniform(0.5, 5.0, items.size).astype(np.float32)
        conf = (1.0 + 8.0 * r).astype(np.float32)
        row_ptr = np.arange(users + 1, dtype=np.int64) * ratings
        res = dict(items=ITEMS, k=k, users=users, ratings=ratings, epochs=epochs, runs=RUNS)
        with mf.MatrixFactorizationSGD(4, ITEMS, k, LR, LAM, 3) as m:
            m.set_factors(np.zeros((4, k), np.float32), Q)
            m.gram("items")  # (the factors go to the device here, once)
            level = mf.debug_device_bytes()
            calls = dict(fold_in_exact=lambda: m.fold_in_exact(row_ptr, items, r, status=True),
                         fold_in_sgd=lambda: m.fold_in(row_ptr, items, r, epochs),
                         fold_in_implicit=lambda: m.fold_in_implicit(row_ptr, items, conf, 0.1, status=True))
            times = {name: [] for name in calls}
            out = {}
            for _ in range(RUNS + 1):  # (the first round is the warm-up)
                for name, call in calls.items():
                    t0 = time.perf_counter()
                    out[name] = call()
                    times[name].append((time.perf_counter() - t0) * 1e3)
            assert mf.debug_device_bytes() == level
            for name, t in times.items():
                res[f"{name}_ms"], res[f"{name}_runs_ms"] = round(float(np.median(t[1:])), 3), [round(x, 3) for x in t[1:]]
            assert not out["fold_in_exact"][1].any() and not out["fold_in_implicit"][1].any()
            res["sgd_over_exact"] = round(res["fold_in_sgd_ms"] / res["fold_in_exact_ms"], 2)
            res["max_abs_distance_sgd_to_exact"] = float(np.abs(out["fold_in_sgd"] - out["fold_in_exact"][0]).max())
            res["max_abs_exact"] = float(np.abs(out["fold_in_exact"][0]).max())
        print(json.dumps(res), flush=True)


if __name__ == "__main__":
    main()
