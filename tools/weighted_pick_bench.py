"""What weighted candidates cost the picks beside uniform ones ("Weighted picks").

cfg2_ml20m (138 K users, 27 K items), k = 64; its 20 M pairs are the seen-item index, the item weights are
set_popularity_weights() of it, the factors are seeded.  Wall times through the C-ABI from Python (host arrays in and
out), each the median of 3 rounds after a warm-up round, all on one handle in one run:

    sample_unseen_hard(u, m)            m = 4, 16     uniform and weighted, the first ROWS pairs as rows
    sample_unseen_violating(u, i, m)    m = 10        margin 1.0 (the walk stops at the first violator) and a margin
                                                      nothing falls below (every candidate is walked)
    fold_in_pairwise                    m = 1, 4      USERS new users of 11 positives each, 5 epochs

Run it with MFSGD_LIBRARY pointing at another build of the library to time that build's uniform calls at the same
shapes (the weighted ones are skipped where the library or the Python surface lacks them).  Prints one JSON line with all of it.

    python tools/weighted_pick_bench.py [WORKLOAD] [SCALE]
"""
import inspect
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import mfsgd_amd as mf  # noqa: E402

RUNS = 3
ROWS = 1 << 21
USERS = 1 << 14


def timed(call):
    times = []
    for _ in range(RUNS + 1):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(times[1:])), 3), [round(t, 3) for t in times[1:]]  # the first is the warm-up


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "cfg2_ml20m"
    scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    w = mf.synth.workload(name, scale)
    U, I, k = int(w["U"]), int(w["I"]), 64
    u, i = np.ascontiguousarray(w["u"], np.int32), np.ascontiguousarray(w["i"], np.int32)
    rows = min(ROWS, u.size)
    ru, ri = u[:rows], i[:rows]
    res = dict(workload=name, scale=scale, users=U, items=I, k=k, rows=int(rows), library=mf.library_path())
    rng = np.random.default_rng(1)
    new = min(USERS, U)
    row_ptr = np.arange(new + 1, dtype=np.int64) * 11
    positives = rng.integers(0, I, new * 11).astype(np.int32)
    with mf.MatrixFactorizationSGD(U, I, k, 0.05, 0.01, 3) as m:
        m.init_factors()
        m.set_seen(u, i)
        m.set_popularity_weights()
        has_weighted = (hasattr(m._lib, "mfsgd_sample_unseen_hard_weighted")
                        and "sampling" in inspect.signature(m.sample_unseen_hard).parameters)
        kinds = [("uniform", {})] + ([("weighted", dict(sampling="weighted"))] if has_weighted else [])
        m.predict(ru[:1], ri[:1])  # the factors go to the device before anything is timed
        level = mf.debug_device_bytes()
        for kind, kw in kinds:
            for per_row in (4, 16):
                key = f"hard_{kind}_m{per_row}"
                res[key + "_ms"], res[key + "_runs_ms"] = timed(lambda: m.sample_unseen_hard(ru, per_row, 7, **kw))
                res[key + "_candidates_per_s"] = round(rows * per_row / (res[key + "_ms"] * 1e-3))
            for label, margin in (("margin1", 1.0), ("walk_all", -1e30)):
                key = f"violating_{kind}_m10_{label}"
                res[key + "_ms"], res[key + "_runs_ms"] = timed(lambda: m.sample_unseen_violating(ru, ri, 10, margin, 7, **kw))
            for per_step in (1, 4):
                key = f"fold_in_{kind}_m{per_step}"
                res[key + "_ms"], res[key + "_runs_ms"] = timed(
                    lambda: m.fold_in_pairwise(row_ptr, positives, 5, candidates=per_step, draw_seed=7, **kw))
            assert mf.debug_device_bytes() == level
        if has_weighted:
            for key in [x[:-3] for x in res if x.startswith(("hard_uniform", "violating_uniform", "fold_in_uniform")) and x.endswith("_ms")
                        and not x.endswith("_runs_ms")]:
                other = key.replace("uniform", "weighted")
                res[other + "_over_uniform"] = round(res[other + "_ms"] / res[key + "_ms"], 3)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
