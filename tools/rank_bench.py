"""rank_items against the recommend call it shares its inputs with ("Ranking held-out items").

cfg2_ml20m (k = 64) after one epoch; 4,096 users spread over the id range, one held-out pair each taken from the
user's own ratings, and ALL training pairs as exclusions.  Two wall times through the C-ABI (host arrays in and out),
each the median of 5 runs after one warm-up:

    rank_items(users, held_out, exclude=(u, i))
    recommend(users, 10, exclude=(u, i))            the yardstick: the fused top-N kernel

Both build the same exclusion lists and stream Q; the rank call must not be the slower one.  Also timed, the same
way: both calls without exclusions (what the lists cost, and the kernels nearly alone); and the ranks of the first
four users are recounted on the host from predict()'s scores (an assertion).  Prints one JSON line with all of it.

    python tools/rank_bench.py [WORKLOAD] [SCALE]
"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import mfsgd_amd as mf  # noqa: E402

RUNS = 5


def median_seconds(call):
    call()  # warm-up
    times = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        call()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), times


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "cfg2_ml20m"
    scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    w = mf.synth.workload(name, scale)
    u, i = np.ascontiguousarray(w["u"], np.int32), np.ascontiguousarray(w["i"], np.int32)
    # users that have a rating, evenly spread over the ids; the held-out pair of each is its first rating
    rated, first = np.unique(u, return_index=True)
    pick = np.linspace(0, rated.size - 1, min(4096, rated.size)).astype(np.int64)
    users, held = rated[pick].astype(np.int32), i[first[pick]].astype(np.int32)
    with mf.MatrixFactorizationSGD(w["U"], w["I"], w["k"], 0.01, 0.05, 3, host_threads=16) as m:
        m.set_ratings(u, i, w["r"])
        m.init_factors()
        m.fit(1, rmse=False)
        out = {}
        t_rank, all_rank = median_seconds(lambda: out.__setitem__("ranks", m.rank_items(users, held, exclude=(u, i))))
        t_rec, all_rec = median_seconds(lambda: out.__setitem__("top", m.recommend(users, 10, exclude=(u, i))))
        # what the lists cost both calls, and the calls without them
        t_rank0, _ = median_seconds(lambda: m.rank_items(users, held))
        t_rec0, _ = median_seconds(lambda: m.recommend(users, 10))
        pred = m.predict(np.repeat(users, w["I"])[: 4 * w["I"]], np.tile(np.arange(w["I"], dtype=np.int32), 4))
    # the ranks of the first four users, recounted from predict()'s scores on the host
    for x in range(4):
        s = pred[x * w["I"]:(x + 1) * w["I"]]
        keep = np.ones(w["I"], bool)
        keep[i[u == users[x]]] = False
        keep[held[x]] = True
        before = (s > s[held[x]]) | ((s == s[held[x]]) & (np.arange(w["I"]) < held[x]))
        assert int(np.count_nonzero(before & keep)) == int(out["ranks"][x]), "rank_items disagrees with predict()"
    print(json.dumps(dict(
        workload=name, scale=scale, users=int(users.size), items=int(w["I"]), k=int(w["k"]), exclusion_pairs=int(u.size),
        rank_items_ms=round(t_rank * 1e3, 3), recommend_top10_ms=round(t_rec * 1e3, 3), ratio=round(t_rank / t_rec, 4),
        rank_items_runs_ms=[round(t * 1e3, 3) for t in all_rank], recommend_runs_ms=[round(t * 1e3, 3) for t in all_rec],
        rank_items_no_exclusions_ms=round(t_rank0 * 1e3, 3), recommend_no_exclusions_ms=round(t_rec0 * 1e3, 3),
        ratio_no_exclusions=round(t_rank0 / t_rec0, 4), median_rank=float(np.median(out["ranks"])))))


if __name__ == "__main__":
    main()
