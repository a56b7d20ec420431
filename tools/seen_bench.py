"""The serving calls against the seen-item index, beside the same calls given the pairs as a list and given no exclusions
("The seen-item index").

cfg2_ml20m (k = 64) after one epoch; ALL training pairs are what the users have seen.  For 1, 64 and 4,096 users spread
over the id range, wall times through the C-ABI (host arrays in and out), each the median of 5 rounds after a warm-up
round, the six forms alternating inside a round:

    recommend(users, 10, exclude=(u, i))      the pair list: checked, uploaded and sorted into lists on every call
    recommend(users, 10, exclude="seen")      the index, built once by set_seen and read where it lies
    recommend(users, 10)                      no exclusions
    rank_items(users, held, ...)              the same three forms, one held-out pair per user (its first rating)

and, the same way, set_seen of all pairs, mark_seen of 2^10, 2^16 and 2^20 pairs the index does not hold (each into the
index of the training pairs, rebuilt before every run), and the bytes the index holds (mfsgd_debug_device_bytes).
Stops if a result from the index differs from the pair list's.  Prints one JSON line with all of it.

    python tools/seen_bench.py [WORKLOAD] [SCALE]
"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import mfsgd_amd as mf  # noqa: E402

RUNS = 5


def median_ms(call, before=None):
    times = []
    for run in range(RUNS + 1):  # the first is the warm-up
        if before:
            before()
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return round(float(np.median(times[1:])), 3), [round(t, 3) for t in times[1:]]


def same(a, b):
    pad = b[0] < 0
    return (np.array_equal(a[0], b[0]) and np.isnan(a[1][pad]).all()
            and np.array_equal(a[1].view(np.uint32)[~pad], b[1].view(np.uint32)[~pad]))


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "cfg2_ml20m"
    scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    w = mf.synth.workload(name, scale)
    U, I = int(w["U"]), int(w["I"])
    u, i = np.ascontiguousarray(w["u"], np.int32), np.ascontiguousarray(w["i"], np.int32)
    rated, first = np.unique(u, return_index=True)
    # pairs the index does not hold, for mark_seen
    rng = np.random.default_rng(1)
    have = np.unique((u.astype(np.int64) << 32) | i)
    cand = np.unique((rng.integers(0, U, 3 << 20).astype(np.int64) << 32) | rng.integers(0, I, 3 << 20))
    at = np.minimum(np.searchsorted(have, cand), have.size - 1)
    fresh = rng.permutation(cand[have[at] != cand])
    fu, fi = (fresh >> 32).astype(np.int32), (fresh & 0xFFFFFFFF).astype(np.int32)
    res = dict(workload=name, scale=scale, users=U, items=I, k=int(w["k"]), pairs=int(u.size), distinct_pairs=int(have.size))
    with mf.MatrixFactorizationSGD(U, I, w["k"], 0.01, 0.05, 3, host_threads=16) as m:
        m.set_ratings(u, i, w["r"])
        m.init_factors()
        m.fit(1, rmse=False)
        level = mf.debug_device_bytes()
        res["set_seen_ms"], res["set_seen_runs_ms"] = median_ms(lambda: m.set_seen(u, i))
        assert m.seen_size() == have.size
        res["index_bytes"] = int(mf.debug_device_bytes() - level)
        res["index_bytes_bound"] = int(4 * have.size + 12 * (m.capacity()[0] + 1) + 64)
        for n_users in (1, 64, 4096):
            pick = np.linspace(0, rated.size - 1, min(n_users, rated.size)).astype(np.int64)
            users, held = rated[pick].astype(np.int32), i[first[pick]].astype(np.int32)
            forms = dict(
                recommend_pairs=lambda: m.recommend(users, 10, exclude=(u, i)),
                recommend_seen=lambda: m.recommend(users, 10, exclude="seen"),
                recommend_none=lambda: m.recommend(users, 10),
                rank_pairs=lambda: m.rank_items(users, held, exclude=(u, i)),
                rank_seen=lambda: m.rank_items(users, held, exclude="seen"),
                rank_none=lambda: m.rank_items(users, held))
            # the six forms alternate inside every round, so that none of them has the warm end of the run to itself
            times, out, halves = {f: [] for f in forms}, {}, {}
            for rnd in range(RUNS + 1):  # the first round is the warm-up
                for f, call in forms.items():
                    t0 = time.perf_counter()
                    out[f] = call()
                    times[f].append((time.perf_counter() - t0) * 1e3)
                    if f.startswith("recommend"):
                        halves[f] = [round(x * 1e3, 3) for x in m.serve_seconds()]
            row = {}
            for f in forms:
                row[f + "_ms"] = round(float(np.median(times[f][1:])), 3)
                row[f + "_runs_ms"] = [round(t, 3) for t in times[f][1:]]
            row["recommend_seen_halves_ms"], row["recommend_none_halves_ms"] = halves["recommend_seen"], halves["recommend_none"]
            if not same(out["recommend_seen"], out["recommend_pairs"]):
                sys.exit(f"{n_users} users: recommend(exclude=\"seen\") differs from recommend(exclude=(u, i))")
            if not np.array_equal(out["rank_seen"], out["rank_pairs"]):
                sys.exit(f"{n_users} users: rank_items(exclude=\"seen\") differs from rank_items(exclude=(u, i))")
            res[f"users_{n_users}"] = row
        for log2 in (10, 16, 20):
            n = min(1 << log2, fu.size)
            key = f"mark_seen_2^{log2}_ms"
            res[key], res[key.replace("_ms", "_runs_ms")] = median_ms(lambda: m.mark_seen(fu[:n], fi[:n]),
                                                                      before=lambda: m.set_seen(u, i))
            assert m.seen_size() == have.size + n
    print(json.dumps(res))


if __name__ == "__main__":
    main()
