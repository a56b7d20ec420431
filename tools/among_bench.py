"""recommend(users, topn, candidates=...) beside the only routes to the same answer without it (DESIGN.md section 5,
"Top-N among candidates").

An ML-20M-sized model (138,493 users x 26,744 items, k = 64) with seeded factors; 4,096 users spread over the ids,
topn = 10.  Cases: a list per row of 256, 1,024 and 4,096 distinct random items, and one shared list of 1,024.  Per case,
alternated in one process, wall times through the C-ABI around calls that end in a synchronise (host arrays in and
out), each the median of RUNS rounds after a warm-up round of the same shape:

    among       recommend(users, topn, candidates=lists): checks, upload, list building, the gathered kernel
    whole       recommend(users, topn) over the whole catalogue: a lower bound on any route that scans Q -- it does not
                even give the filtered answer (the host would need all n_items per row for that)
    predict     predict() of every (user, candidate) pair, then the top 10 of each row on the host (argpartition, then
                a sort of the ten: cheaper than the exact tie rule, so the yardstick is generous)

and for `among` the two device halves apart, as the library's own clock has them (mfsgd_debug_serve_seconds, host
seconds up to each half's synchronise): `lists` = candidate upload, key build, sort, unique; `topn` = the kernel and the
download of the winners.  What is left of the wall time is the host: argument checks and the Python wrapper.
Prints one JSON line.

    python tools/among_bench.py [USERS ITEMS K]
"""
import json
import sys
import time

import numpy as np

sys.path.append(__file__.rsplit("/", 2)[0])  # (appended: a PYTHONPATH entry naming another checkout wins)
import mfsgd_amd as mf  # noqa: E402

RUNS = 5
QUERIES = 4096
TOPN = 10


def host_topn(scores, items, topn):
    """Top `topn` of each row of scores [n, len] (items alike): partition, then order the few that are left."""
    part = np.argpartition(-scores, topn - 1, axis=1)[:, :topn]
    sc, it = np.take_along_axis(scores, part, 1), np.take_along_axis(items, part, 1)
    order = np.lexsort((it, -sc), axis=1)
    return np.take_along_axis(it, order, 1), np.take_along_axis(sc, order, 1)


def alternate(calls, runs=RUNS):
    """calls: name -> function.  One warm-up round, then `runs` rounds, every contender once per round, in turn."""
    times = {name: [] for name in calls}
    extra = {}
    for rnd in range(runs + 1):
        for name, call in calls.items():
            t0 = time.perf_counter()
            more = call()
            if rnd:
                times[name].append((time.perf_counter() - t0) * 1e3)
                for key, value in (more or {}).items():
                    extra.setdefault(key, []).append(value * 1e3)
    out = {name: round(float(np.median(t)), 3) for name, t in times.items()}
    out.update({key: round(float(np.median(v)), 3) for key, v in extra.items()})
    return out


def main():
    U, I, k = (int(x) for x in sys.argv[1:4]) if len(sys.argv) > 3 else (138493, 26744, 64)
    rng = np.random.default_rng(7)
    users = np.linspace(0, U - 1, min(QUERIES, U)).astype(np.int32)
    n = users.size
    out = dict(users=U, items=I, k=k, queries=int(n), topn=TOPN, runs=RUNS, unit="ms", cases={})
    with mf.MatrixFactorizationSGD(U, I, k, 0.01, 0.05, 3) as m:
        m.init_factors()
        m.recommend(users[:1], TOPN)  # the factors go to the device

        def whole():
            m.recommend(users, TOPN)

        for length, shared in ((256, False), (1024, False), (4096, False), (1024, True)):
            length = min(length, I)
            if shared:
                lists = np.tile(rng.choice(I, length, replace=False).astype(np.int32), (n, 1))
                cand = np.ascontiguousarray(lists[0])
            else:
                lists = np.stack([rng.choice(I, length, replace=False) for _ in range(n)]).astype(np.int32)
                cand = (np.arange(n + 1, dtype=np.int64) * length, lists.reshape(-1))
            pair_u = np.repeat(users, length)

            def among():
                m.recommend(users, TOPN, candidates=cand)
                lists_s, topn_s = m.serve_seconds()
                return dict(among_lists=lists_s, among_topn=topn_s)

            def predict():
                sc = m.predict(pair_u, lists.reshape(-1)).reshape(n, length)
                host_topn(sc, lists, TOPN)

            res = alternate(dict(among=among, whole=whole, predict=predict))
            # the figures mean nothing if the answers differ: where the tenth score is no tie the two agree exactly
            got = m.recommend(users[:64], TOPN, candidates=(cand if shared else (cand[0][:65], cand[1][:64 * length])))
            want = host_topn(m.predict(pair_u[:64 * length], lists[:64].reshape(-1)).reshape(64, length), lists[:64], TOPN)
            assert np.array_equal(got[1].view(np.uint32), want[1].view(np.uint32)), "recommend among candidates is wrong"
            out["cases"][("shared_" if shared else "per_row_") + str(length)] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
