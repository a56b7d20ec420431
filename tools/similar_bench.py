"""similar_items beside the recommend call whose kernels it shares ("Cosine neighbours").

An ML-20M-sized model (138,493 users x 26,744 items, k = 64) with seeded factors; 4,096 queries spread over the ids.
Wall times through the C-ABI (host arrays in and out), each the median of RUNS runs after one warm-up, for topn 10
and 128 (both on the fused path):

    recommend(users, topn)         the yardstick: topn_kernel with the plain dot
    similar_items(items, topn)     the same kernel with the cosine policy and the self-exclusion lists, plus one
                                   inverse-norm pass over Q per call

and, once, similar_users for 256 users (the user side is never fused: the batched sort path) and row_inv_norms of both
sides.  On a checkout without the similar calls (the parent of the commit that added them) only recommend is
measured, which is how the two builds are compared: run this file under each, alternating, and compare the
recommend lines.  Prints one JSON line.

    python tools/similar_bench.py [USERS ITEMS K]
"""
import json
import sys
import time

import numpy as np

sys.path.append(__file__.rsplit("/", 2)[0])  # (appended: a PYTHONPATH entry naming another checkout wins)
import mfsgd_amd as mf  # noqa: E402

RUNS = 20
QUERIES = 4096


def median_ms(call, runs=RUNS):
    call()  # warm-up
    times = []
    for _ in range(runs):
        t0 = time.perf_counter()
        call()
        times.append((time.perf_counter() - t0) * 1e3)
    return dict(median=round(float(np.median(times)), 3), min=round(min(times), 3), max=round(max(times), 3))


def main():
    U, I, k = (int(x) for x in sys.argv[1:4]) if len(sys.argv) > 3 else (138493, 26744, 64)
    users = np.linspace(0, U - 1, min(QUERIES, U)).astype(np.int32)
    items = np.linspace(0, I - 1, min(QUERIES, I)).astype(np.int32)
    out = dict(users=U, items=I, k=k, queries=int(items.size), runs=RUNS)
    with mf.MatrixFactorizationSGD(U, I, k, 0.01, 0.05, 3) as m:
        m.init_factors()
        have = hasattr(m, "similar_items")
        out["has_similar"] = have
        for topn in (10, 128):
            topn = min(topn, I - 1)
            out[f"recommend_top{topn}_ms"] = median_ms(lambda: m.recommend(users, topn))
            if have:
                out[f"similar_items_top{topn}_ms"] = median_ms(lambda: m.similar_items(items, topn))
        if have:
            out["similar_users_256_top10_ms"] = median_ms(lambda: m.similar_users(users[:256], 10), runs=3)
            out["row_inv_norms_items_ms"] = median_ms(lambda: m.row_inv_norms("items"))
            out["row_inv_norms_users_ms"] = median_ms(lambda: m.row_inv_norms("users"))
            # the figures mean nothing if the answers are wrong: one row against numpy (fp64, so ranks near ties may
            # differ; the top hit of a random model is far from one)
            P, Q = m.get_factors()
            idx, sc = m.similar_items(items[:4], 10)
            for row, a in enumerate(items[:4]):
                c = (Q @ Q[a].astype(np.float64)) / (np.linalg.norm(Q.astype(np.float64), axis=1) * np.linalg.norm(Q[a].astype(np.float64)))
                c[a] = -np.inf
                assert idx[row, 0] == int(np.argmax(c)) and abs(sc[row, 0] - c[idx[row, 0]]) < 1e-5, "similar_items is wrong"
    print(json.dumps(out))


if __name__ == "__main__":
    main()
