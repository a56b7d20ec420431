"""Top-N users for items beside top-N items for users ("Item-side serving").

An ML-20M-shaped model (cfg2_ml20m: 138 493 x 26 744, k = 64, seeded factors), the workload's pairs as the seen-item
index.  4 096 request rows spread over the id range, top-10, wall times through the C-ABI (host arrays in and out) and
the two device halves mfsgd_debug_serve_seconds reports, each the median of 5 rounds after a warm-up round, the forms
alternating inside a round:

    recommend(users, 10)                          the existing direction, for scale
    recommend_users(items, 10)                    no exclusions
    recommend_users(items, 10, exclude="seen")    the index read by item (csrc/audience.hip), then lists as for pairs
    recommend_users(items, 10, exclude=(u, i))    the pair list: checked, uploaded and sorted into lists on every call

On a build without recommend_users only the first form is measured.  Stops if the index's result differs from the pair
list's.  Prints one JSON line.

    python tools/recommend_users_bench.py [WORKLOAD] [SCALE]
"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import mfsgd_amd as mf  # noqa: E402

RUNS, ROWS, TOPN = 5, 4096, 10


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "cfg2_ml20m"
    scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    w = mf.synth.workload(name, scale)
    U, I = int(w["U"]), int(w["I"])
    u, i = np.ascontiguousarray(w["u"], np.int32), np.ascontiguousarray(w["i"], np.int32)
    users = np.linspace(0, U - 1, min(ROWS, U)).astype(np.int32)
    items = np.linspace(0, I - 1, min(ROWS, I)).astype(np.int32)
    res = dict(workload=name, scale=scale, users=U, items=I, k=int(w["k"]), pairs=int(u.size), rows=int(items.size), topn=TOPN)
    with mf.MatrixFactorizationSGD(U, I, w["k"], 0.01, 0.05, 3) as m:
        m.init_factors()
        m.set_seen(u, i)
        res["index_pairs"] = m.seen_size()
        forms = dict(recommend=lambda: m.recommend(users, TOPN))
        if hasattr(m, "recommend_users"):
            forms.update(recommend_users=lambda: m.recommend_users(items, TOPN),
                         recommend_users_seen=lambda: m.recommend_users(items, TOPN, exclude="seen"),
                         recommend_users_pairs=lambda: m.recommend_users(items, TOPN, exclude=(u, i)))
        times, halves, out = {f: [] for f in forms}, {f: [] for f in forms}, {}
        for rnd in range(RUNS + 1):  # the first round is the warm-up
            for f, call in forms.items():
                t0 = time.perf_counter()
                out[f] = call()
                times[f].append((time.perf_counter() - t0) * 1e3)
                halves[f].append([x * 1e3 for x in m.serve_seconds()])
        for f in forms:
            res[f + "_ms"] = round(float(np.median(times[f][1:])), 3)
            res[f + "_runs_ms"] = [round(t, 3) for t in times[f][1:]]
            res[f + "_halves_ms"] = [round(float(x), 3) for x in np.median(np.array(halves[f][1:]), axis=0)]
        if "recommend_users_seen" in out:
            a, b = out["recommend_users_seen"], out["recommend_users_pairs"]
            if a[0].tobytes() != b[0].tobytes() or a[1].tobytes() != b[1].tobytes():
                sys.exit("recommend_users(exclude=\"seen\") differs from recommend_users(exclude=(u, i))")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
