"""What growing a live model costs ("Growing a live model").

On a synth.workload shape (default cfg2_ml20m at scale 1.0, k = 64), with the part on the device after two epochs:

    (a) add_items(rows) / add_users(rows)       wall time of one append of N_NEW rows of the caller's, (1) reallocating
                                                (no reserve: old rows copied device to device) and (2) in place (inside
                                                a reserve); median of RUNS, each on the grown model of the run before
    (b) the fit(1) that follows each            wall time without RMSE pass: after (1) the training graph is captured
                                                again, after (2) it is replayed (graphs_after_append: the graphs cached
                                                between the append and that fit); and a fit(1) with nothing before it
    (c) the route there was before              get_factors + new handle at the grown size + set_ratings + set_factors,
                                                once (the first epoch's upload is not counted)

Prints one JSON line.  Needs a GPU: nothing here falls back.

    python tools/grow_cost.py [WORKLOAD] [SCALE] [K]
"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import mfsgd_amd as mf  # noqa: E402

RUNS, N_NEW = 7, 64


def timed(call):
    t0 = time.perf_counter()
    call()
    return time.perf_counter() - t0


def main():
    name = sys.argv[1] if len(sys.argv) > 1 else "cfg2_ml20m"
    scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
    w = mf.synth.workload(name, scale)
    k = int(sys.argv[3]) if len(sys.argv) > 3 else 64
    u, i, r = (np.ascontiguousarray(w[x]) for x in ("u", "i", "r"))
    rng = np.random.default_rng(1)
    rows = (rng.standard_normal((N_NEW, k)) * 0.1).astype(np.float32)
    ms = lambda runs: round(float(np.median(runs)) * 1e3, 3)
    out = dict(workload=name, scale=scale, k=k, nnz=int(w["nnz"]), users=int(w["U"]), items=int(w["I"]), n_new=N_NEW)

    def measure(m, tag):
        """RUNS times: an append of each side, then fit(1); the graphs cached before the first pair and right behind it."""
        g0 = m.debug_counters()["graphs"]
        users, items, fits = [], [], []
        for x in range(RUNS):
            users.append(timed(lambda: m.add_users(rows)))
            items.append(timed(lambda: m.add_items(rows)))
            if x == 0:
                g1 = m.debug_counters()["graphs"]   # cached now, before the fit captures again: 0 when they were dropped
            fits.append(timed(lambda: m.fit(1, rmse=False)))
        out[tag] = dict(add_users_ms=ms(users), add_items_ms=ms(items), fit_after_ms=ms(fits),
                        add_users_runs_ms=[round(t * 1e3, 3) for t in users], fit_after_runs_ms=[round(t * 1e3, 3) for t in fits],
                        graphs_before=g0, graphs_after_append=g1)

    with mf.MatrixFactorizationSGD(w["U"], w["I"], k, 0.01, 0.05, 3, host_threads=16) as m:
        m.set_ratings(u, i, r)
        m.init_factors()
        m.fit(2, rmse=False)
        out["fit_plain_ms"] = ms([timed(lambda: m.fit(1, rmse=False)) for _ in range(RUNS)])
        measure(m, "reallocating")
        m.reserve(users=m.users + 2 * RUNS * N_NEW, items=m.items + 2 * RUNS * N_NEW)
        m.fit(1, rmse=False)                      # (the reserve moved P and Q: its re-capture is not the append's)
        measure(m, "in_place")
        out["builds"] = m.debug_counters()["schedule_builds"]
        # (c) the only route there was before
        t0 = time.perf_counter()
        P, Q = m.get_factors()
        big = mf.MatrixFactorizationSGD(m.users + N_NEW, m.items, k, 0.01, 0.05, 3, host_threads=16)
        big.set_ratings(u, i, r)
        big.set_factors(np.vstack([P, rows]), Q)
        out["rebuild_route_ms"] = round((time.perf_counter() - t0) * 1e3, 3)
        out["rebuild_route_schedule_build_ms"] = round(big.schedule_info()["build_seconds"] * 1e3, 3)
        big.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
