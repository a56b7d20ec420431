"""What another lr / lambda costs on a live model ("Changing lr and lambda").

On a synth.workload shape (default cfg2_ml20m at scale 1.0, k = 64), with the part on the device after one epoch:

    (a) set_hyper(lr, lam)                      wall time, median of RUNS after one warm-up; the values alternate, so
                                                every call re-bakes
    (b) get_factors + new handle + set_ratings  the only route there was before: wall time, median of ROUTE_RUNS after
        + set_factors (+ close of the old one)  one warm-up (the first epoch's upload of the new schedule is NOT counted)
    (c) one epoch                               device time, train_timed(EPOCHS) / EPOCHS after a warm-up
    (d) fit_schedule of EPOCHS distinct rates   wall time, against train_timed(EPOCHS) at a constant rate (wall time
                                                around it, and its device time)

Prints one JSON line.  Needs a GPU: nothing here falls back.

    python tools/hyper_cost.py [WORKLOAD] [SCALE] [K]
"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import mfsgd_amd as mf  # noqa: E402

RUNS, ROUTE_RUNS, EPOCHS = 9, 3, 10
A, B = (0.01, 0.05), (0.007, 0.02)


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

    def handle(lr, lam):
        m = mf.MatrixFactorizationSGD(w["U"], w["I"], k, lr, lam, 3, host_threads=16)
        m.set_ratings(u, i, r)
        return m

    m = handle(*A)
    m.init_factors()
    m.fit(1, rmse=False)
    info = m.schedule_info()
    # (a) every call changes both values, so every call re-bakes
    m.set_hyper(*B)
    a_runs = [timed(lambda x=x: m.set_hyper(*(A if x % 2 == 0 else B))) for x in range(RUNS)]
    m.set_hyper(*A)
    # (c) and the constant-rate side of (d)
    m.train_timed(2)
    t0 = time.perf_counter()
    device_ms, _ = m.train_timed(EPOCHS)
    const_wall = time.perf_counter() - t0
    epoch_ms = device_ms / EPOCHS
    # (d) EPOCHS distinct rates, no RMSE passes (train_timed has none either)
    rates = (0.01 * 0.9 ** np.arange(EPOCHS)).astype(np.float32)
    m.fit_schedule(rates[:2] * 1.5, rmse=False)  # warm-up
    sched_wall = timed(lambda: m.fit_schedule(rates, rmse=False))
    graphs = m.debug_counters()["graphs"]

    # (b) the route through a new handle
    def route(m_old, lr, lam):
        P, Q = m_old.get_factors()
        m_old.close()
        m_new = handle(lr, lam)
        m_new.set_factors(P, Q)
        return m_new

    b_runs = []
    for x in range(ROUTE_RUNS + 1):
        t0 = time.perf_counter()
        m = route(m, *(B if x % 2 == 0 else A))
        b_runs.append(time.perf_counter() - t0)
        m.fit(1, rmse=False)  # (the part goes to the device again: outside the timing)
    b_runs = b_runs[1:]
    build_s = m.schedule_info()["build_seconds"]
    m.close()
    a, b = float(np.median(a_runs)), float(np.median(b_runs))
    print(json.dumps(dict(
        workload=name, scale=scale, k=k, nnz=int(w["nnz"]), blocks=info["blocks"], waves=info["waves"], chunks=info["chunks"],
        total_steps=info["total_steps"], entry_records=info["total_steps"] * info["slots"], device_ingest=info["device_ingest"],
        set_hyper_ms=round(a * 1e3, 3), set_hyper_runs_ms=[round(t * 1e3, 3) for t in a_runs],
        rebuild_route_ms=round(b * 1e3, 3), rebuild_route_runs_ms=[round(t * 1e3, 3) for t in b_runs],
        rebuild_route_schedule_build_ms=round(build_s * 1e3, 3), epoch_device_ms=round(epoch_ms, 4),
        route_over_set_hyper=round(b / a, 2), set_hyper_in_epochs=round(a * 1e3 / epoch_ms, 3),
        rebake_bytes=24 * info["total_steps"] * info["slots"],
        rebake_gb_per_s_of_wall=round(24 * info["total_steps"] * info["slots"] / a / 1e9, 1),
        fit_schedule_10_rates_wall_ms=round(sched_wall * 1e3, 3), train_timed_10_wall_ms=round(const_wall * 1e3, 3),
        train_timed_10_device_ms=round(epoch_ms * EPOCHS, 3),
        per_change_ms=round((sched_wall - const_wall) * 1e3 / EPOCHS, 3), graphs=graphs)))


if __name__ == "__main__":
    main()
