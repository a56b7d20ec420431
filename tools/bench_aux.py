"""Timings of the paths around training: predict (batched), recommend (top-N, and top-N that leaves out
the whole rating set), fold-in of users against the trained item factors and top-N for the folded rows, RMSE pass,
set_ratings (schedule build), held-out validation RMSE and early stopping on it, online updates of a live model.  Wall-clock, through the C-ABI (host
arrays in and out, so PCIe copies are included); run it under `rocprofv3 --kernel-trace --stats` for the kernel times.

    python tools/bench_aux.py [WORKLOAD] [SCALE] [validation]      (validation: that leg alone)
    python tools/bench_aux.py [WORKLOAD] [SCALE] online [N ...]    (the online leg alone; batch sizes, default 2^10 2^16 2^20)
"""
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import mfsgd_amd as mf  # noqa: E402


def _median_ms(f, reps=5):
    f()  # warm-up
    t = []
    for _ in range(reps):
        t0 = time.perf_counter()
        f()
        t.append(time.perf_counter() - t0)
    return float(np.median(t)) * 1e3


def validation_leg(m, w, n_held=2_000_000, epochs=10):
    """Held-out RMSE of n_held pairs drawn from the workload's id ranges, on a model that has trained: (a) the set kept
    on the device against predict() of the same pairs plus numpy; (b) early stopping that never stops against fit() of
    as many epochs.  Medians of 5 after a warm-up.  (c), the kernels alone, is the kernel trace of this run:
    pairs_sse_kernel against predict_kernel, which gathers the same rows of the same pairs."""
    rng = np.random.default_rng(17)
    hu = rng.integers(0, w["U"], n_held).astype(np.int32)
    hi = rng.integers(0, w["I"], n_held).astype(np.int32)
    hr = (rng.integers(1, 11, n_held) * 0.5).astype(np.float32)
    m.set_validation(hu, hi, hr)
    got = m.validation_rmse()

    def by_predict():
        e = hr - m.predict(hu, hi)
        return float(np.sqrt(np.mean(e.astype(np.float64) ** 2)))

    want = by_predict()
    t_val = _median_ms(m.validation_rmse)
    t_on = _median_ms(lambda: m.rmse_on(hu, hi, hr))
    t_pred = _median_ms(by_predict)
    t_fit = _median_ms(lambda: m.fit(epochs, rmse=False))
    t_es = _median_ms(lambda: m.fit_early_stopping(epochs, patience=epochs + 1))
    t_es_plain = _median_ms(lambda: m.fit_early_stopping(epochs, patience=epochs + 1, restore_best=False))
    print(f"  validation, {n_held} held-out pairs: rmse {got:.6f} (predict + numpy: {want:.6f})")
    print(f"    (a) validation_rmse(), set on the device  {t_val:9.3f} ms  = {n_held / t_val / 1e6:.2f} G pairs/s")
    print(f"        rmse_on(u, i, r), pairs from the host  {t_on:9.3f} ms")
    print(f"        predict(u, i) + numpy RMSE             {t_pred:9.3f} ms  = {t_pred / t_val:.1f} x validation_rmse()")
    print(f"    (b) fit({epochs})                                {t_fit:9.3f} ms  = {t_fit / epochs:.3f} ms per epoch")
    print(f"        fit_early_stopping({epochs}), never stops     {t_es:9.3f} ms  = +{(t_es - t_fit) / epochs:.3f} ms per epoch "
          f"(+{(t_es - t_fit) / t_fit * 100:.1f} % of the epoch)")
    print(f"        ... with restore_best=False            {t_es_plain:9.3f} ms  = +{(t_es_plain - t_fit) / epochs:.3f} ms per epoch "
          f"(+{(t_es_plain - t_fit) / t_fit * 100:.1f} %)")
    m.set_validation([], [], [])


def online_leg(m, w, sizes=(1 << 10, 1 << 16, 1 << 20)):
    """partial_fit of batches drawn from the workload's own ratings (so users and items come with the workload's
    frequencies), on a model that holds the workload and has trained: host levelling alone (online_levels), the whole
    call with the errors coming back, and what the call leaves for upload, kernels and download; against the only
    route there was before -- set_ratings(batch), fit(1), set_ratings(workload) -- which also applies the batch in the
    scheduler's order, not the given one.  Medians of 5 after a warm-up; the kernels alone (apply_levels_kernel) are
    the kernel trace of this run with one batch size: total time / 6 calls."""
    rng = np.random.default_rng(23)
    print(f"  online updates: batch | levels | widest | launches | levelling ms | partial_fit ms | rest ms | "
          f"old route ms (set batch + fit(1) + set workload)")
    for n in sizes:
        at = rng.integers(0, w["nnz"], n)
        bu, bi, br = w["u"][at].astype(np.int32), w["i"][at].astype(np.int32), w["r"][at].astype(np.float32)
        info = m.partial_fit(bu, bi, br, info=True)
        t_lv = _median_ms(lambda: m.online_levels(bu, bi))
        t_pf = _median_ms(lambda: m.partial_fit(bu, bi, br, errors=True))

        def old_route():
            t0 = time.perf_counter()
            m.set_ratings(bu, bi, br)
            t1 = time.perf_counter()
            m.fit(1, rmse=False)
            t2 = time.perf_counter()
            m.set_ratings(w["u"], w["i"], w["r"])
            return np.array([t1 - t0, t2 - t1, time.perf_counter() - t2]) * 1e3

        old_route()
        parts = np.median([old_route() for _ in range(3)], axis=0)
        print(f"    {n:8d} | {info['levels']:6d} | {info['max_width']:7d} | {info['launches']:6d} | {t_lv:9.3f} | {t_pf:9.3f} | "
              f"{t_pf - t_lv:9.3f} | {parts.sum():9.1f} ({parts[0]:.1f} + {parts[1]:.1f} + {parts[2]:.1f})")


name = sys.argv[1] if len(sys.argv) > 1 else "cfg2_ml20m"
scale = float(sys.argv[2]) if len(sys.argv) > 2 else 1.0
w = mf.synth.workload(name, scale)
k = w["k"]
if len(sys.argv) > 3 and sys.argv[3] == "validation":
    with mf.MatrixFactorizationSGD(w["U"], w["I"], k, 0.01, 0.05, 3, host_threads=16) as m:
        m.set_ratings(w["u"], w["i"], w["r"])
        m.init_factors()
        m.fit(1, rmse=False)
        print(f"{name} x{scale}: {w['nnz']} ratings, {w['U']} x {w['I']}, k = {k}")
        validation_leg(m, w)
    sys.exit(0)
if len(sys.argv) > 3 and sys.argv[3] == "online":
    with mf.MatrixFactorizationSGD(w["U"], w["I"], k, 0.01, 0.05, 3, host_threads=16) as m:
        m.set_ratings(w["u"], w["i"], w["r"])
        m.init_factors()
        m.fit(1, rmse=False)
        print(f"{name} x{scale}: {w['nnz']} ratings, {w['U']} x {w['I']}, k = {k}")
        online_leg(m, w, *([tuple(int(x) for x in sys.argv[4:])] if len(sys.argv) > 4 else []))
    sys.exit(0)
with mf.MatrixFactorizationSGD(w["U"], w["I"], k, 0.01, 0.05, 3, host_threads=16) as m:
    t0 = time.perf_counter()
    m.set_ratings(w["u"], w["i"], w["r"])
    t_set = time.perf_counter() - t0
    m.init_factors()
    m.fit(1, rmse=False)
    m.rmse()
    t0 = time.perf_counter()
    for _ in range(5):
        m.rmse()
    t_rmse = (time.perf_counter() - t0) / 5
    n = w["nnz"]
    m.predict(w["u"][:1000], w["i"][:1000])
    t0 = time.perf_counter()
    out = m.predict(w["u"], w["i"])
    t_pred = time.perf_counter() - t0
    users = np.arange(0, w["U"], max(1, w["U"] // 4096), dtype=np.int32)[:4096]
    m.recommend(users[:16], 10)
    t0 = time.perf_counter()
    items, scores = m.recommend(users, 10)
    t_rec = time.perf_counter() - t0
    m.recommend(users[:16], 10, exclude=(w["u"][:1000], w["i"][:1000]))
    t0 = time.perf_counter()
    items_x, scores_x = m.recommend(users, 10, exclude=(w["u"], w["i"]))
    t_rec_x = time.perf_counter() - t0
    # fold-in: the same users' own lists (in the workload's order) as if they were new, 10 epochs from seeded rows
    mine = np.flatnonzero(np.isin(w["u"], users))
    mine = mine[np.argsort(w["u"][mine], kind="stable")]
    lens = np.bincount(w["u"][mine], minlength=w["U"])[users]
    row_ptr = np.concatenate([[0], np.cumsum(lens)]).astype(np.int64)
    f_items, f_ratings = w["i"][mine].astype(np.int32), w["r"][mine].astype(np.float32)
    fold_epochs = 10
    m.fold_in(row_ptr[:17], f_items[:row_ptr[16]], f_ratings[:row_ptr[16]], 1)
    t0 = time.perf_counter()
    rows = m.fold_in(row_ptr, f_items, f_ratings, fold_epochs)
    t_fold = time.perf_counter() - t0
    f_rows = np.repeat(np.arange(users.size, dtype=np.int32), lens).astype(np.int32)
    m.recommend_rows(rows[:16], 10)
    t0 = time.perf_counter()
    items_r, scores_r = m.recommend_rows(rows, 10, exclude=(f_rows, f_items))
    t_rec_r = time.perf_counter() - t0
    print(f"{name} x{scale}: validation leg (the model has trained one epoch)")
    validation_leg(m, w)
    online_leg(m, w)
kept = int(np.isin(w["u"], users).sum())
print(f"{name} x{scale}: {n} ratings, {w['U']} x {w['I']}, k = {k}")
print(f"  set_ratings (schedule build + ingest)  {t_set * 1e3:9.1f} ms")
print(f"  rmse pass                              {t_rmse * 1e3:9.3f} ms  = {n / t_rmse / 1e9:.2f} G ratings/s")
print(f"  predict, {n} pairs (host in/out)   {t_pred * 1e3:9.1f} ms  = {n / t_pred / 1e9:.3f} G pairs/s")
print(f"  recommend top-10, {users.size} users x {w['I']} items {t_rec * 1e3:9.1f} ms  = "
      f"{users.size * w['I'] / t_rec / 1e9:.2f} G scores/s")
print(f"  recommend top-10 excluding all {n} ratings ({kept} are the requested users'), same users "
      f"{t_rec_x * 1e3:9.1f} ms")
n_fold = int(row_ptr[-1])
print(f"  fold-in, {users.size} users, {n_fold} ratings (longest {int(lens.max())}), {fold_epochs} epochs {t_fold * 1e3:9.1f} ms  = "
      f"{n_fold * fold_epochs / t_fold / 1e9:.3f} G updates/s (rmse pass: {n / t_rmse / 1e9:.2f} G ratings/s)")
print(f"    chain bound: {int(lens.max())} x {fold_epochs} steps x 85 cycles at 2.07 GHz = "
      f"{int(lens.max()) * fold_epochs * 85 / 2.07e9 * 1e3:.3f} ms for the slowest wave")
print(f"  recommend_rows top-10 of the folded rows, excluding their {n_fold} ratings {t_rec_r * 1e3:9.1f} ms")
