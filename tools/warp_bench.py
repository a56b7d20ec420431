"""What the early skip of mfsgd_sample_unseen_violating buys ("WARP").

cfg2_ml20m (138 K users, 27 K items, k = 64); its 20 M pairs, shuffled once, are the positives and the seen-item index.
The first 2^20 positives are the rows; m = 16 candidates each.  Two sets of factors: seeded, where nearly every first draw
violates the margin, and after EPOCHS epochs of fit_warp, where few draws do.  Under each, wall times through the C-ABI
from Python (host arrays in and out, every call ends in a synchronise):

    violating       sample_unseen_violating(u, i, m) with draws, margins and ranks: walks a row's candidates to the first
                    violator and skips the rest
    hard            sample_unseen_hard(u, m) with scores and draws, on the same build: always scores all m candidates
    violating_all   sample_unseen_violating with margin = -Inf: nothing violates, so all m candidates are scored and the
                    skip never fires -- the same kernel without its saving

The three are called in turn, ROUNDS rounds after a warm-up round, each round with counters of its own; medians and every
run are printed, with the share of rows that had a violator and the mean number of draws to it, as one JSON line.  With
`kernel` as the first argument it makes one warm and one measured call of each under both sets of factors and prints
the same line for one round: the run to put under a kernel trace, which gives the kernels' own times.  With `trace DIR`
it reads the kernel trace (csv) such a run left under DIR and prints the time of every dispatch of the two pick kernels
in the first and the last round of calls: 4 pieces of 2^18 rows per call, in the order violating, hard, violating_all.

    python tools/warp_bench.py [kernel] [WORKLOAD] [SCALE]
    python tools/warp_bench.py trace DIR
"""
import csv
import glob
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import mfsgd_amd as mf  # noqa: E402

ROUNDS, EPOCHS, M, MARGIN, ROWS, REFRESH = 7, 4, 16, 1.0, 1 << 20, 1 << 16
# A WARP step is up to L(n_items) = 10.8 times lr, and every step of a block is taken against picks made before the block:
# at lr = 0.05 or 0.005 with blocks of 2^20 the factors of this workload overflow within a few epochs.
LR, LAM = 0.002, 0.01


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


def median(times):
    return round(float(np.median(times[1:])), 3), [round(t, 3) for t in times[1:]]  # the first is the warm-up


def calls(m, u, i, tag, res, rounds):
    n = u.size
    t = dict(violating=[], hard=[], violating_all=[])
    for run in range(rounds + 1):
        first = run * n * M
        t0 = time.perf_counter()
        J, d, x, rk = m.sample_unseen_violating(u, i, M, MARGIN, 7, first, draws=True, margins=True, ranks=True)
        t["violating"].append(ms(t0))
        t0 = time.perf_counter()
        m.sample_unseen_hard(u, M, 7, first, scores=True, draws=True)
        t["hard"].append(ms(t0))
        t0 = time.perf_counter()
        none = m.sample_unseen_violating(u, i, M, -np.inf, 7, first, draws=True, margins=True, ranks=True)[0]
        t["violating_all"].append(ms(t0))
        assert (none == -1).all()
    hit = J >= 0
    res[f"{tag}_violating_share"] = round(float(hit.mean()), 4)
    res[f"{tag}_mean_draws_to_violator"] = round(float((d[hit] + 1).mean()), 3) if hit.any() else None
    res[f"{tag}_mean_candidates_examined"] = round(float(np.where(hit, d + 1, M).mean()), 3)
    for name, times in t.items():
        res[f"{tag}_{name}_ms"], res[f"{tag}_{name}_runs_ms"] = median(times)
    res[f"{tag}_hard_over_violating"] = round(res[f"{tag}_hard_ms"] / res[f"{tag}_violating_ms"], 3)


def trace(directory):
    path = glob.glob(directory + "/**/*kernel_trace.csv", recursive=True)[0]
    rows = sorted(csv.DictReader(open(path)), key=lambda r: int(r["Start_Timestamp"]))
    picks = [r for r in rows if "first_violating" in r["Kernel_Name"] or "hard_negative" in r["Kernel_Name"]]
    per_round = 3 * -(-ROWS * M // (1 << 22))  # three calls of four pieces (at most 2^22 candidates each)
    print("dispatches of the pick kernels:", len(picks))
    for tag, part in (("seeded", picks[:2 * per_round]), ("trained", picks[-2 * per_round:])):
        for r in part:
            name = "violating" if "first_violating" in r["Kernel_Name"] else "hard"
            print(tag, name, "us", (int(r["End_Timestamp"]) - int(r["Start_Timestamp"])) / 1e3)


def main():
    args = sys.argv[1:]
    if args and args[0] == "trace":
        return trace(args[1])
    kernel_only = bool(args) and args[0] == "kernel"
    args = args[1:] if kernel_only else args
    name = args[0] if args else "cfg2_ml20m"
    scale = float(args[1]) if len(args) > 1 else 1.0
    w = mf.synth.workload(name, scale)
    U, I, k = int(w["U"]), int(w["I"]), int(w["k"])
    order = np.random.default_rng(0).permutation(len(w["u"]))
    u, i = np.ascontiguousarray(w["u"], np.int32)[order], np.ascontiguousarray(w["i"], np.int32)[order]
    rows = min(ROWS, u.size)
    res = dict(workload=name, scale=scale, users=U, items=I, k=k, m=M, margin=MARGIN, lr=LR, lam=LAM, refresh=REFRESH, rows=int(rows),
               positives=int(u.size))
    rounds = 1 if kernel_only else ROUNDS
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 3, host_threads=16) as m:
        m.set_seen(u, i)
        m.init_factors()
        level = mf.debug_device_bytes()
        calls(m, u[:rows], i[:rows], "seeded", res, rounds)
        t0 = time.perf_counter()
        stats = m.fit_warp(u, i, EPOCHS, candidates=M, margin=MARGIN, refresh=REFRESH)
        res["fit_warp_epochs"], res["fit_warp_s"] = EPOCHS, round(ms(t0) / 1e3, 2)
        res["fit_warp_violating"] = np.round(stats["violating"], 4).tolist()
        res["fit_warp_trials"] = np.round(stats["trials"], 3).tolist()
        P, Q = m.get_factors()
        res["trained_nonfinite_factors"] = int((~np.isfinite(P)).sum() + (~np.isfinite(Q)).sum())
        res["trained_factors"] = "factors finite" if res["trained_nonfinite_factors"] == 0 else "factors overflowed"
        calls(m, u[:rows], i[:rows], "trained", res, rounds)
        assert mf.debug_device_bytes() == level
    print(json.dumps(res))


if __name__ == "__main__":
    main()
