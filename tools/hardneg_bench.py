"""What hard negatives cost and buy ("Hard negatives").

cfg2_ml20m (138 K users, 27 K items, k = 64); its 20 M pairs, shuffled once, are the positives and the seen-item index.
Wall times through the C-ABI from Python (host arrays in and out), each the median of RUNS rounds after a warm-up round:

    the call against its composition    sample_unseen_hard(u, m) for m = 1, 4, 8, 16, one row per positive, against what a
                                        host had to compose before: sample_unseen(u, m), predict on the n * m pairs, argmax
                                        on the host -- in the same process, and stopped if the two disagree on an item
    one fit_bpr epoch                   candidates = 1 (the uniform draw), then candidates = 4 with refresh = None and with
                                        refresh = 2^20, the steps of trainer.fit_bpr timed one by one: the picks (download
                                        included), the host's look for users without negatives, partial_fit_pairwise
    the planted problem                 tests/test_pairwise_gpu.py's: hit rate at 10 after 8 epochs, candidates 1 and 4

Prints one JSON line with all of it.  With `kernel` as the first argument it only makes one warm and one measured call per
m and prints the gather floor's bytes: the run to put under a kernel trace, which gives the kernel's own time.

    python tools/hardneg_bench.py [kernel] [WORKLOAD] [SCALE]
"""
import json
import sys
import time

import numpy as np

sys.path.insert(0, __file__.rsplit("/", 2)[0])
import mfsgd_amd as mf  # noqa: E402

RUNS = 2
MS = (1, 4, 8, 16)


def ms(t0):
    return (time.perf_counter() - t0) * 1e3


def median(times):
    return round(float(np.median(times[1:])), 3), [round(t, 3) for t in times[1:]]  # the first is the warm-up


def composed(m, u, per_row, seed, first):
    """The picks from public calls alone: every candidate comes down, goes up again as a pair, and its score comes down."""
    cand = m.sample_unseen(u, per_row, seed, first)
    sc = m.predict(np.repeat(u, per_row), cand.ravel()).reshape(cand.shape)
    d = np.argmax(sc, axis=1)  # (no NaN and nobody has seen everything here; the first of equal scores, as the rule has it)
    return cand[np.arange(u.size), d]


def call_against_composition(m, u, res):
    n = u.size
    for per_row in MS:
        hard, comp = [], []
        for run in range(RUNS + 1):
            t0 = time.perf_counter()
            got = m.sample_unseen_hard(u, per_row, 7, run * n * per_row)
            hard.append(ms(t0))
            t0 = time.perf_counter()
            want = composed(m, u, per_row, 7, run * n * per_row)
            comp.append(ms(t0))
            if not np.array_equal(got, want):
                sys.exit(f"m = {per_row}: the call and its composition disagree")
        a, b = median(hard), median(comp)
        res[f"hard_m{per_row}_ms"], res[f"hard_m{per_row}_runs_ms"] = a
        res[f"composed_m{per_row}_ms"], res[f"composed_m{per_row}_runs_ms"] = b
        res[f"composed_over_hard_m{per_row}"] = round(b[0] / a[0], 3)


def bpr_epochs(m, u, i, res):
    n = u.size
    for name, cands, refresh in (("uniform", 1, n), ("hard4", 4, n), ("hard4_refresh_2p20", 4, 1 << 20)):
        m.init_factors()
        steps = dict(pick=[], host=[], apply=[], epoch=[])
        for e in range(RUNS + 1):
            t = dict(pick=0.0, host=0.0, apply=0.0)
            t_epoch = time.perf_counter()
            for a in range(0, n, refresh):
                bu, bi = u[a:a + refresh], i[a:a + refresh]
                t0 = time.perf_counter()
                J = m.sample_unseen(bu, 1, 0, e * n + a)[:, 0] if cands == 1 else m.sample_unseen_hard(bu, cands, 0, (e * n + a) * cands)
                t["pick"] += ms(t0)
                t0 = time.perf_counter()
                assert J.min() >= 0  # (nobody has seen everything: nothing to filter)
                t["host"] += ms(t0)
                t0 = time.perf_counter()
                x = m.partial_fit_pairwise(bu, bi, J, margins=True)
                t["apply"] += ms(t0)
            steps["epoch"].append(ms(t_epoch))
            for step, v in t.items():
                steps[step].append(v)
        for step, times in steps.items():
            res[f"{name}_{step}_ms"], res[f"{name}_{step}_runs_ms"] = median(times)
        x = x.astype(np.float64)
        res[f"{name}_last_block_loss"] = round(float(np.logaddexp(0.0, -x).mean()), 6)


def planted(res):
    U, I, G, k, lr, lam, seed = 600, 400, 20, 16, 0.05, 0.01, 3
    rng = np.random.default_rng(0)
    per = I // G
    its = np.stack([(u % G) * per + rng.choice(per, 12, replace=False) for u in range(U)]).astype(np.int32)
    hu, hi = np.arange(U, dtype=np.int32), its[:, 0].copy()
    pu, pi = np.repeat(hu, 11), its[:, 1:].ravel().copy()
    for name, kw in (("uniform", {}), ("hard4", dict(candidates=4)), ("hard4_refresh_512", dict(candidates=4, refresh=512)),
                     ("hard8", dict(candidates=8)), ("hard8_refresh_512", dict(candidates=8, refresh=512))):
        with mf.MatrixFactorizationSGD(U, I, k, lr, lam, seed) as h:
            h.set_seen(np.concatenate([pu, hu]), np.concatenate([pi, hi]))
            h.init_factors()
            stats = h.fit_bpr(pu, pi, 8, seed=seed, **kw)
            res[f"planted_{name}_hit_rate_at_10_after_8"] = round(h.evaluate_ranking(hu, hi, 10, exclude="seen")["hit_rate"], 4)
            res[f"planted_{name}_loss"] = [round(float(stats["loss"][0]), 4), round(float(stats["loss"][-1]), 4)]


def main():
    args = sys.argv[1:]
    kernel_only = bool(args) and args[0] == "kernel"
    args = args[1:] if kernel_only else args
    name = args[0] if args else "cfg2_ml20m"
    scale = float(args[1]) if len(args) > 1 else 1.0
    w = mf.synth.workload(name, scale)
    U, I, k = int(w["U"]), int(w["I"]), int(w["k"])
    order = np.random.default_rng(0).permutation(len(w["u"]))
    u, i = np.ascontiguousarray(w["u"], np.int32)[order], np.ascontiguousarray(w["i"], np.int32)[order]
    n = u.size
    kp = 4 * (1 << max(0, (k + 3) // 4 - 1).bit_length())
    res = dict(workload=name, scale=scale, users=U, items=I, k=k, kp=kp, rows=int(n))
    with mf.MatrixFactorizationSGD(U, I, k, 0.01, 0.05, 3, host_threads=16) as m:
        m.set_seen(u, i)
        m.init_factors()
        if kernel_only:
            for per_row in MS:
                for run in range(2):
                    m.sample_unseen_hard(u, per_row, 7, run * n * per_row)
                res[f"gather_floor_bytes_m{per_row}"] = int(n) * per_row * 4 * kp
            print(json.dumps(res))
            return
        level = mf.debug_device_bytes()
        call_against_composition(m, u, res)
        assert mf.debug_device_bytes() == level
        bpr_epochs(m, u, i, res)
    planted(res)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
