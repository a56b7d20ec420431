"""The run loop and the general loop of the training kernels (csrc/run_asm.hpp, MFSGD_RUN_LOOP_ASM_TEXT and MFSGD_GEN_HALF)
issue all LDS reads of a step as ONE group behind the first DPP add: the rows of step t + 1 and the entry words of step
t + 2 are fetched earlier in step t than they used to be, and the counted waits rely on the order of issue.  Counted waits
and prefetch distances go wrong at short and odd trip counts, so these problems are small (fewer than 5000 ratings,
B = 4 .. 16, W = 2 and 4, k = 48, 64, 128, 256: L = 16 with padding, 16, 32, 64) and their schedules hold, between them,
sub-cells of 1, 2, 3, 4 and 5 general steps, run loops of 8, 10 and 12 steps (the shortest a schedule can hold; 2, 4 and 6
are driven directly: test_short_loops_driven_directly), forwarded q rows, idle run slots, p rows that recur at distance
two in a wave, and solo runs on both sides of the chain wave's steady body (n < 16 and n >= 32) -- asserted on the debug
schedule (test_the_cases_hold_every_form; the host packer needs no GPU, and `python -m tests.test_loop_groups_gpu` prints
the table).

Persistent and round-launch paths, 2 epochs, factors bit for bit (tobytes) against the oracle replaying the exported
order.  One case per L carries tests/edge_inputs.py's overflow ratings (+-3e38 at the end of the order): Inf and NaN in
the resident rows and the p rows of run steps whose idle slots are masked out of exec beside the moved reads; there the
NaN masks are equal and every other bit is."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests import edge_inputs as E
from tests.conftest import ROOT
from tests.test_chain_scale_edges_gpu import _bit_for_bit

pytestmark = pytest.mark.gpu

EPOCHS = 2
K_RUN_MIN = 8  # csrc/records.hpp: shortest item chain the packer keeps resident for a run


def _problem_mixed(U, I, n_hot, n_mid_items, n_mid, n_other, seed):
    """Item 0 rated by n_hot users (solo runs), items 1 .. n_mid_items by n_mid users each (chains too short for a solo
    run: run loops), n_other ratings of the remaining items (general steps)."""
    rng = np.random.default_rng(seed)
    u = [rng.choice(U, n_hot, replace=False)] + [rng.choice(U, n_mid, replace=False) for _ in range(n_mid_items)]
    i = [np.zeros(n_hot, np.int64)] + [np.full(n_mid, 1 + j, np.int64) for j in range(n_mid_items)]
    u.append(rng.integers(0, U, n_other))
    i.append(rng.integers(1 + n_mid_items, I, n_other))
    u, i = np.concatenate(u).astype(np.int64), np.concatenate(i)
    key = rng.permutation(np.unique(u * I + i))
    return U, I, (key // I).astype(np.int32), (key % I).astype(np.int32), (rng.random(key.size) * 4 + 1).astype(np.float32)


# name -> ((U, I, hot users, mid items, users per mid item, other ratings, seed), k, blocks, waves, overflow ratings)
CASES = {
    "k48_b8_w4": ((600, 60, 300, 8, 60, 2500, 0), 48, 8, 4, False),
    "k64_b4_w2": ((400, 40, 200, 6, 40, 1500, 1), 64, 4, 2, False),
    "k64_b16_w2": ((960, 60, 480, 6, 80, 2500, 0), 64, 16, 2, False),
    "k128_b8_w4": ((600, 60, 300, 8, 60, 2500, 0), 128, 8, 4, False),
    "k128_b6_w2": ((800, 60, 400, 8, 60, 2500, 0), 128, 6, 2, False),
    "k256_b16_w2": ((1400, 60, 700, 6, 80, 2500, 0), 256, 16, 2, False),
    "k256_b4_w4": ((600, 60, 300, 8, 60, 2000, 2), 256, 4, 4, False),
    "k64_b4_w2_overflow": ((400, 40, 200, 6, 40, 1500, 1), 64, 4, 2, True),
    "k128_b8_w4_overflow": ((600, 60, 300, 8, 60, 2500, 0), 128, 8, 4, True),
    "k256_b4_w4_overflow": ((600, 60, 300, 8, 60, 2000, 2), 256, 4, 4, True),
}
OVERFLOW_L = {"k64_b4_w2_overflow": 16, "k128_b8_w4_overflow": 32, "k256_b4_w4_overflow": 64}  # one per L, idle run slots in each


@functools.lru_cache(maxsize=None)
def _problem(args):
    return _problem_mixed(*args)


def forms(sched, W, G, L):
    """What the loops of a schedule run (layout: tests/kernel_emulator.py): the numbers of general steps and of run steps of
    its sub-cells, the lengths of its solo runs, and how many forwarded q rows, idle run slots and p rows recurring at
    distance two in a lane group its general and run steps hold."""
    cells, _, subs, entries = sched
    out = dict(gen=set(), run=set(), solo=set(), forwarded=0, idle=0, distance_two=0)
    for cell in range(cells.shape[0]):
        ent_off, nuni = int(cells[cell][1]), int(cells[cell][3])
        nrows = (nuni & 0xFFFF) + (nuni >> 16)
        if nrows == 0:
            continue
        for sw in range(W * W):
            off, n = (int(v) for v in subs[cell * W * W + sw])
            ng, nr, off, nsolo = n & 0xFFFF, n >> 16, off & 0xFFFF, off >> 16
            out["gen"].add(ng)
            out["run"].add(nr)
            out["solo"].add(nsolo)
            slots = entries[(ent_off + off) * G:(ent_off + off + ng + nr) * G, 0].reshape(ng + nr, G).astype(np.int64)
            p = (slots & 0xFFFF) // L
            flag = (slots >> 31) & 1
            out["forwarded"] += int(flag[1:ng].sum())
            out["idle"] += int(flag[ng:].sum())
            for part in (p[:ng], p[ng:]):  # real rows only: the idle slots' zero rows recur at every distance
                if part.shape[0] > 2:
                    out["distance_two"] += int(((part[2:] == part[:-2]) & (part[2:] < nrows)).sum())
    for key in ("gen", "run", "solo"):
        out[key].discard(0)
    return out


def _fit(mf, U, I, k, u, i, r, P0, Q0, blocks, waves, flags):
    with mf.MatrixFactorizationSGD(U, I, k, E.LR, E.LAM, 11, blocks=blocks, waves=waves, flags=flags) as m:
        m.set_ratings(u, i, r)
        m.set_factors(P0, Q0)
        got = []
        for _ in range(EPOCHS):
            rm = m.fit(1)
            got.append(m.get_factors() + (float(rm[0]),))
        return got, m.order()[0]


def _schedule(mf, name):
    args, k, blocks, waves, _ = CASES[name]
    U, I, u, i, r = _problem(args)
    with mf.MatrixFactorizationSGD(U, I, k, E.LR, E.LAM, 11, blocks=blocks, waves=waves) as m:
        m.set_ratings(u, i, r)
        info = m.schedule_info()
        return forms(m.debug_schedule(), info["waves"], info["slots"], info["group_lanes"]), m.order()[0], info


def _oracle_states(oracle, P0, Q0, u, i, r, order):
    P, Q = P0.copy(), Q0.copy()
    out = []
    for _ in range(EPOCHS):
        oracle.sgd_pass_ordered(P, Q, u, i, r, order, E.LR, E.LAM)
        out.append((P.copy(), Q.copy(), oracle.rmse(P, Q, u, i, r)))
    return out


def _same_but_for_the_nans(what, got, want):
    E.assert_same_but_for_the_nans(f"{what}: P", got[0], want[0])
    E.assert_same_but_for_the_nans(f"{what}: Q", got[1], want[1])
    E.assert_rmse_same_but_for_the_nans(got[2], want[2])


def test_the_cases_hold_every_form(mf):
    """On the debug schedules alone: the cases together contain every trip count and hazard the module docstring names."""
    gen, run, solo, forwarded, idle, distance_two = set(), set(), set(), 0, 0, 0
    for name in sorted(CASES):
        f, _, info = _schedule(mf, name)
        print(name, f, {key: info[key] for key in ("blocks", "waves", "slots", "group_lanes")})
        assert info["nnz"] < 5000 and 4 <= info["blocks"] <= 16
        gen |= f["gen"]
        run |= f["run"]
        solo |= f["solo"]
        forwarded, idle, distance_two = forwarded + f["forwarded"], idle + f["idle"], distance_two + f["distance_two"]
        if name in OVERFLOW_L:
            assert info["group_lanes"] == OVERFLOW_L[name] and f["run"] and f["idle"] >= 1, (name, f)
    assert {1, 2, 3, 4, 5} <= gen, sorted(gen)
    assert {8, 10, 12} <= run and min(run) == K_RUN_MIN, sorted(run)  # (2, 4, 6: test_short_loops_driven_directly)
    assert forwarded >= 1 and idle >= 1 and distance_two >= 1, (forwarded, idle, distance_two)
    assert min(solo) < 16 and max(solo) >= 32, sorted(solo)


@pytest.mark.parametrize("name", sorted(CASES))
def test_loops_bit_for_bit(mf, oracle, name):
    from mfsgd_amd import _lib

    args, k, blocks, waves, overflow = CASES[name]
    U, I, u, i, r = _problem(args)
    assert u.size < 5000 and E.host_keeps_subnormals()
    f, order0, info = _schedule(mf, name)
    assert f["gen"] and (f["run"] or f["solo"]), f
    if overflow:
        r = E.overflow_ratings("last_in_the_order", u, i, order0, None)
    P0, Q0 = E.ordinary_factors(U, I, k)
    seen = {}
    for path, flags in (("persistent", 0), ("round_launch", _lib.FLAG_ROUND_LAUNCH)):
        got, order = _fit(mf, U, I, k, u, i, r, P0, Q0, blocks, waves, flags)
        if order.tobytes() not in seen:
            seen[order.tobytes()] = _oracle_states(oracle, P0, Q0, u, i, r, order)
            if overflow:
                assert np.array_equal(order, order0)  # (the order depends on (u, i) only)
                E.check_overflow_case("last_in_the_order", seen[order.tobytes()])
            else:
                assert all(np.isfinite(P).all() and np.isfinite(Q).all() for P, Q, _ in seen[order.tobytes()])
        for epoch, (g, w) in enumerate(zip(got, seen[order.tobytes()])):
            (_same_but_for_the_nans if overflow else _bit_for_bit)(f"{name} {path} epoch {epoch + 1}", g, w)


@pytest.mark.parametrize("L", [16, 32, 64])
def test_short_loops_driven_directly(tmp_path, L):
    """Run loops of 2, 4 and 6 steps cannot occur in a schedule: an item's chain becomes a run only from kRunMin = 8
    ratings in a sub-cell (csrc/records.hpp), and a run is as long as its longest chain.  tools/ubench3 drives the loop
    itself (as tests/test_solo_chain_unrolled_gpu.py has it do for solo runs below the packer's threshold): the run loop at
    every even n = 2 .. 34 and the longest its LDS image holds, idle slots beside the live one, and the general loop at
    every n = 1 .. 33 and 64 with forwarded q rows and p rows at distance two -- every row against the host restatement."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / f"ub3_{L}")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-ffp-contract=off", f"-DLG={L}", "-w",
                    os.path.join(ROOT, "tools", "ubench3.hip"), "-o", exe], check=True)
    out = subprocess.run([exe, "loops"], check=True, stdout=subprocess.PIPE, text=True, timeout=120).stdout
    assert "  MISMATCH" not in out and "gave up" not in out, out  # (a step line ends in "  bit-exact" or "  MISMATCH")
    run = {int(line.split(" n=")[1].split(":")[0]) for line in out.splitlines() if "mode=3" in line and line.endswith("bit-exact")}
    assert run == set(range(2, 35, 2)) | {{16: 300, 32: 200, 64: 120}[L]}, sorted(run)
    assert " n=1..33 and 64: 34 bit-exact, 0 MISMATCH" in out, out
    flags, dist2 = (int(out.split(word)[0].split()[-1]) for word in (" forwarded-q flags", " p rows at distance two"))
    assert flags >= 1 and dist2 >= 1, out


if __name__ == "__main__":  # the table of forms per case, from the host packer
    import mfsgd_amd

    for case in sorted(CASES):
        print(case, _schedule(mfsgd_amd, case)[0])
