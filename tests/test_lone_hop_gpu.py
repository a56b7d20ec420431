"""The fast lane of the persistent kernel for a lone-tile cell (csrc/epoch.hip run_ring, csrc/cell.hpp lone_round0,
csrc/run_asm.hpp MFSGD_LONE_CHAIN_ASM_TEXT): a tile that is ONE item row, in a cell whose only work is ONE solo run in
sub-cell 0, is taken out of its mailbox by the chain wave itself, straight into the registers of the chain loop, with
everything that does not depend on the row's value done in front of the wait.  Every other cell -- a lone tile whose run
is too short to be a solo run, or is dealt to both sub-cells, the first round, a tile of two items -- goes the way it
went before.  Factors bit for bit and RMSE against the oracle replaying the exported order (tests/test_gpu_parity._run).

Which cells take the fast lane: the scheduler gives an item ALL its ratings in a cell's first sub-cell only when it is a
giant (schedule.cpp lpt_partition: at B = 8 and k = 64 about 380 ratings or more), and the packer builds a solo run from
kSoloMin = 12 steps up.  The run-length sweep therefore makes the item a giant and ONE block's run short (15 .. 33 steps)
for every length a solo run can have; lengths 1 .. 3 stay lone tiles on the old path.  The register start of the chain
loop at every n = 1..33 is driven directly by `tools/ubench3 lone` (modes 6 and 7)."""
import functools

import numpy as np
import pytest

from tests.test_gpu_parity import _run

pytestmark = pytest.mark.gpu

LR, LAM = 0.01, 0.05


@functools.lru_cache(maxsize=None)
def _problem(U, I, fill, seed):
    """test_lone_tile_mailbox_hand_off's problem: item 9 rated by every user, item 17 by every other user, fill * U
    random ratings on top."""
    rng = np.random.default_rng(seed)
    u = list(range(U)) + list(range(0, U, 2)) + list(rng.integers(0, U, fill * U))
    i = [9] * U + [17] * len(range(0, U, 2)) + list(rng.integers(0, I, fill * U))
    key = rng.permutation(np.unique(np.array(u) * I + np.array(i)))
    return U, I, (key // I).astype(np.int32), (key % I).astype(np.int32), (rng.random(key.size) * 4 + 1).astype(np.float32)


def _lone_cells(mf, U, I, k, u, i, r, B, **kw):
    """(number of cells marked lone, per-cell rating counts of the lone tiles' items read back from order / cell_ptr,
    lengths of all solo runs)."""
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 5, blocks=B, waves=2, **kw) as m:
        m.set_ratings(u, i, r)
        cells, _, subs, _ = m.debug_schedule()
        order, cell_ptr = m.order()
        assert m.schedule_info()["blocks"] == B
    runs = []
    for c in range(B * B):  # canonical order: rounds, then blocks; block b holds tile (b + round) % B
        rnd, b = divmod(c, B)
        if cells[b * B + (b + rnd) % B, 5] & 1:
            items = i[order[cell_ptr[c]:cell_ptr[c + 1]]]
            assert np.unique(items).size == 1
            runs.append(int(items.size))
    solo = subs[:, 0] >> 16
    return int((cells[:, 5] & 1).sum()), runs, [int(x) for x in solo[solo > 0]]


K_SOLO_MIN = 12  # csrc/records.hpp: shortest chain the packer turns into a solo run


@functools.lru_cache(maxsize=None)
def _giant_with_a_short_run(mf, m, B):
    """A GIANT lone item (all its ratings in sub-cell 0: the fast lane) whose run in ONE user block is m steps long.
    Users are dealt to blocks by their degrees alone, so: first every user rates item 9 (plus item 17 by every other user
    and random filler) and the users' blocks are read back from the exported order; then the raters of block 0 beyond
    its first m rate a stand-in item instead -- every user's degree, and with it every user's block, stays; item 9 keeps
    m ratings from block 0 and about 72 from each other block, far above the giant threshold (about 420 here)."""
    U, I, u, i, r = _problem(72 * B, 90, 2, 2000 + m)
    with mf.MatrixFactorizationSGD(U, I, 64, LR, LAM, 5, blocks=B, waves=2) as h:
        h.set_ratings(u, i, r)
        order, cell_ptr = h.order()
    block = np.full(U, -1)
    for c in range(B * B):  # canonical order: rounds, then blocks
        block[u[order[cell_ptr[c]:cell_ptr[c + 1]]]] = c % B
    in0 = np.flatnonzero((i == 9) & (block[u] == 0))
    assert in0.size > m, (in0.size, m)
    i = i.copy()
    for x in in0[m:]:  # a stand-in the user has not rated yet (keeps (user, item) pairs unique)
        mine = set(i[u == u[x]].tolist())
        i[x] = next(t for t in range(30, I) if t not in mine and t not in (9, 17))
    return U, I, u, i, r


# users per block of the lone item: below, at and above one steady pass of 16 steps, odd and even
@pytest.mark.parametrize("m", [1, 2, 3, 15, 16, 17, 31, 33, 70])
def test_run_length_sweep(mf, oracle, m):
    """m >= kSoloMin: the lone item is a giant and ONE block rates it m times -- a fast-lane cell whose chain loop is
    entered from the register start with n = m (tail only, one steady pass exactly, a pass plus a short tail, ...).
    m < kSoloMin: the packer never builds a solo run that short (the run loop takes it), so no cell of m steps can take
    the fast lane; those are lone tiles on the old path here (no filler: random filler takes a light item's lone tile
    away), and `tools/ubench3 lone` drives the register start at every n = 1..33."""
    B, k = 8, 64
    if m < K_SOLO_MIN:
        U, I, u, i, r = _problem(m * B, 90, 0, 1000 + m)
    elif m < 70:
        U, I, u, i, r = _giant_with_a_short_run(mf, m, B)
    else:
        U, I, u, i, r = _problem(m * B, 90, 6, 1000 + m)
    n_lone, runs, solo = _lone_cells(mf, U, I, k, u, i, r, B)
    assert n_lone >= B and n_lone % B == 0, n_lone
    assert m in runs, (m, sorted(set(runs)))
    if m >= K_SOLO_MIN:
        assert m in solo, sorted(set(solo))  # one solo run of m steps in sub-cell 0: the fast lane
    _, info = _run(mf, oracle, U, I, k, u, i, r, seed=5, epochs=3, blocks=B, waves=2)
    assert info["split_cells"] == 0


@pytest.mark.parametrize("k", [64, 100, 128, 256])  # L = 16, 32 with padding, 32, 64: 4 L granules, four per lane
def test_row_widths(mf, oracle, k):
    """Four epochs -- every epoch a launch, so the tags carry the launch generation -- in a graph replay and in eager
    launches, and one epoch alone; 150 ratings of the lone item per cell, one solo run each."""
    from mfsgd_amd import _lib

    B = 12
    U, I, u, i, r = _problem(150 * B, 90, 6, k + B)
    n_lone, runs, solo = _lone_cells(mf, U, I, k, u, i, r, B)
    assert n_lone >= B and n_lone % B == 0, n_lone
    assert 150 in runs and 150 in solo, (sorted(set(runs)), sorted(set(solo)))
    got = []
    for flags in (0, _lib.FLAG_NO_GRAPH):
        rm, info = _run(mf, oracle, U, I, k, u, i, r, seed=5, epochs=4, blocks=B, waves=2, flags=flags)
        assert info["split_cells"] == 0
        got.append(rm)
    assert np.array_equal(got[0], got[1])
    rm1, _ = _run(mf, oracle, U, I, k, u, i, r, seed=5, epochs=1, blocks=B, waves=2)
    assert rm1[0] == got[0][0]


def test_same_bits_with_the_mailbox_off(mf, oracle, monkeypatch):
    """The same problem scheduled without lone tiles (MFSGD_NO_MAILBOX): identical RMSE arrays and factors."""
    B, k = 12, 64
    U, I, u, i, r = _problem(150 * B, 90, 6, k + B)
    got = []
    for off in (False, True):
        if off:
            monkeypatch.setenv("MFSGD_NO_MAILBOX", "1")
        n_lone, _, _ = _lone_cells(mf, U, I, k, u, i, r, B)
        assert (n_lone == 0) if off else (n_lone >= B), (n_lone, off)
        with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 5, blocks=B, waves=2) as m:
            rm = m.train(u, i, r, 3)
            got.append((rm, *m.get_factors()))
    for a, b in zip(got[0], got[1]):
        assert np.array_equal(a, b)
    _run(mf, oracle, U, I, k, u, i, r, seed=5, epochs=3, blocks=B, waves=2)  # ... and they are the oracle's


def test_cells_off_the_fast_lane_go_the_old_way(mf, oracle):
    """A tile of two items that looks lone cell by cell, and a scaled cfg2 (split cells, general and run steps beside the
    solo runs): bit-exact as before."""
    from tests.test_schedule_cpu import _two_items_one_tile

    U, I, u, i, r = _two_items_one_tile()
    _run(mf, oracle, U, I, 64, u, i, r, epochs=3, blocks=2, waves=2)
    w = mf.synth.workload("cfg2_ml20m", 0.05)
    _run(mf, oracle, w["U"], w["I"], w["k"], w["u"], w["i"], w["r"], epochs=2, waves=2)
