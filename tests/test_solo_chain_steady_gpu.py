"""The chain wave's loop of a solo run (csrc/run_asm.hpp, MFSGD_SOLO_CHAIN_ASM_TEXT) has two bodies: a steady body of
P steps in a straight line without exits, which runs while at least P steps remain, and the tail -- the four-pair loop
with an exit per step -- for the n < P steps behind it.  The hand-over between the two can go wrong at every remainder,
so the solo runs of these schedules cover them for P = 8 and P = 16 alike: every length 12..27 (tail only, exactly P,
P + every remainder, 2P, 2P + 1, 3P + remainders at P = 8; P, P + 1 at P = 16) at L = 16 and 32, 12..19 and 38..51 at
L = 64, and on an item with a tile of its own every residue modulo 8 between 55 and 70 -- factors bit for bit against
the oracle replaying the exported order.

tools/ubench3 drives the loop directly at every n = 1..33 (tests/test_solo_chain_unrolled_gpu.py::test_ubench3_host_check)."""
import functools

import pytest

from tests.test_gpu_parity import _run
from tests.test_solo_chain_unrolled_gpu import _hot_item_problem, _solo_lengths

pytestmark = pytest.mark.gpu

# B = 16, W = 2: the hot item's users per user bin -- the lengths of its solo runs (host scheduler, debug_schedule())
PROBLEM_A = (960, 60, 480, 3000, 0)    # k = 64, 128, 256: 12..19
PROBLEM_C = (1400, 60, 700, 3000, 2)   # k = 64, 128: 16, 17, 19..27; k = 256: 38, 40..43, 45..51
PROBLEM_LONE = (2048, 60, 1024, 3000, 1)  # k = 64: 55, 57, 59..70, the item in a tile of its own
C_AT_256 = {38, 40, 41, 42, 43, 45, 46, 47, 48, 49, 50, 51}


@functools.lru_cache(maxsize=None)
def _problem(args):
    return _hot_item_problem(*args)


@pytest.mark.parametrize("k", [64, 128, 256])  # L = 16, 32, 64
def test_hand_over_between_steady_body_and_tail_at_every_remainder(mf, oracle, k):
    from mfsgd_amd import _lib

    seen = {}
    for args in (PROBLEM_A, PROBLEM_C):
        U, I, u, i, r = _problem(args)
        assert u.size < 5000
        seen[args] = set()
        for flags in (0, _lib.FLAG_ROUND_LAUNCH):
            lengths, _ = _solo_lengths(mf, U, I, k, u, i, r, blocks=16, waves=2, flags=flags)
            seen[args] |= set(lengths)
            _run(mf, oracle, U, I, k, u, i, r, epochs=2, blocks=16, waves=2, flags=flags)
    print(f"k={k}: solo run lengths A {sorted(seen[PROBLEM_A])}, C {sorted(seen[PROBLEM_C])}")
    both = seen[PROBLEM_A] | seen[PROBLEM_C]
    if k == 256:
        assert set(range(12, 20)) <= seen[PROBLEM_A], sorted(seen[PROBLEM_A])
        assert C_AT_256 <= seen[PROBLEM_C], sorted(seen[PROBLEM_C])
    else:
        assert set(range(12, 28)) <= both, sorted(set(range(12, 28)) - both)


def test_lone_tile_row_posted_from_either_body(mf, oracle):
    """An item with a tile of its own on the persistent kernel: the chain wave posts the row from its registers behind
    the run, whichever body the run ends in -- the steady body (64 = 8 * 8 = 4 * 16 steps) or the tail at every
    remainder modulo 8."""
    U, I, u, i, r = _problem(PROBLEM_LONE)
    assert u.size < 5000
    lengths, cells = _solo_lengths(mf, U, I, 64, u, i, r, blocks=16, waves=2)
    assert int((cells[:, 5] & 1).sum()) == 16  # kCellLoneTile
    assert {63, 64, 65} <= set(lengths), sorted(set(lengths))
    assert {n % 8 for n in lengths} == set(range(8)), sorted(set(lengths))
    _, info = _run(mf, oracle, U, I, 64, u, i, r, seed=5, epochs=3, blocks=16, waves=2)
    assert info["split_cells"] == 0
