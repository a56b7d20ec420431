"""The chain wave's loop of a solo run (csrc/run_asm.hpp, MFSGD_SOLO_CHAIN_ASM_TEXT) is a straight-line body of several
A/B pairs of steps with one forward exit per step, and its prologue takes the header's slots word as an operand and
loads the q row itself.  A body of eight steps can go wrong at its exits, so the solo runs of these schedules cover
every exit: every length 12..17 and 8m - 1, 8m, 8m + 1 for m = 8 -- factors bit for bit against the oracle replaying
the exported order.

Lengths 1..11 cannot occur in a schedule: the packer leaves a chain shorter than kSoloMin = 12 (csrc/records.hpp) to
the one-wave run loop.  They are covered where the loop is driven directly, by tools/ubench3's own host check
(test_ubench3_host_check below: every n = 1..33 and the two longest runs its LDS image holds, at each L)."""
import functools
import os
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT
from tests.test_gpu_parity import _run

pytestmark = pytest.mark.gpu

LR, LAM = 0.01, 0.05
K_SOLO_MIN = 12  # csrc/records.hpp: shortest chain the packer turns into a solo run
REQUIRED = set(range(1, 18)) | {63, 64, 65}  # 1..17, and 8m - 1, 8m, 8m + 1 at m = 8
NEVER_SOLO = set(range(1, K_SOLO_MIN))  # below the packer's own threshold (see the module docstring)


def _hot_item_problem(U, I, n_hot, n_other, seed):
    """Item 0 rated by n_hot distinct users drawn at random, n_other ratings of the other items: the users are dealt
    to the B * W user bins by their counts, so the bins hold varying numbers of the hot item's users -- the lengths of
    its solo runs."""
    rng = np.random.default_rng(seed)
    u = np.concatenate([rng.choice(U, n_hot, replace=False), rng.integers(0, U, n_other)]).astype(np.int64)
    i = np.concatenate([np.zeros(n_hot, np.int64), rng.integers(1, I, n_other)])
    key = rng.permutation(np.unique(u * I + i))
    return U, I, (key // I).astype(np.int32), (key % I).astype(np.int32), (rng.random(key.size) * 4 + 1).astype(np.float32)


@functools.lru_cache(maxsize=None)
def _problems():
    # (U, I, u, i, r) x 2, B = 16, W = 2: about 15 and about 64 of the hot item's users per user bin
    # (the second item has a tile of its own: its 1024 ratings exceed the packer's giant threshold at this size)
    return (_hot_item_problem(960, 60, 480, 3000, 0), _hot_item_problem(2048, 60, 1024, 3000, 1))


def _solo_lengths(mf, U, I, k, u, i, r, **kw):
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 3, **kw) as m:
        m.set_ratings(u, i, r)
        cells, _, subs, _ = m.debug_schedule()
    n = subs[:, 0] >> 16
    return [int(x) for x in n[n > 0]], cells


@pytest.mark.parametrize("k", [64, 100, 128, 256])  # L = 16, 32 with padding, 32, 64
def test_every_exit_of_the_unrolled_chain_loop(mf, oracle, k):
    from mfsgd_amd import _lib

    seen = set()
    for U, I, u, i, r in _problems():
        assert u.size < 5000
        for flags in (0, _lib.FLAG_ROUND_LAUNCH, _lib.FLAG_NO_SOLO):
            lengths, _ = _solo_lengths(mf, U, I, k, u, i, r, blocks=16, waves=2, flags=flags)
            assert (len(lengths) == 0) == (flags == _lib.FLAG_NO_SOLO), (flags, lengths)
            if flags == 0:
                seen |= set(lengths)
            _run(mf, oracle, U, I, k, u, i, r, epochs=2, blocks=16, waves=2, flags=flags)
    print(f"k={k}: solo run lengths {sorted(seen)}")
    assert min(seen) >= K_SOLO_MIN
    assert REQUIRED - NEVER_SOLO <= seen, sorted(REQUIRED - NEVER_SOLO - seen)


def test_lone_tile_hand_off_at_every_exit(mf, oracle):
    """An item with a tile of its own (test_lone_tile_mailbox_hand_off's shape: k = 64, B = 16, W = 2): the chain wave
    posts the row from its registers behind the run, whichever exit the run leaves by.  The item only gets its tile
    when its chain is what the epoch waits for (lpt_partition's giant threshold: about 800 ratings at this size, 50 a
    run), so per-cell runs of 7, 8 and 9 steps cannot be made; the runs here leave by the same three exits of the
    eight-step body -- 63, 64 and 65 steps, 7, 0 and 1 modulo 8 -- over 3 epochs."""
    U, I, u, i, r = _hot_item_problem(2400, 90, 1024, 4000, 1)
    lengths, cells = _solo_lengths(mf, U, I, 64, u, i, r, blocks=16, waves=2)
    n_lone = int((cells[:, 5] & 1).sum())
    assert n_lone >= 16 and n_lone % 16 == 0, n_lone
    assert {63, 64, 65} <= set(lengths), sorted(set(lengths))
    _, info = _run(mf, oracle, U, I, 64, u, i, r, seed=5, epochs=3, blocks=16, waves=2)
    assert info["split_cells"] == 0


@pytest.mark.parametrize("L", [16, 32, 64])
def test_ubench3_host_check(tmp_path, L):
    """tools/ubench3 drives the chain loop and its helper directly and compares every row with a host restatement of
    the arithmetic contract: bit-exact at every n = 1..33 and at the two longest runs its LDS image holds (300 and 299
    steps at L = 16), chain wave + helper."""
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    exe = str(tmp_path / f"ub3_{L}")
    subprocess.run([hipcc, "--offload-arch=gfx950", "-O2", "-ffp-contract=off", f"-DLG={L}", "-w",
                    os.path.join(ROOT, "tools", "ubench3.hip"), "-o", exe], check=True)
    out = subprocess.run([exe, "chain"], check=True, stdout=subprocess.PIPE, text=True, timeout=120).stdout
    longest = {16: 300, 32: 200, 64: 120}[L]
    assert "MISMATCH; chain alone" in out and "MISMATCH\n" not in out and "gave up" not in out, out
    assert " n=1..33: 33 bit-exact, 0 MISMATCH;" in out, out  # chain + helper against the host restatement
    checked = {int(line.split(" n=")[1].split(":")[0]) for line in out.splitlines() if line.endswith("bit-exact")}
    assert checked == {1, 2, 50, 51, longest - 1, longest}, sorted(checked)
