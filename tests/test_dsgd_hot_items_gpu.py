"""Hot items under partitioned handles: the shape DSGD is designed for -- mfsgd_dsgd_plan deals the heaviest items one per
partition, so every partition's epoch is its giant's chain: a lone-tile cell per block, one solo run each, the row hopping
from workgroup to workgroup through the mailbox of that partition (csrc/epoch.hip run_ring), its generation word in that
partition's d_sync, the first round taking the row from a caller-owned block and the last one storing it there, the graph
cache keyed by the block's address.  Every other test with n_parts > 1 meets such cells by chance, if at all.

Items 9 and 17 (rated by every user / every other user) lie once in different partitions (the plan) and once in the same.
What each (handle, partition) schedule holds is asserted from debug_schedule; P, the Q blocks and the SSE trajectory are
compared bit for bit (SSE to 1e-9) with the sequential DSGD definition run by the oracle over global factors, in the
orders the handles export.  A mailbox or a generation word shared between two partitions, or a row carried from one block
into the next launch on another block, shows as a Q block (and then P) that differs from the oracle's: the hopping row
IS item 9's row of that block -- test_two_blocks_alternating_on_one_partition trains the same partition on two blocks
with different rows in turn, every launch a generation of its own."""
import numpy as np
import pytest

from tests import dsgd_common as D

pytestmark = pytest.mark.gpu

EPOCHS = 3
STAGES = ((0.01, 0.05), (0.006, 0.02))  # test_hyper_gpu.test_dsgd_partitions_follow's


# (lone-tile cells, solo runs) of every partition, per handle: read off the host scheduler at these shapes (it needs no
# GPU) and pinned.  "whole": ONE handle holds every user (the native ring at world = 1); "virtual": G handles, a user
# range each.  Item 9, rated by every user of a handle, has a tile of its own and one solo run per block everywhere; item
# 17, rated by every other user, has them too where the handle holds every user at k = 64 and 256 (a giant: all its
# ratings in a cell's first sub-cell) and plain solo runs elsewhere; a partition with neither has none.
FORMS = {
    ("k64", "apart", "whole"): [[(8, 8), (8, 8)]],
    ("k64", "apart", "virtual"): [[(8, 8), (0, 16)], [(8, 8), (0, 16)]],
    ("k64", "together", "whole"): [[(0, 0), (16, 16)]],
    ("k64", "together", "virtual"): [[(0, 0), (8, 24)], [(0, 0), (8, 24)]],
    ("k128", "apart", "whole"): [[(6, 6), (6, 6), (0, 0)]],
    ("k128", "apart", "virtual"): [[(6, 6), (0, 10), (0, 0)], [(6, 6), (0, 8), (0, 0)], [(6, 6), (0, 10), (0, 0)]],
    ("k128", "together", "whole"): [[(6, 18), (0, 0), (0, 0)]],
    ("k128", "together", "virtual"): [[(6, 15), (0, 0), (0, 0)], [(6, 16), (0, 0), (0, 0)], [(6, 15), (0, 0), (0, 0)]],
    ("k256", "apart", "whole"): [[(12, 12), (12, 12)]],
    ("k256", "apart", "virtual"): [[(12, 12), (0, 18)], [(12, 12), (0, 15)]],
    ("k256", "together", "whole"): [[(0, 0), (24, 24)]],
    ("k256", "together", "virtual"): [[(0, 0), (12, 31)], [(0, 0), (12, 31)]],
}


def _check_schedules(trainers, shape, how, kind):
    got = [[D.lone_and_solo(t, part) for part in range(t.n_parts)] for t in trainers]
    print(f"{shape} {how} {kind}: (lone cells, solo runs) per handle and partition {got}")
    assert got == FORMS[(shape, how, kind)], (got, FORMS[(shape, how, kind)])


def _virtual(mf, oracle, shape, how, stages=None, two_blocks=False, **kw):
    """G virtual devices (test_gpu_parity._virtual_dsgd's pattern): G handles each holding a user range, blocks rotated by
    pointer, all on one stream, EPOCHS epochs.  stages: ((lr, lambda) of epoch 1, of the epochs after it), changed with
    set_hyper.  two_blocks: every (device, partition) sub-epoch trains the partition on block A and then on block B (seeded
    differently); the oracle runs the same sequence over QA and QB."""
    import torch

    k, B, G, U, I, u, i, r = D.hot_items_problem(shape)
    ip = D.hot_item_map(mf, how, U, I, u, i, G)
    ub, _, sel = D.plan_shards(mf, U, I, u, i, G)
    lr0, lam0 = stages[0] if stages else (D.LR, D.LAM)
    trainers = [D.plan_trainer(mf, g, ub, ip, sel, I, k, u, i, r, G, lr=lr0, lam=lam0, blocks=B, waves=2, **kw) for g in range(G)]
    try:
        _check_schedules(trainers, shape, how, "virtual")
        dev = torch.device("cuda", 0)
        seeds = (D.SEED, D.SEED + 1) if two_blocks else (D.SEED,)
        blocks = [[torch.from_numpy(trainers[0].part_init_q(part, seed, U)).to(dev) for part in range(G)] for seed in seeds]
        stream = torch.cuda.current_stream(dev).cuda_stream
        P = oracle.init_factors(U, I, k, D.SEED)[0]
        Qs = [oracle.init_factors(U, I, k, seed)[1] for seed in seeds]
        orders = {(g, part): sel[g][trainers[g].order(part)[0]] for g in range(G) for part in range(G)}
        for epoch in range(EPOCHS):
            lr, lam = (stages[min(epoch, 1)] if stages else (D.LR, D.LAM))
            if stages and epoch == 1:
                torch.cuda.synchronize()
                for t in trainers:
                    t.set_hyper(lr, lam)
                _check_schedules(trainers, shape, how, "virtual")  # (the re-bake leaves the structure alone)
            for s in range(G):
                for g in range(G):
                    part = (g + s) % G
                    for blk, Q in zip(blocks, Qs):
                        trainers[g].part_train(part, blk[part].data_ptr(), stream)
                        if orders[(g, part)].size:
                            oracle.sgd_pass_ordered(P, Q, u, i, r, orders[(g, part)], lr, lam)
            torch.cuda.synchronize()
            for blk, Q in zip(blocks, Qs):
                sse = sum(trainers[g].part_sse((g + s) % G, blk[(g + s) % G].data_ptr(), stream) for s in range(G) for g in range(G))
                np.testing.assert_allclose(sse, oracle.sse(P, Q, u, i, r), rtol=1e-9, err_msg=f"SSE after epoch {epoch + 1}")
                got = D.assemble_q_plan({p: blk[p].cpu().numpy() for p in range(G)}, ip, I, k)
                assert np.array_equal(got, Q), f"epoch {epoch + 1}: Q rows {np.flatnonzero((got != Q).any(axis=1))[:8]} differ"
            gotP = np.concatenate([t.get_factors()[0] for t in trainers])
            assert np.array_equal(gotP, P), f"epoch {epoch + 1}: P rows {np.flatnonzero((gotP != P).any(axis=1))[:8]} differ"
    finally:
        for t in trainers:
            t.close()


CASES = [(shape, how) for shape in sorted(D.HOT_SHAPES) for how in ("apart", "together")]


@pytest.mark.parametrize("shape,how", CASES)
def test_virtual_devices(mf, oracle, shape, how):
    _virtual(mf, oracle, shape, how)


@pytest.mark.parametrize("shape,how", CASES)
def test_virtual_devices_eager_launches(mf, oracle, shape, how):
    """The same without the graph cache (every sub-epoch an eager launch)."""
    from mfsgd_amd import _lib

    _virtual(mf, oracle, shape, how, flags=_lib.FLAG_NO_GRAPH)


@pytest.mark.parametrize("shape,how", CASES)
def test_set_hyper_between_epochs(mf, oracle, shape, how):
    """The solo records' lr * r words are re-baked in partitions that have lone tiles."""
    _virtual(mf, oracle, shape, how, stages=STAGES)


@pytest.mark.parametrize("shape,how", CASES)
def test_two_blocks_alternating_on_one_partition(mf, oracle, shape, how):
    """The mailbox of a partition must not carry a row from one block into the launch on the other: the same partition
    of one handle trains on two blocks in turn, two cached graphs, every launch a generation of its own."""
    _virtual(mf, oracle, shape, how, two_blocks=True)


@pytest.mark.parametrize("how", ("apart", "together"))
@pytest.mark.parametrize("shape,nan_block", [("k64", False), ("k128", False), ("k64", True)])
def test_native_ring_world1(mf, oracle, shape, how, nan_block):
    """mfsgd_dsgd at world = 1 (m = 2 at k = 64, m = 3 at k = 128): ONE handle holds every user, the block addresses rotate
    through the graph cache and every sub-epoch is a launch of that partition with its own generation.  nan_block: one
    element of item 9's row, given through mfsgd_dsgd_set_q, is the NaN whose bits are all ones (a solo record's empty
    mailbox word, csrc/records.hpp): NaN exactly where the oracle has NaN, after each epoch."""
    from mfsgd_amd.dsgd import NativeDSGD
    from tests import edge_inputs as E

    k, B, G, U, I, u, i, r = D.hot_items_problem(shape)
    ip = D.hot_item_map(mf, how, U, I, u, i, G)
    Po, Qo = oracle.init_factors(U, I, k, D.SEED)
    got = []
    with mf.MatrixFactorizationSGD(U, I, k, D.LR, D.LAM, D.SEED, n_parts=G, blocks=B, waves=2) as t:
        t.set_item_partition(ip)
        t.set_ratings(u, i, r)
        t.init_p_offset(D.SEED, 0)
        _check_schedules([t], shape, how, "whole")
        orders = [t.order(p)[0] for p in range(G)]
        with NativeDSGD(t, 0, 1, NativeDSGD.unique_id()) as d:
            assert d.m == G
            d.init_q(D.SEED, U)
            if nan_block:
                part = int(ip[D.HOT_A])
                blk = d.home_blocks()[part]
                row = int(np.flatnonzero(np.flatnonzero(ip == part) == D.HOT_A)[0])
                assert np.array_equal(blk[row], Qo[D.HOT_A])
                blk[row, k // 2] = Qo[D.HOT_A, k // 2] = E.ALL_ONES_NAN
                d.set_block(part, blk)
            for _ in range(EPOCHS):
                rm = d.train(1)
                got.append((t.get_factors()[0], D.assemble_q_plan(d.home_blocks(), ip, I, k), float(rm[0])))
    for epoch, (P, Q, rm) in enumerate(got):
        for p in range(G):
            oracle.sgd_pass_ordered(Po, Qo, u, i, r, orders[p], D.LR, D.LAM)
        E.assert_same_but_for_the_nans(f"P after epoch {epoch + 1}", P, Po)
        E.assert_same_but_for_the_nans(f"Q after epoch {epoch + 1}", Q, Qo)
        E.assert_rmse_same_but_for_the_nans(rm, oracle.rmse(Po, Qo, u, i, r))
        assert np.isnan(Po).any() == nan_block and (not nan_block or np.isnan(rm))


def test_two_processes_over_shared_memory(mf, oracle, tmp_path):
    """test_native_dsgd_multi_process_shm at world = 2, m = 1 on the hot-item set: two real processes, a user range each,
    the blocks through the shared-memory rehearsal transport (round launches: the ranks share the GPU).  Each rank's
    partition of item 9 holds a lone-tile cell and a solo run per block."""
    from tests.test_gpu_parity import _multi_process_shm

    forms = _multi_process_shm(mf, oracle, tmp_path, 2, 1, "hot_items")
    k, B, G, U, I, u, i, r = D.hot_items_problem("k64")
    ip = D.hot_item_map(mf, "apart", U, I, u, i, 2)
    print(forms)
    for rank in range(2):
        assert forms[rank][int(ip[D.HOT_A])] == (B, B) and forms[rank][int(ip[D.HOT_B])][1] >= B, forms
