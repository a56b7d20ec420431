"""Device memory has one owner type (csrc/devmem.hpp), which counts the bytes it holds: mfsgd_debug_device_bytes.
Whatever a handle allocates is back when it is closed, and a serving call keeps nothing -- on every route through
set_ratings (whole cells on the device, cut cells, the two-pass packer, the host packer behind the device sort,
partitioned handles).  The arrays of a device-packed schedule are counted from set_ratings on, while they wait for the
first compute call, the canonical order among them.  No call here fails on the device: the counter is compared before
and after calls that work."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LR, LAM = 0.01, 0.05
INVALID_ARG = -1


def _flags(mf):
    from mfsgd_amd import _lib

    return _lib


def test_a_life_cycle_returns_everything(mf):
    F = _flags(mf)
    w = mf.synth.workload("cfg1_ml100k", 1.0)
    live0 = mf.debug_device_bytes()
    with mf.MatrixFactorizationSGD(w["U"], w["I"], w["k"], LR, LAM, 7, flags=F.FLAG_DEVICE_INGEST) as m:
        m.set_ratings(w["u"], w["i"], w["r"])
        assert m.schedule_info()["device_ingest"] == 2  # whole cells, packed on the device
        m.init_factors()
        m.fit(2)
        m.rmse()
        order, _ = m.order()          # downloads after the packed arrays were handed to the handle
        assert np.array_equal(np.sort(order), np.arange(w["nnz"]))
        m.debug_schedule()
        assert mf.debug_device_bytes() > live0
        keep = np.arange(w["nnz"]) % 3 != 0
        m.set_ratings(w["u"][keep], w["i"][keep], w["r"][keep])  # drops the schedule and builds another
        assert m.debug_counters()["schedule_builds"] == 2
        m.init_factors(8)             # releases the device factors and the training graphs
        m.fit(1)
        assert mf.debug_device_bytes() > live0
    assert mf.debug_device_bytes() == live0


def test_packed_arrays_are_counted_while_they_wait(mf):
    """A device-packed schedule holds rows, entries, order and sub-cell tables in DevBufs of its own until the first
    compute call moves three of them on; the order (an int64 per rating) stays where it is."""
    F = _flags(mf)
    w = mf.synth.workload("cfg1_ml100k", 1.0)
    nnz = w["nnz"]
    keep = np.arange(nnz) % 3 != 0
    live0 = mf.debug_device_bytes()
    with mf.MatrixFactorizationSGD(w["U"], w["I"], w["k"], LR, LAM, 7, flags=F.FLAG_DEVICE_INGEST) as m:
        m.set_ratings(w["u"], w["i"], w["r"])
        assert m.schedule_info()["device_ingest"] == 2
        held = mf.debug_device_bytes()
        assert held >= live0 + 8 * nnz
        order0, _ = m.order()         # downloads from the schedule's own buffer
        assert np.array_equal(np.sort(order0), np.arange(nnz))
        assert mf.debug_device_bytes() == held
        # other ratings, then the first set again, still before any compute call: each schedule's arrays go with it
        m.set_ratings(w["u"][keep], w["i"][keep], w["r"][keep])
        assert mf.debug_device_bytes() <= held
        m.set_ratings(w["u"], w["i"], w["r"])
        assert m.debug_counters()["schedule_builds"] == 3
        assert mf.debug_device_bytes() <= held
        m.init_factors()
        m.fit(1)                      # rows, entries and tables move to the partition; the order does not
        order1, _ = m.order()
        assert np.array_equal(order1, order0)
    assert mf.debug_device_bytes() == live0


def _invalid(mf, call, text):
    live = mf.debug_device_bytes()
    with pytest.raises(mf.MfsgdError) as e:
        call()
    assert e.value.code == INVALID_ARG and text in str(e.value), str(e.value)
    assert mf.debug_device_bytes() == live


def test_serving_calls_keep_nothing(mf):
    from tests.test_fold_in_gpu import _csr

    rng = np.random.default_rng(31)
    U, I, k = 40, 700, 12
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    users = rng.integers(0, U, 25).astype(np.int32)
    eu = rng.integers(0, U, 3000).astype(np.int32)
    ei = rng.integers(0, I, 3000).astype(np.int32)
    # three upload batches (more than 2 x 2^22 ratings) and one user far longer than the rest
    lens = rng.integers(10, 51, 300_001)
    lens[100_000] = 200_000
    row_ptr, items, ratings = _csr(lens, I, rng)
    assert row_ptr[-1] > 2 * (1 << 22)
    live0 = mf.debug_device_bytes()
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 3) as m:
        m.set_factors(P, Q)
        m.predict(users, users)  # (the first compute call uploads the factors, which stay)
        held = mf.debug_device_bytes()
        assert held > live0

        def kept_nothing(call):
            out = call()
            assert mf.debug_device_bytes() == held
            return out

        kept_nothing(lambda: m.predict(users, rng.integers(0, I, users.size)))
        kept_nothing(lambda: m.recommend(users, 128))                      # fused
        kept_nothing(lambda: m.recommend(users, 129))                      # sort path
        kept_nothing(lambda: m.recommend(users, 129, exclude=(eu, ei)))
        rows = kept_nothing(lambda: m.fold_in(row_ptr, items, ratings, 1))
        assert np.isfinite(rows).all()
        kept_nothing(lambda: m.fold_in(row_ptr[:101], items[:row_ptr[100]], ratings[:row_ptr[100]], 0))
        kept_nothing(lambda: m.recommend_rows(rows[:30], 129, exclude=(eu[eu < 30], ei[eu < 30])))
        # rejected on the host, before any device work
        _invalid(mf, lambda: m.recommend(users, I + 1), "recommend: topn exceeds the number of items")
        _invalid(mf, lambda: m.recommend([0, U], 5), "recommend: user 1 out of range")
        _invalid(mf, lambda: m.recommend(users, 5, exclude=([0, 1], [3, I])), "recommend: excluded pair 1 out of range")
        _invalid(mf, lambda: m.fold_in([0, 2, 1], [0], [1.0], 1), "fold_in: row_ptr decreases at user 1")
        assert mf.debug_device_bytes() == held
    assert mf.debug_device_bytes() == live0


def test_cut_cells_two_pass_packer_and_host_packer_return_everything(mf, monkeypatch):
    from tests.dsgd_common import fuzz_chunked_cases

    F = _flags(mf)
    monkeypatch.delenv("MFSGD_PACK_TWICE", raising=False)

    def build(c, flags):
        live0 = mf.debug_device_bytes()
        with mf.MatrixFactorizationSGD(c["U"], c["I"], c["k"], LR, LAM, 5, blocks=c["blocks"], waves=c["waves"], flags=flags) as m:
            m.set_ratings(c["u"], c["i"], c["r"])
            info = m.schedule_info()
            if info["device_ingest"] == 2:  # packed on the device: the arrays wait in the schedule, counted
                assert mf.debug_device_bytes() >= live0 + 8 * len(c["u"])
        assert mf.debug_device_bytes() == live0
        return info

    for c in fuzz_chunked_cases(12, seed=515, max_ratings=9000):
        info = build(c, F.FLAG_DEVICE_INGEST)
        if info["device_ingest"] == 2 and info["split_cells"] > 0:
            break
    else:
        raise AssertionError("no case that the device packs with cut cells")
    monkeypatch.setenv("MFSGD_PACK_TWICE", "1")
    info = build(c, F.FLAG_DEVICE_INGEST)
    assert info["device_ingest"] == 2 and info["split_cells"] > 0
    monkeypatch.delenv("MFSGD_PACK_TWICE")
    # the host packs: the sorted indices come down and the pack state is dropped
    assert build(c, F.FLAG_DEVICE_INGEST | F.FLAG_HOST_PACK)["device_ingest"] == 1


def test_a_partitioned_handle_returns_everything(mf):
    import torch

    from tests.dsgd_common import SEED

    F = _flags(mf)
    w = mf.synth.workload("cfg1_ml100k", 0.2)
    dev = torch.device("cuda", 0)
    stream = torch.cuda.current_stream(dev).cuda_stream
    live0 = mf.debug_device_bytes()
    with mf.MatrixFactorizationSGD(w["U"], w["I"], w["k"], LR, LAM, SEED, n_parts=2, flags=F.FLAG_DEVICE_INGEST) as m:
        m.set_ratings(w["u"], w["i"], w["r"])  # (the ingest context forgets its triples between the partitions)
        m.init_factors()
        blocks = [torch.from_numpy(m.part_init_q(part, SEED, w["U"])).to(dev) for part in range(2)]  # torch's: not counted
        for part in range(2):
            m.part_train(part, blocks[part].data_ptr(), stream)
        for part in range(2):
            m.part_sync(part, stream)
        assert mf.debug_device_bytes() > live0
    assert mf.debug_device_bytes() == live0
    assert all(torch.isfinite(b).all() for b in blocks)
