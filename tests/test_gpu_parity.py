"""Parity of the HIP path (through the C-ABI) against the CPU oracle executing
the same schedule sequentially.  The fp32 arithmetic is specified operation by
operation, so the bar is BIT-EXACT factors; RMSE is
compared to 1e-9 relative (only the fp64 accumulation order differs).
BASELINE.json's stated tolerance -- RMSE trajectory within 1e-5 -- is therefore
met with orders of magnitude to spare, and is also asserted explicitly.

PARITY UNPINNED: the reference holds no code or vectors
(/root/reference/README.md:1-2); "oracle" is this repository's own restatement
(oracle/mfsgd_oracle.c), pinned only by the JDK's java.util.Random
specification and a hand-computed known answer (tests/test_oracle.py)."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

LR, LAM = 0.01, 0.05
RMSE_TOL = 1e-5  # BASELINE.json: "RMSE within 1e-5 of the reference"


def _oracle_train(oracle, U, I, k, u, i, r, order, seed, epochs, lr=LR, lam=LAM):
    P, Q = oracle.init_factors(U, I, k, seed)
    rm = []
    for _ in range(epochs):
        oracle.sgd_pass_ordered(P, Q, u, i, r, order, lr, lam)
        rm.append(oracle.rmse(P, Q, u, i, r))
    return P, Q, np.array(rm)


def _run(mf, oracle, U, I, k, u, i, r, seed=11, epochs=3, lr=LR, lam=LAM, **kw):
    u = np.asarray(u, np.int32)
    i = np.asarray(i, np.int32)
    r = np.asarray(r, np.float32)
    with mf.MatrixFactorizationSGD(U, I, k, lr, lam, seed, **kw) as m:
        rm = m.train(u, i, r, epochs)
        P, Q = m.get_factors()
        order, cell_ptr = m.order()
        info = m.schedule_info()
        rm_again = m.rmse()
    assert oracle.check_block_schedule(u, i, U, I, order, cell_ptr, info["rounds"], info["blocks"]) == 0
    Po, Qo, rmo = _oracle_train(oracle, U, I, k, u, i, r, order, seed, epochs, lr, lam)
    assert np.array_equal(P, Po), f"P differs: max abs {np.abs(P - Po).max()}"
    assert np.array_equal(Q, Qo), f"Q differs: max abs {np.abs(Q - Qo).max()}"
    assert np.abs(rm - rmo).max() <= RMSE_TOL
    np.testing.assert_allclose(rm, rmo, rtol=1e-9, atol=1e-12)
    if epochs:
        assert abs(rm_again - rm[-1]) <= 1e-12
    return rm, info


def _wl(mf, oracle, name, scale=1.0, **kw):
    w = mf.synth.workload(name, scale)
    return _run(mf, oracle, w["U"], w["I"], w["k"], w["u"], w["i"], w["r"], **kw)


# ---- BASELINE.json configs --------------------------------------------------------
def test_cfg0_dense(mf, oracle):
    rm, _ = _wl(mf, oracle, "cfg0_dense100x80", epochs=5)
    assert rm[-1] < rm[0]


def test_cfg1_ml100k(mf, oracle):
    rm, _ = _wl(mf, oracle, "cfg1_ml100k", epochs=3)
    assert rm[-1] < rm[0]


def test_cfg2_ml20m_scaled(mf, oracle):
    _wl(mf, oracle, "cfg2_ml20m", scale=0.05, epochs=2)


def test_cfg3_netflix_scaled_k128(mf, oracle):
    _wl(mf, oracle, "cfg3_netflix", scale=0.004, epochs=2)


def test_cfg4_powerlaw_scaled_k256(mf, oracle):
    _wl(mf, oracle, "cfg4_powerlaw", scale=0.0003, epochs=2)


# ---- geometry sweep -----------------------------------------------------------------
@pytest.mark.parametrize("k", [1, 2, 3, 4, 5, 8, 12, 16, 17, 32, 48, 64, 65, 100, 128, 200, 256])
def test_every_k(mf, oracle, k):
    rng = np.random.default_rng(k)
    U, I, n = 300, 200, 12000
    key = rng.choice(U * I, n, replace=False)
    _run(mf, oracle, U, I, k, key // I, key % I, rng.random(n) * 4 + 1, epochs=2)


@pytest.mark.parametrize("B,W", [(1, 1), (2, 2), (3, 4), (7, 8), (16, 4), (32, 2)])
def test_blocks_and_waves(mf, oracle, B, W):
    rng = np.random.default_rng(B * 100 + W)
    U, I = 900, 700
    n = min(40000, 200 * B * B)  # a cell must fit the 160 KiB LDS image
    key = rng.choice(U * I, n, replace=False)
    _, info = _run(mf, oracle, U, I, 64, key // I, key % I, rng.random(n) * 4 + 1, epochs=2, blocks=B, waves=W)
    assert info["blocks"] == B and info["waves"] == W


def test_more_blocks_than_resident_workgroups(mf, oracle):
    """B = 300 > 256 CUs: the persistent kernel's workgroups each own several user blocks."""
    rng = np.random.default_rng(300)
    U, I, n = 2400, 1800, 60000
    key = rng.choice(U * I, n, replace=False)
    _, info = _run(mf, oracle, U, I, 64, key // I, key % I, rng.random(n) * 4 + 1, epochs=2, blocks=300, waves=2)
    assert info["blocks"] == 300


# ---- chunked cells: cells larger than the LDS image are cut into chunks --------------------------
@pytest.mark.parametrize("k,B,W,n", [(256, 1, 2, 900), (128, 2, 4, 4000), (64, 1, 4, 4000), (200, 3, 1, 3000),
                                     (64, 4, 4, 60000)])
def test_chunked_cells(mf, oracle, k, B, W, n):
    rng = np.random.default_rng(k + B)
    U, I = 900, 800
    key = rng.choice(U * I, n, replace=False)
    _, info = _run(mf, oracle, U, I, k, key // I, key % I, rng.random(n) * 4 + 1, epochs=2, blocks=B, waves=W)
    assert info["split_cells"] >= 1 and info["chunks"] > B * B


def test_chunked_cells_round_launch_equals_persistent(mf, oracle):
    from mfsgd_amd import _lib

    rng = np.random.default_rng(77)
    U, I, n = 3000, 400, 40000
    wgt = 1.0 / (np.arange(I) + 3.0)
    key = np.unique(rng.integers(0, U, n).astype(np.int64) * I + rng.choice(I, n, p=wgt / wgt.sum()))
    u, i, r = key // I, key % I, rng.random(key.size) * 4 + 1
    outs = []
    for flags in (0, _lib.FLAG_ROUND_LAUNCH):
        with mf.MatrixFactorizationSGD(U, I, 128, LR, LAM, 5, blocks=8, waves=4, flags=flags) as m:
            rm = m.train(u, i, r, 2)
            assert m.schedule_info()["split_cells"] >= 1
            outs.append((m.get_factors(), rm))
    assert np.array_equal(outs[0][0][0], outs[1][0][0]) and np.array_equal(outs[0][0][1], outs[1][0][1])
    np.testing.assert_allclose(outs[0][1], outs[1][1], rtol=1e-9)
    _run(mf, oracle, U, I, 128, u, i, r, epochs=2, blocks=8, waves=4)


def test_chunked_cells_with_more_blocks_than_workgroups(mf, oracle):
    """Skewed items at k = 256 and B = 320 (> resident workgroups): chunk chains inside a multi-pass ring."""
    rng = np.random.default_rng(320)
    U, I, n = 20000, 3000, 400000
    wgt = 1.0 / (np.arange(I) + 2.0)
    key = np.unique(rng.integers(0, U, n).astype(np.int64) * I + rng.choice(I, n, p=wgt / wgt.sum()))
    _, info = _run(mf, oracle, U, I, 256, key // I, key % I, rng.random(key.size) * 4 + 1, epochs=2, blocks=320,
                   waves=4)
    assert info["blocks"] == 320


def test_auto_blocks_large_k_multi_pass(mf, oracle):
    """k = 128 at 20 M ratings: more blocks than CUs, so every workgroup runs several cells per round
    (and B is a multiple of half the CU count rather than whatever makes the largest cell fit)."""
    w = mf.synth.workload("cfg3_netflix", scale=0.2)
    _, info = _run(mf, oracle, w["U"], w["I"], w["k"], w["u"], w["i"], w["r"], epochs=1)
    assert info["blocks"] > 256 and info["blocks"] % 128 == 0


def test_round_launch_path_equals_persistent(mf, oracle):
    from mfsgd_amd import _lib

    w = mf.synth.workload("cfg2_ml20m", scale=0.03)
    outs = []
    for flags in (0, _lib.FLAG_ROUND_LAUNCH):
        with mf.MatrixFactorizationSGD(w["U"], w["I"], w["k"], LR, LAM, 5, flags=flags) as m:
            m.train(w["u"], w["i"], w["r"], 3)
            outs.append(m.get_factors())
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


def test_eager_launch_equals_graph(mf, oracle):
    from mfsgd_amd import _lib

    w = mf.synth.workload("cfg1_ml100k", scale=0.5)
    outs = []
    for flags in (0, _lib.FLAG_NO_GRAPH):
        with mf.MatrixFactorizationSGD(w["U"], w["I"], w["k"], LR, LAM, 5, flags=flags) as m:
            m.train(w["u"], w["i"], w["r"], 3)
            outs.append(m.get_factors())
    assert np.array_equal(outs[0][0], outs[1][0]) and np.array_equal(outs[0][1], outs[1][1])


# ---- edge cases -----------------------------------------------------------------------
def test_edge_cases(mf, oracle):
    # single rating; pure user chain; pure item chain; duplicates; untouched rows
    _run(mf, oracle, 5, 5, 8, [2], [3], [4.0])
    _run(mf, oracle, 1, 40, 8, [0] * 40, list(range(40)), np.arange(40) * 0.1)
    _run(mf, oracle, 40, 1, 8, list(range(40)), [0] * 40, np.arange(40) * 0.1)
    _run(mf, oracle, 3, 3, 4, [0, 0, 0, 1, 1, 2, 0], [1, 1, 1, 2, 2, 0, 1], [1, 2, 3, 4, 5, 6, 7])
    _run(mf, oracle, 50, 50, 12, [49, 49, 49, 0, 7], [0, 49, 25, 0, 7], [1, 2, 3, 4, 5])


def test_empty_ratings(mf):
    with mf.MatrixFactorizationSGD(5, 4, 8, LR, LAM, 1) as m:
        rm = m.train([], [], [], 2)
        assert (rm == 0).all()
        P, Q = m.get_factors()
        assert np.isfinite(P).all() and np.isfinite(Q).all()


@pytest.mark.parametrize("k", [64, 128, 256])  # 16, 32 and 64 lanes per rating: the three assembly run loops
def test_hot_item_chain_run_mode(mf, oracle, k):
    rng = np.random.default_rng(9)
    U, I = 3000, 60
    u = list(range(U)) + list(rng.integers(0, U, 6000))
    i = [7] * U + list(rng.integers(0, I, 6000))
    key = np.unique(np.array(u) * I + np.array(i))
    _, info = _run(mf, oracle, U, I, k, key // I, key % I, rng.random(key.size) * 4 + 1, epochs=2)
    assert info["waves"] == 2  # one item rated by everybody: chain-bound, two apply waves


@pytest.mark.parametrize("k,W", [(128, 4), (256, 4), (128, 1), (96, 2), (200, 8)])
def test_run_loops_every_wave_count(mf, oracle, k, W):
    """Skewed items so that runs form, explicit wave counts (copy waves exist for W <= 4 only)."""
    rng = np.random.default_rng(k + W)
    U, I, n = 4000, 500, 60000
    wgt = 1.0 / (np.arange(I) + 1.5)
    key = np.unique(rng.integers(0, U, n).astype(np.int64) * I + rng.choice(I, n, p=wgt / wgt.sum()))
    _, info = _run(mf, oracle, U, I, k, key // I, key % I, rng.random(key.size) * 4 + 1, epochs=2, waves=W)
    assert info["waves"] == W


def test_hot_user_chain_swapped_roles(mf, oracle):
    rng = np.random.default_rng(19)
    U, I = 60, 3000
    u = [7] * I + list(rng.integers(0, U, 6000))
    i = list(range(I)) + list(rng.integers(0, I, 6000))
    key = np.unique(np.array(u) * I + np.array(i))
    _, info = _run(mf, oracle, U, I, 64, key // I, key % I, rng.random(key.size) * 4 + 1, epochs=2)
    assert info["swapped"] == 1
    # the hot user's chain is what the solo runs and the lone-tile hop are for: B = 8, 8 lone-tile cells, 13 solo runs
    with mf.MatrixFactorizationSGD(U, I, 64, LR, LAM, 11) as m:
        m.set_ratings((key // I).astype(np.int32), (key % I).astype(np.int32), np.ones(key.size, np.float32))
        cells, _, subs, _ = m.debug_schedule()
        B = m.schedule_info()["blocks"]
    solo = subs[:, 0] >> 16
    assert (cells[:, 5] & 1).sum() >= B and solo.sum() > 0, (B, int((cells[:, 5] & 1).sum()), int(solo.sum()))
    print(f"B {B}, lone cells {(cells[:, 5] & 1).sum()}, solo runs {(solo > 0).sum()}, solo steps {solo.sum()}")


def test_large_values_and_zero_lambda(mf, oracle):
    rng = np.random.default_rng(3)
    U, I, n = 200, 150, 5000
    key = rng.choice(U * I, n, replace=False)
    _run(mf, oracle, U, I, 32, key // I, key % I, rng.standard_normal(n) * 50, epochs=2, lr=0.001, lam=0.0)


def test_fuzz_random_problems(mf, oracle):
    from tests.dsgd_common import fuzz_cases

    ok = 0
    for c in fuzz_cases(120, seed=77):
        try:
            _run(mf, oracle, c["U"], c["I"], c["k"], c["u"], c["i"], c["r"], epochs=2, lr=c["lr"], lam=c["lam"],
                 blocks=c["blocks"], waves=c["waves"])
        except mf.MfsgdError as e:
            assert e.code == -7, e
            continue
        ok += 1
    assert ok >= 90


def test_fuzz_chunked_problems(mf, oracle):
    from tests.dsgd_common import fuzz_chunked_cases

    split = 0
    for c in fuzz_chunked_cases(30):
        _, info = _run(mf, oracle, c["U"], c["I"], c["k"], c["u"], c["i"], c["r"], epochs=2, lr=c["lr"], lam=c["lam"],
                       blocks=c["blocks"], waves=c["waves"])
        split += info["split_cells"] > 0
    assert split >= 15


# ---- predict / factors / repeated training ------------------------------------------
def test_predict_and_set_factors(mf, oracle):
    rng = np.random.default_rng(4)
    U, I, k = 120, 90, 40
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    uu = rng.integers(0, U, 5000).astype(np.int32)
    ii = rng.integers(0, I, 5000).astype(np.int32)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        out = m.predict(uu, ii)
        one = m.predict(int(uu[0]), int(ii[0]))
        P2, Q2 = m.get_factors()
    np.testing.assert_array_equal(out, oracle.predict(P, Q, uu, ii))
    assert one == out[0]
    np.testing.assert_array_equal(P2, P)
    np.testing.assert_array_equal(Q2, Q)


@pytest.mark.parametrize("k", [8, 64, 100])
def test_recommend_topn_equals_sorted_predictions(mf, oracle, k):
    rng = np.random.default_rng(k)
    U, I, topn = 50, 700, 25
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    Q[5] = Q[9]  # exact ties: the smaller item index must come first
    users = np.array([0, 7, 7, 49, 13], np.int32)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        items, scores = m.recommend(users, topn)
        with pytest.raises(mf.MfsgdError):
            m.recommend(users, I + 1)
    allitems = np.arange(I, dtype=np.int32)
    for row, u in enumerate(users):
        s = oracle.predict(P, Q, np.full(I, u, np.int32), allitems)
        order = np.lexsort((allitems, -s.astype(np.float64)))[:topn]
        np.testing.assert_array_equal(items[row], order)
        np.testing.assert_array_equal(scores[row], s[order])


@pytest.mark.parametrize("I,topn,k", [(30000, 10, 64), (61000, 40, 32), (700, 128, 8), (700, 129, 8), (5, 5, 16)])
def test_recommend_fused_select_and_sort_paths(mf, oracle, I, topn, k):
    """The fused score + radix-select kernel (topn <= 128: one tile, three tiles) and the segmented-sort
    path (topn = 129) against sorting the oracle's predictions; many exact ties, including ties that
    straddle the selection threshold, and zero scores.  (The -0.0 entry below does not make a -0.0 SCORE: the zeros
    of mixed sign in the row, and the +0.0 pad columns, sum to +0.0.  Real -0.0 scores: tests/test_serving_edges_gpu.py.)"""
    rng = np.random.default_rng(I + topn)
    U = 40
    P = rng.standard_normal((U, k)).astype(np.float32)
    Q = rng.standard_normal((I, k)).astype(np.float32)
    Q[rng.integers(0, I, I // 3)] = Q[3 % I]  # a third of the catalogue scores exactly alike
    if I > 100:
        Q[50:60] = 0.0  # zero scores ...
        Q[55, 0] = -0.0  # (a -0.0 entry; the row's score is still +0.0)
        P[7] = np.abs(P[7])
        Q[60:5000:7] = -np.abs(Q[60:5000:7])  # ... in the middle of user 7's ranking
    users = np.array([0, 7, 7, U - 1, 13, 21], np.int32)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 1) as m:
        m.set_factors(P, Q)
        items, scores = m.recommend(users, topn)
    allitems = np.arange(I, dtype=np.int32)
    for row, u in enumerate(users):
        sc = oracle.predict(P, Q, np.full(I, u, np.int32), allitems)
        order = np.lexsort((allitems, -sc.astype(np.float64)))[:topn]
        np.testing.assert_array_equal(items[row], order)
        np.testing.assert_array_equal(scores[row], sc[order])


def test_train_from_a_ratings_file(mf, oracle, tmp_path):
    rng = np.random.default_rng(12)
    U, I, n = 400, 300, 9000
    key = rng.choice(U * I, n, replace=False)
    uid, iid = (key // I) * 3 + 11, (key % I) * 7 + 5  # sparse original ids
    r = (rng.integers(1, 11, n) * 0.5).astype(np.float32)
    f = tmp_path / "ratings.csv"
    f.write_text("userId,movieId,rating,timestamp\n" + "".join(f"{a},{b},{c},0\n" for a, b, c in zip(uid, iid, r)))
    d = mf.load_ratings(f)
    np.testing.assert_array_equal(d["user_ids"][d["u"]], uid)
    np.testing.assert_array_equal(d["item_ids"][d["i"]], iid)
    _run(mf, oracle, d["n_users"], d["n_items"], 32, d["u"], d["i"], d["r"], epochs=2)


def _same_schedule(mf, U, I, k, u, i, r, n_parts=0, expect_packed=None, **kw):
    """Builds the schedule three ways -- host loops, device ingest + host packer, device ingest + device
    packer -- and compares every array word for word.  Returns whether the device packed it."""
    from mfsgd_amd import _lib

    got = []
    for flags in (_lib.FLAG_HOST_INGEST, _lib.FLAG_DEVICE_INGEST | _lib.FLAG_HOST_PACK, _lib.FLAG_DEVICE_INGEST):
        with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 5, flags=flags | kw.get("flags", 0), n_parts=n_parts,
                                       **{a: b for a, b in kw.items() if a != "flags"}) as m:
            m.set_ratings(u, i, r)
            per_part = []
            for part in range(max(1, n_parts)):
                info = m.schedule_info(part)
                per_part.append((m.order(part), m.debug_schedule(part), info))
            got.append(per_part)
    packed = []
    for part in range(max(1, n_parts)):
        ref_order, ref_sched, ref_info = got[0][part]
        assert ref_info["device_ingest"] == 0
        assert got[1][part][2]["device_ingest"] == 1
        packed.append(got[2][part][2]["device_ingest"] == 2)
        for other in (got[1][part], got[2][part]):
            order, sched, info = other
            np.testing.assert_array_equal(order[0], ref_order[0])
            np.testing.assert_array_equal(order[1], ref_order[1])
            for a, b, name in zip(sched, ref_sched, ("cells", "rows", "subs", "entries")):
                np.testing.assert_array_equal(a, b, err_msg=name)
            for key in ("nnz", "blocks", "waves", "lds_bytes", "total_steps", "total_rows", "max_cell_nnz", "max_cell_rows",
                        "max_cell_steps", "sum_round_steps", "chunks", "split_cells"):
                assert info[key] == ref_info[key], key
    if expect_packed is not None:
        assert all(packed) == expect_packed, packed
    return all(packed)


def _lib_flag(name):
    from mfsgd_amd import _lib

    return getattr(_lib, name)


def test_device_ingest_and_device_packer_build_the_same_schedule(mf):
    """Degree histograms + bucket order (ingest.hip) and the per-cell step packer (pack.hip) on the GPU
    against the host loops: the same bytes, whoever builds the schedule."""
    for name, scale, packed in (("cfg2_ml20m", 0.02, True), ("cfg1_ml100k", 1.0, True), ("cfg4_powerlaw", 0.0003, None),
                                ("cfg3_netflix", 0.01, None), ("cfg0_dense100x80", 1.0, True)):
        w = mf.synth.workload(name, scale)
        _same_schedule(mf, w["U"], w["I"], w["k"], w["u"], w["i"], w["r"], expect_packed=packed)
    # ratings that are the all-ones NaN (a solo record's empty mailbox word), in solo records and in step entries: every
    # builder writes the quiet NaN for the rating and for lr * r (tests/test_hyper_cpu.py, check_kind "solo_nan")
    from tests.test_hyper_cpu import PROBLEMS, check_kind

    make, k, kw, kind = PROBLEMS["solo_nan_k64_w2"]
    U, I, u, i, r = make()
    _same_schedule(mf, U, I, k, u, i, r, expect_packed=True, **kw)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 5, flags=_lib_flag("FLAG_DEVICE_INGEST"), **kw) as m:
        m.set_ratings(u, i, r)
        check_kind(m, kind)


def test_device_packer_fuzz(mf, oracle):
    """Random small problems (sizes, skew, repeated pairs, every k and explicit B / W) through the device
    packer: byte-identical to the host packer wherever the device takes the job -- and, independently of
    the host packer, a conflict-free permutation by the oracle's checker that trains bit-exactly."""
    from mfsgd_amd import _lib
    from tests.dsgd_common import fuzz_cases

    n_packed = n = 0
    for c in fuzz_cases(80, seed=4321, max_ratings=4000):
        try:
            packed = _same_schedule(mf, c["U"], c["I"], c["k"], c["u"], c["i"], c["r"], blocks=c["blocks"], waves=c["waves"])
        except mf.MfsgdError as e:
            assert e.code == -7, e
            continue
        n += 1
        n_packed += packed
        if packed and n_packed % 4 == 0:  # _run checks the exported order with mfo_check_block_schedule and replays it
            _, info = _run(mf, oracle, c["U"], c["I"], c["k"], c["u"], c["i"], c["r"], epochs=2, lr=c["lr"], lam=c["lam"],
                           blocks=c["blocks"], waves=c["waves"], flags=_lib.FLAG_DEVICE_INGEST)
            assert info["device_ingest"] == 2
    assert n >= 60 and n_packed >= n // 2, (n, n_packed)


@pytest.mark.parametrize("k,W", [(16, 4), (64, 1), (64, 2), (128, 4), (256, 2), (32, 8)])
def test_device_packer_runs_and_solo(mf, k, W):
    """Hot items (runs, solo runs, idle slots, odd run lengths) and repeated pairs through the device packer."""
    rng = np.random.default_rng(k + W)
    U, I = 2500, 120
    u = list(range(U)) + list(range(0, U, 2)) + list(range(0, U, 3)) + list(rng.integers(0, U, 12000)) + [5, 5, 5]
    i = [7] * U + [11] * len(range(0, U, 2)) + [13] * len(range(0, U, 3)) + list(rng.integers(0, I, 12000)) + [7, 7, 11]
    key = np.array(u, np.int64) * I + np.array(i)
    key = rng.permutation(np.concatenate([np.unique(key), key[-3:]]))  # a few repeated (user, item) pairs
    uu, ii, rr = (key // I).astype(np.int32), (key % I).astype(np.int32), (rng.random(key.size) * 4 + 1).astype(np.float32)
    B = 24 if k == 256 else 12  # small enough cells that nothing has to be chunked (the host's job)
    assert _same_schedule(mf, U, I, k, uu, ii, rr, blocks=B, waves=W)


def test_device_packer_mixed_mode_chunked_cells(mf, oracle):
    """Rating sets in which SOME cells have to be chunked (too large for the training kernel's LDS image as
    one chunk): the device keeps the cells that fit, the host decides how the rest are cut, the device packs
    those chunks into the same arrays -- and the result is still the host packer's bytes."""
    from mfsgd_amd import _lib
    from tests.dsgd_common import fuzz_chunked_cases

    n_mixed = 0
    for c in fuzz_chunked_cases(12, seed=515, max_ratings=9000):
        packed = _same_schedule(mf, c["U"], c["I"], c["k"], c["u"], c["i"], c["r"], blocks=c["blocks"], waves=c["waves"])
        with mf.MatrixFactorizationSGD(c["U"], c["I"], c["k"], LR, LAM, 5, blocks=c["blocks"], waves=c["waves"],
                                       flags=_lib.FLAG_DEVICE_INGEST) as m:
            m.set_ratings(c["u"], c["i"], c["r"])
            split = m.schedule_info()["split_cells"]
        n_mixed += bool(packed and split > 0)
    assert n_mixed >= 1, n_mixed  # (with one to four blocks most of these sets have every cell chunked: all host)
    # a skewed k = 128 set at auto geometry: hot cells chunked, the rest on the device; trained bit-exactly
    w = mf.synth.workload("cfg3_netflix", 0.05)
    assert _same_schedule(mf, w["U"], w["I"], w["k"], w["u"], w["i"], w["r"])
    _, info = _run(mf, oracle, w["U"], w["I"], w["k"], w["u"], w["i"], w["r"], epochs=1)
    assert info["device_ingest"] == 2


def test_device_packer_one_pass_and_two_pass_write_the_same_bytes(mf, monkeypatch):
    """[r3] The packing kernel writes what it packs during its COUNT pass (scratch arrays at worst-case offsets, moved by
    compact_kernel); MFSGD_PACK_TWICE=1 keeps the COUNT + EMIT form.  Both against the host packer's bytes, with and
    without cells that are cut (whose scratch is dropped and whose chunks are packed from their lists)."""
    cases = (("cfg2_ml20m", 0.02), ("cfg3_netflix", 0.02), ("cfg4_powerlaw", 0.0003), ("cfg1_ml100k", 1.0))
    for twice in (False, True):
        if twice:
            monkeypatch.setenv("MFSGD_PACK_TWICE", "1")
        else:
            monkeypatch.delenv("MFSGD_PACK_TWICE", raising=False)
        for name, scale in cases:
            w = mf.synth.workload(name, scale)
            _same_schedule(mf, w["U"], w["I"], w["k"], w["u"], w["i"], w["r"])


def test_device_packer_tables_on_the_device_or_through_the_host(mf):
    """[r3] The sub-cell tables of a device-packed schedule are assembled on the device (the cells' tables as counted,
    the chunks' scattered to their descriptors); the route through the host is retired.  The debug getter fetches the
    device's copy: against the host packer's bytes, with and without cut cells."""
    cases = (("cfg2_ml20m", 0.02), ("cfg3_netflix", 0.02), ("cfg4_powerlaw", 0.0003))
    for name, scale in cases:
        w = mf.synth.workload(name, scale)
        _same_schedule(mf, w["U"], w["I"], w["k"], w["u"], w["i"], w["r"])


def test_device_packer_partitioned_handles(mf):
    """n_parts > 1: every partition's schedule through the device packer (the caller-visible rating
    indices go through the `orig` map)."""
    w = mf.synth.workload("cfg2_ml20m", 0.01)
    assert _same_schedule(mf, w["U"], w["I"], w["k"], w["u"], w["i"], w["r"], n_parts=3)


@pytest.mark.parametrize("n_parts", [2, 4])
def test_equal_sized_partitions_do_not_share_a_stale_device_copy(mf, n_parts):
    """Partitions of EQUAL size (a dense set cut by i % n_parts): the per-partition (u, i) buffers of
    mfsgd_set_ratings come back from the allocator at the same addresses, and the ingest context used to take
    them for the triples it already held on the device -- every partition after the first was bucketed from the
    previous partition's (u, i) with its own ratings.  Each partition, device-built, against the host-built
    schedule word for word (advisor finding, round 2; fixed by DeviceIngest::forget between the builds)."""
    U, I, k = 240, 200, 64
    u = np.repeat(np.arange(U), I).astype(np.int32)
    i = np.tile(np.arange(I), U).astype(np.int32)
    rng = np.random.default_rng(n_parts)
    perm = rng.permutation(u.size)
    u, i = u[perm], i[perm]
    r = (rng.random(u.size) * 4 + 1).astype(np.float32)
    assert len({int(np.sum(i % n_parts == p)) for p in range(n_parts)}) == 1  # equal partitions
    _same_schedule(mf, U, I, k, u, i, r, n_parts=n_parts)


def test_train_twice_and_new_ratings(mf, oracle):
    w = mf.synth.workload("cfg1_ml100k", scale=0.2)
    with mf.MatrixFactorizationSGD(w["U"], w["I"], w["k"], LR, LAM, 8) as m:
        r1 = m.train(w["u"], w["i"], w["r"], 2)
        r2 = m.train(w["u"], w["i"], w["r"], 2)  # continues from the current factors
        order, _ = m.order()
        P, Q = m.get_factors()
        Po, Qo, rmo = _oracle_train(oracle, w["U"], w["I"], w["k"], w["u"], w["i"], w["r"], order, 8, 4)
        assert np.array_equal(P, Po) and np.array_equal(Q, Qo)
        np.testing.assert_allclose(np.concatenate([r1, r2]), rmo, rtol=1e-9)
        # a different rating set on the same handle: new schedule, same factors carried over
        half = w["nnz"] // 2
        m.train(w["u"][:half], w["i"][:half], w["r"][:half], 1)
        order2, _ = m.order()
        oracle.sgd_pass_ordered(Po, Qo, w["u"][:half], w["i"][:half], w["r"][:half], order2, LR, LAM)
        P, Q = m.get_factors()
        assert np.array_equal(P, Po) and np.array_equal(Q, Qo)


# ---- DSGD building blocks on one GPU (virtual devices) -------------------------------
@pytest.mark.parametrize("G,k,B", [(2, 64, 0), (4, 64, 0), (3, 256, 1)])  # the last one: every partition chunked
def test_dsgd_virtual_devices(mf, oracle, G, k, B):
    import torch

    from tests.dsgd_common import LAM as DL, LR as DLR, SEED, rank_workload, sequential_dsgd

    U_local, I, nnz, epochs = 500, 333, 20000, 2
    dev = torch.device("cuda", 0)
    trainers, data, blocks = [], [], []
    for g in range(G):
        u, i, r = rank_workload(g, U_local, I, nnz)
        t = mf.MatrixFactorizationSGD(U_local, I, k, DLR, DL, SEED, n_parts=G, blocks=B)
        t.set_ratings(u, i, r)
        assert B == 0 or t.schedule_info(0)["split_cells"] >= 1
        t.init_p_offset(SEED, g * U_local)
        trainers.append(t)
        data.append((u, i, r))
    kp = trainers[0].kp
    for part in range(G):
        blocks.append(torch.from_numpy(trainers[0].part_init_q(part, SEED, U_local * G)).to(dev))
    stream = torch.cuda.current_stream(dev).cuda_stream
    sse = []
    for _ in range(epochs):
        for s in range(G):
            for g in range(G):
                part = (g + s) % G
                trainers[g].part_train(part, blocks[part].data_ptr(), stream)
        torch.cuda.synchronize()
        tot = 0.0
        for s in range(G):
            for g in range(G):
                part = (g + s) % G
                tot += trainers[g].part_sse(part, blocks[part].data_ptr(), stream)
        sse.append(tot)
    P = np.concatenate([t.get_factors()[0] for t in trainers])
    from mfsgd_amd.dsgd import assemble_q

    Q = assemble_q({p: blocks[p].cpu().numpy() for p in range(G)}, I, k, G)
    Ps, Qs, sse_s = sequential_dsgd(oracle, trainers, data, U_local, I, k, G, epochs)
    assert np.array_equal(P, Ps) and np.array_equal(Q, Qs)
    np.testing.assert_allclose(sse, sse_s, rtol=1e-9)
    for t in trainers:
        t.close()


# ---- BASELINE.json's full size: size-independent properties ---------------------------
def test_full_size_ml20m_properties(mf, oracle):
    """20M ratings, k = 64 (the bench workload).  The oracle would need minutes per
    epoch single-threaded, so the full size is checked through properties:
    (1) the schedule is a conflict-free permutation of all ratings;
    (2) two independent handles give bit-identical factors (determinism);
    (3) the multithreaded oracle on the same schedule reproduces them bit for bit
        for one epoch (16 threads: seconds);
    (4) RMSE decreases monotonically over the first epochs and predict() agrees
        with the factors."""
    w = mf.synth.workload("cfg2_ml20m")
    facs, rms = [], []
    for _ in range(2):
        with mf.MatrixFactorizationSGD(w["U"], w["I"], w["k"], LR, LAM, 3, host_threads=16) as m:
            rm = m.train(w["u"], w["i"], w["r"], 3)
            facs.append(m.get_factors())
            rms.append(rm)
            order, cell_ptr = m.order()
            info = m.schedule_info()
            pr = m.predict(w["u"][:1000], w["i"][:1000])
    assert oracle.check_block_schedule(w["u"], w["i"], w["U"], w["I"], order, cell_ptr, info["rounds"], info["blocks"]) == 0
    assert np.array_equal(facs[0][0], facs[1][0]) and np.array_equal(facs[0][1], facs[1][1])
    assert np.array_equal(rms[0], rms[1])
    assert rms[0][0] > rms[0][1] > rms[0][2]
    P, Q = oracle.init_factors(w["U"], w["I"], w["k"], 3)
    for _ in range(3):
        oracle.sgd_epoch_mt(P, Q, w["u"], w["i"], w["r"], order, cell_ptr, info["rounds"], info["blocks"], LR, LAM, 16)
    assert np.array_equal(P, facs[0][0]) and np.array_equal(Q, facs[0][1])
    assert abs(oracle.rmse(P, Q, w["u"], w["i"], w["r"]) - rms[0][2]) <= 1e-9
    np.testing.assert_array_equal(pr, oracle.predict(P, Q, w["u"][:1000], w["i"][:1000]))


# ---- BASELINE configs 3 and 4 in their DSGD form: ONE global rating set, cut by the product's
# partitioner (mfsgd_dsgd_plan) for G = 8 devices, run as 8 virtual devices on this GPU ------------
def _virtual_dsgd(mf, oracle, w, G, epochs, mt_threads=0, check_factors=True, **kw):
    """Trains w over G virtual devices (G handles, real kernels, blocks rotated by pointer) and
    compares with the sequential DSGD definition executed by the oracle over GLOBAL factors."""
    import torch

    from tests.dsgd_common import LAM as DL, LR as DLR, SEED, assemble_q_plan, plan_shards, plan_trainer, sequential_dsgd_plan

    U, I, k, u, i, r = w["U"], w["I"], w["k"], w["u"], w["i"], w["r"]
    dev = torch.device("cuda", 0)
    ub, ip, sel = plan_shards(mf, U, I, u, i, G)
    trainers = [plan_trainer(mf, g, ub, ip, sel, I, k, u, i, r, G, **kw) for g in range(G)]
    blocks = [torch.from_numpy(trainers[0].part_init_q(part, SEED, U)).to(dev) for part in range(G)]
    stream = torch.cuda.current_stream(dev).cuda_stream
    sse = []
    for _ in range(epochs):
        for s in range(G):
            for g in range(G):
                part = (g + s) % G
                trainers[g].part_train(part, blocks[part].data_ptr(), stream)
        torch.cuda.synchronize()
        tot = 0.0
        for s in range(G):
            for g in range(G):
                part = (g + s) % G
                tot += trainers[g].part_sse(part, blocks[part].data_ptr(), stream)
        sse.append(tot)
    P = np.concatenate([t.get_factors()[0] for t in trainers])
    Q = assemble_q_plan({p: blocks[p].cpu().numpy() for p in range(G)}, ip, I, k)
    infos = [[t.schedule_info(p) for p in range(G)] for t in trainers]
    Ps, Qs, sse_s = sequential_dsgd_plan(oracle, trainers, sel, U, I, k, u, i, r, G, epochs, mt_threads=mt_threads)
    for t in trainers:
        t.close()
    assert np.array_equal(P, Ps), f"P differs: max abs {np.abs(P - Ps).max()}"
    assert np.array_equal(Q, Qs), f"Q differs: max abs {np.abs(Q - Qs).max()}"
    np.testing.assert_allclose(sse, sse_s, rtol=1e-9)
    rm = np.sqrt(np.array(sse) / u.size)
    assert np.abs(rm - np.sqrt(np.array(sse_s) / u.size)).max() <= RMSE_TOL
    return rm, ub, ip, infos


@pytest.mark.parametrize("name,scale", [("cfg3_netflix", 0.02), ("cfg4_powerlaw", 0.0005)])
def test_dsgd8_planned_virtual_devices(mf, oracle, name, scale):
    """Netflix shape k = 128 and power-law k = 256, scaled, DSGD x 8 as BASELINE states them."""
    w = mf.synth.workload(name, scale)
    rm, ub, ip, infos = _virtual_dsgd(mf, oracle, w, 8, 2)
    assert rm[1] < rm[0]
    du = np.bincount(w["u"], minlength=w["U"])
    shard = np.array([du[ub[g]:ub[g + 1]].sum() for g in range(8)])
    assert shard.max() <= 1.05 * shard.mean() + du.max()
    assert sum(x["nnz"] for row in infos for x in row) == w["nnz"]


def test_cfg4_one_eighth_dsgd8_virtual_devices(mf, oracle):
    """BASELINE configs[4] (power-law popularity, k = 256, DSGD x 8) at ONE EIGHTH of its full size -- what the 8-GPU job
    gives one GPU: 125 M ratings, 1.25 M x 125 K -- as 8 virtual devices on this GPU: the global set (made on the GPU:
    synth.make_ratings_device) cut by the product's partitioner, 64 device-built schedules, real kernels, blocks rotated
    by pointer, one epoch, factors and SSE bit for bit against the sequential DSGD definition (the oracle runs every
    (device, partition) block multithreaded).  Round 2 ran this builder-side only (tests/gpu_large_extra.py)."""
    w = mf.synth.workload("cfg4_powerlaw", 0.125, generator="device")
    assert w["nnz"] == 125_000_000 and w["k"] == 256
    rm, ub, ip, infos = _virtual_dsgd(mf, oracle, w, 8, 1, mt_threads=16, host_threads=16)
    du = np.bincount(w["u"], minlength=w["U"])
    shard = np.array([du[ub[g]:ub[g + 1]].sum() for g in range(8)])
    assert shard.max() <= 1.01 * shard.mean() + du.max()
    assert sum(x["nnz"] for row in infos for x in row) == w["nnz"]
    assert all(x["device_ingest"] == 2 for row in infos for x in row)


def test_dsgd_planned_three_devices_chunked(mf, oracle):
    """Odd device count, one block per partition: every partition is chunked (k = 256)."""
    rng = np.random.default_rng(31)
    U, I, n = 1500, 999, 60000
    key = rng.permutation(np.unique(rng.integers(0, U, n).astype(np.int64) * I + rng.integers(0, I, n)))
    w = dict(U=U, I=I, k=256, u=(key // I).astype(np.int32), i=(key % I).astype(np.int32),
             r=(rng.random(key.size) * 4 + 1).astype(np.float32))
    _, _, _, infos = _virtual_dsgd(mf, oracle, w, 3, 2, blocks=1)
    assert infos[0][0]["split_cells"] >= 1


@pytest.fixture(scope="module")
def netflix_full(mf):
    return mf.synth.workload("cfg3_netflix")


def test_full_size_netflix_properties(mf, oracle, netflix_full):
    """BASELINE configs[3]'s size on one GPU: 100 M ratings, 480,189 x 17,770, k = 128.  One epoch,
    bit-exact against the multithreaded oracle on the same schedule; the schedule a conflict-free
    permutation; RMSE falls."""
    w = netflix_full
    with mf.MatrixFactorizationSGD(w["U"], w["I"], w["k"], LR, LAM, 3, host_threads=16) as m:
        m.set_ratings(w["u"], w["i"], w["r"])
        m.init_factors(3)
        rm0 = m.rmse()
        rm = m.fit(1)
        P, Q = m.get_factors()
        order, cell_ptr = m.order()
        info = m.schedule_info()
    assert oracle.check_block_schedule(w["u"], w["i"], w["U"], w["I"], order, cell_ptr, info["rounds"], info["blocks"]) == 0
    Po, Qo = oracle.init_factors(w["U"], w["I"], w["k"], 3)
    assert abs(oracle.rmse(Po, Qo, w["u"], w["i"], w["r"]) - rm0) <= 1e-9
    oracle.sgd_epoch_mt(Po, Qo, w["u"], w["i"], w["r"], order, cell_ptr, info["rounds"], info["blocks"], LR, LAM, 16)
    assert np.array_equal(P, Po) and np.array_equal(Q, Qo)
    assert abs(oracle.rmse(Po, Qo, w["u"], w["i"], w["r"]) - rm[0]) <= 1e-9
    assert rm[0] < rm0


def test_full_size_netflix_dsgd8_virtual(mf, oracle, netflix_full):
    """BASELINE configs[3] as stated: Netflix shape, 100 M ratings, k = 128, DSGD x 8 -- the one
    global set cut by mfsgd_dsgd_plan, eight virtual devices on this GPU, one epoch, bit-exact
    against the sequential DSGD definition (oracle, multithreaded inside each sub-epoch block)."""
    rm, ub, ip, infos = _virtual_dsgd(mf, oracle, netflix_full, 8, 1, mt_threads=16, host_threads=16)
    assert rm[0] < 1.5


# ---- re-seeding after training: nothing captured with the old factor buffers may be replayed ------
@pytest.mark.parametrize("n_parts", [1, 3])
def test_reinit_after_training(mf, oracle, n_parts):
    import torch

    rng = np.random.default_rng(8)
    U, I, k, n = 600, 400, 64, 30000
    key = rng.choice(U * I, n, replace=False)
    u, i, r = (key // I).astype(np.int32), (key % I).astype(np.int32), (rng.random(n) * 4 + 1).astype(np.float32)
    if n_parts == 1:
        with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 5) as m:
            m.train(u, i, r, 2)
            hog = [torch.empty(1 << 20, device="cuda") for _ in range(4)]  # make the allocator move things
            m.init_factors(9)
            m.fit(2)
            P, Q = m.get_factors()
            order, _ = m.order()
            m.set_factors(P * 0.5, Q * 0.5)
            m.fit(1)
            P2, Q2 = m.get_factors()
            del hog
        Po, Qo, _ = _oracle_train(oracle, U, I, k, u, i, r, order, 9, 2)
        assert np.array_equal(P, Po) and np.array_equal(Q, Qo)
        Po, Qo = (Po * np.float32(0.5)).astype(np.float32), (Qo * np.float32(0.5)).astype(np.float32)
        oracle.sgd_pass_ordered(Po, Qo, u, i, r, order, LR, LAM)
        assert np.array_equal(P2, Po) and np.array_equal(Q2, Qo)
        return
    dev = torch.device("cuda", 0)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 5, n_parts=n_parts) as m:
        m.set_ratings(u, i, r)
        m.init_p_offset(5, 0)
        blocks = [torch.from_numpy(m.part_init_q(p, 5, U)).to(dev) for p in range(n_parts)]
        st = torch.cuda.current_stream(dev).cuda_stream
        for p in range(n_parts):
            m.part_train(p, blocks[p].data_ptr(), st)
        torch.cuda.synchronize()
        hog = [torch.empty(1 << 20, device="cuda") for _ in range(4)]
        m.init_p_offset(9, 0)  # same Q block pointers, new P buffer
        for p in range(n_parts):
            blocks[p].copy_(torch.from_numpy(m.part_init_q(p, 9, U)))
        for p in range(n_parts):
            m.part_train(p, blocks[p].data_ptr(), st)
        torch.cuda.synchronize()
        P, _ = m.get_factors()
        Po, Qo = oracle.init_factors(U, I, k, 9)
        for p in range(n_parts):
            oracle.sgd_pass_ordered(Po, Qo, u, i, r, m.order(p)[0], LR, LAM)
        from mfsgd_amd.dsgd import assemble_q

        Q = assemble_q({p: blocks[p].cpu().numpy() for p in range(n_parts)}, I, k, n_parts)
        del hog
    assert np.array_equal(P, Po) and np.array_equal(Q, Qo)


# ---- solo runs: chain wave + helper wave (run_asm.hpp), and the one-wave forms of the same records ---
@pytest.mark.parametrize("k,W", [(64, 1), (64, 2), (64, 4), (100, 2), (128, 2), (128, 4), (256, 2), (256, 4)])
def test_solo_runs_every_geometry(mf, oracle, k, W):
    from mfsgd_amd import _lib

    rng = np.random.default_rng(k * 10 + W)
    U, I = 3000, 80
    u = list(range(U)) + list(rng.integers(0, U, 9000))  # item 7 rated by everybody, odd and even run lengths
    i = [7] * U + list(rng.integers(0, I, 9000))
    key = rng.permutation(np.unique(np.array(u) * I + np.array(i)))
    uu, ii, rr = key // I, key % I, rng.random(key.size) * 4 + 1
    B = 24 if k == 256 else 5  # k = 256: a cell holds ~140 rows
    for flags in (0, _lib.FLAG_ROUND_LAUNCH, _lib.FLAG_NO_SOLO):
        with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 3, blocks=B, waves=W, flags=flags) as m:
            m.set_ratings(uu, ii, rr)
            solo = int((m.debug_schedule()[2][:, 0] >> 16).sum())
        assert (solo == 0) == (flags == _lib.FLAG_NO_SOLO), (flags, solo)
        _run(mf, oracle, U, I, k, uu, ii, rr, epochs=2, blocks=B, waves=W, flags=flags)


def test_solo_runs_on_the_bench_shape(mf, oracle):
    """cfg2 scaled: the calibrated head makes solo runs in the hot tile; auto geometry."""
    w = mf.synth.workload("cfg2_ml20m", scale=0.1)
    with mf.MatrixFactorizationSGD(w["U"], w["I"], w["k"], LR, LAM, 3) as m:
        m.set_ratings(w["u"], w["i"], w["r"])
        assert int((m.debug_schedule()[2][:, 0] >> 16).sum()) > 0
    _run(mf, oracle, w["U"], w["I"], w["k"], w["u"], w["i"], w["r"], epochs=2)


# ---- the DSGD driver under the C-ABI (csrc/dsgd.cpp): RCCL self-ring on this one GPU ----------------
@pytest.mark.parametrize("m,k", [(1, 64), (3, 64), (4, 128)])
def test_native_dsgd_world1_self_ring(mf, oracle, m, k):
    """world = 1: ncclSend / ncclRecv to itself move every block through both buffers; with m
    partitions the result must equal the sequential definition (and, for m = 1, mfsgd_train)."""
    from mfsgd_amd.dsgd import NativeDSGD, assemble_q

    rng = np.random.default_rng(m * 100 + k)
    U, I, n, epochs = 700, 500, 40000, 3
    key = rng.choice(U * I, n, replace=False)
    u, i, r = (key // I).astype(np.int32), (key % I).astype(np.int32), (rng.random(n) * 4 + 1).astype(np.float32)
    n_parts = max(m, 2)  # the smallest partitioned handle has two partitions
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 5, n_parts=n_parts) as t:
        t.set_ratings(u, i, r)
        t.init_p_offset(5, 0)
        with NativeDSGD(t, 0, 1, NativeDSGD.unique_id()) as d:
            assert d.m == n_parts
            d.init_q(5, U)
            rm0 = d.rmse()
            rm = d.train(epochs)
            blocks = d.home_blocks()
            tot, cnt = d.allreduce(1.5, 2.0)
            assert (tot, cnt) == (1.5, 2.0)
            ms = d.train_timed(1)
            assert ms > 0
            P1, _ = t.get_factors()
        orders = [t.order(p)[0] for p in range(n_parts)]
    Po, Qo = oracle.init_factors(U, I, k, 5)
    assert abs(oracle.rmse(Po, Qo, u, i, r) - rm0) <= 1e-9
    ref = []
    for _ in range(epochs):
        for p in range(n_parts):
            oracle.sgd_pass_ordered(Po, Qo, u, i, r, orders[p], LR, LAM)
        ref.append(oracle.rmse(Po, Qo, u, i, r))
    Q = assemble_q(blocks, I, k, n_parts)
    assert np.array_equal(Q, Qo), "Q blocks after the self-ring differ from the sequential definition"
    np.testing.assert_allclose(rm, ref, rtol=1e-9)
    for p in range(n_parts):  # the timed epoch on top
        oracle.sgd_pass_ordered(Po, Qo, u, i, r, orders[p], LR, LAM)
    assert np.array_equal(P1, Po)


@pytest.mark.parametrize("k", [100, 5])
def test_native_dsgd_blocks_round_trip_and_rings_come_and_go(mf, oracle, k):
    """Rows narrower than their padding (k = 100 in kp = 128, k = 5 in kp = 8) through mfsgd_dsgd_get_q / set_q, and
    ring after ring on one live trainer: three rings of one epoch each, every one seeded with the blocks its predecessor
    brought home, equal the sequential definition of three epochs bit for bit; a block of ones comes back as it went
    in, and no ring's first RMSE sees anything in the pad columns."""
    from mfsgd_amd.dsgd import NativeDSGD, assemble_q

    rng = np.random.default_rng(300 + k)
    U, I, n, n_parts = 700, 500, 40000, 3
    key = rng.choice(U * I, n, replace=False)
    u, i, r = (key // I).astype(np.int32), (key % I).astype(np.int32), (rng.random(n) * 4 + 1).astype(np.float32)
    rm0, rm, blocks = [], [], None
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 5, n_parts=n_parts) as t:
        t.set_ratings(u, i, r)
        t.init_p_offset(5, 0)
        for ring in range(3):
            with NativeDSGD(t, 0, 1, NativeDSGD.unique_id()) as d:
                assert d.m == n_parts
                for j in range(n_parts):
                    d.set_block(j, np.ones((t.part_rows(j), k), np.float32))
                ones = d.home_blocks()
                assert sorted(ones) == list(range(n_parts))
                for j in range(n_parts):
                    assert ones[j].shape == (t.part_rows(j), k) and np.array_equal(ones[j], np.ones_like(ones[j])), j
                if blocks is None:
                    d.init_q(5, U)
                else:
                    for j in range(n_parts):
                        d.set_block(j, blocks[j])
                rm0.append(d.rmse())
                rm.extend(d.train(1))
                blocks = d.home_blocks()
        P1, _ = t.get_factors()
        orders = [t.order(p)[0] for p in range(n_parts)]
    Po, Qo = oracle.init_factors(U, I, k, 5)
    ref0, ref = [], []
    for _ in range(3):
        ref0.append(oracle.rmse(Po, Qo, u, i, r))
        for p in range(n_parts):
            oracle.sgd_pass_ordered(Po, Qo, u, i, r, orders[p], LR, LAM)
        ref.append(oracle.rmse(Po, Qo, u, i, r))
    assert np.array_equal(P1, Po), "P after three rings differs from the sequential definition"
    assert np.array_equal(assemble_q(blocks, I, k, n_parts), Qo), "Q blocks after three rings differ from the sequential definition"
    np.testing.assert_allclose(rm, ref, rtol=1e-9)
    np.testing.assert_allclose(rm0, ref0, rtol=0, atol=1e-9)


def test_native_dsgd_recovers_when_a_persistent_launch_is_not_resident(mf, oracle):
    """The ring's recovery point (csrc/dsgd.cpp enqueue_epoch, mfsgd_part_settle): a foreign kernel holds the LDS of
    all but four CUs while the ring trains, so the persistent launches of its partitions find their workgroups not
    co-resident and change nothing.  The driver notices BEFORE the block is passed on, trains the sub-epoch as round
    launches and carries on: factors and Q blocks bit-exact against the sequential definition, the RMSE trajectory
    too, at least one sub-epoch re-run, and no 'factors invalid'."""
    from mfsgd_amd.dsgd import NativeDSGD, assemble_q

    rng = np.random.default_rng(321)
    U, I, k, n, epochs, n_parts = 2000, 1500, 64, 120000, 3, 2
    key = rng.choice(U * I, n, replace=False)
    u, i, r = (key // I).astype(np.int32), (key % I).astype(np.int32), (rng.random(n) * 4 + 1).astype(np.float32)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 5, n_parts=n_parts, blocks=64, waves=2) as t:
        t.set_ratings(u, i, r)
        t.init_p_offset(5, 0)
        with NativeDSGD(t, 0, 1, NativeDSGD.unique_id()) as d:
            d.init_q(5, U)
            first = d.train(1)  # a normal epoch first: persistent launches
            c0 = t.debug_counters()
            assert c0["persistent_parts"] == n_parts and c0["not_resident"] == 0, c0
            assert d.stats()["rerun_as_round_launches"] == 0
            t.debug_occupy(600)  # 0.6 s: longer than the residency check waits
            rm = d.train(epochs)
            st = d.stats()
            blocks = d.home_blocks()
            P1, _ = t.get_factors()
        c1 = t.debug_counters()
        orders = [t.order(p)[0] for p in range(n_parts)]
    assert st["rerun_as_round_launches"] >= 1 and st["checked"] == st["trained"], st
    assert c1["not_resident"] == st["rerun_as_round_launches"] and c1["persistent_parts"] < n_parts, (c1, st)
    Po, Qo = oracle.init_factors(U, I, k, 5)
    ref = []
    for _ in range(epochs + 1):
        for p in range(n_parts):
            oracle.sgd_pass_ordered(Po, Qo, u, i, r, orders[p], LR, LAM)
        ref.append(oracle.rmse(Po, Qo, u, i, r))
    assert np.array_equal(P1, Po), "P after the recovered epochs differs from the sequential definition"
    assert np.array_equal(assemble_q(blocks, I, k, n_parts), Qo)
    np.testing.assert_allclose(np.concatenate([first, rm]), ref, rtol=1e-9)


@pytest.mark.parametrize("k,B", [(64, 16), (64, 40), (128, 16), (256, 24), (100, 12)])
def test_lone_tile_mailbox_hand_off(mf, oracle, monkeypatch, k, B):
    """An item with a tile of its own travels from workgroup to workgroup through the tile's mailbox ({value, tag}
    granules, epoch.hip run_ring) instead of store + flag + gather: factors and RMSE bit-exact against the
    oracle over several epochs (every epoch is a launch of its own: the tags carry the launch generation), for
    one, two and four granules per lane, in a graph replay and in eager launches; and the same schedule with the
    mailbox switched off (MFSGD_NO_MAILBOX) gives the same bits."""
    from mfsgd_amd import _lib

    rng = np.random.default_rng(k + B)
    U, I = 150 * B, 90
    u = list(range(U)) + list(range(0, U, 2)) + list(rng.integers(0, U, 6 * U))
    i = [9] * U + [17] * (U // 2) + list(rng.integers(0, I, 6 * U))  # item 9 rated by everybody, item 17 by every other user
    key = rng.permutation(np.unique(np.array(u) * I + np.array(i)))
    uu, ii, rr = key // I, key % I, (rng.random(key.size) * 4 + 1).astype(np.float32)
    got = []
    for flags, off in ((0, False), (_lib.FLAG_NO_GRAPH, False), (0, True)):
        if off:
            monkeypatch.setenv("MFSGD_NO_MAILBOX", "1")
        with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 5, blocks=B, waves=2, flags=flags) as m:
            m.set_ratings(uu, ii, rr)
            n_lone = int((m.debug_schedule()[0][:, 5] & 1).sum())
            assert (n_lone == 0) if off else (n_lone >= B and n_lone % B == 0), (n_lone, off)
            assert m.debug_counters()["persistent_parts"] in (0, 1)
        rm, info = _run(mf, oracle, U, I, k, uu, ii, rr, seed=5, epochs=4, blocks=B, waves=2, flags=flags)
        assert info["split_cells"] == 0
        got.append(rm)
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], got[2])


def test_two_items_sharing_a_tile_do_not_use_the_mailbox(mf, oracle):
    """One item row per cell is not "a tile of one row": items 1 and 2 share a tile and are rated from different
    blocks (found by tests/gpu_fuzz_extra.py case 263 while the mailbox hand-off was being written)."""
    from tests.test_schedule_cpu import _two_items_one_tile

    U, I, u, i, r = _two_items_one_tile()
    for k in (64, 128):
        _run(mf, oracle, U, I, k, u, i, r, epochs=3, blocks=2, waves=1)


@pytest.mark.parametrize("world,m", [(2, 1), (3, 1), (2, 2)])
def test_native_dsgd_multi_process_shm(mf, oracle, tmp_path, monkeypatch, world, m):
    """The ring under the C-ABI with SEVERAL REAL PROCESSES (world 2 and 3, one and two partitions per rank):
    one global rating set cut by mfsgd_dsgd_plan, every rank a process of its own driving csrc/dsgd.cpp, the
    blocks moved by the driver's shared-memory rehearsal transport (RCCL refuses two ranks on one GPU; with
    RCCL only ncclSend / ncclRecv / ncclAllReduce differ).  Factors, Q blocks and the RMSE trajectory against
    the sequential DSGD definition run by the oracle over global factors: bit-exact."""
    _multi_process_shm(mf, oracle, tmp_path, world, m, "skewed")


def _multi_process_shm(mf, oracle, tmp_path, world, m, problem):
    """problem: a name of tests/dsgd_common.native_problem_named, which every rank rebuilds.  Returns the trainers' (lone-tile
    cells, solo runs) per (rank, partition)."""
    import os
    import subprocess
    import sys

    from mfsgd_amd import _lib
    from tests.conftest import ROOT
    from tests.dsgd_common import LAM as DL, LR as DLR, SEED, lone_and_solo, native_problem_named, plan_shards, plan_trainer

    # the rehearsal transport is in lib/libmfsgd_rehearsal.so only: the ranks load that one (this process keeps the product library)
    env = dict(os.environ, MFSGD_DSGD_TRANSPORT="shm", MFSGD_LIBRARY=_lib.rehearsal_library_path())
    procs = [subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "dsgd_native_worker.py"), str(rk), str(world), str(m),
                               str(tmp_path), problem], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
             for rk in range(world)]
    outs = []
    for pr in procs:
        try:
            outs.append(pr.communicate(timeout=600)[0])
        except subprocess.TimeoutExpired:
            for q in procs:
                q.kill()
            raise
    for rk, (pr, o) in enumerate(zip(procs, outs)):
        assert pr.returncode == 0, f"rank {rk}:\n{o[-3000:]}"
    U, I, k, u, i, r, epochs, kw = native_problem_named(problem)
    n_parts = world * m
    ub, _, sel = plan_shards(mf, U, I, u, i, world)
    _, ip = mf.dsgd_plan(np.bincount(u, minlength=U), np.bincount(i, minlength=I), n_parts)
    got = [np.load(tmp_path / f"rank{rk}.npz") for rk in range(world)]
    P = np.concatenate([g["P"] for g in got])
    Q = np.zeros((I, k), np.float32)
    seen = []
    for g in got:
        for part in g["parts"]:
            idx = np.flatnonzero(ip == part)
            Q[idx] = g[f"q{part}"][: idx.size]
            seen.append(int(part))
    assert sorted(seen) == list(range(n_parts))
    # the sequential definition: sub-epoch s, rank g trains the partitions of group (g + s) % world, one after another
    trainers = [plan_trainer(mf, g, ub, ip, sel, I, k, u, i, r, n_parts, **kw) for g in range(world)]
    forms = [[lone_and_solo(t, part) for part in range(n_parts)] for t in trainers]
    Po, Qo = oracle.init_factors(U, I, k, SEED)
    rm0 = oracle.rmse(Po, Qo, u, i, r)
    ref = []
    for _ in range(epochs):
        for s in range(world):
            for g in range(world):
                for j in range(m):
                    part = ((g + s) % world) * m + j
                    oracle.sgd_pass_ordered(Po, Qo, u, i, r, sel[g][trainers[g].order(part)[0]], DLR, DL)
        ref.append(oracle.rmse(Po, Qo, u, i, r))
    for t in trainers:
        t.close()
    assert np.array_equal(P, Po), "P differs from the sequential DSGD definition"
    assert np.array_equal(Q, Qo), "Q differs from the sequential DSGD definition"
    for g in got:
        assert abs(float(g["rm0"]) - rm0) <= 1e-9
        np.testing.assert_allclose(g["rm"], ref, rtol=1e-9)
        assert np.abs(g["rm"] - np.array(ref)).max() <= RMSE_TOL
    return forms


def test_native_dsgd_rejects_bad_arguments(mf):
    from mfsgd_amd.dsgd import NativeDSGD

    uid = NativeDSGD.unique_id()
    assert len(uid) == 128
    with mf.MatrixFactorizationSGD(10, 9, 8, LR, LAM, 1, n_parts=3) as t:
        with pytest.raises(mf.MfsgdError):
            NativeDSGD(t, 0, 1, uid)  # no ratings yet
        t.set_ratings([0, 1, 2], [0, 1, 2], [1.0, 2.0, 3.0])
        with pytest.raises(mf.MfsgdError):
            NativeDSGD(t, 0, 2, uid)  # 3 partitions cannot be dealt to 2 ranks
        with pytest.raises(mf.MfsgdError):
            NativeDSGD(t, 2, 1, uid)  # rank out of range


# ---- the persistent epoch kernel when its workgroups cannot all be resident ---------------------------
def test_persistent_kernel_not_resident_falls_back_to_round_launches(mf, oracle):
    """A foreign kernel holds every CU's LDS while training is launched: the epoch kernel's residency
    check gives up before touching anything, the library re-runs the epochs as one launch per round,
    and the factors still equal the oracle's bit for bit (no 'results invalid')."""
    rng = np.random.default_rng(88)
    U, I, k, n, epochs = 2000, 1500, 64, 120000, 3
    key = rng.choice(U * I, n, replace=False)
    u, i, r = (key // I).astype(np.int32), (key % I).astype(np.int32), (rng.random(n) * 4 + 1).astype(np.float32)
    for with_rmse in (False, True):
        with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 4, blocks=64, waves=2) as m:
            m.set_ratings(u, i, r)
            m.init_factors(4)
            first = m.fit(1)  # a normal persistent epoch first
            assert m.debug_counters()["persistent_parts"] == 1 and m.debug_counters()["not_resident"] == 0
            m.debug_occupy(600)  # 0.6 s: longer than the residency check waits
            rm = m.fit(epochs, rmse=with_rmse)
            c = m.debug_counters()
            assert (c["not_resident"], c["persistent_parts"], c["graphs"]) == (1, 0, 1), c
            P, Q = m.get_factors()
            order, _ = m.order()
            rm_after = m.fit(1)  # and the handle keeps working (round launches from now on)
            P2, Q2 = m.get_factors()
        Po, Qo, rmo = _oracle_train(oracle, U, I, k, u, i, r, order, 4, epochs + 1)
        assert np.array_equal(P, Po) and np.array_equal(Q, Qo)
        assert abs(first[0] - rmo[0]) <= 1e-9
        if with_rmse:
            np.testing.assert_allclose(rm, rmo[1:], rtol=1e-9)
        oracle.sgd_pass_ordered(Po, Qo, u, i, r, order, LR, LAM)
        assert np.array_equal(P2, Po) and np.array_equal(Q2, Qo)
        assert abs(rm_after[0] - oracle.rmse(Po, Qo, u, i, r)) <= 1e-9


# ---- hosts above the C-ABI ---------------------------------------------------------------------------
def test_train_after_editing_one_rating_in_the_middle(mf, oracle):
    """train(u, i, r) twice with ONE rating changed in the middle of the arrays in between (round 1's
    Python-side sampled fingerprint trained on the stale schedule): the second call must see the new
    value -- factors bit-exact against the oracle run on the edited ratings."""
    rng = np.random.default_rng(5)
    U, I, k, n = 3000, 2500, 32, 300_000
    key = rng.choice(U * I, n, replace=False)
    u, i, r = (key // I).astype(np.int32), (key % I).astype(np.int32), (rng.random(n) * 4 + 1).astype(np.float32)
    with mf.MatrixFactorizationSGD(U, I, k, LR, LAM, 6) as m:
        m.train(u, i, r, 1)
        order1, _ = m.order()
        m.train(u, i, r, 1)  # same triples: the schedule is kept
        assert m.debug_counters()["schedule_builds"] == 1
        r0 = r.copy()
        r[100_000] = 9.0
        m.train(u, i, r, 1)
        assert m.debug_counters()["schedule_builds"] == 2
        order2, _ = m.order()
        P, Q = m.get_factors()
    Po, Qo = oracle.init_factors(U, I, k, 6)
    oracle.sgd_pass_ordered(Po, Qo, u, i, r0, order1, LR, LAM)
    oracle.sgd_pass_ordered(Po, Qo, u, i, r0, order1, LR, LAM)
    oracle.sgd_pass_ordered(Po, Qo, u, i, r, order2, LR, LAM)
    assert np.array_equal(P, Po) and np.array_equal(Q, Qo)


def test_compiled_cpp_host_example(mf, oracle):
    """lib/mfsgd_example -- the compiled C++ mirror of the Java class (cpp/MatrixFactorizationSGD.hpp,
    the only compiled stand-in for the Java host) -- in a fresh process: its RMSE lines and its
    predict() against the oracle on the same ratings, seed and order."""
    import os
    import re
    import subprocess

    from tests.conftest import ROOT

    exe = os.path.join(ROOT, "matrixfactorizationsgd.java_amd", "lib", "mfsgd_example")
    assert os.path.exists(exe), "build it with __graft_entry__.build()"
    p = subprocess.run([exe], stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=300)
    assert p.returncode == 0, p.stdout
    got = [float(x) for x in re.findall(r"^epoch \d+ rmse ([0-9.]+)", p.stdout, re.M)]
    pred = float(re.search(r"predict\(3,4\) = ([-0-9.]+)", p.stdout).group(1))
    U, I, k = 100, 80, 8
    u = np.repeat(np.arange(U), I).astype(np.int32)
    i = np.tile(np.arange(I), U).astype(np.int32)
    r = (1.0 + ((u * 7 + i * 3) % 5)).astype(np.float32)
    with mf.MatrixFactorizationSGD(U, I, k, 0.01, 0.05, 42) as m:
        m.set_ratings(u, i, r)
        order, _ = m.order()
    Po, Qo, rmo = _oracle_train(oracle, U, I, k, u, i, r, order, 42, 5, 0.01, 0.05)
    assert len(got) == 5
    np.testing.assert_allclose(got, rmo, atol=1e-6)  # printed with six decimals
    assert abs(pred - oracle.predict(Po, Qo, np.array([3], np.int32), np.array([4], np.int32))[0]) <= 1e-6
    # the distributed surface of the same host (trainDistributed: world = 1, RCCL self-ring, two item partitions):
    # its RMSE lines against the sequential definition -- partition 0 then partition 1, each in its exported order
    dgot = [float(x) for x in re.findall(r"dsgd epoch \d+ rmse ([0-9.]+)", p.stdout)]
    assert len(dgot) == 3 and re.search(r"dsgd blocks 2 \(partitions 0 1\) trained 6 bytes_sent [1-9]", p.stdout), p.stdout
    with mf.MatrixFactorizationSGD(U, I, k, 0.01, 0.05, 42, n_parts=2) as m:
        m.set_ratings(u, i, r)
        orders = [m.order(part)[0] for part in range(2)]
    Po, Qo = oracle.init_factors(U, I, k, 42)
    ref = []
    for _ in range(3):
        for part in range(2):
            oracle.sgd_pass_ordered(Po, Qo, u, i, r, orders[part], 0.01, 0.05)
        ref.append(oracle.rmse(Po, Qo, u, i, r))
    np.testing.assert_allclose(dgot, ref, atol=1e-6)


# ---- bench.py as the driver calls it ---------------------------------------------------------------------
@pytest.mark.parametrize("args,scaling", [(["--gpus", "2"], "weak"), (["--gpus", "3", "--workload", "cfg3_netflix"], "strong"),
                                          (["--gpus", "2", "--parts-per-rank", "2", "--scaling", "strong"], "strong")])
def test_bench_launches_its_own_ranks(args, scaling):
    """`python bench.py --gpus N` -- no torch.distributed.run in front -- starts its N ranks itself and prints ONE JSON
    line with n_gpus == N from the ring under the C-ABI.  On this one-GPU box the ranks share the GPU
    (--rehearse-on-one-gpu: the driver's shared-memory transport, round launches; not a measurement), everything else is
    the code path of the 8-GPU run: launcher, global plan, id broadcast, ring, timing, the line on stdout."""
    import json
    import os
    import subprocess
    import sys

    from tests.conftest import ROOT

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), *args, "--rehearse-on-one-gpu", "--steps", "2", "--warmup", "1",
                        "--scale", "0.01"], cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=900)
    assert p.returncode == 0, p.stderr[-3000:]
    lines = [x for x in p.stdout.splitlines() if x.strip()]
    assert len(lines) == 1, p.stdout
    out = json.loads(lines[0])
    n = int(args[1])
    assert out["n_gpus"] == n and out["steps"] == 2 and out["scaling"] == scaling
    assert out["config"]["parallelism"] == f"dsgd{n}-native-shm-ring-one-gpu-rehearsal"
    assert out["value"] > 0 and out["rmse_after"] < out["rmse_before"]
    assert out["ring"]["trained"] >= 3 * n * out["config"]["parts_per_rank"] and out["ring"]["bytes_sent"] > 0
    if scaling == "strong":
        assert out["config"]["nnz_global"] > out["config"]["nnz_per_gpu"]


def test_bench_fails_loudly_when_a_rank_fails():
    """A rank that cannot start (here: a workload name that does not exist) makes the launcher exit non-zero without a JSON line."""
    import os
    import subprocess
    import sys

    from tests.conftest import ROOT

    env = {k: v for k, v in os.environ.items() if k not in ("RANK", "LOCAL_RANK", "WORLD_SIZE", "MASTER_ADDR", "MASTER_PORT")}
    p = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "2", "--rehearse-on-one-gpu", "--workload", "no_such"],
                       cwd=ROOT, env=env, stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, timeout=600)
    assert p.returncode != 0 and p.stdout.strip() == ""
