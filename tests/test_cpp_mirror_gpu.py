"""cpp/MatrixFactorizationSGD.hpp, every public method, against the Python surface.

tests/cpp_mirror_driver.cpp is built here with g++ against the header and lib/libmfsgd.so.  On the device it reads one
problem file, calls every public method of the header in a fixed script and writes each result as raw bytes; the test
replays the script through the Python surface and compares the bytes, step by step.  The script grows the model in the
middle (addUsers / addItems) and goes on reading it: the header caches its row counts, and that is where it could go
wrong.  Without a device: the guard that the driver calls every public method the header has, and the header's own
std::invalid_argument screens."""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

from tests.conftest import ROOT

PKG = os.path.join(ROOT, "matrixfactorizationsgd.java_amd")
HEADER = os.path.join(PKG, "cpp", "MatrixFactorizationSGD.hpp")
DRIVER = os.path.join(ROOT, "tests", "cpp_mirror_driver.cpp")

U, I, K, SEED = 48, 40, 10, 5
LR, LAM = 0.02, 0.05


@pytest.fixture(scope="module")
def driver(mf, tmp_path_factory):
    """The driver program, built once."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    libdir = os.path.join(PKG, "lib")
    exe = str(tmp_path_factory.mktemp("cpp_mirror") / "cpp_mirror_driver")
    p = subprocess.run([cxx, "-std=c++17", "-O1", "-Wall", "-Wextra", "-Werror", DRIVER, "-L" + libdir, "-lmfsgd",
                        "-Wl,-rpath," + libdir, "-Wl,-rpath,/opt/rocm/lib", "-o", exe],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    return exe


# ---- without a device --------------------------------------------------------------------------------------------------

def public_methods():
    """The names of the public member functions of the header's class (constructor, destructor and operators aside)."""
    text = open(HEADER).read()
    body = text[text.index("   public:"):text.index("   private:")]
    body = re.sub(r"//[^\n]*", "", body)
    names = set(re.findall(r"^    (?:static )?(?:[\w:]+(?:<[^;(){}]*>)?[&*]?) (\w+)\(", body, flags=re.M))
    return names - {"MatrixFactorizationSGD", "operator"}


# the driver calls every method, these included, so nothing is exempt; a method that cannot be driven goes here with its reason
EXEMPT = set()


def test_the_driver_calls_every_public_method_of_the_header():
    """A method added to the header without a line in the driver fails here."""
    methods = public_methods()
    assert {"train", "predict", "recommendRowsAmong", "seen", "foldInItems", "addUsers", "trainEarlyStopping", "plan",
            "distributedId", "itemBlocks", "ringStats", "close", "users", "items", "evaluateRankingUnseen"} <= methods
    assert len(methods) >= 50, sorted(methods)
    src = re.sub(r"//[^\n]*", "", open(DRIVER).read())
    run_part = src[src.index("int run("):src.index("template <class F>")]
    called = set(re.findall(r"\bmf_\w+\.(\w+)\(", run_part)) | set(re.findall(r"MatrixFactorizationSGD::(\w+)\(", run_part))
    assert methods - called - EXEMPT == set(), f"public methods the driver never calls: {sorted(methods - called - EXEMPT)}"
    assert called - methods == set(), f"the driver calls what the header does not have: {sorted(called - methods)}"


SCREENS = """train\tinvalid_argument\tlength mismatch
train r\tinvalid_argument\tlength mismatch
predict\tinvalid_argument\tlength mismatch
recommend\tinvalid_argument\tlength mismatch
foldIn empty rowPtr\tinvalid_argument\tlength mismatch
foldIn ratings\tinvalid_argument\tlength mismatch
foldIn rowPtr end\tinvalid_argument\tlength mismatch
foldIn init is n x kp\tinvalid_argument\tlength mismatch
foldInItems ratings\tinvalid_argument\tlength mismatch
foldInItems init is n x kp\tinvalid_argument\tlength mismatch
addUsers\tinvalid_argument\trows must be n x k
addItems\tinvalid_argument\trows must be n x k
counts\t6\t5
recommendRows rows\tinvalid_argument\tlength mismatch
recommendRows excl\tinvalid_argument\tlength mismatch
recommendAmong candPtr\tinvalid_argument\tlength mismatch
recommendAmong excl\tinvalid_argument\tlength mismatch
recommendRowsAmong rows\tinvalid_argument\tlength mismatch
recommendRowsAmong candPtr\tinvalid_argument\tlength mismatch
recommendRowsAmong excl\tinvalid_argument\tlength mismatch
similarRows\tinvalid_argument\tlength mismatch
rowInvNorms\tinvalid_argument\tside
rankItems\tinvalid_argument\tlength mismatch
rankItems excl\tinvalid_argument\tlength mismatch
rankItemsRows rows\tinvalid_argument\tlength mismatch
rankItemsRows pairs\tinvalid_argument\tlength mismatch
evaluateRanking\tinvalid_argument\tlength mismatch
setSeen\tinvalid_argument\tlength mismatch
markSeen\tinvalid_argument\tlength mismatch
recommendUnseenAmong\tinvalid_argument\tlength mismatch
rankItemsUnseen\tinvalid_argument\tlength mismatch
evaluateRankingUnseen\tinvalid_argument\tlength mismatch
trainSchedule\tinvalid_argument\tlength mismatch
trainBoldDriver\tinvalid_argument\tnegative epochs
partialFit\tinvalid_argument\tlength mismatch
onlineLevels\tinvalid_argument\tlength mismatch
setValidation\tinvalid_argument\tlength mismatch
rmseOn\tinvalid_argument\tlength mismatch
trainEarlyStopping epochs\tinvalid_argument\tnegative maxEpochs
trainEarlyStopping lr\tinvalid_argument\tlength mismatch
trainEarlyStopping lambda\tinvalid_argument\tlength mismatch
plan\tinvalid_argument\tplan: bad argument
trainDistributed without partitions\tlogic_error\tcreated without item partitions
trainDistributed lengths\tinvalid_argument\tlength mismatch
trainDistributed itemPart\tinvalid_argument\titemPart must have one entry per item
capacity\t8\t5
hyper\t0.00999999978\t0.0500000007
sizes\t0\t-1
create\truntime_error\tmfsgd_create: mfsgd_create: k exceeds MFSGD_MAX_K (256)
"""


def test_the_headers_argument_screens(driver):
    """Every std::invalid_argument screen of the header (`length mismatch`, `rows must be n x k`, ...) fires before the
    library is reached -- the counts, capacity, hyper-parameters and set sizes afterwards are those of a fresh model --
    and k = 10 rows of kp = 12 floats are refused wherever rows are taken.  Needs no device."""
    p = subprocess.run(["timeout", "-k", "10", "60", driver, "screens"], stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0, (p.returncode, p.stderr)
    assert p.stdout.splitlines() == SCREENS.splitlines()


# ---- on the device -----------------------------------------------------------------------------------------------------

def problem():
    rng = np.random.default_rng(4048)
    pairs = [(u, int(i)) for u in range(U) for i in rng.choice(I, 32 if u < 5 else 10, replace=False)]
    have = set(pairs)
    order = rng.permutation(len(pairs))
    u = np.array([pairs[x][0] for x in order], np.int32)
    i = np.array([pairs[x][1] for x in order], np.int32)
    held = [(uu, ii) for uu in range(0, U, 2) for ii in range(I) if (uu, ii) not in have and (uu * 7 + ii) % 5 == 0]
    lists = [rng.choice(I, n, replace=False).astype(np.int32) for n in (12, 0, 3, 40, 1, 9, 20)]
    cand = np.concatenate(lists)
    fold_ptr = np.array([0, 6, 6, 15], np.int64)
    d = dict(
        sizes=np.array([U, I, K, SEED], np.int32), hyper=np.array([LR, LAM], np.float32),
        u=u, i=i, r=(rng.random(u.size) * 4 + 1).astype(np.float32),
        hu=np.array([p[0] for p in held], np.int32), hi=np.array([p[1] for p in held], np.int32),
        hr=(rng.random(len(held)) * 4 + 1).astype(np.float32),
        users=np.array([0, 7, 3, 47, 0, 20, 4], np.int32),
        shared=np.array([5, 39, 0, 17, 5, 22, 8, 30, 31, 2, 11], np.int32),
        cand=cand, cand_ptr=np.concatenate([[0], np.cumsum([x.size for x in lists])]).astype(np.int64),
        rows_cand_ptr=np.array([0, 30, 30, cand.size], np.int64),
        excl_row=np.array([1, 1, 2, 0], np.int32), excl_item=np.array([3, 5, 7, 0], np.int32),
        row_of_pair=np.array([0, 1, 2, 1, 0], np.int32), item_of_pair=np.array([4, 9, 30, 0, 39], np.int32),
        fold_ptr=fold_ptr, fold_items=rng.integers(0, I, 15).astype(np.int32), fold_users=rng.integers(0, U, 15).astype(np.int32),
        fold_r=(rng.random(15) * 4 + 1).astype(np.float32), fold_init=rng.random(3 * K, dtype=np.float32),
        queries=np.array([39, 0, 17, 0], np.int32),
        online_u=np.concatenate([u[:40], np.zeros(6, np.int32)]).astype(np.int32),
        online_i=np.concatenate([i[40:80], np.arange(6, dtype=np.int32)]).astype(np.int32),
        online_r=(rng.random(46) * 4 + 1).astype(np.float32),
        sched_lr=np.array([0.03, 0.03, 0.01], np.float32), sched_lam=np.array([0.05, 0.02, 0.02], np.float32),
        stop_lr=np.array([0.02, 0.04, 0.08, 0.08], np.float32), stop_lam=np.array([0.05, 0.05, 0.01, 0.01], np.float32),
        grown_users=np.array([U + 4, 0, U], np.int32),
        deg_user=np.bincount(u, minlength=U).astype(np.int64), deg_item=np.bincount(i, minlength=I).astype(np.int64),
    )
    assert u.size == 590 and d["hu"].size >= 40
    return d


def replay(mf, d):
    """The driver's script through the Python surface: {step: bytes}."""
    from mfsgd_amd.dsgd import NativeDSGD

    out = {}

    def put(step, a, dtype):
        out[step] = np.ascontiguousarray(a, dtype).tobytes()

    def two(step, pair, a=np.int32, b=np.float32):
        put(step + ".0", pair[0], a)
        put(step + ".1", pair[1], b)

    def metrics(step, m):
        put(step + ".metrics", [m["n_pairs"], m["n_users"], m["hit_rate"], m["precision"], m["recall"], m["ndcg"], m["mrr"]], np.float64)
        put(step + ".ranks", m["ranks"], np.int32)

    def info(step, x):
        put(step, [x["n"], x["pieces"], x["levels"], x["max_width"], x["launches"]], np.int64)

    def early(step, e):
        put(step + ".val", e["val_rmse"], np.float64)
        put(step + ".train", [] if e["train_rmse"] is None else e["train_rmse"], np.float64)
        put(step + ".ran_best", [e["epochs_run"], e["best_epoch"]], np.int32)

    u, i, r, hu, hi, hr, users = (d[x] for x in ("u", "i", "r", "hu", "hi", "hr", "users"))
    excl = (d["excl_row"], d["excl_item"])
    with mf.MatrixFactorizationSGD(U, I, K, LR, LAM, SEED) as m:
        put("a01_train", m.train(u, i, r, 2), np.float64)
        put("a02_rmse", m.rmse(), np.float64)
        put("a03_predict_one", m.predict(int(hu[0]), int(hi[0])), np.float32)
        put("a04_predict", m.predict(hu, hi), np.float32)
        two("a05_hyper", m.hyper(), np.float32)
        two("a06_factors", m.get_factors(), np.float32)
        two("a07_recommend", m.recommend(users, 7))
        two("a08_recommend_excluding", m.recommend(users, 10, exclude=(u, i)))
        two("a09_among_shared", m.recommend(users, 4, exclude=(u, i), candidates=d["shared"]))
        two("a10_among_rows", m.recommend(users, 5, candidates=(d["cand_ptr"], d["cand"])))
        two("a11_among_rows_excluding", m.recommend(users, 5, exclude=(u, i), candidates=(d["cand_ptr"], d["cand"])))

        rows = m.fold_in(d["fold_ptr"], d["fold_items"], d["fold_r"], 3, seed=1234)
        put("b01_fold_in_seeded", rows, np.float32)
        put("b02_fold_in_init", m.fold_in(d["fold_ptr"], d["fold_items"], d["fold_r"], 2, init=d["fold_init"].reshape(3, K)), np.float32)
        item_rows = m.fold_in_items(d["fold_ptr"], d["fold_users"], d["fold_r"], 3, seed=4321)
        put("b03_fold_in_items_seeded", item_rows, np.float32)
        put("b04_fold_in_items_init", m.fold_in_items(d["fold_ptr"], d["fold_users"], d["fold_r"], 2, init=d["fold_init"].reshape(3, K)), np.float32)
        two("b05_recommend_rows", m.recommend_rows(rows, 6, exclude=excl))
        two("b06_recommend_rows_all", m.recommend_rows(rows, I))
        two("b07_rows_among_shared", m.recommend_rows(rows, 4, exclude=excl, candidates=d["shared"]))
        two("b08_rows_among_rows", m.recommend_rows(rows, 4, candidates=(d["rows_cand_ptr"], d["cand"])))

        put("c01_rank_items", m.rank_items(hu, hi), np.int32)
        put("c02_rank_items_excluding", m.rank_items(hu, hi, exclude=(u, i)), np.int32)
        put("c03_rank_items_rows", m.rank_items_rows(rows, d["row_of_pair"], d["item_of_pair"], exclude=excl), np.int32)
        metrics("c04_evaluate_ranking", m.evaluate_ranking(hu, hi, 5, exclude=(u, i)))
        two("c05_similar_items", m.similar_items(d["queries"], 5))
        two("c06_similar_users", m.similar_users(d["queries"], 5))
        two("c07_similar_rows_items", m.similar_rows(rows, 4, side="items"))
        two("c08_similar_rows_users", m.similar_rows(rows, 4, side="users"))
        put("c09_inv_norms_users", m.row_inv_norms("users"), np.float32)
        put("c10_inv_norms_items", m.row_inv_norms("items"), np.float32)

        put("d01_seen_size_none", m.seen_size(), np.int64)
        m.set_seen(u[:400], i[:400])
        put("d02_seen_size_set", m.seen_size(), np.int64)
        m.mark_seen(u[350:], i[350:])
        put("d03_seen_size_marked", m.seen_size(), np.int64)
        two("d04_seen", m.seen(users), np.int64, np.int32)
        two("d05_recommend_unseen", m.recommend(users, 10, exclude="seen"))
        two("d06_unseen_among_shared", m.recommend(users, 4, exclude="seen", candidates=d["shared"]))
        two("d07_unseen_among_rows", m.recommend(users, 4, exclude="seen", candidates=(d["cand_ptr"], d["cand"])))
        put("d08_rank_unseen", m.rank_items(hu, hi, exclude="seen"), np.int32)
        metrics("d09_evaluate_unseen", m.evaluate_ranking(hu, hi, 5, exclude="seen"))
        m.clear_seen()
        put("d10_seen_size_cleared", m.seen_size(), np.int64)

        m.set_validation(hu, hi, hr)
        put("e01_validation_size", m.validation_size(), np.int64)
        rm, sse = m.validation_rmse(sse=True)
        put("e02_validation_rmse", rm, np.float64)
        put("e03_validation_sse", sse, np.float64)
        rm, sse = m.rmse_on(u[:100], i[:100], r[:100], sse=True)
        put("e04_rmse_on", rm, np.float64)
        put("e05_rmse_on_sse", sse, np.float64)
        m.set_hyper(np.float32(0.015), np.float32(0.04))
        two("e06_hyper", m.hyper(), np.float32)
        put("e07_schedule", m.fit_schedule(d["sched_lr"]), np.float64)
        put("e08_schedule_lambda", m.fit_schedule(d["sched_lr"], d["sched_lam"]), np.float64)
        two("e09_bold_driver", m.fit_bold_driver(3, np.float32(1.1), np.float32(0.5)), np.float32, np.float64)
        early("e10_early_stop", m.fit_early_stopping(4, 1, 0.0, True, d["stop_lr"], d["stop_lam"], True))
        early("e11_early_stop_defaults", m.fit_early_stopping(3))
        two("e12_factors", m.get_factors(), np.float32)

        levels, x = m.online_levels(d["online_u"], d["online_i"])
        put("f01_levels", levels, np.int32)
        info("f02_levels_info", x)
        err, x = m.partial_fit(d["online_u"], d["online_i"], d["online_r"], errors=True, info=True)
        put("f03_partial_fit", err, np.float32)
        info("f04_partial_fit_info", x)

        m.reserve(U + 3, None)
        put("g01_capacity", m.capacity(), np.int32)
        put("g02_add_users_rows", m.add_users(rows), np.int32)
        put("g03_add_users_seeded", m.add_users(n=2, seed=99), np.int32)
        put("g04_add_items_rows", m.add_items(item_rows), np.int32)
        put("g05_add_items_seeded", m.add_items(n=2, seed=77), np.int32)
        put("g06_counts", [m.users, m.items], np.int32)
        put("g07_capacity", m.capacity(), np.int32)
        two("g08_factors", m.get_factors(), np.float32)
        two("g09_recommend", m.recommend(d["grown_users"], I + 5))
        put("g10_inv_norms_users", m.row_inv_norms("users"), np.float32)
        put("g11_inv_norms_items", m.row_inv_norms("items"), np.float32)
        two("g12_similar_users", m.similar_users(d["grown_users"], 4))
        put("g13_train_again", m.train(u, i, r, 1), np.float64)
        two("g14_factors", m.get_factors(), np.float32)
        assert (m.users, m.items) == (U + 5, I + 5)

    plan = mf.trainer.dsgd_plan(d["deg_user"], d["deg_item"], 2)
    two("h01_plan", plan, np.int32, np.int32)
    with mf.MatrixFactorizationSGD(U, I, K, LR, LAM, SEED, n_parts=2) as t:
        t.set_item_partition(plan[1])
        t.set_ratings(u, i, r)
        t.init_p_offset(SEED, 0)
        with NativeDSGD(t, 0, 1, NativeDSGD.unique_id()) as ring:
            ring.init_q(SEED, U)
            put("h02_train_distributed", ring.train(3), np.float64)
            put("h03_rmse_distributed", ring.rmse(), np.float64)
            put("h04_user_factors", t.get_factors()[0], np.float32)
            for j, (part, block) in enumerate(ring.home_blocks().items()):  # in slot order
                put(f"h05_block{j}.part", part, np.int32)
                put(f"h05_block{j}.rows", block, np.float32)
            s = ring.stats()
            put("h06_ring_trained_and_bytes", [s["trained"], s["bytes_sent"]], np.int64)
            put("h07_train_distributed_again", ring.train(1), np.float64)
    return out


@pytest.mark.gpu
def test_every_method_of_the_cpp_mirror_returns_what_the_python_surface_returns(mf, driver, tmp_path):
    d = problem()
    path = tmp_path / "problem.bin"
    with open(path, "wb") as f:
        for name, a in d.items():
            raw = np.ascontiguousarray(a).tobytes()
            f.write(struct.pack("<i", len(name)) + name.encode() + struct.pack("<q", len(raw)) + raw)
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    # a fresh child process under its own time limit
    p = subprocess.run(["timeout", "-k", "10", "120", driver, "run", str(path), str(out_dir)], stdout=subprocess.PIPE,
                       stderr=subprocess.PIPE, text=True)
    assert p.returncode == 0 and p.stdout.splitlines()[-1:] == ["done"], (p.returncode, p.stdout, p.stderr)  # (RCCL prints its banner)
    got = {f[:-4]: open(out_dir / f, "rb").read() for f in sorted(os.listdir(out_dir)) if f.endswith(".bin")}
    want = replay(mf, d)
    assert sorted(got) == sorted(want)
    assert len(want["g08_factors.0"]) == (U + 5) * K * 4 and len(want["g10_inv_norms_users"]) == (U + 5) * 4
    assert len(want["d04_seen.1"]) > 32 * 4 and b"\xff\xff\xff\xff" in want["a08_recommend_excluding.0"]  # item -1: a padded row
    different = [step for step in sorted(want) if got[step] != want[step]]
    assert different == [], f"steps whose bytes differ from the Python surface's: {different}"
