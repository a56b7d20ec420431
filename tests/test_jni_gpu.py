"""The JNI shim's compute natives on the device (tests/jni_fake.py), against the Python surface.

One small problem for every test: 48 users, 40 items, 590 distinct ratings from a fixed seed, k = 10 (kp = 12), and once
more with k = 64 for the training natives.  Five users have 32 ratings each, so exclusion, seen and candidate lists are
not trivial and top-N rows run out of eligible items (padding).  For every native one handle is driven through the fake
JVM and a twin handle through the Python surface with the same calls in the same order; every output must be the same
bytes -- ints, floats, the RMSE and metric doubles -- and the stand-in must have recorded no violation.  No tolerance
appears anywhere."""
import struct

import numpy as np
import pytest

from tests import jni_fake
from tests.jni_fake import Call, Out

pytestmark = pytest.mark.gpu

IAE = "java/lang/IllegalArgumentException"
RTE = "java/lang/RuntimeException"
U, I = 48, 40
LR, LAM, SEED = 0.02, 0.05, 5
HEAVY = 5  # users 0 .. 4 rated 32 of the 40 items


@pytest.fixture(scope="module")
def jvm(mf):
    return jni_fake.load()  # the shim's shared object: built once


def problem():
    """(u, i, r) training triples in a shuffled order, and (hu, hi, hr) held-out pairs that are not among them."""
    rng = np.random.default_rng(2024)
    pairs = [(u, int(i)) for u in range(U) for i in rng.choice(I, 32 if u < HEAVY else 10, replace=False)]
    have = set(pairs)
    order = rng.permutation(len(pairs))
    u = np.array([pairs[x][0] for x in order], np.int32)
    i = np.array([pairs[x][1] for x in order], np.int32)
    r = (rng.random(u.size) * 4 + 1).astype(np.float32)
    held = [(uu, ii) for uu in range(0, U, 2) for ii in range(I) if (uu, ii) not in have and (uu * 7 + ii) % 5 == 0]
    hu, hi = np.array([p[0] for p in held], np.int32), np.array([p[1] for p in held], np.int32)
    hr = (rng.random(hu.size) * 4 + 1).astype(np.float32)
    assert u.size == 590 and hu.size >= 40
    return (u, i, r), (hu, hi, hr)


TRAIN, HELD = problem()
USERS = np.array([0, 7, 3, 47, 0, 20, 4], np.int32)  # heavy and light users, one asked for twice, not sorted


def same(got, want, what=""):
    got, want = np.asarray(got), np.asarray(want)
    assert got.dtype == want.dtype, (what, got.dtype, want.dtype)
    assert got.tobytes() == want.tobytes(), what


def same_double(a, b, what=""):
    assert struct.pack("d", a) == struct.pack("d", b), (what, a, b)


def metrics7(d):
    return np.array([d["n_pairs"], d["n_users"], d["hit_rate"], d["precision"], d["recall"], d["ndcg"], d["mrr"]], np.float64)


class Twins:
    """A handle behind the fake JVM (h) and its twin behind the Python surface (m)."""

    def __init__(self, mf, jvm, k, n_parts=0):
        self.jvm, self.k, self.calls = jvm, k, []
        self.h = jvm.nativeCreate(U, I, k, LR, LAM, 0, n_parts)
        jvm.ok()
        self.m = mf.MatrixFactorizationSGD(U, I, k, LR, LAM, SEED, n_parts=n_parts)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        for c in self.calls:
            c.close()
        self.jvm.nativeDestroy(self.h)
        self.m.close()
        if exc[0] is None:
            self.jvm.ok()
        else:
            self.jvm.pending(), self.jvm.violations()

    def call(self, name, **args):
        """The native on h: no exception, no violation, no input touched."""
        c = Call(self.jvm, name, dict(args, h=self.h))
        self.calls.append(c)
        assert c.pending is None and c.violations == [], (name, c.pending, c.violations)
        c.inputs_intact()
        return c

    def scalar(self, name, *args):
        ret = getattr(self.jvm, name)(self.h, *args)
        self.jvm.ok()
        return ret

    def start(self, epochs=2):
        """Ratings, seeded factors and `epochs` of training on both."""
        u, i, r = TRAIN
        self.call("nativeSetRatings", u=u, i=i, r=r)
        self.m.set_ratings(u, i, r)
        self.scalar("nativeInitFactors", SEED)
        self.m.init_factors()
        if epochs:
            c = self.call("nativeTrain", epochs=epochs, rmsePerEpoch=Out("d", epochs))
            same(c.read("rmsePerEpoch"), self.m.fit(epochs), "nativeTrain: RMSE per epoch")
        return self

    def same_factors(self, what):
        P, Q = self.m.get_factors()
        c = self.call("nativeGetFactors", p=Out("f", P.size), q=Out("f", Q.size))
        same(c.read("p"), P.ravel(), what + ": P")
        same(c.read("q"), Q.ravel(), what + ": Q")

    def top(self, name, n, topn, want, **args):
        """A top-N native: items / scores one element longer than n x topn -- the prefix is the Python surface's, the
        rest keeps its sentinel."""
        c = self.call(name, topN=topn, **args, **{k: Out(e, n * topn + 1) for k, e in self.out_names(name)})
        (ki, _), (ks, _) = self.out_names(name)
        same(c.read(ki)[:-1], want[0].ravel(), name + ": " + ki)
        same(c.read(ks)[:-1], want[1].ravel(), name + ": " + ks)
        assert self.jvm.untouched(c.ref[ki], n * topn) and self.jvm.untouched(c.ref[ks], n * topn), name
        return c

    @staticmethod
    def out_names(name):
        return (("index", "i"), ("scores", "f")) if name.startswith("nativeSimilar") else (("items", "i"), ("scores", "f"))


# ---- training ----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [10, 64])
def test_train_and_rmse(mf, jvm, k):
    with Twins(mf, jvm, k) as t:
        t.start(epochs=0)
        c = t.call("nativeTrain", epochs=3, rmsePerEpoch=Out("d", 5))  # a longer array: the rest keeps its sentinel
        same(c.read("rmsePerEpoch")[:3], t.m.fit(3), "RMSE per epoch")
        assert jvm.untouched(c.ref["rmsePerEpoch"], 3)
        same_double(t.scalar("nativeRmse"), t.m.rmse(), "nativeRmse")
        t.same_factors("after nativeTrain")
        c = t.call("nativeTrain", epochs=0, rmsePerEpoch=Out("d", 1))
        t.m.fit(0)
        assert jvm.untouched(c.ref["rmsePerEpoch"])
        t.same_factors("after zero epochs")


@pytest.mark.parametrize("k", [10, 64])
def test_set_hyper_and_train_schedule_with_and_without_lambda(mf, jvm, k):
    lr = np.array([0.03, 0.03, 0.01], np.float32)
    lam = np.array([0.05, 0.02, 0.02], np.float32)
    with Twins(mf, jvm, k) as t:
        t.start(epochs=1)
        t.scalar("nativeSetHyper", 0.015, 0.04)
        t.m.set_hyper(0.015, 0.04)
        c = t.call("nativeGetHyper", lrLambda=Out("f", 2))
        same(c.read("lrLambda"), np.array(t.m.hyper(), np.float32), "nativeGetHyper")
        for lams in (None, lam):
            c = t.call("nativeTrainSchedule", lr=lr, **{"lambda": lams}, rmsePerEpoch=Out("d", 4))
            same(c.read("rmsePerEpoch")[:3], t.m.fit_schedule(lr, lams), "nativeTrainSchedule")
            assert jvm.untouched(c.ref["rmsePerEpoch"], 3)
            c = t.call("nativeGetHyper", lrLambda=Out("f", 2))
            same(c.read("lrLambda"), np.array(t.m.hyper(), np.float32), "the model keeps the last epoch's values")
            t.same_factors("after nativeTrainSchedule")


@pytest.mark.parametrize("k", [10, 64])
def test_train_bold_driver(mf, jvm, k):
    with Twins(mf, jvm, k) as t:
        t.start(epochs=1)
        c = t.call("nativeTrainBoldDriver", epochs=3, up=1.1, down=0.5, lrUsed=Out("f", 3), rmsePerEpoch=Out("d", 3))
        used, rm = t.m.fit_bold_driver(3, 1.1, 0.5)
        same(c.read("lrUsed"), used, "lrUsed")
        same(c.read("rmsePerEpoch"), rm, "RMSE per epoch")
        t.same_factors("after nativeTrainBoldDriver")
        c = t.call("nativeGetHyper", lrLambda=Out("f", 2))
        same(c.read("lrLambda"), np.array(t.m.hyper(), np.float32), "the rate the next epoch would use")


def test_validation_set_its_rmse_and_the_rmse_of_pairs(mf, jvm):
    hu, hi, hr = HELD
    with Twins(mf, jvm, 10) as t:
        t.start()
        t.call("nativeSetValidation", u=hu, i=hi, r=hr)
        t.m.set_validation(hu, hi, hr)
        assert t.scalar("nativeValidationSize") == t.m.validation_size() == hu.size
        c = t.call("nativeValidationRmse", rmseSse=Out("d", 3))
        same(c.read("rmseSse")[:2], np.array(t.m.validation_rmse(sse=True), np.float64), "nativeValidationRmse")
        assert jvm.untouched(c.ref["rmseSse"], 2)
        u, i, r = TRAIN
        c = t.call("nativeRmsePairs", u=u[:100], i=i[:100], r=r[:100], rmseSse=Out("d", 2))
        same(c.read("rmseSse"), np.array(t.m.rmse_on(u[:100], i[:100], r[:100], sse=True), np.float64), "nativeRmsePairs")


@pytest.mark.parametrize("k", [10, 64])
@pytest.mark.parametrize("full", [False, True])
def test_train_early_stop_with_every_nullable_array_null_and_not(mf, jvm, k, full):
    hu, hi, hr = HELD
    n = 4
    lr = np.array([0.02, 0.04, 0.08, 0.08], np.float32) if full else None
    lam = np.array([0.05, 0.05, 0.01, 0.01], np.float32) if full else None
    with Twins(mf, jvm, k) as t:
        t.start(epochs=1)
        t.call("nativeSetValidation", u=hu, i=hi, r=hr)
        t.m.set_validation(hu, hi, hr)
        c = t.call("nativeTrainEarlyStop", maxEpochs=n, patience=1, minDelta=0.0, restoreBest=1, lr=lr, **{"lambda": lam},
                   valRmse=Out("d", n), trainRmse=Out("d", n) if full else None, epochsRunBestEpoch=Out("i", 2))
        want = t.m.fit_early_stopping(n, patience=1, min_delta=0.0, restore_best=True, lr=lr, lam=lam, train_rmse=full)
        ran = want["epochs_run"]
        same(c.read("epochsRunBestEpoch"), np.array([ran, want["best_epoch"]], np.int32), "{epochs run, best epoch}")
        assert 1 <= ran <= n
        same(c.read("valRmse")[:ran], want["val_rmse"], "valRmse")
        assert jvm.untouched(c.ref["valRmse"], ran)
        if full:
            same(c.read("trainRmse")[:ran], want["train_rmse"], "trainRmse")
            assert jvm.untouched(c.ref["trainRmse"], ran)
        t.same_factors("after nativeTrainEarlyStop")
        c = t.call("nativeGetHyper", lrLambda=Out("f", 2))
        same(c.read("lrLambda"), np.array(t.m.hyper(), np.float32), "lr and lambda of the last epoch run")


def test_apply_ratings_returns_the_errors(mf, jvm):
    hu, hi, hr = HELD
    u = np.concatenate([hu[:30], hu[:5], np.zeros(6, np.int32)])  # pairs twice, and one user six times in a row
    i = np.concatenate([hi[:30], hi[:5], np.arange(6, dtype=np.int32)])
    r = np.concatenate([hr[:30], hr[5:10], hr[:6]])
    with Twins(mf, jvm, 10) as t:
        t.start()
        c = t.call("nativeApplyRatings", u=u, i=i, r=r, err=Out("f", u.size))
        same(c.read("err"), t.m.partial_fit(u, i, r, errors=True), "the errors")
        t.same_factors("after nativeApplyRatings")


# ---- serving -----------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def served(mf, jvm):
    """Trained twins that the serving tests share: none of those calls modifies the model."""
    with Twins(mf, jvm, 10) as t:
        yield t.start()


def test_predict(served):
    u, i, _ = TRAIN
    hu, hi, _ = HELD
    uu, ii = np.concatenate([u[:50], hu]), np.concatenate([i[:50], hi])
    c = served.call("nativePredict", u=uu, i=ii, out=Out("f", uu.size + 2))
    same(c.read("out")[:uu.size], served.m.predict(uu, ii), "nativePredict")
    assert served.jvm.untouched(c.ref["out"], uu.size)


def test_recommend_and_recommend_excluding(served):
    u, i, _ = TRAIN
    served.top("nativeRecommend", USERS.size, 7, served.m.recommend(USERS, 7), users=USERS)
    served.top("nativeRecommend", USERS.size, I, served.m.recommend(USERS, I), users=USERS)
    # with the training pairs excluded a heavy user has 8 items left: topN = 10 pads with -1 / NaN, the same bytes
    want = served.m.recommend(USERS, 10, exclude=(u, i))
    assert (want[0][0] == -1).sum() == 2 and np.isnan(want[1][0]).sum() == 2
    served.top("nativeRecommendExcluding", USERS.size, 10, want, users=USERS, exclU=u, exclI=i)
    none = np.empty(0, np.int32)
    served.top("nativeRecommendExcluding", USERS.size, 3, served.m.recommend(USERS, 3), users=USERS, exclU=none, exclI=none)


def test_recommend_among_a_shared_list_and_per_row_lists(served):
    u, i, _ = TRAIN
    shared = np.array([5, 39, 0, 17, 5, 22, 8, 30, 31, 2, 11], np.int32)  # unsorted, an item twice
    served.top("nativeRecommendAmong", USERS.size, 4, served.m.recommend(USERS, 4, exclude=(u, i), candidates=shared),
               users=USERS, candPtr=None, candItems=shared, exclU=u, exclI=i)
    rng = np.random.default_rng(9)
    lists = [rng.choice(I, n, replace=False).astype(np.int32) for n in (12, 0, 3, 40, 1, 9, 20)]  # an empty one, every item
    ptr = np.zeros(USERS.size + 1, np.int64)
    np.cumsum([x.size for x in lists], out=ptr[1:])
    items = np.concatenate(lists)
    none = np.empty(0, np.int32)
    for eu, ei in ((none, none), (u, i)):
        want = served.m.recommend(USERS, 5, exclude=(eu, ei), candidates=(ptr, items))
        served.top("nativeRecommendAmong", USERS.size, 5, want, users=USERS, candPtr=ptr, candItems=items, exclU=eu, exclI=ei)
    assert (want[0] == -1).any()


def test_the_seen_index_and_the_unseen_natives(mf, jvm):
    u, i, _ = TRAIN
    hu, hi, _ = HELD
    with Twins(mf, jvm, 10) as t:
        t.start()
        assert t.scalar("nativeSeenSize") == t.m.seen_size() == -1
        t.call("nativeSeenUpdate", op=0, u=u[:400], i=i[:400])  # setSeen
        t.m.set_seen(u[:400], i[:400])
        assert t.scalar("nativeSeenSize") == t.m.seen_size() == 400
        t.call("nativeSeenUpdate", op=1, u=u[350:], i=i[350:])  # markSeen: fifty pairs the index already has
        t.m.mark_seen(u[350:], i[350:])
        assert t.scalar("nativeSeenSize") == t.m.seen_size() == u.size
        # seen(): the offsets alone, then with the items; the shim narrows the library's int64 offsets to Java ints
        ptr, items = t.m.seen(USERS)
        assert ptr.dtype == np.int64 and items.size == ptr[-1] > 32
        c = t.call("nativeGetSeen", users=USERS, rowPtr=Out("i", USERS.size + 1), items=None)
        same(c.read("rowPtr"), ptr.astype(np.int32), "offsets only")
        assert np.array_equal(c.read("rowPtr").astype(np.int64), ptr)
        c = t.call("nativeGetSeen", users=USERS, rowPtr=Out("i", USERS.size + 1), items=Out("i", items.size + 3))
        same(c.read("rowPtr"), ptr.astype(np.int32), "offsets")
        same(c.read("items")[:items.size], items, "the lists")
        assert jvm.untouched(c.ref["items"], items.size)
        c = Call(jvm, "nativeGetSeen", dict(h=t.h, users=USERS, rowPtr=Out("i", USERS.size + 1), items=Out("i", items.size - 1)))
        t.calls.append(c)  # too small for the lists: the library's refusal, nothing written
        assert c.pending == (RTE, jvm.last_error(t.h)) and c.violations == []
        c.nothing_written()
        # recommendUnseen in its three forms
        t.top("nativeRecommendUnseen", USERS.size, 10, t.m.recommend(USERS, 10, exclude="seen"), users=USERS, candPtr=None,
              candItems=None)
        shared = np.array([5, 39, 0, 17, 5, 22, 8, 30, 31, 2, 11], np.int32)
        t.top("nativeRecommendUnseen", USERS.size, 4, t.m.recommend(USERS, 4, exclude="seen", candidates=shared), users=USERS,
              candPtr=None, candItems=shared)
        ptr = np.array([0, 11, 11, 14, 20, 21, 30, 31], np.int64)
        cand = (np.arange(31, dtype=np.int32) * 7) % I
        t.top("nativeRecommendUnseen", USERS.size, 4, t.m.recommend(USERS, 4, exclude="seen", candidates=(ptr, cand)),
              users=USERS, candPtr=ptr, candItems=cand)
        # rankItemsUnseen / evaluateRankingUnseen
        c = t.call("nativeRankUnseen", u=hu, i=hi, topN=0, metrics7=None, ranks=Out("i", hu.size + 1))
        same(c.read("ranks")[:hu.size], t.m.rank_items(hu, hi, exclude="seen"), "ranks")
        assert jvm.untouched(c.ref["ranks"], hu.size)
        want = t.m.evaluate_ranking(hu, hi, 5, exclude="seen")
        c = t.call("nativeRankUnseen", u=hu, i=hi, topN=5, metrics7=Out("d", 8), ranks=Out("i", hu.size))
        same(c.read("ranks"), want["ranks"], "ranks with the metrics")
        same(c.read("metrics7")[:7], metrics7(want), "the seven metrics in order")
        assert jvm.untouched(c.ref["metrics7"], 7)
        t.scalar("nativeSeenUpdate", 2, None, None)  # clearSeen
        t.m.clear_seen()
        assert t.scalar("nativeSeenSize") == t.m.seen_size() == -1


def fold_problem(side_size):
    """Three new rows with 6, 0 and 9 ratings (an index twice among them) against `side_size` fixed rows."""
    rng = np.random.default_rng(77)
    ptr = np.array([0, 6, 6, 15], np.int64)
    ids = rng.integers(0, side_size, 15).astype(np.int32)
    ids[7] = ids[8]
    return ptr, ids, (rng.random(15) * 4 + 1).astype(np.float32)


def test_fold_in_users_and_items_seeded_and_from_init(served):
    k = served.k
    init = np.random.default_rng(3).random(3 * k, dtype=np.float32)
    for name, ids_name, fold, size in (("nativeFoldIn", "items", served.m.fold_in, I), ("nativeFoldInItems", "users", served.m.fold_in_items, U)):
        ptr, ids, r = fold_problem(size)
        c = served.call(name, rowPtr=ptr, **{ids_name: ids}, ratings=r, epochs=3, init=None, seed=1234, rows=Out("f", 3 * k))
        same(c.read("rows"), fold(ptr, ids, r, 3, seed=1234).ravel(), name + ": seeded")
        c = served.call(name, rowPtr=ptr, **{ids_name: ids}, ratings=r, epochs=2, init=init, seed=0, rows=Out("f", 3 * k))
        same(c.read("rows"), fold(ptr, ids, r, 2, init=init.reshape(3, k)).ravel(), name + ": from init")
        c = served.call(name, rowPtr=ptr, **{ids_name: ids}, ratings=r, epochs=0, init=init, seed=0, rows=Out("f", 3 * k))
        same(c.read("rows"), init, name + ": zero epochs give the start rows back")


def test_rank_items_rank_items_rows_and_evaluate_ranking(served):
    u, i, _ = TRAIN
    hu, hi, _ = HELD
    none = np.empty(0, np.int32)
    for eu, ei in ((none, none), (u, i)):
        c = served.call("nativeRankItems", u=hu, i=hi, exclU=eu, exclI=ei, ranks=Out("i", hu.size + 1))
        same(c.read("ranks")[:hu.size], served.m.rank_items(hu, hi, exclude=(eu, ei)), "nativeRankItems")
        assert served.jvm.untouched(c.ref["ranks"], hu.size)
        want = served.m.evaluate_ranking(hu, hi, 5, exclude=(eu, ei))
        c = served.call("nativeEvaluateRanking", u=hu, i=hi, topN=5, exclU=eu, exclI=ei, metrics7=Out("d", 7), ranks=Out("i", hu.size))
        same(c.read("ranks"), want["ranks"], "nativeEvaluateRanking: ranks")
        same(c.read("metrics7"), metrics7(want), "nativeEvaluateRanking: the seven metrics in order")
    assert want["n_pairs"] == hu.size and want["n_users"] == np.unique(hu).size
    rows = served.m.get_factors()[0][[3, 0, 20]].copy()
    row, item = np.array([0, 1, 2, 1, 0], np.int32), np.array([4, 9, 30, 0, 39], np.int32)
    er, ei = np.array([1, 1, 2], np.int32), np.array([3, 5, 7], np.int32)
    c = served.call("nativeRankItemsRows", rows=rows.ravel(), row=row, i=item, exclRow=er, exclItem=ei, ranks=Out("i", row.size))
    same(c.read("ranks"), served.m.rank_items_rows(rows, row, item, exclude=(er, ei)), "nativeRankItemsRows")


def test_recommend_rows(served):
    rows = served.m.get_factors()[0][[3, 0, 20]].copy()
    er, ei = np.array([1, 1, 2, 0], np.int32), np.array([3, 5, 7, 0], np.int32)
    served.top("nativeRecommendRows", 3, 6, served.m.recommend_rows(rows, 6, exclude=(er, ei)), rows=rows.ravel(), exclRow=er, exclItem=ei)
    none = np.empty(0, np.int32)
    served.top("nativeRecommendRows", 3, I, served.m.recommend_rows(rows, I), rows=rows.ravel(), exclRow=none, exclItem=none)


def test_similar_items_users_rows_and_the_inverse_norms(served):
    jvm = served.jvm
    q = np.array([39, 0, 17, 0], np.int32)
    served.top("nativeSimilar", q.size, 5, served.m.similar_items(q, 5), side=1, queries=q)
    served.top("nativeSimilar", q.size, 5, served.m.similar_users(q, 5), side=0, queries=q)
    served.top("nativeSimilar", q.size, I, served.m.similar_items(q, I), side=1, queries=q)  # topN = the side: one slot pads
    c = Call(jvm, "nativeSimilar", dict(h=served.h, side=2, queries=q, topN=5, index=Out("i", 20), scores=Out("f", 20)))
    served.calls.append(c)
    assert c.pending is not None and c.pending[0] == IAE and c.violations == []
    c.nothing_written()
    rows = served.m.get_factors()[1][[4, 11]].copy() * np.float32(3)
    for side, name in ((1, "items"), (0, "users")):
        served.top("nativeSimilarRows", 2, 4, served.m.similar_rows(rows, 4, side=name), side=side, rows=rows.ravel())
        n = I if side else U
        c = served.call("nativeRowInvNorms", side=side, out=Out("f", n + 1))
        same(c.read("out")[:n], served.m.row_inv_norms(name), "nativeRowInvNorms")
        assert jvm.untouched(c.ref["out"], n)


# ---- growing -----------------------------------------------------------------------------------------------------------

def test_append_both_sides_rows_and_seeded_then_the_new_sizes_hold(mf, jvm):
    k = 10
    with Twins(mf, jvm, k) as t:
        t.start()
        ptr, ids, r = fold_problem(I)
        new_users = t.m.fold_in(ptr, ids, r, 2, seed=8)
        ptr, ids, r = fold_problem(U)
        new_items = t.m.fold_in_items(ptr, ids, r, 2, seed=9)
        for side, rows, add, old in ((0, new_users, t.m.add_users, U), (1, new_items, t.m.add_items, I)):
            c = t.call("nativeAppend", side=side, rows=rows.ravel(), n=0, seed=0)
            assert c.ret == add(rows) == old
            c = t.call("nativeAppend", side=side, rows=None, n=2, seed=4321)
            assert c.ret == add(n=2, seed=4321) == old + 3
        assert (t.m.users, t.m.items) == (U + 5, I + 5)
        t.same_factors("after nativeAppend")  # arrays of the NEW size succeed ...
        c = Call(jvm, "nativeGetFactors", dict(h=t.h, p=Out("f", U * k), q=Out("f", I * k)))  # ... of the old size are refused
        t.calls.append(c)
        assert c.pending is not None and c.pending[0] == IAE and c.violations == []
        c.nothing_written()
        c = t.call("nativeCapacity", usersItems=Out("i", 2))
        same(c.read("usersItems"), np.array(t.m.capacity(), np.int32), "nativeCapacity")
        # the grown model serves and trains like its twin: the new rows are candidates, neighbours and sized outputs
        users = np.array([U + 4, 0, U], np.int32)
        t.top("nativeRecommend", 3, I + 5, t.m.recommend(users, I + 5), users=users)
        c = t.call("nativeRowInvNorms", side=0, out=Out("f", U + 5))
        same(c.read("out"), t.m.row_inv_norms("users"), "nativeRowInvNorms over the grown side")
        c = Call(jvm, "nativeRowInvNorms", dict(h=t.h, side=0, out=Out("f", U)))
        t.calls.append(c)
        assert c.pending is not None and c.pending[0] == IAE and c.violations == []
        c.nothing_written()
        t.top("nativeSimilar", 3, 4, t.m.similar_users(users, 4), side=0, queries=users)
        c = t.call("nativeTrain", epochs=1, rmsePerEpoch=Out("d", 1))
        same(c.read("rmsePerEpoch"), t.m.fit(1), "training after the appends")
        t.same_factors("after training the grown model")


# ---- DSGD ----------------------------------------------------------------------------------------------------------------

def test_the_ring_natives_at_world_one_with_two_item_partitions(mf, jvm):
    """nativeDsgdUniqueId -> nativeDsgdCreate -> nativeDsgdInitQ -> nativeDsgdTrain -> nativeDsgdRmse -> nativeDsgdGetQ
    (sizes only, then the block) -> nativeDsgdDestroy, against NativeDSGD on the twin: a self-ring whose blocks go
    through both buffers.  The two rings live one after the other."""
    from mfsgd_amd import _lib
    from mfsgd_amd.dsgd import NativeDSGD

    u, i, r = TRAIN
    k, epochs = 10, 3
    with Twins(mf, jvm, k, n_parts=2) as t:
        t.m.set_ratings(u, i, r)
        t.m.init_p_offset(SEED, 0)
        with NativeDSGD(t.m, 0, 1, NativeDSGD.unique_id()) as d:
            d.init_q(SEED, U)
            rm0, rm, rm1 = d.rmse(), d.train(epochs), d.rmse()
            blocks = d.home_blocks()
        P = t.m.get_factors()[0]

        _lib.share_torch_rccl()
        t.call("nativeSetRatings", u=u, i=i, r=r)
        t.scalar("nativeInitPOffset", SEED, 0)
        ident = jvm.nativeDsgdUniqueId()
        jvm.ok()
        assert ident and jvm.read(ident).size == 128 and jvm.written(ident)
        ring = jvm.nativeDsgdCreate(t.h, 0, 1, ident)
        jvm.ok()
        assert ring
        try:
            jvm.nativeDsgdInitQ(ring, SEED, U)
            jvm.ok()
            same_double(jvm.nativeDsgdRmse(ring), rm0, "nativeDsgdRmse before training")
            jvm.ok()
            c = Call(jvm, "nativeDsgdTrain", dict(d=ring, epochs=epochs, rmsePerEpoch=Out("d", epochs + 1)))
            t.calls.append(c)
            assert c.pending is None and c.violations == []
            same(c.read("rmsePerEpoch")[:epochs], rm, "nativeDsgdTrain")
            assert jvm.untouched(c.ref["rmsePerEpoch"], epochs)
            same_double(jvm.nativeDsgdRmse(ring), rm1, "nativeDsgdRmse after training")
            jvm.ok()
            seen_parts = set()
            for slot in range(2):
                c = Call(jvm, "nativeDsgdGetQ", dict(d=ring, slot=slot, partRows=Out("i", 2), block=None))  # the sizes only
                t.calls.append(c)
                assert c.pending is None and c.violations == []
                part, rows = (int(x) for x in c.read("partRows"))
                assert rows == blocks[part].shape[0]
                c = Call(jvm, "nativeDsgdGetQ", dict(d=ring, slot=slot, partRows=Out("i", 2), block=Out("f", rows * k)))
                t.calls.append(c)
                assert c.pending is None and c.violations == []
                same(c.read("partRows"), np.array([part, rows], np.int32), "partRows")
                same(c.read("block"), blocks[part].ravel(), f"the block of partition {part}")
                seen_parts.add(part)
            assert seen_parts == set(blocks) == {0, 1}
            c = Call(jvm, "nativeDsgdGetQ", dict(d=ring, slot=2, partRows=Out("i", 2), block=None))  # no such slot
            t.calls.append(c)
            assert c.pending is not None and c.pending[0] == RTE and c.pending[1] and c.violations == []
            c.nothing_written()
        finally:
            jvm.nativeDsgdDestroy(ring)
            jvm.free(ident)
        jvm.ok()
        c = t.call("nativeGetUserFactors", p=Out("f", U * k))
        same(c.read("p"), P.ravel(), "P after the ring")
