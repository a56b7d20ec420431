"""The JNI shim, executed (tests/jni_fake.py): what needs no GPU.

Signature conformance of all natives with the Java class; argument screening of every native, one broken argument at a
time, and the class and text of every such refusal against a recorded file; status -> exception; no exception without
a message; the natives that run on the host compared bit for bit with the Python surface on a twin handle; array
handling; and the guard that every native the shim defines is named by a test here or in tests/test_jni_gpu.py.  Every
comparison is of bytes."""
import contextlib
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests import jni_fake
from tests.jni_fake import Call, Out
from tests.conftest import ROOT, have_gpu

NPE = "java/lang/NullPointerException"
IAE = "java/lang/IllegalArgumentException"
RTE = "java/lang/RuntimeException"

U, I, K, KP = 6, 5, 10, 12  # k = 10 lives in rows of kp = 12 floats on the device: a shim that mixes them up shows here
LR, LAM, SEED = 0.01, 0.05, 11
N, TOPN, EPOCHS = 4, 2, 2

@pytest.fixture(scope="module")
def jvm(mf):
    return jni_fake.load()


@contextlib.contextmanager
def adopted(mf, h, k=K):
    """The Python surface over a handle the shim created: for looking at the handle's state (it is not closed here)."""
    m = object.__new__(mf.MatrixFactorizationSGD)
    m._lib, m._h, m.k, m.n_parts = mf.load_library(), C.c_void_p(h), k, 1
    try:
        m._dims()
        yield m
    finally:
        m._h = C.c_void_p()


def state(mf, jvm, h):
    """Everything observable of a single-partition handle that a call into the C-ABI could have changed."""
    with adopted(mf, h) as m:
        P, Q = m.get_factors()
        return (m.users, m.items, P.tobytes(), Q.tobytes(), m.hyper(), m.capacity(), m.seen_size(), m.validation_size(),
                tuple(sorted(m.debug_counters().items())), jvm.last_error(h))


@pytest.fixture(scope="module")
def model(mf, jvm):
    """A handle made through the shim: ratings and seeded factors on the host, and a known text in mfsgd_last_error."""
    h = jvm.nativeCreate(U, I, K, LR, LAM, 0, 0)
    jvm.ok()
    tri = triples()
    a = [jvm.arr(x) for x in tri]
    jvm.nativeSetRatings(h, *a)
    jvm.ok()
    jvm.nativeInitFactors(h, SEED)
    jvm.ok()
    jvm.free(*a)
    jvm.nativeSetHyper(h, float("nan"), LAM)  # refused: leaves "set_hyper: ..." as the handle's last error
    assert jvm.pending()[0] == RTE and jvm.last_error(h).startswith("set_hyper")
    yield h
    jvm.nativeDestroy(h)


def triples():
    return (np.array([0, 1, 2, 5], np.int32), np.array([0, 1, 4, 2], np.int32), np.array([1.0, 2.5, 4.0, 3.0], np.float32))


def i32(*v):
    return np.array(v, np.int32)


def f32(n, seed=3):
    return np.random.default_rng(seed).random(n, dtype=np.float32)


def valid(h):
    """{native: {parameter name: value}} -- for every native that takes an array, a call that passes every screen of the
    shim on the module's model.  Arrays are numpy arrays (inputs) or Out (outputs)."""
    u, i, r = triples()
    eu, ei = i32(0, 1), i32(3, 1)
    rows = f32(2 * K)
    rp = np.array([0, 1, N], np.int64)
    rec = dict(items=Out("i", N * TOPN), scores=Out("f", N * TOPN))
    fold = dict(h=h, rowPtr=rp, ratings=r, epochs=1, init=f32(2 * K, 4), seed=7, rows=Out("f", 2 * K))
    return {
        "nativeSetRatings": dict(h=h, u=u, i=i, r=r),
        "nativeSetFactors": dict(h=h, p=f32(U * K, 1), q=f32(I * K, 2)),
        "nativeGetFactors": dict(h=h, p=Out("f", U * K), q=Out("f", I * K)),
        "nativeTrain": dict(h=h, epochs=EPOCHS, rmsePerEpoch=Out("d", EPOCHS)),
        "nativeGetHyper": dict(h=h, lrLambda=Out("f", 2)),
        "nativeTrainSchedule": dict(h=h, lr=f32(EPOCHS), **{"lambda": f32(EPOCHS)}, rmsePerEpoch=Out("d", EPOCHS)),
        "nativeTrainBoldDriver": dict(h=h, epochs=EPOCHS, up=1.05, down=0.5, lrUsed=Out("f", EPOCHS),
                                      rmsePerEpoch=Out("d", EPOCHS)),
        "nativeSetValidation": dict(h=h, u=u, i=i, r=r),
        "nativeValidationRmse": dict(h=h, rmseSse=Out("d", 2)),
        "nativeRmsePairs": dict(h=h, u=u, i=i, r=r, rmseSse=Out("d", 2)),
        "nativeTrainEarlyStop": dict(h=h, maxEpochs=EPOCHS, patience=1, minDelta=0.0, restoreBest=1, lr=f32(EPOCHS),
                                     **{"lambda": f32(EPOCHS)}, valRmse=Out("d", EPOCHS), trainRmse=Out("d", EPOCHS),
                                     epochsRunBestEpoch=Out("i", 2)),
        "nativeApplyRatings": dict(h=h, u=u, i=i, r=r, err=Out("f", N)),
        "nativePredict": dict(h=h, u=u, i=i, out=Out("f", N)),
        "nativeRecommend": dict(h=h, users=u, topN=TOPN, **rec),
        "nativeRecommendExcluding": dict(h=h, users=u, topN=TOPN, exclU=eu, exclI=ei, **rec),
        "nativeRecommendAmong": dict(h=h, users=u, topN=TOPN, candPtr=np.array([0, 1, 2, 3, 3], np.int64),
                                     candItems=i32(0, 1, 2), exclU=eu, exclI=ei, **rec),
        "nativeSeenUpdate": dict(h=h, op=0, u=u, i=i),
        "nativeGetSeen": dict(h=h, users=u, rowPtr=Out("i", N + 1), items=Out("i", 8)),
        "nativeRecommendUnseen": dict(h=h, users=u, topN=TOPN, candPtr=np.array([0, 1, 2, 3, 3], np.int64),
                                      candItems=i32(0, 1, 2), **rec),
        "nativeRankUnseen": dict(h=h, u=u, i=i, topN=TOPN, metrics7=Out("d", 7), ranks=Out("i", N)),
        "nativeFoldIn": dict(fold, items=i),
        "nativeFoldInItems": dict(fold, users=u),
        "nativeAppend": dict(h=h, side=0, rows=rows, n=0, seed=1),
        "nativeCapacity": dict(h=h, usersItems=Out("i", 2)),
        "nativeSimilar": dict(h=h, side=1, queries=i32(0, 3), topN=TOPN, index=Out("i", 2 * TOPN), scores=Out("f", 2 * TOPN)),
        "nativeSimilarRows": dict(h=h, side=1, rows=rows, topN=TOPN, index=Out("i", 2 * TOPN), scores=Out("f", 2 * TOPN)),
        "nativeRowInvNorms": dict(h=h, side=1, out=Out("f", I)),
        "nativeRankItems": dict(h=h, u=u, i=i, exclU=eu, exclI=ei, ranks=Out("i", N)),
        "nativeRankItemsRows": dict(h=h, rows=rows, row=i32(0, 1, 1, 0), i=i, exclRow=i32(0, 1), exclItem=ei,
                                    ranks=Out("i", N)),
        "nativeEvaluateRanking": dict(h=h, u=u, i=i, topN=TOPN, exclU=eu, exclI=ei, metrics7=Out("d", 7), ranks=Out("i", N)),
        "nativeRecommendRows": dict(h=h, rows=rows, topN=TOPN, exclRow=i32(0, 1), exclItem=ei,
                                    items=Out("i", 2 * TOPN), scores=Out("f", 2 * TOPN)),
        "nativeDsgdPlan": dict(degUser=np.array([3, 1, 2, 2], np.int64), degItem=np.array([4, 1, 3], np.int64), nParts=2,
                               userBegin=Out("i", 3), itemPart=Out("i", 3)),
        "nativeSetItemPartition": dict(h=h, itemPart=i32(0, 1, 0, 1, 0)),
        "nativeGetUserFactors": dict(h=h, p=Out("f", U * K)),
        # (world = 2 on a handle without item partitions: should the call get through the shim, the library refuses it
        # before it looks at the id -- a made-up id must never reach a communicator)
        "nativeDsgdCreate": dict(h=h, rank=0, world=2, id=np.zeros(128, np.int8)),
        "nativeDsgdTrain": dict(d=0, epochs=EPOCHS, rmsePerEpoch=Out("d", EPOCHS)),
        "nativeDsgdGetQ": dict(d=0, slot=0, partRows=Out("i", 2), block=Out("f", 4)),
    }


# the natives that take no array: nothing for the shim to screen
SCALAR_ONLY = {"nativeCreate", "nativeDestroy", "nativeInitFactors", "nativeRmse", "nativeSetHyper", "nativeValidationSize",
               "nativeSeenSize", "nativeReserve", "nativeInitPOffset", "nativeDsgdUniqueId", "nativeDsgdDestroy",
               "nativeDsgdInitQ", "nativeDsgdRmse"}

# array parameters that may be null, as the shim documents them
NULLABLE = {
    "nativeTrainSchedule": {"lambda"},
    "nativeTrainEarlyStop": {"lr", "lambda", "trainRmse"},
    "nativeRecommendAmong": {"candPtr"},
    "nativeGetSeen": {"items"},
    "nativeRecommendUnseen": {"candPtr", "candItems"},  # but candPtr without candItems is refused: below
    "nativeRankUnseen": {"metrics7"},
    "nativeFoldIn": {"init"},
    "nativeFoldInItems": {"init"},
    "nativeAppend": {"rows"},
    "nativeDsgdGetQ": {"block"},
}

R3 = np.array([1.0, 2.0, 3.0], np.float32)
REC_BREAKS = [("items shorter than n x topN", dict(items=Out("i", N * TOPN - 1))),
              ("scores shorter than n x topN", dict(scores=Out("f", N * TOPN - 1))), ("topN < 1", dict(topN=0))]
ROWS_REC_BREAKS = [("items shorter than rows x topN", dict(items=Out("i", 2 * TOPN - 1))),
                   ("scores shorter than rows x topN", dict(scores=Out("f", 2 * TOPN - 1))), ("topN < 1", dict(topN=0))]
TRIPLE_BREAKS = [("i shorter than u", dict(i=i32(0, 1, 2))), ("r shorter than u", dict(r=R3))]
FOLD_BREAKS = [("empty rowPtr", dict(rowPtr=np.empty(0, np.int64))), ("ratings shorter than the index", dict(ratings=R3)),
               ("init is not nNew x k", dict(init=f32(2 * KP))), ("rows are nNew x kp, not nNew x k", dict(rows=Out("f", 2 * KP))),
               ("rowPtr does not end at the index length", dict(rowPtr=np.array([0, 1, N - 1], np.int64)))]

# every length relation the shim states, broken one at a time: {native: [(what, {parameter: broken value})]}
BREAKS = {
    "nativeSetRatings": TRIPLE_BREAKS,
    "nativeSetValidation": TRIPLE_BREAKS,
    "nativeRmsePairs": TRIPLE_BREAKS + [("out shorter than two", dict(rmseSse=Out("d", 1)))],
    "nativeApplyRatings": TRIPLE_BREAKS + [("err shorter than u", dict(err=Out("f", N - 1))),
                                           ("err longer than u", dict(err=Out("f", N + 1)))],
    "nativePredict": [("i shorter than u", dict(i=i32(0, 1, 2))), ("out shorter than u", dict(out=Out("f", N - 1)))],
    "nativeSetFactors": [("P is users x kp", dict(p=f32(U * KP))), ("Q is items x kp", dict(q=f32(I * KP))),
                         ("P one short", dict(p=f32(U * K - 1)))],
    "nativeGetFactors": [("P is users x kp", dict(p=Out("f", U * KP))), ("Q is items x kp", dict(q=Out("f", I * KP))),
                         ("Q one short", dict(q=Out("f", I * K - 1)))],
    "nativeGetUserFactors": [("P is users x kp", dict(p=Out("f", U * KP))), ("P one long", dict(p=Out("f", U * K + 1)))],
    "nativeTrain": [("rmse shorter than epochs", dict(rmsePerEpoch=Out("d", EPOCHS - 1))), ("negative epochs", dict(epochs=-1))],
    "nativeDsgdTrain": [("rmse shorter than epochs", dict(rmsePerEpoch=Out("d", EPOCHS - 1))),
                        ("negative epochs", dict(epochs=-1))],
    "nativeTrainSchedule": [("lambda shorter than lr", {"lambda": f32(EPOCHS - 1)}),
                            ("rmse shorter than lr", dict(rmsePerEpoch=Out("d", EPOCHS - 1)))],
    "nativeTrainBoldDriver": [("lrUsed shorter than epochs", dict(lrUsed=Out("f", EPOCHS - 1))),
                              ("rmse shorter than epochs", dict(rmsePerEpoch=Out("d", EPOCHS - 1))),
                              ("negative epochs", dict(epochs=-1))],
    "nativeGetHyper": [("out shorter than two", dict(lrLambda=Out("f", 1)))],
    "nativeValidationRmse": [("out shorter than two", dict(rmseSse=Out("d", 1)))],
    "nativeCapacity": [("int[1]", dict(usersItems=Out("i", 1))), ("int[3]", dict(usersItems=Out("i", 3)))],
    "nativeTrainEarlyStop": [("valRmse shorter than maxEpochs", dict(valRmse=Out("d", EPOCHS - 1))),
                             ("trainRmse shorter than maxEpochs", dict(trainRmse=Out("d", EPOCHS - 1))),
                             ("out shorter than two", dict(epochsRunBestEpoch=Out("i", 1))),
                             ("lr not maxEpochs long", dict(lr=f32(EPOCHS + 1))),
                             ("lambda not maxEpochs long", {"lambda": f32(EPOCHS - 1)}),
                             ("negative maxEpochs", dict(maxEpochs=-1))],
    "nativeRecommend": REC_BREAKS,
    "nativeRecommendExcluding": REC_BREAKS + [("exclI shorter than exclU", dict(exclI=i32(1)))],
    "nativeRecommendAmong": REC_BREAKS + [("exclI shorter than exclU", dict(exclI=i32(1))),
                                          ("candPtr has n entries", dict(candPtr=np.array([0, 1, 2, 3], np.int64))),
                                          ("candPtr has n + 2 entries", dict(candPtr=np.array([0, 1, 2, 3, 3, 3], np.int64)))],
    "nativeRecommendUnseen": REC_BREAKS + [("candPtr has n entries", dict(candPtr=np.array([0, 1, 2, 3], np.int64)))],
    "nativeSeenUpdate": [("setSeen: i shorter than u", dict(i=i32(0, 1, 2))), ("markSeen: i longer than u", dict(op=1, i=i32(0, 1, 2, 3, 4)))],
    "nativeGetSeen": [("rowPtr has n entries", dict(rowPtr=Out("i", N))), ("rowPtr has n + 2 entries", dict(rowPtr=Out("i", N + 2)))],
    "nativeRankUnseen": [("i shorter than u", dict(i=i32(0, 1, 2))), ("ranks shorter than u", dict(ranks=Out("i", N - 1))),
                         ("six metrics", dict(metrics7=Out("d", 6)))],
    "nativeFoldIn": FOLD_BREAKS,
    "nativeFoldInItems": FOLD_BREAKS,
    "nativeAppend": [("rows % k", dict(rows=f32(2 * K + 1))), ("rows are n x kp", dict(rows=f32(KP)))],
    "nativeSimilar": [("side 2", dict(side=2)), ("index shorter than queries x topN", dict(index=Out("i", 2 * TOPN - 1))),
                      ("scores shorter than queries x topN", dict(scores=Out("f", 2 * TOPN - 1))), ("topN < 1", dict(topN=0))],
    "nativeSimilarRows": [("rows % k", dict(rows=f32(2 * K - 1))), ("index shorter than rows x topN", dict(index=Out("i", 2 * TOPN - 1))),
                          ("scores shorter than rows x topN", dict(scores=Out("f", 2 * TOPN - 1))), ("topN < 1", dict(topN=0))],
    "nativeRowInvNorms": [("side 2", dict(side=2)), ("out shorter than the side", dict(out=Out("f", I - 1))),
                          ("out has the other side's length minus", dict(side=0, out=Out("f", I)))],
    "nativeRankItems": [("i shorter than u", dict(i=i32(0, 1, 2))), ("exclI shorter than exclU", dict(exclI=i32(1))),
                        ("ranks shorter than u", dict(ranks=Out("i", N - 1)))],
    "nativeRankItemsRows": [("rows % k", dict(rows=f32(2 * K + 3))), ("i shorter than row", dict(i=i32(0, 1, 2))),
                            ("exclItem shorter than exclRow", dict(exclItem=i32(1))), ("ranks shorter", dict(ranks=Out("i", N - 1)))],
    "nativeEvaluateRanking": [("six metrics", dict(metrics7=Out("d", 6))), ("i shorter than u", dict(i=i32(0, 1, 2))),
                              ("ranks shorter than u", dict(ranks=Out("i", N - 1)))],
    "nativeRecommendRows": ROWS_REC_BREAKS + [("rows % k", dict(rows=f32(KP))), ("exclItem shorter than exclRow", dict(exclItem=i32(1)))],
    "nativeDsgdPlan": [("userBegin has nParts entries", dict(userBegin=Out("i", 2))), ("itemPart shorter than degItem", dict(itemPart=Out("i", 2))),
                       ("nParts < 1", dict(nParts=0, userBegin=Out("i", 1)))],
    "nativeSetItemPartition": [("itemPart shorter than the items", dict(itemPart=i32(0, 1, 0, 1))),
                               ("itemPart longer than the items", dict(itemPart=i32(0, 1, 0, 1, 0, 1)))],
    "nativeDsgdCreate": [("a 127-byte id", dict(id=np.zeros(127, np.int8))), ("a 129-byte id", dict(id=np.zeros(129, np.int8)))],
    "nativeDsgdGetQ": [("partRows shorter than two", dict(partRows=Out("i", 1)))],
}


def refused(mf, jvm, h, name, args, classes, what):
    """The call is refused by the shim itself: an exception of one of `classes` with a text, no violation, nothing
    written, and the C-ABI not reached -- the handle's state and its mfsgd_last_error are what they were."""
    before = state(mf, jvm, h)
    c = Call(jvm, name, args)
    try:
        assert c.violations == [], (name, what, c.violations)
        assert c.pending is not None, f"{name}: {what}: accepted"
        assert c.pending[0] in classes, (name, what, c.pending)
        assert c.pending[1], (name, what, "empty message")
        c.nothing_written()
        assert state(mf, jvm, h) == before, f"{name}: {what}: the handle changed"
        if jvm.natives[name][0] == "int":
            assert c.ret == -1
        elif jvm.natives[name][0] in ("long", "byte[]"):
            assert not c.ret
    finally:
        c.close()


# ---- signatures -------------------------------------------------------------------------------------------------------

def test_every_native_has_the_signature_its_java_declaration_promises():
    """A JVM calls a native with the arguments of its Java declaration; a definition that takes anything else is
    undefined behaviour that no compiler sees.  Return and parameter types, mapped int -> jint, long[] -> jlongArray and
    so on, must equal the definition's after (JNIEnv*, jclass) -- for all natives."""
    java, shim = jni_fake.java_natives(), jni_fake.shim_natives()
    assert set(java) == set(shim) and len(java) == 50
    for name, (ret, params) in java.items():
        want = (jni_fake.jni_type(ret), ["JNIEnv*", "jclass"] + [jni_fake.jni_type(t) for t, _ in params])
        assert shim[name] == want, f"{name}: Java promises {want}, the shim defines {shim[name]}"


def test_the_signature_check_sees_a_wrong_type_and_a_missing_parameter():
    src = open(jni_fake.SHIM).read()
    one = "Java_MatrixFactorizationSGD_nativeInitFactors(JNIEnv* env, jclass, jlong h, jlong seed)"
    assert one in src
    assert jni_fake.shim_natives(src.replace(one, one.replace("jlong seed", "jint seed")))["nativeInitFactors"][1][-1] == "jint"
    assert len(jni_fake.shim_natives(src.replace(one, one.replace(", jlong seed", "")))["nativeInitFactors"][1]) == 3
    assert jni_fake.java_natives("private static native long[] nativeRmse(long h, float[] a);") == {
        "nativeRmse": ("long[]", [("long", "h"), ("float[]", "a")])}


# ---- screening --------------------------------------------------------------------------------------------------------

def screened():
    return sorted(set(jni_fake.java_natives()) - SCALAR_ONLY)


def test_the_tables_cover_every_native_that_takes_an_array(jvm):
    with_arrays = {n for n, (_, params) in jvm.natives.items() if any(t.endswith("[]") for t, _ in params)}
    assert with_arrays == set(valid(0)) == set(BREAKS) == set(screened())


@pytest.mark.parametrize("name", screened())
def test_a_null_array_is_refused_before_anything_happens(mf, jvm, model, name):
    """Every array parameter null in turn (the documented nullable ones aside): NullPointerException or
    IllegalArgumentException, nothing written, the C-ABI not reached."""
    args = valid(model)[name]
    arrays = [p for p, v in args.items() if isinstance(v, (Out, np.ndarray))]
    assert arrays
    for p in arrays:
        if p in NULLABLE.get(name, ()):
            continue
        refused(mf, jvm, model, name, dict(args, **{p: None}), (NPE, IAE), f"{p} = null")
    if name == "nativeRecommendUnseen":
        refused(mf, jvm, model, name, dict(args, candItems=None), (NPE,), "candPtr without candItems")
    if name == "nativeSeenUpdate":  # markSeen screens as setSeen does
        refused(mf, jvm, model, name, dict(args, op=1, u=None), (NPE,), "markSeen: u = null")


@pytest.mark.parametrize("name", screened())
def test_each_length_relation_is_checked_by_the_shim(mf, jvm, model, name):
    """Every length relation the shim states, broken one at a time: IllegalArgumentException, nothing written, the C-ABI
    not reached."""
    args = valid(model)[name]
    for what, change in BREAKS[name]:
        refused(mf, jvm, model, name, dict(args, **change), (IAE,), what)


def test_a_bad_handle_is_refused_where_the_shim_needs_the_dimensions(jvm):
    """The natives that size their buffers from mfsgd_get_dims cannot go on without a handle."""
    v = valid(0)
    for name, cls in (("nativeSetFactors", IAE), ("nativeGetFactors", IAE), ("nativeAppend", IAE), ("nativeSetItemPartition", IAE),
                      ("nativeGetUserFactors", IAE), ("nativeRecommendRows", RTE), ("nativeSimilarRows", RTE),
                      ("nativeRowInvNorms", RTE), ("nativeRankItems", RTE), ("nativeRankItemsRows", RTE),
                      ("nativeEvaluateRanking", RTE)):
        c = Call(jvm, name, v[name])
        assert c.violations == [] and c.pending is not None and c.pending[0] == cls and c.pending[1], (name, c.pending)
        c.nothing_written()
        if name == "nativeAppend":
            assert c.ret == -1
        c.close()


BAD_HANDLE = ("nativeSetFactors", "nativeGetFactors", "nativeAppend", "nativeSetItemPartition", "nativeGetUserFactors",
              "nativeRecommendRows", "nativeSimilarRows", "nativeRowInvNorms", "nativeRankItems", "nativeRankItemsRows",
              "nativeEvaluateRanking")
REFUSALS = os.path.join(ROOT, "tests", "golden", "jni_refusals.json")


def refusal_cases(jvm, h):
    """(key, native, arguments or None) of every refusal the screening tests above and the handle-zero test below
    provoke, from the same tables: each non-nullable array null in turn and the two extra null cases, every entry of
    BREAKS, the bad-handle natives, and every native with handle 0 (arguments None: a native that takes no array)."""
    v, v0 = valid(h), valid(0)
    for name in screened():
        for p, x in v[name].items():
            if isinstance(x, (Out, np.ndarray)) and p not in NULLABLE.get(name, ()):
                yield f"{name} | {p} = null", name, dict(v[name], **{p: None})
        for what, change in BREAKS[name]:
            yield f"{name} | {what}", name, dict(v[name], **change)
    yield "nativeRecommendUnseen | candPtr without candItems", "nativeRecommendUnseen", dict(v["nativeRecommendUnseen"], candItems=None)
    yield "nativeSeenUpdate | markSeen: u = null", "nativeSeenUpdate", dict(v["nativeSeenUpdate"], op=1, u=None)
    for name in BAD_HANDLE:
        yield f"{name} | bad handle", name, v0[name]
    for name in sorted(set(jvm.natives) - {"nativeCreate", "nativeDsgdUniqueId", "nativeDsgdPlan"}):
        yield f"{name} | handle 0", name, v0.get(name)


def recorded_refusals(jvm, h):
    """{key: [exception class, message]} (null where nothing was thrown) of refusal_cases, as the shim answers now."""
    out = {}
    for key, name, args in refusal_cases(jvm, h):
        assert key not in out, key
        if args is None:
            getattr(jvm, name)(*[0 if t in ("int", "long") else 0.5 for t, _ in jvm.natives[name][1]])
            pend, viol = jvm.pending(), jvm.violations()
        else:
            c = Call(jvm, name, args)
            pend, viol = c.pending, c.violations
            c.close()
        assert viol == [], (key, viol)
        out[key] = list(pend) if pend else None
    return out


def test_every_refusal_is_the_recorded_one_class_and_text(jvm, model):
    """The screening tests accept any text and one of two classes.  Here every refusal they provoke is compared with
    tests/golden/jni_refusals.json, recorded from the shim before its natives were rebuilt on shared helpers
    (tests/golden/make_jni_refusals.py writes it): the same cases, the same exception class, the same message, byte for
    byte.  A text changed on purpose is re-recorded, and the diff of that file shows it."""
    import json

    with open(REFUSALS) as f:
        want = json.load(f)
    got = recorded_refusals(jvm, model)
    assert set(got) == set(want), (sorted(set(got) - set(want)), sorted(set(want) - set(got)))
    assert got == want, {k: (got[k], want[k]) for k in got if got[k] != want[k]}


# ---- status -> exception ----------------------------------------------------------------------------------------------

def test_a_failed_create_throws_the_librarys_text_and_returns_no_handle(jvm):
    assert jvm.nativeCreate(10, 10, 300, LR, LAM, 0, 0) == 0
    cls, msg = jvm.pending()
    assert cls == RTE and msg == jvm.last_error(0) and "MFSGD_MAX_K" in msg and jvm.violations() == []
    assert jvm.nativeCreate(0, 10, 8, LR, LAM, 0, 0) == 0
    assert jvm.pending() == (RTE, jvm.last_error(0)) and jvm.violations() == []


def test_a_failing_call_throws_exactly_the_handles_last_error(mf, jvm):
    """Train without ratings, append before the factors exist, a capacity that overflows: RuntimeException carrying
    exactly mfsgd_last_error(h); outputs keep their sentinel; the scalars are the documented ones."""
    h = jvm.nativeCreate(U, I, K, LR, LAM, 0, 0)
    jvm.ok()
    try:
        v = valid(h)
        c = Call(jvm, "nativeTrain", v["nativeTrain"])
        assert c.pending == (RTE, jvm.last_error(h)) and c.pending[1] and c.violations == []
        c.nothing_written()
        c.close()
        for args in (v["nativeAppend"], dict(v["nativeAppend"], rows=None, n=3), dict(v["nativeAppend"], side=1)):
            c = Call(jvm, "nativeAppend", args)  # append before init: MFSGD_ERR_STATE
            assert c.ret == -1 and c.pending == (RTE, jvm.last_error(h)) and "append_" in c.pending[1] and c.violations == []
            c.inputs_intact()
            c.close()
        assert jvm.nativeRmse(h) == 0.0
        assert jvm.pending() == (RTE, jvm.last_error(h)) and jvm.violations() == []
        jvm.nativeReserve(h, -1, 0)
        cls, msg = jvm.pending()
        assert (cls, msg) == (RTE, jvm.last_error(h)) and msg.startswith("reserve_rows") and jvm.violations() == []
        jvm.nativeSetHyper(h, float("nan"), 0.0)
        cls, msg = jvm.pending()
        assert (cls, msg) == (RTE, jvm.last_error(h)) and msg.startswith("set_hyper") and jvm.violations() == []
        c = Call(jvm, "nativeGetSeen", v["nativeGetSeen"])  # no seen set
        assert c.pending == (RTE, jvm.last_error(h)) and "seen" in c.pending[1] and c.violations == []
        c.nothing_written()
        c.close()
        assert jvm.nativeSeenSize(h) == -1  # no index: a value, not an error
        jvm.ok()
    finally:
        jvm.nativeDestroy(h)


# what every one of these does on a machine without a device: the status becomes the exception, nothing is written
COMPUTE = ["nativeTrain", "nativeTrainSchedule", "nativeTrainBoldDriver", "nativeRmsePairs", "nativeApplyRatings",
           "nativePredict", "nativeRecommend", "nativeRecommendExcluding", "nativeRecommendAmong", "nativeSeenUpdate",
           "nativeRankItems", "nativeRankItemsRows", "nativeEvaluateRanking", "nativeRecommendRows", "nativeFoldIn",
           "nativeFoldInItems", "nativeSimilar", "nativeSimilarRows", "nativeRowInvNorms", "nativeTrainEarlyStop",
           "nativeValidationRmse", "nativeRecommendUnseen", "nativeRankUnseen"]


@pytest.mark.parametrize("name", COMPUTE)
def test_without_a_device_a_compute_native_throws_and_writes_nothing(mf, jvm, name):
    """There is no CPU fallback: on a machine without a device the C call fails, and the native turns that into a
    RuntimeException with exactly mfsgd_last_error(h), leaving every output at its sentinel and every input alone."""
    if have_gpu():
        pytest.skip("with a device these natives succeed: tests/test_jni_gpu.py compares what they return")
    h = jvm.nativeCreate(U, I, K, LR, LAM, 0, 0)
    jvm.ok()
    try:
        v = valid(h)
        for pre in ("nativeSetRatings", "nativeSetValidation"):
            Call(jvm, pre, v[pre]).close()
        jvm.nativeInitFactors(h, SEED)
        jvm.ok()
        c = Call(jvm, name, v[name])
        assert c.violations == []
        assert c.pending == (RTE, jvm.last_error(h)), (name, c.pending)
        assert c.pending[1]
        c.nothing_written(c_call_failed=True)
        c.close()
    finally:
        jvm.nativeDestroy(h)


def test_the_ring_natives_throw_with_a_text_when_there_is_no_ring(mf, jvm):
    """nativeDsgdCreate on a handle without item partitions (or without a device) fails in the library; the natives
    that take a ring refuse a null one.  Each throws RuntimeException with a text and returns 0."""
    lib = mf.load_library()
    h = jvm.nativeCreate(U, I, K, LR, LAM, 0, 0)
    jvm.ok()
    try:
        v = valid(h)
        c = Call(jvm, "nativeDsgdCreate", v["nativeDsgdCreate"])
        assert c.ret in (0, None) and c.violations == []
        assert c.pending == (RTE, lib.mfsgd_dsgd_last_error(None).decode()) and c.pending[1]
        c.inputs_intact()
        c.close()
    finally:
        jvm.nativeDestroy(h)
    for name in ("nativeDsgdTrain", "nativeDsgdGetQ"):
        c = Call(jvm, name, valid(0)[name])
        assert c.pending is not None and c.pending[0] == RTE and c.pending[1] and c.violations == [], (name, c.pending)
        c.nothing_written()
        c.close()
    jvm.nativeDsgdInitQ(0, 1, 1)
    assert jvm.pending() == (RTE, "mfsgd: null or closed ring") and jvm.violations() == []
    assert jvm.nativeDsgdRmse(0) == 0.0
    assert jvm.pending() == (RTE, "mfsgd: null or closed ring") and jvm.violations() == []
    jvm.nativeDsgdDestroy(0)  # allowed, like close() twice
    jvm.ok()
    ident = jvm.nativeDsgdUniqueId()  # a byte[128] made by NewByteArray, or (no RCCL) null and the library's text
    if ident:
        jvm.ok()
        assert jvm.read(ident).dtype == np.int8 and jvm.read(ident).size == 128 and jvm.written(ident)
        jvm.free(ident)
    else:
        cls, msg = jvm.pending()
        assert cls == RTE and msg == lib.mfsgd_dsgd_last_error(None).decode() and msg and jvm.violations() == []


# ---- no exception without a message -----------------------------------------------------------------------------------

def test_every_native_called_with_handle_zero_throws_with_a_message(jvm):
    """A closed Java object calls its natives with handle 0.  mfsgd_last_error(NULL) holds nothing then (or the text of
    an unrelated failed create), so the shim supplies its own: no exception may carry an empty message."""
    v = valid(0)
    silent = {"nativeDestroy", "nativeDsgdDestroy"}  # null is allowed
    free = {"nativeCreate", "nativeDsgdUniqueId", "nativeDsgdPlan"}  # take no handle
    for name, (ret, params) in sorted(jvm.natives.items()):
        if name in free:
            continue
        if name in v:
            c = Call(jvm, name, v[name])
            pend, viol = c.pending, c.violations
            c.nothing_written(c_call_failed=True)
            c.close()
        else:
            getattr(jvm, name)(*[0 if t in ("int", "long") else 0.5 for t, _ in params])
            pend, viol = jvm.pending(), jvm.violations()
        assert viol == [], (name, viol)
        if name in silent:
            assert pend is None
            continue
        assert pend is not None, f"{name}(0) was accepted"
        assert pend[0] in (RTE, IAE) and pend[1].strip(), f"{name}(0): {pend}"
    jvm.nativeRmse(0)
    assert jvm.pending() == (RTE, "mfsgd: null or closed handle")
    # ... also after a failed create has left ITS text with the thread: that text is not this call's
    assert jvm.nativeCreate(10, 10, 300, LR, LAM, 0, 0) == 0 and jvm.pending()[1] == jvm.last_error(0)
    jvm.nativeRmse(0)
    assert jvm.pending() == (RTE, "mfsgd: null or closed handle") and jvm.violations() == []


# ---- what runs on the host, against the Python surface ----------------------------------------------------------------

def test_create_ratings_init_and_factors_equal_the_python_surface(mf, jvm):
    u, i, r = triples()
    h = jvm.nativeCreate(U, I, K, LR, LAM, 0, 0)
    jvm.ok()
    with mf.MatrixFactorizationSGD(U, I, K, LR, LAM, SEED) as m:
        c = Call(jvm, "nativeSetRatings", dict(h=h, u=u, i=i, r=r))
        assert c.pending is None and c.violations == []
        c.inputs_intact()
        c.close()
        m.set_ratings(u, i, r)
        jvm.nativeInitFactors(h, SEED)
        jvm.ok()
        m.init_factors()
        P, Q = m.get_factors()
        c = Call(jvm, "nativeGetFactors", dict(h=h, p=Out("f", U * K), q=Out("f", I * K)))
        assert c.pending is None and c.violations == []
        assert c.read("p").tobytes() == P.tobytes() and c.read("q").tobytes() == Q.tobytes()
        c.close()
        c = Call(jvm, "nativeGetUserFactors", dict(h=h, p=Out("f", U * K)))
        assert c.pending is None and c.violations == [] and c.read("p").tobytes() == P.tobytes()
        c.close()
        with adopted(mf, h) as a:  # the ratings reached the library as given: the same schedule, the same order
            assert a.schedule_info()["nnz"] == N and np.array_equal(a.order()[0], m.order()[0])
            assert a.debug_counters()["schedule_builds"] == 1
        c = Call(jvm, "nativeGetHyper", dict(h=h, lrLambda=Out("f", 5)))
        assert c.pending is None and c.violations == []
        got = c.read("lrLambda")
        assert got[:2].tobytes() == np.array(m.hyper(), np.float32).tobytes() and jvm.untouched(c.ref["lrLambda"], 2)
        c.close()
        jvm.nativeSetHyper(h, 0.02, 0.07)
        jvm.ok()
        m.set_hyper(0.02, 0.07)
        c = Call(jvm, "nativeGetHyper", dict(h=h, lrLambda=Out("f", 2)))
        assert c.read("lrLambda").tobytes() == np.array(m.hyper(), np.float32).tobytes() and c.pending is None
        c.close()
    jvm.nativeDestroy(h)
    jvm.ok()


def test_set_factors_round_trip_where_k_is_not_kp(mf, jvm):
    """k = 10: host rows are 10 floats, device rows 12.  What goes in through nativeSetFactors comes back through
    nativeGetFactors byte for byte, and is what the Python surface holds after the same call."""
    P, Q = f32(U * K, 21), f32(I * K, 22)
    P[3] = -0.0
    h = jvm.nativeCreate(U, I, K, LR, LAM, 0, 0)
    with mf.MatrixFactorizationSGD(U, I, K, LR, LAM, SEED) as m:
        c = Call(jvm, "nativeSetFactors", dict(h=h, p=P, q=Q))
        assert c.pending is None and c.violations == []
        c.inputs_intact()
        c.close()
        m.set_factors(P.reshape(U, K), Q.reshape(I, K))
        Pm, Qm = m.get_factors()
        c = Call(jvm, "nativeGetFactors", dict(h=h, p=Out("f", U * K), q=Out("f", I * K)))
        assert c.pending is None and c.violations == []
        assert c.read("p").tobytes() == Pm.tobytes() == P.tobytes() and c.read("q").tobytes() == Qm.tobytes() == Q.tobytes()
        c.close()
    jvm.nativeDestroy(h)


def test_reserve_capacity_and_append_on_host_staging_equal_the_python_surface(mf, jvm):
    """nativeReserve / nativeCapacity, and nativeAppend with the factors on host staging (no device needed): rows and
    seeded, both sides; afterwards nativeGetFactors wants arrays of the NEW size and refuses the old."""
    h = jvm.nativeCreate(U, I, K, LR, LAM, 0, 0)
    with mf.MatrixFactorizationSGD(U, I, K, LR, LAM, SEED) as m:
        def capacity():
            c = Call(jvm, "nativeCapacity", dict(h=h, usersItems=Out("i", 2)))
            assert c.pending is None and c.violations == []
            got = tuple(int(x) for x in c.read("usersItems"))
            c.close()
            return got

        assert capacity() == m.capacity() == (U, I)
        jvm.nativeReserve(h, U + 3, 0)
        jvm.ok()
        m.reserve(U + 3, None)
        assert capacity() == m.capacity() == (U + 3, I)
        jvm.nativeInitFactors(h, SEED)
        jvm.ok()
        m.init_factors()
        rows = f32(2 * K, 31)
        for side, add in ((0, m.add_users), (1, m.add_items)):
            c = Call(jvm, "nativeAppend", dict(h=h, side=side, rows=rows, n=77, seed=0))  # n is ignored: rows decide
            assert c.pending is None and c.violations == []
            c.inputs_intact()
            assert c.ret == add(rows.reshape(2, K)) == (U, I)[side]
            c.close()
            c = Call(jvm, "nativeAppend", dict(h=h, side=side, rows=None, n=3, seed=99))
            assert c.pending is None and c.violations == [] and c.ret == add(n=3, seed=99) == (U, I)[side] + 2
            c.close()
        assert capacity() == m.capacity()
        P, Q = m.get_factors()
        assert P.shape == (U + 5, K) and Q.shape == (I + 5, K)
        c = Call(jvm, "nativeGetFactors", dict(h=h, p=Out("f", (U + 5) * K), q=Out("f", (I + 5) * K)))
        assert c.pending is None and c.violations == []
        assert c.read("p").tobytes() == P.tobytes() and c.read("q").tobytes() == Q.tobytes()
        c.close()
        before = state(mf, jvm, h)
        c = Call(jvm, "nativeGetFactors", dict(h=h, p=Out("f", U * K), q=Out("f", I * K)))
        assert c.pending is not None and c.pending[0] == IAE and c.violations == []
        c.nothing_written()
        c.close()
        assert state(mf, jvm, h) == before
    jvm.nativeDestroy(h)


def test_plan_item_partition_and_offset_seeding_equal_the_python_surface(mf, jvm):
    rng = np.random.default_rng(5)
    du, di = rng.integers(0, 50, 37).astype(np.int64), rng.integers(0, 90, 23).astype(np.int64)
    for parts in (1, 2, 5):
        c = Call(jvm, "nativeDsgdPlan", dict(degUser=du, degItem=di, nParts=parts, userBegin=Out("i", parts + 1), itemPart=Out("i", di.size)))
        assert c.pending is None and c.violations == []
        c.inputs_intact()
        ub, ip = mf.trainer.dsgd_plan(du, di, parts)
        assert c.read("userBegin").tobytes() == ub.tobytes() and c.read("itemPart").tobytes() == ip.tobytes()
        c.close()
    c = Call(jvm, "nativeDsgdPlan", dict(degUser=-du - 1, degItem=di, nParts=2, userBegin=Out("i", 3), itemPart=Out("i", di.size)))
    assert c.pending is not None and c.pending[0] == IAE and c.pending[1] and c.violations == []  # the library refuses it
    c.nothing_written()
    c.close()
    # a partitioned handle: the plan's item map, then P seeded at a user offset
    _, ip = mf.trainer.dsgd_plan(np.ones(U, np.int64), np.arange(I, dtype=np.int64), 2)
    h = jvm.nativeCreate(U, I, K, LR, LAM, 0, 2)
    jvm.ok()
    with mf.MatrixFactorizationSGD(U, I, K, LR, LAM, SEED, n_parts=2) as m:
        c = Call(jvm, "nativeSetItemPartition", dict(h=h, itemPart=ip))
        assert c.pending is None and c.violations == []
        c.inputs_intact()
        c.close()
        m.set_item_partition(ip)
        with adopted(mf, h) as a:
            for x, y in zip(a.item_partition(), m.item_partition()):
                assert x.tobytes() == y.tobytes()
        jvm.nativeInitPOffset(h, SEED, 1000)
        jvm.ok()
        m.init_p_offset(SEED, 1000)
        c = Call(jvm, "nativeGetUserFactors", dict(h=h, p=Out("f", U * K)))
        assert c.pending is None and c.violations == [] and c.read("p").tobytes() == m.get_factors()[0].tobytes()
        c.close()
        c = Call(jvm, "nativeSetItemPartition", dict(h=h, itemPart=i32(0, 1, 2, 0, 1)))  # partition 2 of 2: the library refuses
        assert c.pending == (RTE, jvm.last_error(h)) and c.pending[1] and c.violations == []
        c.close()
    jvm.nativeDestroy(h)


def test_validation_set_and_its_size_on_the_host(mf, jvm):
    u, i, r = triples()
    h = jvm.nativeCreate(U, I, K, LR, LAM, 0, 0)
    with mf.MatrixFactorizationSGD(U, I, K, LR, LAM, SEED) as m:
        assert jvm.nativeValidationSize(h) == m.validation_size() == 0
        c = Call(jvm, "nativeSetValidation", dict(h=h, u=u, i=i, r=r))
        assert c.pending is None and c.violations == []
        c.inputs_intact()
        c.close()
        m.set_validation(u, i, r)
        assert jvm.nativeValidationSize(h) == m.validation_size() == N
        c = Call(jvm, "nativeSetValidation", dict(h=h, u=i32(0, U), i=i32(0, 1), r=R3[:2]))  # user out of range
        assert c.pending == (RTE, jvm.last_error(h)) and c.pending[1].startswith("set_validation") and c.violations == []
        c.close()
        assert jvm.nativeValidationSize(h) == N
        # the empty seen index is host-only too: setSeen of nothing, its size, clearSeen
        assert jvm.nativeSeenSize(h) == m.seen_size() == -1
        c = Call(jvm, "nativeSeenUpdate", dict(h=h, op=0, u=i32(), i=i32()))
        assert c.pending is None and c.violations == []
        c.close()
        m.set_seen([], [])
        assert jvm.nativeSeenSize(h) == m.seen_size() == 0
        jvm.nativeSeenUpdate(h, 2, None, None)  # clearSeen takes no arrays
        jvm.ok()
        assert jvm.nativeSeenSize(h) == -1
    jvm.ok()
    jvm.nativeDestroy(h)


# ---- array handling ---------------------------------------------------------------------------------------------------

def test_longer_output_arrays_keep_their_sentinel_beyond_what_is_written(mf, jvm):
    h = jvm.nativeCreate(U, I, K, LR, LAM, 0, 0)
    jvm.nativeInitFactors(h, SEED)
    jvm.ok()
    c = Call(jvm, "nativeDsgdPlan", dict(degUser=np.array([3, 1, 2, 2], np.int64), degItem=np.array([4, 1, 3], np.int64), nParts=2,
                                         userBegin=Out("i", 3), itemPart=Out("i", 3)))
    ub = c.read("userBegin")
    c.close()
    assert ub[0] == 0 and ub[-1] == 4
    for name, p, used in (("nativeGetHyper", "lrLambda", 2),):
        c = Call(jvm, name, dict(valid(h)[name], **{p: Out("f", used + 3)}))
        assert c.pending is None and c.violations == [] and jvm.written(c.ref[p])
        assert not jvm.untouched(c.ref[p]) and jvm.untouched(c.ref[p], used)
        c.close()
    jvm.nativeDestroy(h)


def test_the_fake_jvm_records_what_a_checking_jvm_would_abort_on(jvm):
    """The stand-in's own rules, each shown once on the shim or on the JNIEnv directly: without them a clean run would
    prove nothing."""
    h = jvm.nativeCreate(U, I, K, LR, LAM, 0, 0)
    jvm.nativeInitFactors(h, SEED)
    jvm.ok()
    p, q, wrong = jvm.out("f", U * K), jvm.out("f", I * K), jvm.out("i", I * K)
    jvm.nativeGetFactors(h, p, wrong)  # a float[] parameter handed an int[]: the type tag
    assert jvm.pending() is None and any("element type" in x for x in jvm.violations()) and jvm.untouched(wrong)
    jvm.nativeGetFactors(h, p, 0x1234)  # a reference that is no array
    assert any("unknown array" in x for x in jvm.violations())
    jvm.pending()
    jvm.free(q)
    jvm.nativeGetFactors(h, p, q)  # ... or is one no longer
    assert any("unknown array" in x for x in jvm.violations())
    jvm.pending()
    # a second native while the first one's exception is pending: every JNIEnv call but ExceptionCheck is a breach
    jvm.nativeRmse(0)
    a = jvm.out("f", 2)
    jvm.nativeGetHyper(h, a)
    assert any("pending" in x for x in jvm.violations()) and jvm.untouched(a)
    assert jvm.pending() == (RTE, "mfsgd: null or closed handle")
    jvm.free(p, wrong, a)
    jvm.nativeDestroy(h)
    jvm.ok()
    # the rules no line of the shim trips, each through one JNIEnv call of the stand-in's probe
    AIOOBE = "java/lang/ArrayIndexOutOfBoundsException"
    for what in (0, 1, 2):  # a region past the end, a negative start, a negative length: nothing copied, AIOOBE pending
        x = jvm.arr(i32(7, 8, 9))
        assert jvm.probe(what, x) in (0, 1)  # (the probe's own buffer starts with 1: nothing was copied into it)
        assert jvm.pending()[0] == AIOOBE and jvm.violations() == []
        assert jvm.read(x).tolist() == [7, 8, 9] and not jvm.written(x)
        jvm.free(x)
    x = jvm.arr(i32(7, 8, 9))
    assert jvm.probe(3, x) == 0 and jvm.pending() == ("java/lang/NoClassDefFoundError", "java/lang/Strin") and jvm.violations() == []
    assert jvm.probe(4, x) == 0 and len([v for v in jvm.violations() if "Critical" in v]) == 2 and jvm.pending() is None
    assert jvm.probe(5, x) == -1 and jvm.violations() == ["ThrowNew called while java/lang/RuntimeException is pending"]
    assert jvm.pending() == (RTE, "first")
    jvm.probe(6, x)
    assert jvm.violations() == ["SetIntArrayRegion called while java/lang/IllegalStateException is pending"]
    assert jvm.pending() == ("java/lang/IllegalStateException", "thrown") and jvm.read(x).tolist() == [7, 8, 9]
    jvm.free(x)
    jvm.ok()


# ---- the guard --------------------------------------------------------------------------------------------------------

def test_every_native_the_shim_defines_is_named_by_a_test():
    """A native added later without a test fails here."""
    named = set()
    for f in ("test_jni_cpu.py", "test_jni_gpu.py"):
        named |= set(re.findall(r"\bnative[A-Z]\w*", open(os.path.join(ROOT, "tests", f)).read()))
    defined = set(jni_fake.shim_natives())
    assert defined - named == set(), f"natives without a test: {sorted(defined - named)}"
    assert named - defined == set(), f"tests name natives the shim does not define: {sorted(named - defined)}"
