// mfsgd_jni.cpp -- JNI shim between java/MatrixFactorizationSGD.java and the C-ABI
// of include/mfsgd.h.
//
// NEVER RUN UNDER A REAL JVM: there is no JDK (no jni.h) in this container or on the
// GPU box.  What the test-suite does instead: every native below is executed under a JVM
// stand-in (tests/jni_stub/jni.h + fake_jvm.cpp) that enforces the JNI rules a shim can
// break -- typed arrays, region bounds, no call but ExceptionCheck while an exception is
// pending, no critical regions, known classes only -- and each result is compared byte for
// byte with what the Python surface returns for the same call on a twin handle
// (tests/test_jni_cpu.py, tests/test_jni_gpu.py).  java/MatrixFactorizationSGD.java itself
// is still unchecked: there is no javac.  Build, where a JDK exists:
//   g++ -std=c++17 -fPIC -shared -I$JAVA_HOME/include -I$JAVA_HOME/include/linux ...
//       -I../../include mfsgd_jni.cpp -L../lib -lmfsgd -Wl,-rpath,'$ORIGIN' -o libmfsgd_jni.so
//
// Rules followed: NO Java array is ever pinned
// (Get/ReleasePrimitiveArrayCritical is not used: every C-ABI call may launch a
// kernel, start threads or wait for the device -- even set_factors waits for the
// device to go idle before it frees the old buffers -- and no JNI call may be made
// inside a critical region); every call works on NATIVE copies made with
// Get*ArrayRegion; array lengths are checked here, not only in Java; a failed native
// allocation throws OutOfMemoryError; a non-zero status becomes a RuntimeException
// carrying mfsgd_last_error(), or a fixed text where the library has none (a null or
// closed handle): no exception has an empty message; no C++ exception crosses the boundary.
#include <jni.h>

#include <cstdint>
#include <memory>
#include <new>

#include "mfsgd.h"

namespace {

void throw_new(JNIEnv* env, const char* cls_name, const char* msg) {
    jclass cls = env->FindClass(cls_name);
    if (cls) env->ThrowNew(cls, msg);
}

// An exception never carries an empty message: where the library has no text the shim says what it knows.
const char* text_or(const char* msg, const char* fallback) { return msg && *msg ? msg : fallback; }

mfsgd_handle* H(jlong h) { return reinterpret_cast<mfsgd_handle*>(h); }
mfsgd_dsgd* D(jlong d) { return reinterpret_cast<mfsgd_dsgd*>(d); }

// h == nullptr: the Java object was closed or never created.  mfsgd_last_error(nullptr) is the message of the last
// failed mfsgd_create on this thread (empty when there was none): it says nothing about this call.
void throw_status(JNIEnv* env, mfsgd_handle* h, int rc) {
    if (rc == MFSGD_OK) return;
    throw_new(env, "java/lang/RuntimeException",
              h ? text_or(mfsgd_last_error(h), "mfsgd: the call failed without a message") : "mfsgd: null or closed handle");
}

void throw_dsgd(JNIEnv* env, mfsgd_dsgd* d, int rc) {
    if (rc == MFSGD_OK) return;
    throw_new(env, "java/lang/RuntimeException",
              d ? text_or(mfsgd_dsgd_last_error(d), "mfsgd: the ring call failed without a message") : "mfsgd: null or closed ring");
}

// the calls that have no object yet (mfsgd_create, mfsgd_dsgd_unique_id, mfsgd_dsgd_create) leave their message with
// the thread
void throw_text(JNIEnv* env, int rc, const char* msg, const char* fallback) {
    if (rc != MFSGD_OK) throw_new(env, "java/lang/RuntimeException", text_or(msg, fallback));
}

// new[] that reports failure to Java instead of throwing across the boundary
template <class T>
std::unique_ptr<T[]> alloc(JNIEnv* env, size_t n) {
    std::unique_ptr<T[]> p(new (std::nothrow) T[n ? n : 1]);
    if (!p) throw_new(env, "java/lang/OutOfMemoryError", "mfsgd_jni: native buffer");
    return p;
}

}  // namespace

extern "C" {

JNIEXPORT jlong JNICALL Java_MatrixFactorizationSGD_nativeCreate(JNIEnv* env, jclass, jint users, jint items, jint k,
                                                                 jfloat lr, jfloat lambda, jint device, jint n_parts) {
    mfsgd_config cfg = {};
    cfg.n_users = users;
    cfg.n_items = items;
    cfg.k = k;
    cfg.lr = lr;
    cfg.lambda = lambda;
    cfg.device = device;
    cfg.n_parts = n_parts;
    mfsgd_handle* h = nullptr;
    const int rc = mfsgd_create(&cfg, &h);
    throw_text(env, rc, mfsgd_last_error(nullptr), "mfsgd_create failed");
    return reinterpret_cast<jlong>(h);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeDestroy(JNIEnv*, jclass, jlong h) { mfsgd_destroy(H(h)); }

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeSetRatings(JNIEnv* env, jclass, jlong h, jintArray u,
                                                                    jintArray i, jfloatArray r) {
    if (!u || !i || !r) return throw_new(env, "java/lang/NullPointerException", "ratings");
    const jsize n = env->GetArrayLength(u);
    if (env->GetArrayLength(i) != n || env->GetArrayLength(r) != n)
        return throw_new(env, "java/lang/IllegalArgumentException", "u, i and r must have the same length");
    // mfsgd_set_ratings hashes the triples, and when they are new it launches the ingest kernels, sorts on
    // the device and runs the packer on host threads (0.1 - 3 s): it gets native copies, nothing stays pinned
    auto cu = alloc<int32_t>(env, (size_t)n);
    auto ci = alloc<int32_t>(env, (size_t)n);
    auto cr = alloc<float>(env, (size_t)n);
    if (!cu || !ci || !cr) return;
    env->GetIntArrayRegion(u, 0, n, reinterpret_cast<jint*>(cu.get()));
    env->GetIntArrayRegion(i, 0, n, reinterpret_cast<jint*>(ci.get()));
    env->GetFloatArrayRegion(r, 0, n, cr.get());
    if (env->ExceptionCheck()) return;
    throw_status(env, H(h), mfsgd_set_ratings(H(h), cu.get(), ci.get(), cr.get(), n));
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeInitFactors(JNIEnv* env, jclass, jlong h, jlong seed) {
    throw_status(env, H(h), mfsgd_init_factors(H(h), seed));
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeSetFactors(JNIEnv* env, jclass, jlong h, jfloatArray p,
                                                                    jfloatArray q) {
    int32_t users = 0, items = 0, k = 0;
    if (!p || !q || mfsgd_get_dims(H(h), &users, &items, &k) != MFSGD_OK)
        return throw_new(env, "java/lang/IllegalArgumentException", "setFactors: bad handle or null array");
    if ((jlong)env->GetArrayLength(p) != (jlong)users * k || (jlong)env->GetArrayLength(q) != (jlong)items * k)
        return throw_new(env, "java/lang/IllegalArgumentException", "setFactors: P must be users x k, Q items x k");
    // native copies, nothing pinned: mfsgd_set_factors waits for the device to go idle before it frees the old
    // device buffers, and a pinned array would keep the collector out for as long as that takes
    const size_t np = (size_t)users * k, nq = (size_t)items * k;
    auto cp = alloc<float>(env, np);
    auto cq = alloc<float>(env, nq);
    if (!cp || !cq) return;
    env->GetFloatArrayRegion(p, 0, (jsize)np, cp.get());
    env->GetFloatArrayRegion(q, 0, (jsize)nq, cq.get());
    if (env->ExceptionCheck()) return;
    const int rc = mfsgd_set_factors(H(h), cp.get(), cq.get());
    throw_status(env, H(h), rc);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeGetFactors(JNIEnv* env, jclass, jlong h, jfloatArray p,
                                                                    jfloatArray q) {
    int32_t users = 0, items = 0, k = 0;
    if (!p || !q || mfsgd_get_dims(H(h), &users, &items, &k) != MFSGD_OK)
        return throw_new(env, "java/lang/IllegalArgumentException", "factors: bad handle or null array");
    const size_t np = (size_t)users * k, nq = (size_t)items * k;
    if ((size_t)env->GetArrayLength(p) != np || (size_t)env->GetArrayLength(q) != nq)
        return throw_new(env, "java/lang/IllegalArgumentException", "factors: P must be users x k, Q items x k");
    // mfsgd_get_factors waits for the stream and copies from the device: native buffers, no pins
    auto cp = alloc<float>(env, np);
    auto cq = alloc<float>(env, nq);
    if (!cp || !cq) return;
    const int rc = mfsgd_get_factors(H(h), cp.get(), cq.get());
    if (rc == MFSGD_OK) {
        env->SetFloatArrayRegion(p, 0, (jsize)np, cp.get());
        env->SetFloatArrayRegion(q, 0, (jsize)nq, cq.get());
    }
    throw_status(env, H(h), rc);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeTrain(JNIEnv* env, jclass, jlong h, jint epochs,
                                                               jdoubleArray rmse) {
    if (epochs < 0 || !rmse || env->GetArrayLength(rmse) < epochs)
        return throw_new(env, "java/lang/IllegalArgumentException", "rmse array shorter than epochs");
    // the kernels run with NO Java array pinned: results land in a native buffer first
    auto tmp = alloc<double>(env, (size_t)epochs);
    if (!tmp) return;  // OutOfMemoryError pending: never train with the RMSE silently dropped
    const int rc = mfsgd_train(H(h), epochs, tmp.get());
    if (rc == MFSGD_OK && epochs > 0) env->SetDoubleArrayRegion(rmse, 0, epochs, tmp.get());
    throw_status(env, H(h), rc);
}

JNIEXPORT jdouble JNICALL Java_MatrixFactorizationSGD_nativeRmse(JNIEnv* env, jclass, jlong h) {
    double out = 0.0;
    throw_status(env, H(h), mfsgd_rmse(H(h), &out));
    return out;
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeSetHyper(JNIEnv* env, jclass, jlong h, jfloat lr, jfloat lambda) {
    throw_status(env, H(h), mfsgd_set_hyper(H(h), lr, lambda));
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeGetHyper(JNIEnv* env, jclass, jlong h, jfloatArray out) {
    if (!out || env->GetArrayLength(out) < 2) return throw_new(env, "java/lang/IllegalArgumentException", "hyper: out needs two entries");
    float v[2] = {0.f, 0.f};
    const int rc = mfsgd_get_hyper(H(h), &v[0], &v[1]);
    if (rc == MFSGD_OK) env->SetFloatArrayRegion(out, 0, 2, v);
    throw_status(env, H(h), rc);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeTrainSchedule(JNIEnv* env, jclass, jlong h, jfloatArray lr,
                                                                       jfloatArray lambda, jdoubleArray rmse) {
    if (!lr || !rmse) return throw_new(env, "java/lang/NullPointerException", "trainSchedule");
    const jsize epochs = env->GetArrayLength(lr);
    if ((lambda && env->GetArrayLength(lambda) != epochs) || env->GetArrayLength(rmse) < epochs)
        return throw_new(env, "java/lang/IllegalArgumentException", "lr, lambda and rmse must have one entry per epoch");
    // native copies, nothing pinned: the call trains and re-bakes the schedule between epochs
    auto clr = alloc<float>(env, (size_t)epochs);
    auto clam = alloc<float>(env, (size_t)epochs);
    auto tmp = alloc<double>(env, (size_t)epochs);
    if (!clr || !clam || !tmp) return;
    env->GetFloatArrayRegion(lr, 0, epochs, clr.get());
    if (lambda) env->GetFloatArrayRegion(lambda, 0, epochs, clam.get());
    if (env->ExceptionCheck()) return;
    const int rc = mfsgd_train_schedule(H(h), epochs, clr.get(), lambda ? clam.get() : nullptr, tmp.get());
    if (rc == MFSGD_OK && epochs > 0) env->SetDoubleArrayRegion(rmse, 0, epochs, tmp.get());
    throw_status(env, H(h), rc);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeTrainBoldDriver(JNIEnv* env, jclass, jlong h, jint epochs, jfloat up,
                                                                         jfloat down, jfloatArray lr_used, jdoubleArray rmse) {
    if (epochs < 0 || !lr_used || !rmse || env->GetArrayLength(lr_used) < epochs || env->GetArrayLength(rmse) < epochs)
        return throw_new(env, "java/lang/IllegalArgumentException", "lrUsed / rmse array shorter than epochs");
    auto used = alloc<float>(env, (size_t)epochs);
    auto tmp = alloc<double>(env, (size_t)epochs);
    if (!used || !tmp) return;
    const int rc = mfsgd_train_bold_driver(H(h), epochs, up, down, used.get(), tmp.get());
    if (rc == MFSGD_OK && epochs > 0) {
        env->SetFloatArrayRegion(lr_used, 0, epochs, used.get());
        env->SetDoubleArrayRegion(rmse, 0, epochs, tmp.get());
    }
    throw_status(env, H(h), rc);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeSetValidation(JNIEnv* env, jclass, jlong h, jintArray u, jintArray i,
                                                                       jfloatArray r) {
    if (!u || !i || !r) return throw_new(env, "java/lang/NullPointerException", "setValidation");
    const jsize n = env->GetArrayLength(u);
    if (env->GetArrayLength(i) != n || env->GetArrayLength(r) != n)
        return throw_new(env, "java/lang/IllegalArgumentException", "u, i and r must have the same length");
    auto cu = alloc<int32_t>(env, (size_t)n);
    auto ci = alloc<int32_t>(env, (size_t)n);
    auto cr = alloc<float>(env, (size_t)n);
    if (!cu || !ci || !cr) return;
    env->GetIntArrayRegion(u, 0, n, reinterpret_cast<jint*>(cu.get()));
    env->GetIntArrayRegion(i, 0, n, reinterpret_cast<jint*>(ci.get()));
    env->GetFloatArrayRegion(r, 0, n, cr.get());
    if (env->ExceptionCheck()) return;
    throw_status(env, H(h), mfsgd_set_validation(H(h), cu.get(), ci.get(), cr.get(), n));
}

JNIEXPORT jlong JNICALL Java_MatrixFactorizationSGD_nativeValidationSize(JNIEnv* env, jclass, jlong h) {
    int64_t n = 0;
    throw_status(env, H(h), mfsgd_validation_size(H(h), &n));
    return n;
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeValidationRmse(JNIEnv* env, jclass, jlong h, jdoubleArray out) {
    if (!out || env->GetArrayLength(out) < 2)
        return throw_new(env, "java/lang/IllegalArgumentException", "validationRmse: out needs two entries");
    double v[2] = {0.0, 0.0};
    const int rc = mfsgd_validation_rmse(H(h), &v[0], &v[1]);
    if (rc == MFSGD_OK) env->SetDoubleArrayRegion(out, 0, 2, v);
    throw_status(env, H(h), rc);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRmsePairs(JNIEnv* env, jclass, jlong h, jintArray u, jintArray i,
                                                                   jfloatArray r, jdoubleArray out) {
    if (!u || !i || !r || !out) return throw_new(env, "java/lang/NullPointerException", "rmseOn");
    const jsize n = env->GetArrayLength(u);
    if (env->GetArrayLength(i) != n || env->GetArrayLength(r) != n || env->GetArrayLength(out) < 2)
        return throw_new(env, "java/lang/IllegalArgumentException", "u, i and r must have the same length, out two entries");
    // copies, not pins: mfsgd_rmse_pairs launches a kernel per piece and waits for it
    auto cu = alloc<int32_t>(env, (size_t)n);
    auto ci = alloc<int32_t>(env, (size_t)n);
    auto cr = alloc<float>(env, (size_t)n);
    if (!cu || !ci || !cr) return;
    env->GetIntArrayRegion(u, 0, n, reinterpret_cast<jint*>(cu.get()));
    env->GetIntArrayRegion(i, 0, n, reinterpret_cast<jint*>(ci.get()));
    env->GetFloatArrayRegion(r, 0, n, cr.get());
    if (env->ExceptionCheck()) return;
    double v[2] = {0.0, 0.0};
    const int rc = mfsgd_rmse_pairs(H(h), cu.get(), ci.get(), cr.get(), n, &v[0], &v[1]);
    if (rc == MFSGD_OK) env->SetDoubleArrayRegion(out, 0, 2, v);
    throw_status(env, H(h), rc);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeApplyRatings(JNIEnv* env, jclass, jlong h, jintArray u, jintArray i,
                                                                      jfloatArray r, jfloatArray err) {
    if (!u || !i || !r || !err) return throw_new(env, "java/lang/NullPointerException", "partialFit");
    const jsize n = env->GetArrayLength(u);
    if (env->GetArrayLength(i) != n || env->GetArrayLength(r) != n || env->GetArrayLength(err) != n)
        return throw_new(env, "java/lang/IllegalArgumentException", "u, i, r and err must have the same length");
    // copies, not pins: mfsgd_apply_ratings launches a kernel per level or run of levels and waits for the device
    auto cu = alloc<int32_t>(env, (size_t)n);
    auto ci = alloc<int32_t>(env, (size_t)n);
    auto cr = alloc<float>(env, (size_t)n);
    auto ce = alloc<float>(env, (size_t)n);
    if (!cu || !ci || !cr || !ce) return;
    env->GetIntArrayRegion(u, 0, n, reinterpret_cast<jint*>(cu.get()));
    env->GetIntArrayRegion(i, 0, n, reinterpret_cast<jint*>(ci.get()));
    env->GetFloatArrayRegion(r, 0, n, cr.get());
    if (env->ExceptionCheck()) return;
    const int rc = mfsgd_apply_ratings(H(h), cu.get(), ci.get(), cr.get(), n, ce.get(), nullptr);
    if (rc == MFSGD_OK && n > 0) env->SetFloatArrayRegion(err, 0, n, ce.get());
    throw_status(env, H(h), rc);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeTrainEarlyStop(JNIEnv* env, jclass, jlong h, jint max_epochs,
                                                                        jint patience, jdouble min_delta, jint restore_best,
                                                                        jfloatArray lr, jfloatArray lambda, jdoubleArray val_rmse,
                                                                        jdoubleArray train_rmse, jintArray out) {
    if (!val_rmse || !out) return throw_new(env, "java/lang/NullPointerException", "trainEarlyStopping");
    if (max_epochs < 0 || env->GetArrayLength(val_rmse) < max_epochs || env->GetArrayLength(out) < 2 ||
        (lr && env->GetArrayLength(lr) != max_epochs) || (lambda && env->GetArrayLength(lambda) != max_epochs) ||
        (train_rmse && env->GetArrayLength(train_rmse) < max_epochs))
        return throw_new(env, "java/lang/IllegalArgumentException", "lr, lambda, valRmse and trainRmse need one entry per epoch, out two");
    // native copies, nothing pinned: the call trains, measures and re-bakes the schedule between epochs
    auto clr = alloc<float>(env, (size_t)max_epochs);
    auto clam = alloc<float>(env, (size_t)max_epochs);
    auto cval = alloc<double>(env, (size_t)max_epochs);
    auto ctrn = alloc<double>(env, (size_t)max_epochs);
    if (!clr || !clam || !cval || !ctrn) return;
    if (lr) env->GetFloatArrayRegion(lr, 0, max_epochs, clr.get());
    if (lambda) env->GetFloatArrayRegion(lambda, 0, max_epochs, clam.get());
    if (env->ExceptionCheck()) return;
    int32_t ran[2] = {0, -1};
    const int rc = mfsgd_train_early_stop(H(h), max_epochs, patience, min_delta, restore_best, lr ? clr.get() : nullptr,
                                          lambda ? clam.get() : nullptr, cval.get(), train_rmse ? ctrn.get() : nullptr, &ran[0],
                                          &ran[1]);
    // (the epochs that ran are reported even when a later one failed: they stay applied)
    if (ran[0] > 0) {
        env->SetDoubleArrayRegion(val_rmse, 0, ran[0], cval.get());
        if (train_rmse) env->SetDoubleArrayRegion(train_rmse, 0, ran[0], ctrn.get());
    }
    env->SetIntArrayRegion(out, 0, 2, reinterpret_cast<const jint*>(ran));
    throw_status(env, H(h), rc);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativePredict(JNIEnv* env, jclass, jlong h, jintArray u, jintArray i,
                                                                 jfloatArray out) {
    if (!u || !i || !out) return throw_new(env, "java/lang/NullPointerException", "predict");
    const jsize n = env->GetArrayLength(u);
    if (env->GetArrayLength(i) != n || env->GetArrayLength(out) < n)
        return throw_new(env, "java/lang/IllegalArgumentException", "u, i and out must have the same length");
    // copies, not pins: mfsgd_predict launches a kernel and waits for it
    auto cu = alloc<int32_t>(env, (size_t)n);
    auto ci = alloc<int32_t>(env, (size_t)n);
    auto co = alloc<float>(env, (size_t)n);
    if (!cu || !ci || !co) return;
    env->GetIntArrayRegion(u, 0, n, reinterpret_cast<jint*>(cu.get()));
    env->GetIntArrayRegion(i, 0, n, reinterpret_cast<jint*>(ci.get()));
    if (env->ExceptionCheck()) return;
    const int rc = mfsgd_predict(H(h), cu.get(), ci.get(), co.get(), n);
    if (rc == MFSGD_OK && n > 0) env->SetFloatArrayRegion(out, 0, n, co.get());
    throw_status(env, H(h), rc);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRecommend(JNIEnv* env, jclass, jlong h, jintArray users,
                                                                   jint topn, jintArray items, jfloatArray scores) {
    if (!users || !items || !scores) return throw_new(env, "java/lang/NullPointerException", "recommend");
    const jsize n = env->GetArrayLength(users);
    if (topn < 1 || (jlong)env->GetArrayLength(items) < (jlong)n * topn || (jlong)env->GetArrayLength(scores) < (jlong)n * topn)
        return throw_new(env, "java/lang/IllegalArgumentException", "items / scores shorter than users x topN");
    auto cu = alloc<int32_t>(env, (size_t)n);
    auto ci = alloc<int32_t>(env, (size_t)n * (size_t)topn);
    auto cs = alloc<float>(env, (size_t)n * (size_t)topn);
    if (!cu || !ci || !cs) return;
    env->GetIntArrayRegion(users, 0, n, reinterpret_cast<jint*>(cu.get()));
    if (env->ExceptionCheck()) return;
    const int rc = mfsgd_recommend(H(h), cu.get(), n, topn, ci.get(), cs.get());
    if (rc == MFSGD_OK && n > 0) {
        env->SetIntArrayRegion(items, 0, n * topn, reinterpret_cast<const jint*>(ci.get()));
        env->SetFloatArrayRegion(scores, 0, n * topn, cs.get());
    }
    throw_status(env, H(h), rc);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRecommendExcluding(JNIEnv* env, jclass, jlong h, jintArray users,
                                                                            jint topn, jintArray excl_u, jintArray excl_i,
                                                                            jintArray items, jfloatArray scores) {
    if (!users || !excl_u || !excl_i || !items || !scores)
        return throw_new(env, "java/lang/NullPointerException", "recommend");
    const jsize n = env->GetArrayLength(users);
    const jsize ne = env->GetArrayLength(excl_u);
    if (env->GetArrayLength(excl_i) != ne)
        return throw_new(env, "java/lang/IllegalArgumentException", "exclU and exclI must have the same length");
    if (topn < 1 || (jlong)env->GetArrayLength(items) < (jlong)n * topn || (jlong)env->GetArrayLength(scores) < (jlong)n * topn)
        return throw_new(env, "java/lang/IllegalArgumentException", "items / scores shorter than users x topN");
    auto cu = alloc<int32_t>(env, (size_t)n);
    auto ceu = alloc<int32_t>(env, (size_t)ne);
    auto cei = alloc<int32_t>(env, (size_t)ne);
    auto ci = alloc<int32_t>(env, (size_t)n * (size_t)topn);
    auto cs = alloc<float>(env, (size_t)n * (size_t)topn);
    if (!cu || !ceu || !cei || !ci || !cs) return;
    env->GetIntArrayRegion(users, 0, n, reinterpret_cast<jint*>(cu.get()));
    env->GetIntArrayRegion(excl_u, 0, ne, reinterpret_cast<jint*>(ceu.get()));
    env->GetIntArrayRegion(excl_i, 0, ne, reinterpret_cast<jint*>(cei.get()));
    if (env->ExceptionCheck()) return;
    const int rc = mfsgd_recommend_excluding(H(h), cu.get(), n, topn, ceu.get(), cei.get(), (int64_t)ne, ci.get(), cs.get());
    if (rc == MFSGD_OK && n > 0) {
        env->SetIntArrayRegion(items, 0, n * topn, reinterpret_cast<const jint*>(ci.get()));
        env->SetFloatArrayRegion(scores, 0, n * topn, cs.get());
    }
    throw_status(env, H(h), rc);
}

// cand_ptr == null: one candidate list (cand_items) for every row; otherwise CSR over the rows of `users`
JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRecommendAmong(JNIEnv* env, jclass, jlong h, jintArray users,
                                                                        jint topn, jlongArray cand_ptr, jintArray cand_items,
                                                                        jintArray excl_u, jintArray excl_i, jintArray items,
                                                                        jfloatArray scores) {
    if (!users || !cand_items || !excl_u || !excl_i || !items || !scores)
        return throw_new(env, "java/lang/NullPointerException", "recommendAmong");
    const jsize n = env->GetArrayLength(users);
    const jsize nc = env->GetArrayLength(cand_items);
    const jsize ne = env->GetArrayLength(excl_u);
    if (env->GetArrayLength(excl_i) != ne)
        return throw_new(env, "java/lang/IllegalArgumentException", "exclU and exclI must have the same length");
    if (cand_ptr && (jlong)env->GetArrayLength(cand_ptr) != (jlong)n + 1)
        return throw_new(env, "java/lang/IllegalArgumentException", "candPtr must have users.length + 1 entries");
    if (topn < 1 || (jlong)env->GetArrayLength(items) < (jlong)n * topn || (jlong)env->GetArrayLength(scores) < (jlong)n * topn)
        return throw_new(env, "java/lang/IllegalArgumentException", "items / scores shorter than users x topN");
    auto cu = alloc<int32_t>(env, (size_t)n);
    auto cp = alloc<int64_t>(env, (size_t)n + 1);
    auto cc = alloc<int32_t>(env, (size_t)nc);
    auto ceu = alloc<int32_t>(env, (size_t)ne);
    auto cei = alloc<int32_t>(env, (size_t)ne);
    auto ci = alloc<int32_t>(env, (size_t)n * (size_t)topn);
    auto cs = alloc<float>(env, (size_t)n * (size_t)topn);
    if (!cu || !cp || !cc || !ceu || !cei || !ci || !cs) return;
    env->GetIntArrayRegion(users, 0, n, reinterpret_cast<jint*>(cu.get()));
    if (cand_ptr) env->GetLongArrayRegion(cand_ptr, 0, n + 1, reinterpret_cast<jlong*>(cp.get()));
    env->GetIntArrayRegion(cand_items, 0, nc, reinterpret_cast<jint*>(cc.get()));
    env->GetIntArrayRegion(excl_u, 0, ne, reinterpret_cast<jint*>(ceu.get()));
    env->GetIntArrayRegion(excl_i, 0, ne, reinterpret_cast<jint*>(cei.get()));
    if (env->ExceptionCheck()) return;
    const int rc = mfsgd_recommend_among(H(h), cu.get(), n, topn, cand_ptr ? cp.get() : nullptr, cc.get(), (int64_t)nc, ceu.get(),
                                         cei.get(), (int64_t)ne, ci.get(), cs.get());
    if (rc == MFSGD_OK && n > 0) {
        env->SetIntArrayRegion(items, 0, n * topn, reinterpret_cast<const jint*>(ci.get()));
        env->SetFloatArrayRegion(scores, 0, n * topn, cs.get());
    }
    throw_status(env, H(h), rc);
}

// ---- the seen-item index: setSeen / markSeen / clearSeen (op 0 / 1 / 2), seenSize, seen, and the ...Unseen calls ----
JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeSeenUpdate(JNIEnv* env, jclass, jlong h, jint op, jintArray u, jintArray i) {
    if (op == 2) return throw_status(env, H(h), mfsgd_clear_seen(H(h)));
    if (!u || !i) return throw_new(env, "java/lang/NullPointerException", op == 0 ? "setSeen" : "markSeen");
    const jsize n = env->GetArrayLength(u);
    if (env->GetArrayLength(i) != n) return throw_new(env, "java/lang/IllegalArgumentException", "u and i must have the same length");
    // copies, not pins: the call uploads the pairs and waits for the device
    auto cu = alloc<int32_t>(env, (size_t)n);
    auto ci = alloc<int32_t>(env, (size_t)n);
    if (!cu || !ci) return;
    env->GetIntArrayRegion(u, 0, n, reinterpret_cast<jint*>(cu.get()));
    env->GetIntArrayRegion(i, 0, n, reinterpret_cast<jint*>(ci.get()));
    if (env->ExceptionCheck()) return;
    throw_status(env, H(h), (op == 0 ? mfsgd_set_seen : mfsgd_mark_seen)(H(h), cu.get(), ci.get(), (int64_t)n));
}

JNIEXPORT jlong JNICALL Java_MatrixFactorizationSGD_nativeSeenSize(JNIEnv* env, jclass, jlong h) {
    int64_t n = -1;
    throw_status(env, H(h), mfsgd_seen_size(H(h), &n));
    return (jlong)n;
}

// items == null: the offsets only.  The offsets come back as ints: the lists of one call fill a Java array, so their total
// is below 2^31 or the call is refused.
JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeGetSeen(JNIEnv* env, jclass, jlong h, jintArray users, jintArray row_ptr,
                                                                 jintArray items) {
    if (!users || !row_ptr) return throw_new(env, "java/lang/NullPointerException", "seen");
    const jsize n = env->GetArrayLength(users);
    const jsize ni = items ? env->GetArrayLength(items) : 0;
    if ((jlong)env->GetArrayLength(row_ptr) != (jlong)n + 1)
        return throw_new(env, "java/lang/IllegalArgumentException", "rowPtr must have users.length + 1 entries");
    auto cu = alloc<int32_t>(env, (size_t)n);
    auto cp = alloc<int64_t>(env, (size_t)n + 1);
    auto cp32 = alloc<int32_t>(env, (size_t)n + 1);
    auto ci = alloc<int32_t>(env, (size_t)ni);
    if (!cu || !cp || !cp32 || !ci) return;
    env->GetIntArrayRegion(users, 0, n, reinterpret_cast<jint*>(cu.get()));
    if (env->ExceptionCheck()) return;
    const int rc = mfsgd_get_seen(H(h), cu.get(), n, cp.get(), items ? ci.get() : nullptr, (int64_t)ni);
    if (rc == MFSGD_OK) {
        if (cp.get()[n] > (int64_t)INT32_MAX)
            return throw_new(env, "java/lang/IllegalArgumentException", "seen: the lists hold more than 2^31 - 1 items; ask for fewer users");
        for (jsize x = 0; x <= n; ++x) cp32.get()[x] = (int32_t)cp.get()[x];
        env->SetIntArrayRegion(row_ptr, 0, n + 1, reinterpret_cast<const jint*>(cp32.get()));
        if (items && cp.get()[n] > 0) env->SetIntArrayRegion(items, 0, (jsize)cp.get()[n], reinterpret_cast<const jint*>(ci.get()));
    }
    throw_status(env, H(h), rc);
}

// cand_items == null: every item (mfsgd_recommend_unseen); otherwise the candidates as nativeRecommendAmong takes them
JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRecommendUnseen(JNIEnv* env, jclass, jlong h, jintArray users, jint topn,
                                                                         jlongArray cand_ptr, jintArray cand_items,
                                                                         jintArray items, jfloatArray scores) {
    if (!users || !items || !scores || (cand_ptr && !cand_items))
        return throw_new(env, "java/lang/NullPointerException", "recommendUnseen");
    const jsize n = env->GetArrayLength(users);
    const jsize nc = cand_items ? env->GetArrayLength(cand_items) : 0;
    if (cand_ptr && (jlong)env->GetArrayLength(cand_ptr) != (jlong)n + 1)
        return throw_new(env, "java/lang/IllegalArgumentException", "candPtr must have users.length + 1 entries");
    if (topn < 1 || (jlong)env->GetArrayLength(items) < (jlong)n * topn || (jlong)env->GetArrayLength(scores) < (jlong)n * topn)
        return throw_new(env, "java/lang/IllegalArgumentException", "items / scores shorter than users x topN");
    auto cu = alloc<int32_t>(env, (size_t)n);
    auto cp = alloc<int64_t>(env, (size_t)n + 1);
    auto cc = alloc<int32_t>(env, (size_t)nc);
    auto ci = alloc<int32_t>(env, (size_t)n * (size_t)topn);
    auto cs = alloc<float>(env, (size_t)n * (size_t)topn);
    if (!cu || !cp || !cc || !ci || !cs) return;
    env->GetIntArrayRegion(users, 0, n, reinterpret_cast<jint*>(cu.get()));
    if (cand_ptr) env->GetLongArrayRegion(cand_ptr, 0, n + 1, reinterpret_cast<jlong*>(cp.get()));
    if (cand_items) env->GetIntArrayRegion(cand_items, 0, nc, reinterpret_cast<jint*>(cc.get()));
    if (env->ExceptionCheck()) return;
    const int rc = cand_items ? mfsgd_recommend_unseen_among(H(h), cu.get(), n, topn, cand_ptr ? cp.get() : nullptr, cc.get(),
                                                             (int64_t)nc, ci.get(), cs.get())
                              : mfsgd_recommend_unseen(H(h), cu.get(), n, topn, ci.get(), cs.get());
    if (rc == MFSGD_OK && n > 0) {
        env->SetIntArrayRegion(items, 0, n * topn, reinterpret_cast<const jint*>(ci.get()));
        env->SetFloatArrayRegion(scores, 0, n * topn, cs.get());
    }
    throw_status(env, H(h), rc);
}

// metrics7 == null: the ranks alone (mfsgd_rank_items_unseen); otherwise mfsgd_evaluate_ranking_unseen at topn
JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRankUnseen(JNIEnv* env, jclass, jlong h, jintArray u, jintArray i, jint topn,
                                                                    jdoubleArray metrics7, jintArray ranks) {
    if (!u || !i || !ranks) return throw_new(env, "java/lang/NullPointerException", "rankItemsUnseen");
    const jsize n = env->GetArrayLength(u);
    if (env->GetArrayLength(i) != n || env->GetArrayLength(ranks) < n || (metrics7 && env->GetArrayLength(metrics7) < 7))
        return throw_new(env, "java/lang/IllegalArgumentException", "rankItemsUnseen: length mismatch");
    auto cu = alloc<int32_t>(env, (size_t)n);
    auto ci = alloc<int32_t>(env, (size_t)n);
    auto cr = alloc<int32_t>(env, (size_t)n);
    if (!cu || !ci || !cr) return;
    env->GetIntArrayRegion(u, 0, n, reinterpret_cast<jint*>(cu.get()));
    env->GetIntArrayRegion(i, 0, n, reinterpret_cast<jint*>(ci.get()));
    if (env->ExceptionCheck()) return;
    mfsgd_ranking_metrics m = {};
    const int rc = metrics7 ? mfsgd_evaluate_ranking_unseen(H(h), cu.get(), ci.get(), (int64_t)n, topn, &m, cr.get())
                            : mfsgd_rank_items_unseen(H(h), cu.get(), ci.get(), (int64_t)n, cr.get());
    if (rc == MFSGD_OK && n > 0) env->SetIntArrayRegion(ranks, 0, n, reinterpret_cast<const jint*>(cr.get()));
    if (rc == MFSGD_OK && metrics7) {
        const jdouble v[7] = {(jdouble)m.n_pairs, (jdouble)m.n_users, m.hit_rate, m.precision, m.recall, m.ndcg, m.mrr};
        env->SetDoubleArrayRegion(metrics7, 0, 7, v);
    }
    throw_status(env, H(h), rc);
}

namespace {

// Body of the two fold-in natives: new users against Q (items_side false; `items` are the ids of items), new items
// against P (`items` are the ids of users).  `what` names the Java method; the length messages fit both.
void fold_in_native(JNIEnv* env, jlong h, bool items_side, const char* what, jlongArray row_ptr, jintArray items,
                    jfloatArray ratings, jint epochs, jfloatArray init, jlong seed, jfloatArray rows) {
    if (!row_ptr || !items || !ratings || !rows) return throw_new(env, "java/lang/NullPointerException", what);
    const jsize np = env->GetArrayLength(row_ptr);
    const jsize nr = env->GetArrayLength(items);
    const jsize nw = env->GetArrayLength(rows);
    if (np < 1 || env->GetArrayLength(ratings) != nr || (init && env->GetArrayLength(init) != nw))
        return throw_new(env, "java/lang/IllegalArgumentException", "fold-in: length mismatch");
    auto cp = alloc<int64_t>(env, (size_t)np);
    auto ci = alloc<int32_t>(env, (size_t)nr);
    auto cr = alloc<float>(env, (size_t)nr);
    auto c0 = alloc<float>(env, (size_t)nw);
    auto cw = alloc<float>(env, (size_t)nw);
    if (!cp || !ci || !cr || !c0 || !cw) return;
    env->GetLongArrayRegion(row_ptr, 0, np, reinterpret_cast<jlong*>(cp.get()));
    env->GetIntArrayRegion(items, 0, nr, reinterpret_cast<jint*>(ci.get()));
    env->GetFloatArrayRegion(ratings, 0, nr, cr.get());
    if (init) env->GetFloatArrayRegion(init, 0, nw, c0.get());
    if (env->ExceptionCheck()) return;
    int32_t n_users = 0, n_items = 0, k = 0;
    int rc = mfsgd_get_dims(H(h), &n_users, &n_items, &k);
    if (rc == MFSGD_OK && (jlong)nw != (jlong)(np - 1) * k)
        return throw_new(env, "java/lang/IllegalArgumentException", "fold-in: rows must be nNew x k");
    // (the last offset is checked against the arrays here: the C call cannot know their lengths)
    if (rc == MFSGD_OK && cp.get()[np - 1] != (int64_t)nr)
        return throw_new(env, "java/lang/IllegalArgumentException", "fold-in: rowPtr must end at the length of the index array");
    if (rc == MFSGD_OK)
        rc = (items_side ? mfsgd_fold_in_items : mfsgd_fold_in_users)(H(h), (int32_t)(np - 1), cp.get(), ci.get(), cr.get(), epochs,
                                                                      init ? c0.get() : nullptr, (int64_t)seed, cw.get());
    if (rc == MFSGD_OK && nw > 0) env->SetFloatArrayRegion(rows, 0, nw, cw.get());
    throw_status(env, H(h), rc);
}

}  // namespace

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeFoldIn(JNIEnv* env, jclass, jlong h, jlongArray row_ptr, jintArray items,
                                                                jfloatArray ratings, jint epochs, jfloatArray init, jlong seed,
                                                                jfloatArray rows) {
    fold_in_native(env, h, false, "foldIn", row_ptr, items, ratings, epochs, init, seed, rows);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeFoldInItems(JNIEnv* env, jclass, jlong h, jlongArray row_ptr,
                                                                     jintArray users, jfloatArray ratings, jint epochs,
                                                                     jfloatArray init, jlong seed, jfloatArray rows) {
    fold_in_native(env, h, true, "foldInItems", row_ptr, users, ratings, epochs, init, seed, rows);
}

// Growing a live model: side 0 appends users, side 1 items; rows (n x k) or, rows == null, n seeded rows.  Returns the
// index of the first new row.
JNIEXPORT jint JNICALL Java_MatrixFactorizationSGD_nativeAppend(JNIEnv* env, jclass, jlong h, jint side, jfloatArray rows, jint n,
                                                                jlong seed) {
    int32_t n_users = 0, n_items = 0, k = 0, first = -1;
    int rc = mfsgd_get_dims(H(h), &n_users, &n_items, &k);
    if (rc != MFSGD_OK) {
        throw_new(env, "java/lang/IllegalArgumentException", "append: bad handle");
        return -1;
    }
    std::unique_ptr<float[]> cr;
    if (rows) {
        const jsize len = env->GetArrayLength(rows);
        if (len % k != 0) {
            throw_new(env, "java/lang/IllegalArgumentException", "append: rows must be n x k");
            return -1;
        }
        // native copy, nothing pinned: a reallocating append waits for the device
        cr = alloc<float>(env, (size_t)len);
        if (!cr) return -1;
        env->GetFloatArrayRegion(rows, 0, len, cr.get());
        if (env->ExceptionCheck()) return -1;
        n = len / k;
    }
    rc = (side == 0 ? mfsgd_append_users : mfsgd_append_items)(H(h), n, rows ? cr.get() : nullptr, (int64_t)seed, &first);
    throw_status(env, H(h), rc);
    return first;
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeReserve(JNIEnv* env, jclass, jlong h, jint users, jint items) {
    throw_status(env, H(h), mfsgd_reserve_rows(H(h), users, items));
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeCapacity(JNIEnv* env, jclass, jlong h, jintArray users_items) {
    if (!users_items || env->GetArrayLength(users_items) != 2)
        return throw_new(env, "java/lang/IllegalArgumentException", "capacity: an int[2] is needed");
    int32_t cap[2] = {0, 0};
    const int rc = mfsgd_get_capacity(H(h), &cap[0], &cap[1]);
    if (rc == MFSGD_OK) env->SetIntArrayRegion(users_items, 0, 2, reinterpret_cast<const jint*>(cap));
    throw_status(env, H(h), rc);
}

namespace {

// Body of the three rank natives: rows == nullptr ranks against P, metrics7 != nullptr adds the metrics at topn.
void rank_native(JNIEnv* env, jlong h, jfloatArray rows, jintArray u, jintArray i, jint topn, jintArray excl_u,
                 jintArray excl_i, jdoubleArray metrics7, jintArray ranks, const char* what) {
    if (!u || !i || !excl_u || !excl_i || !ranks) return throw_new(env, "java/lang/NullPointerException", what);
    int32_t n_users = 0, n_items = 0, k = 0;
    int rc = mfsgd_get_dims(H(h), &n_users, &n_items, &k);
    if (rc != MFSGD_OK) return throw_status(env, H(h), rc);
    const jsize n = env->GetArrayLength(u);
    const jsize ne = env->GetArrayLength(excl_u);
    const jsize nf = rows ? env->GetArrayLength(rows) : 0;
    if (env->GetArrayLength(i) != n || env->GetArrayLength(excl_i) != ne || env->GetArrayLength(ranks) < n ||
        (rows && (k < 1 || nf % k != 0)) || (metrics7 && env->GetArrayLength(metrics7) < 7))
        return throw_new(env, "java/lang/IllegalArgumentException", "rankItems: length mismatch");
    // copies, not pins: the call launches kernels and waits for them
    auto cf = alloc<float>(env, (size_t)nf);
    auto cu = alloc<int32_t>(env, (size_t)n);
    auto ci = alloc<int32_t>(env, (size_t)n);
    auto ceu = alloc<int32_t>(env, (size_t)ne);
    auto cei = alloc<int32_t>(env, (size_t)ne);
    auto cr = alloc<int32_t>(env, (size_t)n);
    if (!cf || !cu || !ci || !ceu || !cei || !cr) return;
    if (rows) env->GetFloatArrayRegion(rows, 0, nf, cf.get());
    env->GetIntArrayRegion(u, 0, n, reinterpret_cast<jint*>(cu.get()));
    env->GetIntArrayRegion(i, 0, n, reinterpret_cast<jint*>(ci.get()));
    env->GetIntArrayRegion(excl_u, 0, ne, reinterpret_cast<jint*>(ceu.get()));
    env->GetIntArrayRegion(excl_i, 0, ne, reinterpret_cast<jint*>(cei.get()));
    if (env->ExceptionCheck()) return;
    mfsgd_ranking_metrics m = {};
    if (rows)
        rc = mfsgd_rank_items_rows(H(h), cf.get(), nf / k, cu.get(), ci.get(), (int64_t)n, ceu.get(), cei.get(), (int64_t)ne,
                                   cr.get());
    else if (metrics7)
        rc = mfsgd_evaluate_ranking(H(h), cu.get(), ci.get(), (int64_t)n, topn, ceu.get(), cei.get(), (int64_t)ne, &m, cr.get());
    else
        rc = mfsgd_rank_items(H(h), cu.get(), ci.get(), (int64_t)n, ceu.get(), cei.get(), (int64_t)ne, cr.get());
    if (rc == MFSGD_OK && n > 0) env->SetIntArrayRegion(ranks, 0, n, reinterpret_cast<const jint*>(cr.get()));
    if (rc == MFSGD_OK && metrics7) {
        const jdouble v[7] = {(jdouble)m.n_pairs, (jdouble)m.n_users, m.hit_rate, m.precision, m.recall, m.ndcg, m.mrr};
        env->SetDoubleArrayRegion(metrics7, 0, 7, v);
    }
    throw_status(env, H(h), rc);
}

}  // namespace

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRankItems(JNIEnv* env, jclass, jlong h, jintArray u, jintArray i,
                                                                   jintArray excl_u, jintArray excl_i, jintArray ranks) {
    rank_native(env, h, nullptr, u, i, 0, excl_u, excl_i, nullptr, ranks, "rankItems");
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRankItemsRows(JNIEnv* env, jclass, jlong h, jfloatArray rows,
                                                                       jintArray row, jintArray i, jintArray excl_row,
                                                                       jintArray excl_item, jintArray ranks) {
    if (!rows) return throw_new(env, "java/lang/NullPointerException", "rankItemsRows");
    rank_native(env, h, rows, row, i, 0, excl_row, excl_item, nullptr, ranks, "rankItemsRows");
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeEvaluateRanking(JNIEnv* env, jclass, jlong h, jintArray u, jintArray i,
                                                                         jint topn, jintArray excl_u, jintArray excl_i,
                                                                         jdoubleArray metrics7, jintArray ranks) {
    if (!metrics7) return throw_new(env, "java/lang/NullPointerException", "evaluateRanking");
    rank_native(env, h, nullptr, u, i, topn, excl_u, excl_i, metrics7, ranks, "evaluateRanking");
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRecommendRows(JNIEnv* env, jclass, jlong h, jfloatArray rows, jint topn,
                                                                       jintArray excl_row, jintArray excl_item, jintArray items,
                                                                       jfloatArray scores) {
    if (!rows || !excl_row || !excl_item || !items || !scores)
        return throw_new(env, "java/lang/NullPointerException", "recommendRows");
    int32_t n_users = 0, n_items = 0, k = 0;
    int rc = mfsgd_get_dims(H(h), &n_users, &n_items, &k);
    if (rc != MFSGD_OK) return throw_status(env, H(h), rc);
    const jsize nf = env->GetArrayLength(rows);
    const jsize ne = env->GetArrayLength(excl_row);
    if (k < 1 || nf % k != 0 || env->GetArrayLength(excl_item) != ne)
        return throw_new(env, "java/lang/IllegalArgumentException", "recommendRows: length mismatch");
    const jsize n = nf / k;
    if (topn < 1 || (jlong)env->GetArrayLength(items) < (jlong)n * topn || (jlong)env->GetArrayLength(scores) < (jlong)n * topn)
        return throw_new(env, "java/lang/IllegalArgumentException", "items / scores shorter than rows x topN");
    auto cr = alloc<float>(env, (size_t)nf);
    auto cer = alloc<int32_t>(env, (size_t)ne);
    auto cei = alloc<int32_t>(env, (size_t)ne);
    auto ci = alloc<int32_t>(env, (size_t)n * (size_t)topn);
    auto cs = alloc<float>(env, (size_t)n * (size_t)topn);
    if (!cr || !cer || !cei || !ci || !cs) return;
    env->GetFloatArrayRegion(rows, 0, nf, cr.get());
    env->GetIntArrayRegion(excl_row, 0, ne, reinterpret_cast<jint*>(cer.get()));
    env->GetIntArrayRegion(excl_item, 0, ne, reinterpret_cast<jint*>(cei.get()));
    if (env->ExceptionCheck()) return;
    rc = mfsgd_recommend_rows(H(h), cr.get(), n, topn, cer.get(), cei.get(), (int64_t)ne, ci.get(), cs.get());
    if (rc == MFSGD_OK && n > 0) {
        env->SetIntArrayRegion(items, 0, n * topn, reinterpret_cast<const jint*>(ci.get()));
        env->SetFloatArrayRegion(scores, 0, n * topn, cs.get());
    }
    throw_status(env, H(h), rc);
}

// ---- cosine neighbours: similarItems / similarUsers (queries by index), similarRows (query vectors), rowInvNorms ----

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeSimilar(JNIEnv* env, jclass, jlong h, jint side, jintArray queries,
                                                                 jint topn, jintArray index, jfloatArray scores) {
    if (!queries || !index || !scores) return throw_new(env, "java/lang/NullPointerException", "similar");
    if (side != MFSGD_SIDE_USERS && side != MFSGD_SIDE_ITEMS)
        return throw_new(env, "java/lang/IllegalArgumentException", "similar: side");
    const jsize n = env->GetArrayLength(queries);
    if (topn < 1 || (jlong)env->GetArrayLength(index) < (jlong)n * topn || (jlong)env->GetArrayLength(scores) < (jlong)n * topn)
        return throw_new(env, "java/lang/IllegalArgumentException", "index / scores shorter than queries x topN");
    auto cq = alloc<int32_t>(env, (size_t)n);
    auto ci = alloc<int32_t>(env, (size_t)n * (size_t)topn);
    auto cs = alloc<float>(env, (size_t)n * (size_t)topn);
    if (!cq || !ci || !cs) return;
    env->GetIntArrayRegion(queries, 0, n, reinterpret_cast<jint*>(cq.get()));
    if (env->ExceptionCheck()) return;
    const int rc = side == MFSGD_SIDE_ITEMS ? mfsgd_similar_items(H(h), cq.get(), n, topn, ci.get(), cs.get())
                                            : mfsgd_similar_users(H(h), cq.get(), n, topn, ci.get(), cs.get());
    if (rc == MFSGD_OK && n > 0) {
        env->SetIntArrayRegion(index, 0, n * topn, reinterpret_cast<const jint*>(ci.get()));
        env->SetFloatArrayRegion(scores, 0, n * topn, cs.get());
    }
    throw_status(env, H(h), rc);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeSimilarRows(JNIEnv* env, jclass, jlong h, jint side, jfloatArray rows,
                                                                     jint topn, jintArray index, jfloatArray scores) {
    if (!rows || !index || !scores) return throw_new(env, "java/lang/NullPointerException", "similarRows");
    int32_t n_users = 0, n_items = 0, k = 0;
    int rc = mfsgd_get_dims(H(h), &n_users, &n_items, &k);
    if (rc != MFSGD_OK) return throw_status(env, H(h), rc);
    const jsize nf = env->GetArrayLength(rows);
    if (k < 1 || nf % k != 0) return throw_new(env, "java/lang/IllegalArgumentException", "similarRows: length mismatch");
    const jsize n = nf / k;
    if (topn < 1 || (jlong)env->GetArrayLength(index) < (jlong)n * topn || (jlong)env->GetArrayLength(scores) < (jlong)n * topn)
        return throw_new(env, "java/lang/IllegalArgumentException", "index / scores shorter than rows x topN");
    auto cr = alloc<float>(env, (size_t)nf);
    auto ci = alloc<int32_t>(env, (size_t)n * (size_t)topn);
    auto cs = alloc<float>(env, (size_t)n * (size_t)topn);
    if (!cr || !ci || !cs) return;
    env->GetFloatArrayRegion(rows, 0, nf, cr.get());
    if (env->ExceptionCheck()) return;
    rc = mfsgd_similar_rows(H(h), side, cr.get(), n, topn, ci.get(), cs.get());
    if (rc == MFSGD_OK && n > 0) {
        env->SetIntArrayRegion(index, 0, n * topn, reinterpret_cast<const jint*>(ci.get()));
        env->SetFloatArrayRegion(scores, 0, n * topn, cs.get());
    }
    throw_status(env, H(h), rc);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRowInvNorms(JNIEnv* env, jclass, jlong h, jint side, jfloatArray out) {
    if (!out) return throw_new(env, "java/lang/NullPointerException", "rowInvNorms");
    int32_t n_users = 0, n_items = 0, k = 0;
    int rc = mfsgd_get_dims(H(h), &n_users, &n_items, &k);
    if (rc != MFSGD_OK) return throw_status(env, H(h), rc);
    if (side != MFSGD_SIDE_USERS && side != MFSGD_SIDE_ITEMS)
        return throw_new(env, "java/lang/IllegalArgumentException", "rowInvNorms: side");
    const jsize n = side == MFSGD_SIDE_ITEMS ? n_items : n_users;
    if (env->GetArrayLength(out) < n)
        return throw_new(env, "java/lang/IllegalArgumentException", "rowInvNorms: out shorter than the side");
    auto co = alloc<float>(env, (size_t)n);
    if (!co) return;
    rc = mfsgd_row_inv_norms(H(h), side, co.get());
    if (rc == MFSGD_OK && n > 0) env->SetFloatArrayRegion(out, 0, n, co.get());
    throw_status(env, H(h), rc);
}

// ---- DSGD: the ring under the C-ABI (mfsgd_dsgd_*) for MatrixFactorizationSGD.trainDistributed ------------------

JNIEXPORT jbyteArray JNICALL Java_MatrixFactorizationSGD_nativeDsgdUniqueId(JNIEnv* env, jclass) {
    signed char id[MFSGD_DSGD_ID_BYTES];
    const int rc = mfsgd_dsgd_unique_id(id);
    if (rc != MFSGD_OK) {
        throw_text(env, rc, mfsgd_dsgd_last_error(nullptr), "mfsgd_dsgd_unique_id failed");
        return nullptr;
    }
    jbyteArray out = env->NewByteArray(MFSGD_DSGD_ID_BYTES);
    if (out) env->SetByteArrayRegion(out, 0, MFSGD_DSGD_ID_BYTES, id);
    return out;  // null with OutOfMemoryError pending if the allocation failed
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeDsgdPlan(JNIEnv* env, jclass, jlongArray deg_user, jlongArray deg_item,
                                                                  jint n_parts, jintArray user_begin, jintArray item_part) {
    if (!deg_user || !deg_item || !user_begin || !item_part) return throw_new(env, "java/lang/NullPointerException", "plan");
    const jsize nu = env->GetArrayLength(deg_user), ni = env->GetArrayLength(deg_item);
    if (n_parts < 1 || env->GetArrayLength(user_begin) != n_parts + 1 || env->GetArrayLength(item_part) != ni)
        return throw_new(env, "java/lang/IllegalArgumentException", "plan: userBegin needs nParts + 1 entries, itemPart one per item");
    auto du = alloc<int64_t>(env, (size_t)nu);
    auto di = alloc<int64_t>(env, (size_t)ni);
    auto ub = alloc<int32_t>(env, (size_t)n_parts + 1);
    auto ip = alloc<int32_t>(env, (size_t)ni);
    if (!du || !di || !ub || !ip) return;
    env->GetLongArrayRegion(deg_user, 0, nu, reinterpret_cast<jlong*>(du.get()));
    env->GetLongArrayRegion(deg_item, 0, ni, reinterpret_cast<jlong*>(di.get()));
    if (env->ExceptionCheck()) return;
    if (mfsgd_dsgd_plan(du.get(), di.get(), nu, ni, n_parts, ub.get(), ip.get()) != MFSGD_OK)
        return throw_new(env, "java/lang/IllegalArgumentException", "plan: bad argument (empty array or negative degree)");
    env->SetIntArrayRegion(user_begin, 0, n_parts + 1, reinterpret_cast<const jint*>(ub.get()));
    env->SetIntArrayRegion(item_part, 0, ni, reinterpret_cast<const jint*>(ip.get()));
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeSetItemPartition(JNIEnv* env, jclass, jlong h, jintArray item_part) {
    int32_t items = 0;
    if (!item_part || mfsgd_get_dims(H(h), nullptr, &items, nullptr) != MFSGD_OK || env->GetArrayLength(item_part) != items)
        return throw_new(env, "java/lang/IllegalArgumentException", "itemPart must have one entry per item");
    auto ip = alloc<int32_t>(env, (size_t)items);
    if (!ip) return;
    env->GetIntArrayRegion(item_part, 0, items, reinterpret_cast<jint*>(ip.get()));
    if (env->ExceptionCheck()) return;
    throw_status(env, H(h), mfsgd_set_item_partition(H(h), ip.get()));
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeInitPOffset(JNIEnv* env, jclass, jlong h, jlong seed, jlong user_offset) {
    throw_status(env, H(h), mfsgd_init_p_offset(H(h), seed, user_offset));
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeGetUserFactors(JNIEnv* env, jclass, jlong h, jfloatArray p) {
    int32_t users = 0, k = 0;
    if (!p || mfsgd_get_dims(H(h), &users, nullptr, &k) != MFSGD_OK || (jlong)env->GetArrayLength(p) != (jlong)users * k)
        return throw_new(env, "java/lang/IllegalArgumentException", "userFactors: P must be users x k");
    const size_t np = (size_t)users * k;
    auto cp = alloc<float>(env, np);
    if (!cp) return;
    const int rc = mfsgd_get_factors(H(h), cp.get(), nullptr);
    if (rc == MFSGD_OK) env->SetFloatArrayRegion(p, 0, (jsize)np, cp.get());
    throw_status(env, H(h), rc);
}

JNIEXPORT jlong JNICALL Java_MatrixFactorizationSGD_nativeDsgdCreate(JNIEnv* env, jclass, jlong h, jint rank, jint world,
                                                                     jbyteArray id) {
    if (!id || env->GetArrayLength(id) != MFSGD_DSGD_ID_BYTES) {
        throw_new(env, "java/lang/IllegalArgumentException", "id must be the 128 bytes of distributedId()");
        return 0;
    }
    signed char raw[MFSGD_DSGD_ID_BYTES];
    env->GetByteArrayRegion(id, 0, MFSGD_DSGD_ID_BYTES, raw);
    if (env->ExceptionCheck()) return 0;
    mfsgd_dsgd* d = nullptr;
    const int rc = mfsgd_dsgd_create(H(h), rank, world, raw, &d);  // collective: ncclCommInitRank
    throw_text(env, rc, mfsgd_dsgd_last_error(nullptr), "mfsgd_dsgd_create failed");
    return reinterpret_cast<jlong>(d);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeDsgdDestroy(JNIEnv*, jclass, jlong d) { mfsgd_dsgd_destroy(D(d)); }

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeDsgdInitQ(JNIEnv* env, jclass, jlong d, jlong seed, jlong users_total) {
    throw_dsgd(env, D(d), mfsgd_dsgd_init_q(D(d), seed, users_total));
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeDsgdTrain(JNIEnv* env, jclass, jlong d, jint epochs, jdoubleArray rmse) {
    if (epochs < 0 || !rmse || env->GetArrayLength(rmse) < epochs)
        return throw_new(env, "java/lang/IllegalArgumentException", "rmse array shorter than epochs");
    auto tmp = alloc<double>(env, (size_t)epochs);
    if (!tmp) return;
    const int rc = mfsgd_dsgd_train(D(d), epochs, tmp.get());
    if (rc == MFSGD_OK && epochs > 0) env->SetDoubleArrayRegion(rmse, 0, epochs, tmp.get());
    throw_dsgd(env, D(d), rc);
}

JNIEXPORT jdouble JNICALL Java_MatrixFactorizationSGD_nativeDsgdRmse(JNIEnv* env, jclass, jlong d) {
    double out = 0.0;
    throw_dsgd(env, D(d), mfsgd_dsgd_rmse(D(d), &out));
    return out;
}

// part_rows[0] = partition id of slot j, part_rows[1] = its rows; block (nullable) receives rows x k floats
JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeDsgdGetQ(JNIEnv* env, jclass, jlong d, jint slot, jintArray part_rows,
                                                                  jfloatArray block) {
    if (!part_rows || env->GetArrayLength(part_rows) < 2) return throw_new(env, "java/lang/IllegalArgumentException", "partRows needs two entries");
    int32_t pr[2] = {0, 0};
    int rc = mfsgd_dsgd_get_q(D(d), slot, &pr[0], &pr[1], nullptr);
    if (rc != MFSGD_OK) return throw_dsgd(env, D(d), rc);
    env->SetIntArrayRegion(part_rows, 0, 2, reinterpret_cast<const jint*>(pr));
    if (!block) return;
    const jsize have = env->GetArrayLength(block);
    if (pr[1] > 0 && have % pr[1] != 0) return throw_new(env, "java/lang/IllegalArgumentException", "block must be rows x k");
    auto tmp = alloc<float>(env, (size_t)have);
    if (!tmp) return;
    rc = mfsgd_dsgd_get_q(D(d), slot, &pr[0], &pr[1], tmp.get());  // writes rows x k: the caller sized the array from k
    if (rc == MFSGD_OK && have > 0) env->SetFloatArrayRegion(block, 0, have, tmp.get());
    throw_dsgd(env, D(d), rc);
}

}  // extern "C"
