// mfsgd_jni.cpp -- JNI shim between java/MatrixFactorizationSGD.java and the C-ABI
// of include/mfsgd.h.
//
// NEVER RUN UNDER A REAL JVM: there is no JDK (no jni.h) in this container or on the
// GPU box.  What the test-suite does instead: every native below is executed under a JVM
// stand-in (tests/jni_stub/jni.h + fake_jvm.cpp) that enforces the JNI rules a shim can
// break -- typed arrays, region bounds, no call but ExceptionCheck while an exception is
// pending, no critical regions, known classes only -- and each result is compared byte for
// byte with what the Python surface returns for the same call on a twin handle
// (tests/test_jni_cpu.py, tests/test_jni_gpu.py); the class and text of every refusal are
// pinned in tests/golden/jni_refusals.json.  java/MatrixFactorizationSGD.java itself is
// still unchecked: there is no javac.  Build, where a JDK exists:
//   g++ -std=c++17 -fPIC -shared -I$JAVA_HOME/include -I$JAVA_HOME/include/linux ...
//       -I../../include mfsgd_jni.cpp -L../lib -lmfsgd -Wl,-rpath,'$ORIGIN' -o libmfsgd_jni.so
//
// Rules, upheld by the vocabulary below and not by each native again:
// NO Java array is ever pinned (Get/ReleasePrimitiveArrayCritical is not used: every C-ABI
// call may launch a kernel, start threads or wait for the device -- even set_factors waits
// for the device to go idle before it frees the old buffers -- and no JNI call may be made
// inside a critical region): every call works on NATIVE copies (In, Out); array lengths are
// checked here, not only in Java; once an exception is pending no JNI call but ExceptionCheck
// is made and nothing is written (Ctx); a failed native allocation throws OutOfMemoryError
// (Buf); a non-zero status becomes a RuntimeException carrying mfsgd_last_error(), or a fixed
// text where the library has none (a null or closed handle): no exception has an empty
// message; no C++ exception crosses the boundary (nothing here throws).
//
// A native, top to bottom:  Ctx cx(env);  the null screen (npe_if), then the length screens
// (iae_if);  the copies and buffers (In, Out, Buf, Triple, TopN), which allocate;  screens that
// need the data;  `if (cx.ok()) cx.status(H(h), mfsgd_...(...));` -- the one question before the
// C call;  commit(count) / put per output, which write only while nothing has been thrown.  After
// a refusal every piece of the vocabulary does nothing, so there is no early return to forget.
// To add a native: declare it in the Java class; define it here in that shape, written out like
// its neighbours (a JVM resolves the name and the tests read the definitions: no macro, no
// template); give it its rows in valid() and BREAKS of tests/test_jni_cpu.py and a comparison
// with the Python surface; re-record the refusals (tests/golden/make_jni_refusals.py).
#include <jni.h>

#include <cstdint>
#include <memory>
#include <new>

#include "mfsgd.h"

namespace {

const char* const NPE = "java/lang/NullPointerException";
const char* const IAE = "java/lang/IllegalArgumentException";
const char* const RTE = "java/lang/RuntimeException";

// An exception never carries an empty message: where the library has no text the shim says what it knows.
const char* text_or(const char* msg, const char* fallback) { return msg && *msg ? msg : fallback; }

mfsgd_handle* H(jlong h) { return reinterpret_cast<mfsgd_handle*>(h); }
mfsgd_dsgd* D(jlong d) { return reinterpret_cast<mfsgd_dsgd*>(d); }
jlong J(const void* p) { return reinterpret_cast<jlong>(p); }  // the handle of a new object, as Java keeps it

// One call's context.  It remembers that this native has thrown -- a screen, a failed allocation, a status -- and from
// then on it, and everything built on it, does nothing.  ok() is the whole question, an exception raised by a JNI
// call included.
class Ctx {
  public:
    explicit Ctx(JNIEnv* e) : env(e) {}
    JNIEnv* const env;

    bool ok() {
        if (!thrown_) thrown_ = env->ExceptionCheck();
        return !thrown_;
    }
    void raise(const char* cls_name, const char* msg) {
        if (thrown_) return;
        thrown_ = true;
        jclass cls = env->FindClass(cls_name);
        if (cls) env->ThrowNew(cls, msg);
    }
    void npe_if(bool refused, const char* what) { if (refused) raise(NPE, what); }
    void iae_if(bool refused, const char* text) { if (refused) raise(IAE, text); }
    // 0 for a null array (a nullable parameter) and after a refusal
    jsize len(jarray a) { return a && !thrown_ ? env->GetArrayLength(a) : 0; }

    // h == nullptr: the Java object was closed or never created.  mfsgd_last_error(nullptr) is the message of the last
    // failed mfsgd_create on this thread (empty when there was none): it says nothing about this call.
    void status(mfsgd_handle* h, int rc) {
        if (rc != MFSGD_OK)
            raise(RTE, h ? text_or(mfsgd_last_error(h), "mfsgd: the call failed without a message") : "mfsgd: null or closed handle");
    }
    void dsgd(mfsgd_dsgd* d, int rc) {
        if (rc != MFSGD_OK)
            raise(RTE, d ? text_or(mfsgd_dsgd_last_error(d), "mfsgd: the ring call failed without a message") : "mfsgd: null or closed ring");
    }
    // the calls that have no object yet (mfsgd_create, mfsgd_dsgd_unique_id, mfsgd_dsgd_create) leave their message
    // with the thread.  `rc` is a finished call's: written as an argument beside `msg`, the call could run after the read.
    void text(int rc, const char* msg, const char* fallback) { if (rc != MFSGD_OK) raise(RTE, text_or(msg, fallback)); }

  private:
    bool thrown_ = false;
};

// Per element type of the C-ABI: the Java array and JNI's element type; then the region calls the shim needs, by type.
template <class T> struct Jni;
template <> struct Jni<int32_t> { using array = jintArray; using elem = jint; };
template <> struct Jni<int64_t> { using array = jlongArray; using elem = jlong; };
template <> struct Jni<float> { using array = jfloatArray; using elem = jfloat; };
template <> struct Jni<double> { using array = jdoubleArray; using elem = jdouble; };
template <> struct Jni<signed char> { using array = jbyteArray; using elem = jbyte; };
void get_region(JNIEnv* env, jintArray a, jsize n, jint* p) { env->GetIntArrayRegion(a, 0, n, p); }
void get_region(JNIEnv* env, jlongArray a, jsize n, jlong* p) { env->GetLongArrayRegion(a, 0, n, p); }
void get_region(JNIEnv* env, jfloatArray a, jsize n, jfloat* p) { env->GetFloatArrayRegion(a, 0, n, p); }
void get_region(JNIEnv* env, jbyteArray a, jsize n, jbyte* p) { env->GetByteArrayRegion(a, 0, n, p); }
void set_region(JNIEnv* env, jintArray a, jsize n, const jint* p) { env->SetIntArrayRegion(a, 0, n, p); }
void set_region(JNIEnv* env, jfloatArray a, jsize n, const jfloat* p) { env->SetFloatArrayRegion(a, 0, n, p); }
void set_region(JNIEnv* env, jdoubleArray a, jsize n, const jdouble* p) { env->SetDoubleArrayRegion(a, 0, n, p); }
void set_region(JNIEnv* env, jbyteArray a, jsize n, const jbyte* p) { env->SetByteArrayRegion(a, 0, n, p); }

// the one place where int32_t meets jint and int64_t jlong (In and put go through it)
template <class T> typename Jni<T>::elem* as_jni(T* p) {
    static_assert(sizeof(typename Jni<T>::elem) == sizeof(T), "the JNI element type and the C-ABI's differ in size");
    return reinterpret_cast<typename Jni<T>::elem*>(p);
}

// A native buffer of n elements (never of none: an empty array still has an address for the C-ABI); new[] that
// reports failure to Java instead of throwing across the boundary.  data() == nullptr when it is not `wanted`, after
// a refusal and after the OutOfMemoryError.
template <class T> class Buf {
  public:
    Buf(Ctx& cx, size_t n, bool wanted = true) {
        if (!wanted || !cx.ok()) return;
        p_.reset(new (std::nothrow) T[n ? n : 1]);
        if (!p_) cx.raise("java/lang/OutOfMemoryError", "mfsgd_jni: native buffer");
    }
    T* data() const { return p_.get(); }

  private:
    std::unique_ptr<T[]> p_;
};

// The native copy of a Java array.  A null array -- a parameter the native documents as nullable -- gives size() 0 and
// data() == nullptr, which is how the C-ABI takes "not given".
template <class T> class In : public Buf<T> {
  public:
    In(Ctx& cx, typename Jni<T>::array a) : In(cx, a, cx.len(a)) {}
    jsize size() const { return n_; }

  private:
    In(Ctx& cx, typename Jni<T>::array a, jsize n) : Buf<T>(cx, (size_t)n, a != nullptr), n_(n) {
        if (this->data()) get_region(cx.env, a, n, as_jni(this->data()));
    }
    jsize n_;
};

// v[0 .. count) into the Java array: no JNI call for an empty region, and none once anything has been thrown -- which
// is what keeps a failed call from writing (the native reports its status first)
template <class T> void put(Ctx& cx, typename Jni<T>::array a, const T* v, jsize count) {
    if (count > 0 && cx.ok()) set_region(cx.env, a, count, as_jni(const_cast<T*>(v)));
}

// The native buffer that a C call fills for a Java output array of at least n elements (none, data() == nullptr, for
// a null array); commit() copies its first `count` back under put's conditions.
template <class T> class Out : public Buf<T> {
  public:
    Out(Ctx& cx, typename Jni<T>::array a, jlong n) : Buf<T>(cx, (size_t)n, a != nullptr), cx_(cx), a_(a) {}
    void commit(jsize count) { if (this->data()) put(cx_, a_, this->data(), count); }

  private:
    Ctx& cx_;
    typename Jni<T>::array a_;
};

// (u, i, r) of equal lengths.  `or_refused`: whatever else the native's one length message covers.
struct Triple {
    Triple(Ctx& cx, jintArray ju, jintArray ji, jfloatArray jr, bool or_refused, const char* refusal)
        : n(screen(cx, ju, ji, jr, or_refused, refusal)), u(cx, ju), i(cx, ji), r(cx, jr) {}
    const jsize n;
    In<int32_t> u, i;
    In<float> r;

  private:
    static jsize screen(Ctx& cx, jintArray ju, jintArray ji, jfloatArray jr, bool or_refused, const char* refusal) {
        const jsize n = cx.len(ju);
        cx.iae_if(cx.len(ji) != n || cx.len(jr) != n || or_refused, refusal);
        return n;
    }
};

// The two outputs of a top-N call, n x topn entries each; `refusal` names the rows: "... shorter than users x topN".
struct TopN {
    TopN(Ctx& cx, jsize n, jint topn, jintArray ji, jfloatArray js, const char* refusal)
        : total(screen(cx, n, topn, ji, js, refusal)), index(cx, ji, total), scores(cx, js, total) {}
    void commit() {
        index.commit((jsize)total);
        scores.commit((jsize)total);
    }
    const jlong total;
    Out<int32_t> index;
    Out<float> scores;

  private:
    static jlong screen(Ctx& cx, jsize n, jint topn, jintArray ji, jfloatArray js, const char* refusal) {
        const jlong total = (jlong)n * topn;
        cx.iae_if(topn < 1 || cx.len(ji) < total || cx.len(js) < total, refusal);
        return total;
    }
};

// mfsgd_get_dims.  A handle that has none is refused with `refusal` where the native has a text for that, and as any
// failed call is (cx.status) where it has not.  All three are 0 then, and after an earlier refusal, which does not ask.
struct Dims {
    int32_t users = 0, items = 0, k = 0;
};
Dims dims(Ctx& cx, jlong h, const char* refusal = nullptr) {
    Dims d;
    const int rc = cx.ok() ? mfsgd_get_dims(H(h), &d.users, &d.items, &d.k) : MFSGD_OK;
    if (refusal)
        cx.iae_if(rc != MFSGD_OK, refusal);
    else
        cx.status(H(h), rc);
    return rc == MFSGD_OK ? d : Dims();
}

void put_metrics(Ctx& cx, jdoubleArray metrics7, const mfsgd_ranking_metrics& m) {
    const jdouble v[7] = {(jdouble)m.n_pairs, (jdouble)m.n_users, m.hit_rate, m.precision, m.recall, m.ndcg, m.mrr};
    put(cx, metrics7, v, 7);
}

}  // namespace

extern "C" {

JNIEXPORT jlong JNICALL Java_MatrixFactorizationSGD_nativeCreate(JNIEnv* env, jclass, jint users, jint items, jint k, jfloat lr,
        jfloat lambda, jint device, jint n_parts) {
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
    Ctx(env).text(rc, mfsgd_last_error(nullptr), "mfsgd_create failed");
    return J(h);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeDestroy(JNIEnv*, jclass, jlong h) { mfsgd_destroy(H(h)); }

// (mfsgd_set_ratings hashes the triples, and when they are new it launches the ingest kernels, sorts on the device and
// runs the packer on host threads, 0.1 - 3 s: the reason why it gets copies and nothing stays pinned)
JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeSetRatings(JNIEnv* env, jclass, jlong h, jintArray u, jintArray i,
        jfloatArray r) {
    Ctx cx(env);
    cx.npe_if(!u || !i || !r, "ratings");
    Triple t(cx, u, i, r, false, "u, i and r must have the same length");
    if (cx.ok()) cx.status(H(h), mfsgd_set_ratings(H(h), t.u.data(), t.i.data(), t.r.data(), t.n));
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeInitFactors(JNIEnv* env, jclass, jlong h, jlong seed) {
    Ctx(env).status(H(h), mfsgd_init_factors(H(h), seed));
}

// (mfsgd_set_factors waits for the device to go idle before it frees the old device buffers: a pinned array would keep
// the collector out for as long as that takes)
JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeSetFactors(JNIEnv* env, jclass, jlong h, jfloatArray p, jfloatArray q) {
    Ctx cx(env);
    cx.iae_if(!p || !q, "setFactors: bad handle or null array");
    const Dims d = dims(cx, h, "setFactors: bad handle or null array");
    cx.iae_if(cx.len(p) != (jlong)d.users * d.k || cx.len(q) != (jlong)d.items * d.k, "setFactors: P must be users x k, Q items x k");
    In<float> cp(cx, p), cq(cx, q);
    if (cx.ok()) cx.status(H(h), mfsgd_set_factors(H(h), cp.data(), cq.data()));
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeGetFactors(JNIEnv* env, jclass, jlong h, jfloatArray p, jfloatArray q) {
    Ctx cx(env);
    cx.iae_if(!p || !q, "factors: bad handle or null array");
    const Dims d = dims(cx, h, "factors: bad handle or null array");
    const jlong np = (jlong)d.users * d.k, nq = (jlong)d.items * d.k;
    cx.iae_if(cx.len(p) != np || cx.len(q) != nq, "factors: P must be users x k, Q items x k");
    Out<float> cp(cx, p, np), cq(cx, q, nq);
    if (cx.ok()) cx.status(H(h), mfsgd_get_factors(H(h), cp.data(), cq.data()));
    cp.commit((jsize)np);
    cq.commit((jsize)nq);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeTrain(JNIEnv* env, jclass, jlong h, jint epochs, jdoubleArray rmse) {
    Ctx cx(env);
    cx.iae_if(epochs < 0 || !rmse || cx.len(rmse) < epochs, "rmse array shorter than epochs");
    Out<double> tmp(cx, rmse, epochs);  // (OutOfMemoryError: never train with the RMSE silently dropped)
    if (cx.ok()) cx.status(H(h), mfsgd_train(H(h), epochs, tmp.data()));
    tmp.commit(epochs);
}

JNIEXPORT jdouble JNICALL Java_MatrixFactorizationSGD_nativeRmse(JNIEnv* env, jclass, jlong h) {
    double out = 0.0;
    Ctx(env).status(H(h), mfsgd_rmse(H(h), &out));
    return out;
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeSetHyper(JNIEnv* env, jclass, jlong h, jfloat lr, jfloat lambda) {
    Ctx(env).status(H(h), mfsgd_set_hyper(H(h), lr, lambda));
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeGetHyper(JNIEnv* env, jclass, jlong h, jfloatArray out) {
    Ctx cx(env);
    cx.iae_if(!out || cx.len(out) < 2, "hyper: out needs two entries");
    float v[2] = {0.f, 0.f};
    if (cx.ok()) cx.status(H(h), mfsgd_get_hyper(H(h), &v[0], &v[1]));
    put(cx, out, v, 2);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeTrainSchedule(JNIEnv* env, jclass, jlong h, jfloatArray lr,
        jfloatArray lambda, jdoubleArray rmse) {
    Ctx cx(env);
    cx.npe_if(!lr || !rmse, "trainSchedule");
    const jsize epochs = cx.len(lr);
    cx.iae_if((lambda && cx.len(lambda) != epochs) || cx.len(rmse) < epochs, "lr, lambda and rmse must have one entry per epoch");
    In<float> clr(cx, lr), clam(cx, lambda);
    Out<double> tmp(cx, rmse, epochs);
    if (cx.ok()) cx.status(H(h), mfsgd_train_schedule(H(h), epochs, clr.data(), clam.data(), tmp.data()));
    tmp.commit(epochs);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeTrainBoldDriver(JNIEnv* env, jclass, jlong h, jint epochs, jfloat up,
        jfloat down, jfloatArray lr_used, jdoubleArray rmse) {
    Ctx cx(env);
    cx.iae_if(epochs < 0 || !lr_used || !rmse || cx.len(lr_used) < epochs || cx.len(rmse) < epochs,
              "lrUsed / rmse array shorter than epochs");
    Out<float> used(cx, lr_used, epochs);
    Out<double> tmp(cx, rmse, epochs);
    if (cx.ok()) cx.status(H(h), mfsgd_train_bold_driver(H(h), epochs, up, down, used.data(), tmp.data()));
    used.commit(epochs);
    tmp.commit(epochs);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeSetValidation(JNIEnv* env, jclass, jlong h, jintArray u, jintArray i,
        jfloatArray r) {
    Ctx cx(env);
    cx.npe_if(!u || !i || !r, "setValidation");
    Triple t(cx, u, i, r, false, "u, i and r must have the same length");
    if (cx.ok()) cx.status(H(h), mfsgd_set_validation(H(h), t.u.data(), t.i.data(), t.r.data(), t.n));
}

JNIEXPORT jlong JNICALL Java_MatrixFactorizationSGD_nativeValidationSize(JNIEnv* env, jclass, jlong h) {
    int64_t n = 0;
    Ctx(env).status(H(h), mfsgd_validation_size(H(h), &n));
    return n;
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeValidationRmse(JNIEnv* env, jclass, jlong h, jdoubleArray out) {
    Ctx cx(env);
    cx.iae_if(!out || cx.len(out) < 2, "validationRmse: out needs two entries");
    double v[2] = {0.0, 0.0};
    if (cx.ok()) cx.status(H(h), mfsgd_validation_rmse(H(h), &v[0], &v[1]));
    put(cx, out, v, 2);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRmsePairs(JNIEnv* env, jclass, jlong h, jintArray u, jintArray i,
        jfloatArray r, jdoubleArray out) {
    Ctx cx(env);
    cx.npe_if(!u || !i || !r || !out, "rmseOn");
    Triple t(cx, u, i, r, cx.len(out) < 2, "u, i and r must have the same length, out two entries");
    double v[2] = {0.0, 0.0};
    if (cx.ok()) cx.status(H(h), mfsgd_rmse_pairs(H(h), t.u.data(), t.i.data(), t.r.data(), t.n, &v[0], &v[1]));
    put(cx, out, v, 2);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeApplyRatings(JNIEnv* env, jclass, jlong h, jintArray u, jintArray i,
        jfloatArray r, jfloatArray err) {
    Ctx cx(env);
    cx.npe_if(!u || !i || !r || !err, "partialFit");
    Triple t(cx, u, i, r, cx.len(err) != cx.len(u), "u, i, r and err must have the same length");
    Out<float> ce(cx, err, t.n);
    if (cx.ok()) cx.status(H(h), mfsgd_apply_ratings(H(h), t.u.data(), t.i.data(), t.r.data(), t.n, ce.data(), nullptr));
    ce.commit(t.n);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeTrainEarlyStop(JNIEnv* env, jclass, jlong h, jint max_epochs,
        jint patience, jdouble min_delta, jint restore_best, jfloatArray lr, jfloatArray lambda, jdoubleArray val_rmse,
        jdoubleArray train_rmse, jintArray out) {
    Ctx cx(env);
    cx.npe_if(!val_rmse || !out, "trainEarlyStopping");
    cx.iae_if(max_epochs < 0 || cx.len(val_rmse) < max_epochs || cx.len(out) < 2 || (lr && cx.len(lr) != max_epochs) ||
                  (lambda && cx.len(lambda) != max_epochs) || (train_rmse && cx.len(train_rmse) < max_epochs),
              "lr, lambda, valRmse and trainRmse need one entry per epoch, out two");
    In<float> clr(cx, lr), clam(cx, lambda);
    Out<double> cval(cx, val_rmse, max_epochs), ctrn(cx, train_rmse, max_epochs);
    if (!cx.ok()) return;
    int32_t ran[2] = {0, -1};
    const int rc = mfsgd_train_early_stop(H(h), max_epochs, patience, min_delta, restore_best, clr.data(), clam.data(), cval.data(),
                                          ctrn.data(), &ran[0], &ran[1]);
    // the epochs that ran are reported even when a later one failed, for they stay applied: here the outputs are
    // written BEFORE the status is thrown
    cval.commit(ran[0]);
    ctrn.commit(ran[0]);
    put(cx, out, ran, 2);
    cx.status(H(h), rc);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativePredict(JNIEnv* env, jclass, jlong h, jintArray u, jintArray i,
        jfloatArray out) {
    Ctx cx(env);
    cx.npe_if(!u || !i || !out, "predict");
    const jsize n = cx.len(u);
    cx.iae_if(cx.len(i) != n || cx.len(out) < n, "u, i and out must have the same length");
    In<int32_t> cu(cx, u), ci(cx, i);
    Out<float> co(cx, out, n);
    if (cx.ok()) cx.status(H(h), mfsgd_predict(H(h), cu.data(), ci.data(), co.data(), n));
    co.commit(n);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRecommend(JNIEnv* env, jclass, jlong h, jintArray users, jint topn,
        jintArray items, jfloatArray scores) {
    Ctx cx(env);
    cx.npe_if(!users || !items || !scores, "recommend");
    const jsize n = cx.len(users);
    TopN top(cx, n, topn, items, scores, "items / scores shorter than users x topN");
    In<int32_t> cu(cx, users);
    if (cx.ok()) cx.status(H(h), mfsgd_recommend(H(h), cu.data(), n, topn, top.index.data(), top.scores.data()));
    top.commit();
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRecommendExcluding(JNIEnv* env, jclass, jlong h, jintArray users,
        jint topn, jintArray excl_u, jintArray excl_i, jintArray items, jfloatArray scores) {
    Ctx cx(env);
    cx.npe_if(!users || !excl_u || !excl_i || !items || !scores, "recommend");
    const jsize n = cx.len(users), ne = cx.len(excl_u);
    cx.iae_if(cx.len(excl_i) != ne, "exclU and exclI must have the same length");
    TopN top(cx, n, topn, items, scores, "items / scores shorter than users x topN");
    In<int32_t> cu(cx, users), ceu(cx, excl_u), cei(cx, excl_i);
    if (cx.ok())
        cx.status(H(h), mfsgd_recommend_excluding(H(h), cu.data(), n, topn, ceu.data(), cei.data(), (int64_t)ne, top.index.data(),
                                                  top.scores.data()));
    top.commit();
}

// cand_ptr == null: one candidate list (cand_items) for every row; otherwise CSR over the rows of `users`
JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRecommendAmong(JNIEnv* env, jclass, jlong h, jintArray users, jint topn,
        jlongArray cand_ptr, jintArray cand_items, jintArray excl_u, jintArray excl_i, jintArray items, jfloatArray scores) {
    Ctx cx(env);
    cx.npe_if(!users || !cand_items || !excl_u || !excl_i || !items || !scores, "recommendAmong");
    const jsize n = cx.len(users), nc = cx.len(cand_items), ne = cx.len(excl_u);
    cx.iae_if(cx.len(excl_i) != ne, "exclU and exclI must have the same length");
    cx.iae_if(cand_ptr && cx.len(cand_ptr) != (jlong)n + 1, "candPtr must have users.length + 1 entries");
    TopN top(cx, n, topn, items, scores, "items / scores shorter than users x topN");
    In<int32_t> cu(cx, users), cc(cx, cand_items), ceu(cx, excl_u), cei(cx, excl_i);
    In<int64_t> cp(cx, cand_ptr);
    if (cx.ok())
        cx.status(H(h), mfsgd_recommend_among(H(h), cu.data(), n, topn, cp.data(), cc.data(), (int64_t)nc, ceu.data(), cei.data(),
                                              (int64_t)ne, top.index.data(), top.scores.data()));
    top.commit();
}

// ---- the seen-item index: setSeen / markSeen / clearSeen (op 0 / 1 / 2), seenSize, seen, and the ...Unseen calls ----
JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeSeenUpdate(JNIEnv* env, jclass, jlong h, jint op, jintArray u, jintArray i) {
    Ctx cx(env);
    if (op == 2) return cx.status(H(h), mfsgd_clear_seen(H(h)));
    cx.npe_if(!u || !i, op == 0 ? "setSeen" : "markSeen");
    const jsize n = cx.len(u);
    cx.iae_if(cx.len(i) != n, "u and i must have the same length");
    In<int32_t> cu(cx, u), ci(cx, i);
    if (cx.ok()) cx.status(H(h), (op == 0 ? mfsgd_set_seen : mfsgd_mark_seen)(H(h), cu.data(), ci.data(), (int64_t)n));
}

JNIEXPORT jlong JNICALL Java_MatrixFactorizationSGD_nativeSeenSize(JNIEnv* env, jclass, jlong h) {
    int64_t n = -1;
    Ctx(env).status(H(h), mfsgd_seen_size(H(h), &n));
    return (jlong)n;
}

// items == null: the offsets only.  The offsets come back as ints: the lists of one call fill a Java array, so their total
// is below 2^31 or the call is refused.
JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeGetSeen(JNIEnv* env, jclass, jlong h, jintArray users, jintArray row_ptr,
        jintArray items) {
    Ctx cx(env);
    cx.npe_if(!users || !row_ptr, "seen");
    const jsize n = cx.len(users), ni = cx.len(items);
    cx.iae_if(cx.len(row_ptr) != (jlong)n + 1, "rowPtr must have users.length + 1 entries");
    In<int32_t> cu(cx, users);
    Buf<int64_t> cp(cx, (size_t)n + 1);
    Out<int32_t> cp32(cx, row_ptr, (jlong)n + 1), ci(cx, items, ni);
    if (cx.ok()) cx.status(H(h), mfsgd_get_seen(H(h), cu.data(), n, cp.data(), ci.data(), (int64_t)ni));
    if (!cx.ok()) return;
    cx.iae_if(cp.data()[n] > (int64_t)INT32_MAX, "seen: the lists hold more than 2^31 - 1 items; ask for fewer users");
    for (jsize x = 0; x <= n; ++x) cp32.data()[x] = (int32_t)cp.data()[x];
    cp32.commit(n + 1);
    ci.commit((jsize)cp32.data()[n]);
}

// cand_items == null: every item (mfsgd_recommend_unseen); otherwise the candidates as nativeRecommendAmong takes them
JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRecommendUnseen(JNIEnv* env, jclass, jlong h, jintArray users, jint topn,
        jlongArray cand_ptr, jintArray cand_items, jintArray items, jfloatArray scores) {
    Ctx cx(env);
    cx.npe_if(!users || !items || !scores || (cand_ptr && !cand_items), "recommendUnseen");
    const jsize n = cx.len(users), nc = cx.len(cand_items);
    cx.iae_if(cand_ptr && cx.len(cand_ptr) != (jlong)n + 1, "candPtr must have users.length + 1 entries");
    TopN top(cx, n, topn, items, scores, "items / scores shorter than users x topN");
    In<int32_t> cu(cx, users), cc(cx, cand_items);
    In<int64_t> cp(cx, cand_ptr);
    if (cx.ok())
        cx.status(H(h), cand_items ? mfsgd_recommend_unseen_among(H(h), cu.data(), n, topn, cp.data(), cc.data(), (int64_t)nc,
                                                                  top.index.data(), top.scores.data())
                                   : mfsgd_recommend_unseen(H(h), cu.data(), n, topn, top.index.data(), top.scores.data()));
    top.commit();
}

// metrics7 == null: the ranks alone (mfsgd_rank_items_unseen); otherwise mfsgd_evaluate_ranking_unseen at topn
JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRankUnseen(JNIEnv* env, jclass, jlong h, jintArray u, jintArray i, jint topn,
        jdoubleArray metrics7, jintArray ranks) {
    Ctx cx(env);
    cx.npe_if(!u || !i || !ranks, "rankItemsUnseen");
    const jsize n = cx.len(u);
    cx.iae_if(cx.len(i) != n || cx.len(ranks) < n || (metrics7 && cx.len(metrics7) < 7), "rankItemsUnseen: length mismatch");
    In<int32_t> cu(cx, u), ci(cx, i);
    Out<int32_t> cr(cx, ranks, n);
    mfsgd_ranking_metrics m = {};
    if (cx.ok())
        cx.status(H(h), metrics7 ? mfsgd_evaluate_ranking_unseen(H(h), cu.data(), ci.data(), (int64_t)n, topn, &m, cr.data())
                                 : mfsgd_rank_items_unseen(H(h), cu.data(), ci.data(), (int64_t)n, cr.data()));
    cr.commit(n);
    if (metrics7) put_metrics(cx, metrics7, m);
}

namespace {

// Body of the two fold-in natives: new users against Q (items_side false; `items` are the ids of items), new items
// against P (`items` are the ids of users).  `what` names the Java method; the length messages fit both.
void fold_in_native(JNIEnv* env, jlong h, bool items_side, const char* what, jlongArray row_ptr, jintArray items,
                    jfloatArray ratings, jint epochs, jfloatArray init, jlong seed, jfloatArray rows) {
    Ctx cx(env);
    cx.npe_if(!row_ptr || !items || !ratings || !rows, what);
    const jsize np = cx.len(row_ptr), nr = cx.len(items), nw = cx.len(rows);
    cx.iae_if(np < 1 || cx.len(ratings) != nr || (init && cx.len(init) != nw), "fold-in: length mismatch");
    In<int64_t> cp(cx, row_ptr);
    In<int32_t> ci(cx, items);
    In<float> cr(cx, ratings), c0(cx, init);
    Out<float> cw(cx, rows, nw);
    const Dims d = dims(cx, h);
    cx.iae_if(nw != (jlong)(np - 1) * d.k, "fold-in: rows must be nNew x k");
    // (the last offset is checked against the arrays here: the C call cannot know their lengths)
    cx.iae_if(cx.ok() && cp.data()[np - 1] != (int64_t)nr, "fold-in: rowPtr must end at the length of the index array");
    if (cx.ok())
        cx.status(H(h), (items_side ? mfsgd_fold_in_items : mfsgd_fold_in_users)(H(h), (int32_t)(np - 1), cp.data(), ci.data(), cr.data(),
                                                                                 epochs, c0.data(), (int64_t)seed, cw.data()));
    cw.commit(nw);
}

}  // namespace

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeFoldIn(JNIEnv* env, jclass, jlong h, jlongArray row_ptr, jintArray items,
        jfloatArray ratings, jint epochs, jfloatArray init, jlong seed, jfloatArray rows) {
    fold_in_native(env, h, false, "foldIn", row_ptr, items, ratings, epochs, init, seed, rows);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeFoldInItems(JNIEnv* env, jclass, jlong h, jlongArray row_ptr,
        jintArray users, jfloatArray ratings, jint epochs, jfloatArray init, jlong seed, jfloatArray rows) {
    fold_in_native(env, h, true, "foldInItems", row_ptr, users, ratings, epochs, init, seed, rows);
}

// Growing a live model: side 0 appends users, side 1 items; rows (n x k) or, rows == null, n seeded rows.  Returns the
// index of the first new row.
JNIEXPORT jint JNICALL Java_MatrixFactorizationSGD_nativeAppend(JNIEnv* env, jclass, jlong h, jint side, jfloatArray rows, jint n,
        jlong seed) {
    Ctx cx(env);
    const Dims d = dims(cx, h, "append: bad handle");
    if (!cx.ok()) return -1;
    cx.iae_if(cx.len(rows) % d.k != 0, "append: rows must be n x k");
    In<float> cr(cx, rows);
    int32_t first = -1;
    if (cx.ok())
        cx.status(H(h), (side == 0 ? mfsgd_append_users : mfsgd_append_items)(H(h), rows ? cr.size() / d.k : n, cr.data(),
                                                                              (int64_t)seed, &first));
    return first;
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeReserve(JNIEnv* env, jclass, jlong h, jint users, jint items) {
    Ctx(env).status(H(h), mfsgd_reserve_rows(H(h), users, items));
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeCapacity(JNIEnv* env, jclass, jlong h, jintArray users_items) {
    Ctx cx(env);
    cx.iae_if(!users_items || cx.len(users_items) != 2, "capacity: an int[2] is needed");
    int32_t cap[2] = {0, 0};
    if (cx.ok()) cx.status(H(h), mfsgd_get_capacity(H(h), &cap[0], &cap[1]));
    put(cx, users_items, cap, 2);
}

namespace {

// Body of the three rank natives: rows == nullptr ranks against P, metrics7 != nullptr adds the metrics at topn.
void rank_native(Ctx& cx, jlong h, jfloatArray rows, jintArray u, jintArray i, jint topn, jintArray excl_u, jintArray excl_i,
                 jdoubleArray metrics7, jintArray ranks, const char* what) {
    cx.npe_if(!u || !i || !excl_u || !excl_i || !ranks, what);
    const Dims d = dims(cx, h);
    const jsize n = cx.len(u), ne = cx.len(excl_u), nf = cx.len(rows);
    cx.iae_if(cx.len(i) != n || cx.len(excl_i) != ne || cx.len(ranks) < n || (rows && (d.k < 1 || nf % d.k != 0)) ||
                  (metrics7 && cx.len(metrics7) < 7),
              "rankItems: length mismatch");
    In<float> cf(cx, rows);
    In<int32_t> cu(cx, u), ci(cx, i), ceu(cx, excl_u), cei(cx, excl_i);
    Out<int32_t> cr(cx, ranks, n);
    if (!cx.ok()) return;
    mfsgd_ranking_metrics m = {};
    if (rows)
        cx.status(H(h), mfsgd_rank_items_rows(H(h), cf.data(), nf / d.k, cu.data(), ci.data(), (int64_t)n, ceu.data(), cei.data(),
                                              (int64_t)ne, cr.data()));
    else if (metrics7)
        cx.status(H(h), mfsgd_evaluate_ranking(H(h), cu.data(), ci.data(), (int64_t)n, topn, ceu.data(), cei.data(), (int64_t)ne, &m,
                                               cr.data()));
    else
        cx.status(H(h), mfsgd_rank_items(H(h), cu.data(), ci.data(), (int64_t)n, ceu.data(), cei.data(), (int64_t)ne, cr.data()));
    cr.commit(n);
    if (metrics7) put_metrics(cx, metrics7, m);
}

}  // namespace

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRankItems(JNIEnv* env, jclass, jlong h, jintArray u, jintArray i,
        jintArray excl_u, jintArray excl_i, jintArray ranks) {
    Ctx cx(env);
    rank_native(cx, h, nullptr, u, i, 0, excl_u, excl_i, nullptr, ranks, "rankItems");
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRankItemsRows(JNIEnv* env, jclass, jlong h, jfloatArray rows, jintArray row,
        jintArray i, jintArray excl_row, jintArray excl_item, jintArray ranks) {
    Ctx cx(env);
    cx.npe_if(!rows, "rankItemsRows");
    rank_native(cx, h, rows, row, i, 0, excl_row, excl_item, nullptr, ranks, "rankItemsRows");
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeEvaluateRanking(JNIEnv* env, jclass, jlong h, jintArray u, jintArray i,
        jint topn, jintArray excl_u, jintArray excl_i, jdoubleArray metrics7, jintArray ranks) {
    Ctx cx(env);
    cx.npe_if(!metrics7, "evaluateRanking");
    rank_native(cx, h, nullptr, u, i, topn, excl_u, excl_i, metrics7, ranks, "evaluateRanking");
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRecommendRows(JNIEnv* env, jclass, jlong h, jfloatArray rows, jint topn,
        jintArray excl_row, jintArray excl_item, jintArray items, jfloatArray scores) {
    Ctx cx(env);
    cx.npe_if(!rows || !excl_row || !excl_item || !items || !scores, "recommendRows");
    const Dims d = dims(cx, h);
    const jsize nf = cx.len(rows), ne = cx.len(excl_row);
    cx.iae_if(d.k < 1 || nf % d.k != 0 || cx.len(excl_item) != ne, "recommendRows: length mismatch");
    const jsize n = cx.ok() ? nf / d.k : 0;
    TopN top(cx, n, topn, items, scores, "items / scores shorter than rows x topN");
    In<float> cr(cx, rows);
    In<int32_t> cer(cx, excl_row), cei(cx, excl_item);
    if (cx.ok())
        cx.status(H(h), mfsgd_recommend_rows(H(h), cr.data(), n, topn, cer.data(), cei.data(), (int64_t)ne, top.index.data(),
                                             top.scores.data()));
    top.commit();
}

// ---- cosine neighbours: similarItems / similarUsers (queries by index), similarRows (query vectors), rowInvNorms ----

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeSimilar(JNIEnv* env, jclass, jlong h, jint side, jintArray queries,
        jint topn, jintArray index, jfloatArray scores) {
    Ctx cx(env);
    cx.npe_if(!queries || !index || !scores, "similar");
    cx.iae_if(side != MFSGD_SIDE_USERS && side != MFSGD_SIDE_ITEMS, "similar: side");
    const jsize n = cx.len(queries);
    TopN top(cx, n, topn, index, scores, "index / scores shorter than queries x topN");
    In<int32_t> cq(cx, queries);
    if (cx.ok())
        cx.status(H(h), (side == MFSGD_SIDE_ITEMS ? mfsgd_similar_items : mfsgd_similar_users)(H(h), cq.data(), n, topn,
                                                                                               top.index.data(), top.scores.data()));
    top.commit();
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeSimilarRows(JNIEnv* env, jclass, jlong h, jint side, jfloatArray rows,
        jint topn, jintArray index, jfloatArray scores) {
    Ctx cx(env);
    cx.npe_if(!rows || !index || !scores, "similarRows");
    const Dims d = dims(cx, h);
    const jsize nf = cx.len(rows);
    cx.iae_if(d.k < 1 || nf % d.k != 0, "similarRows: length mismatch");
    const jsize n = cx.ok() ? nf / d.k : 0;
    TopN top(cx, n, topn, index, scores, "index / scores shorter than rows x topN");
    In<float> cr(cx, rows);
    if (cx.ok()) cx.status(H(h), mfsgd_similar_rows(H(h), side, cr.data(), n, topn, top.index.data(), top.scores.data()));
    top.commit();
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeRowInvNorms(JNIEnv* env, jclass, jlong h, jint side, jfloatArray out) {
    Ctx cx(env);
    cx.npe_if(!out, "rowInvNorms");
    const Dims d = dims(cx, h);
    cx.iae_if(side != MFSGD_SIDE_USERS && side != MFSGD_SIDE_ITEMS, "rowInvNorms: side");
    const jsize n = side == MFSGD_SIDE_ITEMS ? d.items : d.users;
    cx.iae_if(cx.len(out) < n, "rowInvNorms: out shorter than the side");
    Out<float> co(cx, out, n);
    if (cx.ok()) cx.status(H(h), mfsgd_row_inv_norms(H(h), side, co.data()));
    co.commit(n);
}

// ---- DSGD: the ring under the C-ABI (mfsgd_dsgd_*) for MatrixFactorizationSGD.trainDistributed ------------------

JNIEXPORT jbyteArray JNICALL Java_MatrixFactorizationSGD_nativeDsgdUniqueId(JNIEnv* env, jclass) {
    Ctx cx(env);
    signed char id[MFSGD_DSGD_ID_BYTES];
    const int rc = mfsgd_dsgd_unique_id(id);
    cx.text(rc, mfsgd_dsgd_last_error(nullptr), "mfsgd_dsgd_unique_id failed");
    jbyteArray out = cx.ok() ? env->NewByteArray(MFSGD_DSGD_ID_BYTES) : nullptr;
    if (out) put(cx, out, id, MFSGD_DSGD_ID_BYTES);
    return out;  // null with OutOfMemoryError pending if the allocation failed
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeDsgdPlan(JNIEnv* env, jclass, jlongArray deg_user, jlongArray deg_item,
        jint n_parts, jintArray user_begin, jintArray item_part) {
    Ctx cx(env);
    cx.npe_if(!deg_user || !deg_item || !user_begin || !item_part, "plan");
    const jsize nu = cx.len(deg_user), ni = cx.len(deg_item);
    cx.iae_if(n_parts < 1 || cx.len(user_begin) != n_parts + 1 || cx.len(item_part) != ni,
              "plan: userBegin needs nParts + 1 entries, itemPart one per item");
    In<int64_t> du(cx, deg_user), di(cx, deg_item);
    Out<int32_t> ub(cx, user_begin, (jlong)n_parts + 1), ip(cx, item_part, ni);
    if (cx.ok())
        cx.iae_if(mfsgd_dsgd_plan(du.data(), di.data(), nu, ni, n_parts, ub.data(), ip.data()) != MFSGD_OK,
                  "plan: bad argument (empty array or negative degree)");
    ub.commit(n_parts + 1);
    ip.commit(ni);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeSetItemPartition(JNIEnv* env, jclass, jlong h, jintArray item_part) {
    Ctx cx(env);
    cx.iae_if(!item_part, "itemPart must have one entry per item");
    const Dims d = dims(cx, h, "itemPart must have one entry per item");
    cx.iae_if(cx.len(item_part) != d.items, "itemPart must have one entry per item");
    In<int32_t> ip(cx, item_part);
    if (cx.ok()) cx.status(H(h), mfsgd_set_item_partition(H(h), ip.data()));
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeInitPOffset(JNIEnv* env, jclass, jlong h, jlong seed, jlong user_offset) {
    Ctx(env).status(H(h), mfsgd_init_p_offset(H(h), seed, user_offset));
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeGetUserFactors(JNIEnv* env, jclass, jlong h, jfloatArray p) {
    Ctx cx(env);
    cx.iae_if(!p, "userFactors: P must be users x k");
    const Dims d = dims(cx, h, "userFactors: P must be users x k");
    const jlong np = (jlong)d.users * d.k;
    cx.iae_if(cx.len(p) != np, "userFactors: P must be users x k");
    Out<float> cp(cx, p, np);
    if (cx.ok()) cx.status(H(h), mfsgd_get_factors(H(h), cp.data(), nullptr));
    cp.commit((jsize)np);
}

JNIEXPORT jlong JNICALL Java_MatrixFactorizationSGD_nativeDsgdCreate(JNIEnv* env, jclass, jlong h, jint rank, jint world,
        jbyteArray id) {
    Ctx cx(env);
    cx.iae_if(!id || cx.len(id) != MFSGD_DSGD_ID_BYTES, "id must be the 128 bytes of distributedId()");
    In<signed char> raw(cx, id);
    if (!cx.ok()) return 0;
    mfsgd_dsgd* d = nullptr;
    const int rc = mfsgd_dsgd_create(H(h), rank, world, raw.data(), &d);  // collective: ncclCommInitRank
    cx.text(rc, mfsgd_dsgd_last_error(nullptr), "mfsgd_dsgd_create failed");  // (the message is read after the call)
    return J(d);
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeDsgdDestroy(JNIEnv*, jclass, jlong d) { mfsgd_dsgd_destroy(D(d)); }

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeDsgdInitQ(JNIEnv* env, jclass, jlong d, jlong seed, jlong users_total) {
    Ctx(env).dsgd(D(d), mfsgd_dsgd_init_q(D(d), seed, users_total));
}

JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeDsgdTrain(JNIEnv* env, jclass, jlong d, jint epochs, jdoubleArray rmse) {
    Ctx cx(env);
    cx.iae_if(epochs < 0 || !rmse || cx.len(rmse) < epochs, "rmse array shorter than epochs");
    Out<double> tmp(cx, rmse, epochs);
    if (cx.ok()) cx.dsgd(D(d), mfsgd_dsgd_train(D(d), epochs, tmp.data()));
    tmp.commit(epochs);
}

JNIEXPORT jdouble JNICALL Java_MatrixFactorizationSGD_nativeDsgdRmse(JNIEnv* env, jclass, jlong d) {
    double out = 0.0;
    Ctx(env).dsgd(D(d), mfsgd_dsgd_rmse(D(d), &out));
    return out;
}

// part_rows[0] = partition id of slot j, part_rows[1] = its rows; block (nullable) receives rows x k floats
JNIEXPORT void JNICALL Java_MatrixFactorizationSGD_nativeDsgdGetQ(JNIEnv* env, jclass, jlong d, jint slot, jintArray part_rows,
        jfloatArray block) {
    Ctx cx(env);
    cx.iae_if(!part_rows || cx.len(part_rows) < 2, "partRows needs two entries");
    int32_t pr[2] = {0, 0};
    if (cx.ok()) cx.dsgd(D(d), mfsgd_dsgd_get_q(D(d), slot, &pr[0], &pr[1], nullptr));
    put(cx, part_rows, pr, 2);
    const jsize have = cx.len(block);
    cx.iae_if(pr[1] > 0 && have % pr[1] != 0, "block must be rows x k");
    Out<float> tmp(cx, block, have);  // sized from the Java array while the library writes rows x k: see ADVICE.md
    if (cx.ok() && block) cx.dsgd(D(d), mfsgd_dsgd_get_q(D(d), slot, &pr[0], &pr[1], tmp.data()));
    tmp.commit(have);
}

}  // extern "C"
