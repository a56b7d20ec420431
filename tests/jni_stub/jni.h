/*
 * STUB of the handful of JNI names jni/mfsgd_jni.cpp uses, transcribed from the Java Native
 * Interface specification (types, the JNIEnv member functions' signatures).  There is no JDK in
 * this image, so the real <jni.h> does not exist here; this is the one header the shim is compiled
 * against in the test-suite: for syntax and types (g++ -fsyntax-only), and for real, together with
 * fake_jvm.cpp beside it, which defines the member functions declared below over a registry of
 * typed arrays and records every breach of the JNI rules (tests/jni_fake.py, tests/test_jni_*.py).
 * It is TEST INFRASTRUCTURE: the header itself implements nothing, and a shim that passes these
 * tests has run under that stand-in, still never under a JVM.
 */
#ifndef MFSGD_TEST_JNI_STUB_H
#define MFSGD_TEST_JNI_STUB_H
#include <cstdint>
typedef int32_t jint;
typedef int64_t jlong;
typedef float jfloat;
typedef double jdouble;
typedef jint jsize;
typedef unsigned char jboolean;
typedef signed char jbyte;
class _jobject {};
class _jclass : public _jobject {};
class _jarray : public _jobject {};
class _jintArray : public _jarray {};
class _jfloatArray : public _jarray {};
class _jdoubleArray : public _jarray {};
class _jbyteArray : public _jarray {};
class _jlongArray : public _jarray {};
typedef _jobject* jobject;
typedef _jclass* jclass;
typedef _jarray* jarray;
typedef _jintArray* jintArray;
typedef _jfloatArray* jfloatArray;
typedef _jdoubleArray* jdoubleArray;
typedef _jbyteArray* jbyteArray;
typedef _jlongArray* jlongArray;
#define JNIEXPORT __attribute__((visibility("default")))
#define JNICALL
#define JNI_ABORT 2
struct JNIEnv {
    jclass FindClass(const char* name);
    jint ThrowNew(jclass cls, const char* msg);
    jboolean ExceptionCheck();
    jsize GetArrayLength(jarray a);
    void* GetPrimitiveArrayCritical(jarray a, jboolean* is_copy);
    void ReleasePrimitiveArrayCritical(jarray a, void* carray, jint mode);
    void GetIntArrayRegion(jintArray a, jsize start, jsize len, jint* buf);
    void GetFloatArrayRegion(jfloatArray a, jsize start, jsize len, jfloat* buf);
    void SetIntArrayRegion(jintArray a, jsize start, jsize len, const jint* buf);
    void SetFloatArrayRegion(jfloatArray a, jsize start, jsize len, const jfloat* buf);
    void SetDoubleArrayRegion(jdoubleArray a, jsize start, jsize len, const jdouble* buf);
    jbyteArray NewByteArray(jsize len);
    void GetByteArrayRegion(jbyteArray a, jsize start, jsize len, jbyte* buf);
    void SetByteArrayRegion(jbyteArray a, jsize start, jsize len, const jbyte* buf);
    void GetLongArrayRegion(jlongArray a, jsize start, jsize len, jlong* buf);
};
#endif
