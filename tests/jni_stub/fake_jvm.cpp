// fake_jvm.cpp -- a functional stand-in for the part of a JVM that jni/mfsgd_jni.cpp talks to, so that the shim's
// functions run inside an ordinary process (tests/jni_fake.py builds the two into one shared object and drives the
// natives through ctypes).  It defines the JNIEnv member functions that tests/jni_stub/jni.h declares over a registry
// of typed arrays, and behaves as a JVM under -Xcheck:jni would, except that it NEVER aborts: a breach of the JNI
// rules is recorded as a violation string, the call returns harmlessly, and the test asserts that none was recorded.
//
// The rules enforced:
//   * arrays carry their element type: Get/Set<T>ArrayRegion on an array of another type is a violation;
//   * a null or unknown array handed to any JNIEnv function is a violation;
//   * Get/Set*ArrayRegion with start < 0, len < 0 or start + len > length copies nothing and leaves
//     java/lang/ArrayIndexOutOfBoundsException pending (what the JVM does; not a violation by itself);
//   * while an exception is pending every JNIEnv function but ExceptionCheck is a violation (ThrowNew over a pending
//     exception and a Set*ArrayRegion after a throw among them);
//   * FindClass knows the classes the shim throws; any other name returns null with NoClassDefFoundError pending;
//   * Get/ReleasePrimitiveArrayCritical are violations: the shim's rule is that nothing is pinned;
//   * per array, whether a Set* call touched it is remembered.
// Single-threaded by design, like the tests.  This is not a JVM: the Java class itself never runs here.
#include <jni.h>

#include <cstring>
#include <set>
#include <string>
#include <vector>

namespace {

struct Array : _jarray {
    char type;  // 'i' int, 'j' long, 'f' float, 'd' double, 'b' byte
    size_t elem;
    std::vector<unsigned char> bytes;
    bool written = false;
    size_t length() const { return bytes.size() / elem; }
};

struct Class : _jclass {
    const char* name;
};

Class g_classes[] = {{{}, "java/lang/RuntimeException"},
                     {{}, "java/lang/IllegalArgumentException"},
                     {{}, "java/lang/NullPointerException"},
                     {{}, "java/lang/OutOfMemoryError"},
                     {{}, "java/lang/IllegalStateException"},
                     {{}, "java/lang/ArrayIndexOutOfBoundsException"}};

JNIEnv g_env;
std::set<Array*> g_arrays;
std::vector<std::string> g_violations;
bool g_pending = false;
std::string g_pending_class, g_pending_message;

size_t elem_size(char type) {
    switch (type) {
        case 'i': case 'f': return 4;
        case 'j': case 'd': return 8;
        case 'b': return 1;
    }
    return 0;
}

void violation(const std::string& what) { g_violations.push_back(what); }

void raise(const char* cls, const std::string& msg) {
    g_pending = true;
    g_pending_class = cls;
    g_pending_message = msg;
}

// true (and a violation recorded) when an exception is pending: the caller then does nothing
bool blocked(const char* fn) {
    if (!g_pending) return false;
    violation(std::string(fn) + " called while " + g_pending_class + " is pending");
    return true;
}

Array* lookup(const char* fn, jarray a) {
    if (!a) {
        violation(std::string(fn) + ": null array");
        return nullptr;
    }
    Array* p = static_cast<Array*>(a);
    if (!g_arrays.count(p)) {
        violation(std::string(fn) + ": unknown array reference");
        return nullptr;
    }
    return p;
}

Array* new_array(char type, const void* src, size_t len) {
    Array* a = new Array();
    a->type = type;
    a->elem = elem_size(type);
    a->bytes.resize(len * a->elem);
    if (src && len) std::memcpy(a->bytes.data(), src, a->bytes.size());
    g_arrays.insert(a);
    return a;
}

// The typed region calls: type tag, bounds, then the copy.  Returns the array when the copy may proceed.
Array* region(const char* fn, jarray a, char type, jsize start, jsize len) {
    if (blocked(fn)) return nullptr;
    Array* p = lookup(fn, a);
    if (!p) return nullptr;
    if (p->type != type) {
        violation(std::string(fn) + " on an array of element type '" + p->type + "'");
        return nullptr;
    }
    if (start < 0 || len < 0 || (size_t)start + (size_t)len > p->length()) {
        raise("java/lang/ArrayIndexOutOfBoundsException",
              std::string(fn) + ": start " + std::to_string(start) + ", len " + std::to_string(len) + ", length " +
                  std::to_string(p->length()));
        return nullptr;
    }
    return p;
}

void get_region(const char* fn, jarray a, char type, jsize start, jsize len, void* buf) {
    Array* p = region(fn, a, type, start, len);
    if (!p || len == 0) return;
    if (!buf) return violation(std::string(fn) + ": null buffer");
    std::memcpy(buf, p->bytes.data() + (size_t)start * p->elem, (size_t)len * p->elem);
}

void set_region(const char* fn, jarray a, char type, jsize start, jsize len, const void* buf) {
    Array* p = region(fn, a, type, start, len);
    if (!p) return;
    p->written = true;
    if (len == 0) return;
    if (!buf) return violation(std::string(fn) + ": null buffer");
    std::memcpy(p->bytes.data() + (size_t)start * p->elem, buf, (size_t)len * p->elem);
}

}  // namespace

// ---- the JNIEnv member functions the stub declares --------------------------------------------------------------

jclass JNIEnv::FindClass(const char* name) {
    if (blocked("FindClass")) return nullptr;
    if (!name) {
        violation("FindClass: null name");
        return nullptr;
    }
    for (Class& c : g_classes)
        if (std::strcmp(c.name, name) == 0) return &c;
    raise("java/lang/NoClassDefFoundError", name);
    return nullptr;
}

jint JNIEnv::ThrowNew(jclass cls, const char* msg) {
    if (blocked("ThrowNew")) return -1;
    for (Class& c : g_classes)
        if (cls == &c) {
            if (!msg) violation(std::string("ThrowNew(") + c.name + "): null message");
            raise(c.name, msg ? msg : "");
            return 0;
        }
    violation("ThrowNew: null or unknown class");
    return -1;
}

jboolean JNIEnv::ExceptionCheck() { return g_pending ? 1 : 0; }

jsize JNIEnv::GetArrayLength(jarray a) {
    if (blocked("GetArrayLength")) return 0;
    Array* p = lookup("GetArrayLength", a);
    return p ? (jsize)p->length() : 0;
}

void* JNIEnv::GetPrimitiveArrayCritical(jarray, jboolean* is_copy) {
    violation("GetPrimitiveArrayCritical: the shim's rule is that nothing is pinned");
    if (is_copy) *is_copy = 0;
    return nullptr;
}

void JNIEnv::ReleasePrimitiveArrayCritical(jarray, void*, jint) {
    violation("ReleasePrimitiveArrayCritical: the shim's rule is that nothing is pinned");
}

void JNIEnv::GetIntArrayRegion(jintArray a, jsize start, jsize len, jint* buf) {
    get_region("GetIntArrayRegion", a, 'i', start, len, buf);
}
void JNIEnv::GetFloatArrayRegion(jfloatArray a, jsize start, jsize len, jfloat* buf) {
    get_region("GetFloatArrayRegion", a, 'f', start, len, buf);
}
void JNIEnv::GetLongArrayRegion(jlongArray a, jsize start, jsize len, jlong* buf) {
    get_region("GetLongArrayRegion", a, 'j', start, len, buf);
}
void JNIEnv::GetByteArrayRegion(jbyteArray a, jsize start, jsize len, jbyte* buf) {
    get_region("GetByteArrayRegion", a, 'b', start, len, buf);
}
void JNIEnv::SetIntArrayRegion(jintArray a, jsize start, jsize len, const jint* buf) {
    set_region("SetIntArrayRegion", a, 'i', start, len, buf);
}
void JNIEnv::SetFloatArrayRegion(jfloatArray a, jsize start, jsize len, const jfloat* buf) {
    set_region("SetFloatArrayRegion", a, 'f', start, len, buf);
}
void JNIEnv::SetDoubleArrayRegion(jdoubleArray a, jsize start, jsize len, const jdouble* buf) {
    set_region("SetDoubleArrayRegion", a, 'd', start, len, buf);
}
void JNIEnv::SetByteArrayRegion(jbyteArray a, jsize start, jsize len, const jbyte* buf) {
    set_region("SetByteArrayRegion", a, 'b', start, len, buf);
}

jbyteArray JNIEnv::NewByteArray(jsize len) {
    if (blocked("NewByteArray")) return nullptr;
    if (len < 0) {
        raise("java/lang/NegativeArraySizeException", std::to_string(len));
        return nullptr;
    }
    return static_cast<jbyteArray>(static_cast<_jarray*>(new_array('b', nullptr, (size_t)len)));
}

// ---- the control surface for Python (ctypes) ---------------------------------------------------------------------

extern "C" {

JNIEXPORT void* fake_jvm_env() { return &g_env; }

// a new array of element type `type` ('i', 'j', 'f', 'd', 'b') holding a copy of `len` elements; null for a bad type
JNIEXPORT void* fake_jvm_new_array(char type, const void* bytes, int64_t len) {
    if (!elem_size(type) || len < 0) return nullptr;
    return static_cast<_jarray*>(new_array(type, bytes, (size_t)len));
}

JNIEXPORT void fake_jvm_free_array(void* a) {
    Array* p = static_cast<Array*>(static_cast<_jarray*>(a));
    if (g_arrays.erase(p)) delete p;
}

// the control surface looks arrays up without recording violations: -1 for an unknown reference
JNIEXPORT int64_t fake_jvm_array_length(void* a) {
    Array* p = static_cast<Array*>(static_cast<_jarray*>(a));
    return g_arrays.count(p) ? (int64_t)p->length() : -1;
}
JNIEXPORT int fake_jvm_array_type(void* a) {
    Array* p = static_cast<Array*>(static_cast<_jarray*>(a));
    return g_arrays.count(p) ? p->type : 0;
}
JNIEXPORT int fake_jvm_array_written(void* a) {
    Array* p = static_cast<Array*>(static_cast<_jarray*>(a));
    return g_arrays.count(p) ? (p->written ? 1 : 0) : -1;
}
// copies the array's bytes out; returns their number, -1 for an unknown reference or a buffer that is too small
JNIEXPORT int64_t fake_jvm_array_read(void* a, void* out, int64_t capacity) {
    Array* p = static_cast<Array*>(static_cast<_jarray*>(a));
    if (!g_arrays.count(p) || capacity < (int64_t)p->bytes.size()) return -1;
    if (!p->bytes.empty()) std::memcpy(out, p->bytes.data(), p->bytes.size());
    return (int64_t)p->bytes.size();
}

JNIEXPORT int fake_jvm_pending() { return g_pending ? 1 : 0; }
JNIEXPORT const char* fake_jvm_pending_class() { return g_pending_class.c_str(); }
JNIEXPORT const char* fake_jvm_pending_message() { return g_pending_message.c_str(); }
JNIEXPORT void fake_jvm_clear_pending() {
    g_pending = false;
    g_pending_class.clear();
    g_pending_message.clear();
}

JNIEXPORT int64_t fake_jvm_violation_count() { return (int64_t)g_violations.size(); }
JNIEXPORT const char* fake_jvm_violation(int64_t x) {
    return x >= 0 && (size_t)x < g_violations.size() ? g_violations[(size_t)x].c_str() : "";
}
JNIEXPORT void fake_jvm_clear_violations() { g_violations.clear(); }

JNIEXPORT int64_t fake_jvm_live_arrays() { return (int64_t)g_arrays.size(); }

// One JNIEnv call that a correct shim never makes, on an int[] of the test's, so that the test-suite can see each rule
// fire: 0 a region that ends past the array, 1 a negative start, 2 a negative length, 3 FindClass of an unknown name,
// 4 a critical region, 5 ThrowNew twice, 6 a Set after a throw.  Returns what the call returned where it returns.
JNIEXPORT int64_t fake_jvm_probe(int what, void* a) {
    JNIEnv* env = &g_env;
    jintArray arr = static_cast<jintArray>(static_cast<_jarray*>(a));
    jint buf[4] = {1, 2, 3, 4};
    const jsize n = g_arrays.count(static_cast<Array*>(static_cast<_jarray*>(a))) ? (jsize)static_cast<Array*>(static_cast<_jarray*>(a))->length() : 0;
    switch (what) {
        case 0: env->GetIntArrayRegion(arr, n - 1, 2, buf); return buf[0];
        case 1: env->SetIntArrayRegion(arr, -1, 1, buf); return 0;
        case 2: env->SetIntArrayRegion(arr, 0, -1, buf); return 0;
        case 3: return env->FindClass("java/lang/Strin") != nullptr;
        case 4: {
            void* p = env->GetPrimitiveArrayCritical(arr, nullptr);
            env->ReleasePrimitiveArrayCritical(arr, p, JNI_ABORT);
            return p != nullptr;
        }
        case 5:
            env->ThrowNew(env->FindClass("java/lang/RuntimeException"), "first");
            return env->ThrowNew(&g_classes[1], "second");
        case 6:
            env->ThrowNew(env->FindClass("java/lang/IllegalStateException"), "thrown");
            env->SetIntArrayRegion(arr, 0, 1, buf);
            return 0;
    }
    return -1;
}

}  // extern "C"
