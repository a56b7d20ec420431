"""The JNI shim (jni/mfsgd_jni.cpp) running for real, without a JVM.

There is no JDK here, so the shim is compiled against tests/jni_stub/jni.h together with tests/jni_stub/fake_jvm.cpp,
which defines the JNIEnv functions the shim uses over a registry of typed arrays and RECORDS every breach of the JNI
rules instead of aborting (type tags, null / unknown arrays, region bounds, calls while an exception is pending, unknown
classes, critical regions).  The two become one shared object, linked against the built lib/libmfsgd.so, and every
``Java_MatrixFactorizationSGD_native*`` function is called through ctypes with argument types DERIVED FROM THE JAVA
DECLARATION (``private static native ...`` in java/MatrixFactorizationSGD.java), not written by hand: a native whose
C++ definition disagrees with its Java declaration is called the way a JVM would call it.

    jvm = jni_fake.load()
    h = jvm.nativeCreate(48, 40, 10, 0.01, 0.05, 0, 0)
    p, q = jvm.out("f", 480), jvm.out("f", 400)     # arrays filled with the sentinel byte
    jvm.nativeGetFactors(h, p, q)
    assert jvm.pending() is None and jvm.violations() == []
    P = jvm.read(p)

A plain module, not a conftest: nothing here changes how the suite runs.  Nothing is put into LD_PRELOAD and no sanitizer
is involved.  This is a stand-in, not a JVM: the Java class itself never runs."""
import atexit
import ctypes as C
import os
import re
import shutil
import subprocess
import tempfile
from collections import namedtuple

import numpy as np

from tests.conftest import ROOT

PKG = os.path.join(ROOT, "matrixfactorizationsgd.java_amd")
SHIM = os.path.join(PKG, "jni", "mfsgd_jni.cpp")
JAVA = os.path.join(PKG, "java", "MatrixFactorizationSGD.java")
STUB_DIR = os.path.join(ROOT, "tests", "jni_stub")
FAKE = os.path.join(STUB_DIR, "fake_jvm.cpp")
PREFIX = "Java_MatrixFactorizationSGD_"

SENTINEL = 0xA5  # every byte of an output array before the call

_SCALAR = {"int": ("jint", C.c_int32), "long": ("jlong", C.c_int64), "float": ("jfloat", C.c_float),
           "double": ("jdouble", C.c_double), "void": ("void", None)}
_DTYPE = {"i": np.int32, "j": np.int64, "f": np.float32, "d": np.float64, "b": np.int8}


def jni_type(java_type):
    """The JNI C type of a Java primitive or primitive-array type: int -> jint, long[] -> jlongArray."""
    if java_type.endswith("[]"):
        return "j" + java_type[:-2] + "Array"
    return _SCALAR[java_type][0]


def _ctype(java_type):
    return C.c_void_p if java_type.endswith("[]") else _SCALAR[java_type][1]


def java_natives(text=None):
    """{name: (return type, [(parameter type, parameter name), ...])} of every ``private static native`` declaration of
    the Java class, in Java's type names."""
    text = open(JAVA).read() if text is None else text
    out = {}
    for ret, name, params in re.findall(r"private\s+static\s+native\s+([\w\[\]]+)\s+(native\w+)\s*\(([^)]*)\)\s*;", text):
        plist = []
        for p in (x.strip() for x in params.split(",")):
            if p:
                typ, pname = p.split()
                plist.append((typ, pname))
        out[name] = (ret, plist)
    return out


def shim_natives(text=None):
    """{name: (return type, [parameter type, ...])} of every Java_MatrixFactorizationSGD_native* DEFINITION of the shim, in
    JNI's C type names, the leading (JNIEnv*, jclass) included."""
    text = open(SHIM).read() if text is None else text
    out = {}
    for ret, name, params in re.findall(r"JNIEXPORT\s+(\w+)\s+JNICALL\s+" + PREFIX + r"(native\w+)\s*\(([^)]*)\)\s*\{", text):
        out[name] = (ret, [p.split()[0] for p in (x.strip() for x in params.split(",")) if p])
    return out


def build(out_dir):
    """mfsgd_jni.cpp + fake_jvm.cpp -> out_dir/libmfsgd_jni_fake.so, g++ only, warnings are errors; linked against the
    built libmfsgd.so with an rpath."""
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    libdir = os.path.join(PKG, "lib")
    assert os.path.exists(os.path.join(libdir, "libmfsgd.so")), "libmfsgd.so is not built"
    so = os.path.join(out_dir, "libmfsgd_jni_fake.so")
    cmd = [cxx, "-std=c++17", "-O1", "-fPIC", "-shared", "-Wall", "-Wextra", "-Werror", "-I" + STUB_DIR,
           "-I" + os.path.join(ROOT, "include"), SHIM, FAKE, "-L" + libdir, "-lmfsgd", "-Wl,-rpath," + libdir,
           "-Wl,-rpath,/opt/rocm/lib", "-o", so]
    p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    return so


class FakeJVM:
    """The loaded shim + stand-in.  ``jvm.nativeX(...)`` calls the native with (env, null class, ...); array arguments
    are the references arr() / out() return, or None for a Java null."""

    def __init__(self, so_path):
        import mfsgd_amd

        self.lib = mfsgd_amd.load_library()  # first: the shim's libmfsgd.so is then the one the Python surface uses
        self.so = C.CDLL(so_path)
        s = self.so
        s.fake_jvm_env.restype = C.c_void_p
        s.fake_jvm_new_array.restype = C.c_void_p
        s.fake_jvm_new_array.argtypes = [C.c_char, C.c_void_p, C.c_int64]
        s.fake_jvm_free_array.argtypes = [C.c_void_p]
        for f in (s.fake_jvm_array_length, s.fake_jvm_array_type, s.fake_jvm_array_written):
            f.argtypes = [C.c_void_p]
        s.fake_jvm_array_length.restype = C.c_int64
        s.fake_jvm_array_read.restype = C.c_int64
        s.fake_jvm_array_read.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        s.fake_jvm_pending_class.restype = C.c_char_p
        s.fake_jvm_pending_message.restype = C.c_char_p
        s.fake_jvm_violation_count.restype = C.c_int64
        s.fake_jvm_violation.restype = C.c_char_p
        s.fake_jvm_violation.argtypes = [C.c_int64]
        s.fake_jvm_live_arrays.restype = C.c_int64
        s.fake_jvm_probe.restype = C.c_int64
        s.fake_jvm_probe.argtypes = [C.c_int, C.c_void_p]
        self.env = s.fake_jvm_env()
        self.natives = java_natives()
        self._fn = {}
        for name, (ret, params) in self.natives.items():
            fn = getattr(s, PREFIX + name)
            fn.restype = _ctype(ret)
            fn.argtypes = [C.c_void_p, C.c_void_p] + [_ctype(t) for t, _ in params]
            self._fn[name] = fn

    def __getattr__(self, name):
        fn = self.__dict__.get("_fn", {}).get(name)
        if fn is None:
            raise AttributeError(name)
        return lambda *args: fn(self.env, None, *args)

    # -- arrays -------------------------------------------------------------------------------------------------
    def arr(self, a, element=None):
        """A Java array holding a copy of the numpy array: int32 -> int[], int64 -> long[], float32 -> float[],
        float64 -> double[], int8 / uint8 -> byte[].  `element` forces a type tag of the same width."""
        a = np.ascontiguousarray(a)
        assert a.ndim == 1
        if element is None:
            element = {"int32": "i", "int64": "j", "float32": "f", "float64": "d", "int8": "b", "uint8": "b"}[a.dtype.name]
        assert a.dtype.itemsize == np.dtype(_DTYPE[element]).itemsize
        h = self.so.fake_jvm_new_array(element.encode(), a.ctypes.data if a.size else None, a.size)
        assert h
        return h

    def out(self, element, n):
        """An array of n elements whose every byte is SENTINEL, for a native to write into."""
        dt = np.dtype(_DTYPE[element])
        return self.arr(np.frombuffer(bytes([SENTINEL]) * (n * dt.itemsize), dt), element)

    def read(self, h):
        """The array's present content, as a numpy array of its element type."""
        n = self.so.fake_jvm_array_length(h)
        assert n >= 0, "unknown array reference"
        a = np.empty(n, _DTYPE[chr(self.so.fake_jvm_array_type(h))])
        assert self.so.fake_jvm_array_read(h, a.ctypes.data, a.nbytes) == a.nbytes
        return a

    def written(self, h):
        """Whether any Set*ArrayRegion call touched the array."""
        w = self.so.fake_jvm_array_written(h)
        assert w >= 0, "unknown array reference"
        return bool(w)

    def untouched(self, h, start=0):
        """True when every byte from element `start` on is still SENTINEL."""
        a = self.read(h)
        return bool(np.all(a[start:].view(np.uint8) == SENTINEL))

    def free(self, *handles):
        for h in handles:
            if h:
                self.so.fake_jvm_free_array(h)

    # -- what the natives left behind -----------------------------------------------------------------------------
    def pending(self):
        """(class name, message) of the pending exception, which is cleared; None when there is none."""
        if not self.so.fake_jvm_pending():
            return None
        res = (self.so.fake_jvm_pending_class().decode(), self.so.fake_jvm_pending_message().decode())
        self.so.fake_jvm_clear_pending()
        return res

    def violations(self):
        """The breaches of the JNI rules recorded since the last call, which are cleared."""
        res = [self.so.fake_jvm_violation(x).decode() for x in range(self.so.fake_jvm_violation_count())]
        self.so.fake_jvm_clear_violations()
        return res

    def ok(self):
        """Asserts that the last native left no exception and broke no rule."""
        pend, viol = self.pending(), self.violations()
        assert pend is None and viol == [], (pend, viol)

    def probe(self, what, h):
        """One JNIEnv call a correct shim never makes, on the int[] h (fake_jvm.cpp lists them): the stand-in's own rules,
        made visible."""
        return self.so.fake_jvm_probe(what, h)

    def last_error(self, h):
        """mfsgd_last_error of a native handle (0: the thread's), through the library the shim is linked against."""
        return self.lib.mfsgd_last_error(C.c_void_p(h) if h else None).decode()


Out = namedtuple("Out", "element n")  # an output array of n elements, filled with the sentinel byte


class Call:
    """One native call through the fake JVM: makes the arrays, calls, and keeps the references for the checks."""

    def __init__(self, jvm, name, args):
        self.jvm, self.name, self.args = jvm, name, args
        params = [p for _, p in jvm.natives[name][1]]
        assert set(params) == set(args), (name, params, sorted(args))
        self.ref = {}
        for p in params:
            v = args[p]
            if isinstance(v, Out):
                self.ref[p] = jvm.out(v.element, v.n)
            elif isinstance(v, np.ndarray):
                self.ref[p] = jvm.arr(v)
        self.ret = getattr(jvm, name)(*[self.ref.get(p, args[p]) for p in params])
        self.pending = jvm.pending()
        self.violations = jvm.violations()

    def inputs_intact(self):
        """No input array was written, and each still holds the bytes given."""
        for p, v in self.args.items():
            if isinstance(v, np.ndarray):
                assert not self.jvm.written(self.ref[p]), (self.name, p)
                assert self.jvm.read(self.ref[p]).tobytes() == v.tobytes(), (self.name, p)

    def nothing_written(self, c_call_failed=False):
        """c_call_failed: the shim let the call through and the library refused it.  nativeTrainEarlyStop then still
        reports {epochs run, best epoch} with the exception, as documented (the epochs that ran stay applied when a
        later one fails) -- {0, -1} when none ran.  A call the shim screens out writes nothing at all."""
        self.inputs_intact()
        for p, v in self.args.items():
            if c_call_failed and self.name == "nativeTrainEarlyStop" and p == "epochsRunBestEpoch":
                assert self.read(p).tolist() == [0, -1]
            elif isinstance(v, Out):
                assert not self.jvm.written(self.ref[p]) and self.jvm.untouched(self.ref[p]), (self.name, p)

    def read(self, p):
        return self.jvm.read(self.ref[p])

    def close(self):
        self.jvm.free(*self.ref.values())


_JVM = None


def load():
    """Builds the shared object once per process, in a temporary directory removed at exit, and loads it."""
    global _JVM
    if _JVM is None:
        d = tempfile.mkdtemp(prefix="mfsgd_jni_fake_")
        atexit.register(shutil.rmtree, d, ignore_errors=True)
        _JVM = FakeJVM(build(d))
    return _JVM
