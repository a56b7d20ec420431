"""Host-side behaviour of the C-ABI that needs no GPU: the library loads, exports
every symbol include/mfsgd.h declares, validates arguments, seeds factors like
java.util.Random, and fails loudly (no CPU fallback) when compute is requested
without a device."""
import ctypes as C
import os
import re

import numpy as np
import pytest

from tests.conftest import ROOT, have_gpu


def test_exports_every_declared_symbol(mf):
    hdr = open(os.path.join(ROOT, "include", "mfsgd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(mfsgd_[a-z0-9_]+)\s*\(", hdr))
    assert len(declared) >= 20
    lib = C.CDLL(mf.library_path())
    for name in sorted(declared):
        assert hasattr(lib, name), f"{name} declared in mfsgd.h but not exported"
    from mfsgd_amd import _lib

    assert declared == set(_lib.SIGNATURES), "ctypes binding out of sync with mfsgd.h"
    assert lib.mfsgd_abi_version() == 3


def test_create_validation(mf):
    M = mf.MatrixFactorizationSGD
    for bad in (dict(users=0), dict(items=0), dict(k=0), dict(k=257), dict(waves=3), dict(n_parts=-1)):
        kw = dict(users=10, items=10, k=8, lr=0.01, lam=0.05, seed=1)
        extra = {}
        for key, v in bad.items():
            if key in kw:
                kw[key] = v
            else:
                extra[key] = v
        with pytest.raises(mf.MfsgdError):
            M(kw["users"], kw["items"], kw["k"], kw["lr"], kw["lam"], kw["seed"], **extra)
    with pytest.raises(mf.MfsgdError) as ei:
        M(10, 10, 300, 0.01, 0.05, 1)
    assert ei.value.code == -6  # MFSGD_ERR_UNSUPPORTED


def test_set_ratings_validation(mf):
    with mf.MatrixFactorizationSGD(4, 3, 8, 0.01, 0.05, 1) as m:
        with pytest.raises(mf.MfsgdError):
            m.set_ratings([0, 4], [0, 1], [1.0, 2.0])  # user out of range
        with pytest.raises(mf.MfsgdError):
            m.set_ratings([0, 1], [0, -1], [1.0, 2.0])
        with pytest.raises(mf.MfsgdError):
            m.schedule_info()  # nothing set yet
        m.set_ratings([], [], [])
        assert m.schedule_info()["nnz"] == 0


def test_init_matches_java_random(mf, oracle):
    for (U, I, k) in ((7, 5, 8), (3, 9, 5), (2, 2, 64), (4, 4, 100)):
        with mf.MatrixFactorizationSGD(U, I, k, 0.01, 0.05, 123) as m:
            m.init_factors()
            P, Q = m.get_factors()
        Po, Qo = oracle.init_factors(U, I, k, 123)
        np.testing.assert_array_equal(P, Po)
        np.testing.assert_array_equal(Q, Qo)


def test_set_get_factors_roundtrip(mf):
    rng = np.random.default_rng(0)
    P = rng.random((6, 10), dtype=np.float32)
    Q = rng.random((4, 10), dtype=np.float32)
    with mf.MatrixFactorizationSGD(6, 4, 10, 0.01, 0.05, 1) as m:
        m.set_factors(P, Q)
        P2, Q2 = m.get_factors()
    np.testing.assert_array_equal(P, P2)
    np.testing.assert_array_equal(Q, Q2)


def test_a_host_only_life_cycle_holds_no_device_memory(mf):
    """Ratings ingested on the host, factors seeded, set and read back: nothing of it is device memory, and after
    the handle is closed the library's count of the device bytes it holds (mfsgd_debug_device_bytes) is zero."""
    from mfsgd_amd import _lib

    rng = np.random.default_rng(1)
    U, I, k = 9, 7, 5
    u, i = rng.integers(0, U, 60), rng.integers(0, I, 60)
    with mf.MatrixFactorizationSGD(U, I, k, 0.01, 0.05, 1, flags=_lib.FLAG_HOST_INGEST) as m:
        m.set_ratings(u, i, rng.random(60, dtype=np.float32))
        m.init_factors()
        P, Q = m.get_factors()
        m.set_factors(P, Q)
        P2, Q2 = m.get_factors()
    np.testing.assert_array_equal(P, P2)
    np.testing.assert_array_equal(Q, Q2)
    assert mf.debug_device_bytes() == 0


def test_part_init_q_is_a_slice_of_the_full_init(mf, oracle):
    U_total, I, k, G, seed = 11, 13, 6, 3, 77
    _, Qo = oracle.init_factors(U_total, I, k, seed)
    with mf.MatrixFactorizationSGD(5, I, k, 0.01, 0.05, seed, n_parts=G) as m:
        for part in range(G):
            blk = m.part_init_q(part, seed, U_total)
            idx = np.arange(part, I, G)
            assert m.part_rows(part) == idx.size
            np.testing.assert_array_equal(blk[:, :k], Qo[idx])
            assert not blk[:, k:].any()
        # P of a rank that holds users [4, 9)
        m.init_p_offset(seed, 4)
        P, _ = m.get_factors()
    Po, _ = oracle.init_factors(U_total, I, k, seed)
    np.testing.assert_array_equal(P, Po[4:9])


def test_a_single_partition_handle_seeded_by_init_p_offset_has_no_q(mf, oracle, tmp_path):
    """mfsgd_init_p_offset seeds P alone.  On a single-partition handle every call that reads the handle's own Q is
    MFSGD_ERR_STATE from then on, with the call's prefix, before a device is asked for (so the code is the same with and
    without a GPU, and nothing is launched); the calls that need P alone go on working; init_factors, set_factors and
    load_factors make the handle whole again."""
    from tests.handle_model import q_less_calls
    from tests.test_validation_cpu import STATE, _raises

    U_total, U, I, k, seed, off = 11, 5, 7, 6, 77, 4
    Po, Qo = oracle.init_factors(U_total, I, k, seed)
    with mf.MatrixFactorizationSGD(U, I, k, 0.01, 0.05, seed) as m:
        m.set_ratings([0, 1, 2, 4], [0, 1, 2, 6], [1.0, 2.0, 3.0, 4.0])
        m.set_validation([3, 4], [4, 6], [2.5, 3.5])
        m.init_factors()
        full = m.get_factors()
        path = str(tmp_path / "whole.bin")
        m.save_factors(path)

        def lose_q():
            m.init_p_offset(seed, off)
            for prefix, call in q_less_calls(m):
                _raises(mf, STATE, prefix, call)
                assert "Q is not initialised" in m._lib.mfsgd_last_error(m._handle()).decode(), prefix
            with pytest.raises(mf.MfsgdError) as ei:
                m.save_factors(str(tmp_path / "none.bin"))
            assert ei.value.code == STATE
            # P alone is still there, and so is everything that needs no Q of the handle's
            P = np.empty((U, k), np.float32)
            m._check(m._lib.mfsgd_get_factors(m._handle(), P.ctypes.data_as(C.POINTER(C.c_float)), None))
            np.testing.assert_array_equal(P, Po[off:off + U])
            assert m.part_rows(0) == I and np.array_equal(m.part_init_q(0, seed, U_total)[:, :k], Qo)
            assert m.hyper() == (float(np.float32(0.01)), float(np.float32(0.05))) and m.validation_size() == 2
            if not have_gpu():
                for call in (lambda: m.similar_users([0], 1), lambda: m.row_inv_norms("users")):
                    with pytest.raises(mf.MfsgdError) as ei:
                        call()
                    assert ei.value.code == -2, ei.value  # MFSGD_ERR_NO_DEVICE: past the state checks
            else:
                assert m.similar_users([0], 1)[0].shape == (1, 1) and m.row_inv_norms("users").shape == (U,)

        lose_q()
        m.set_factors(*full)
        for a, b in zip(m.get_factors(), full):
            np.testing.assert_array_equal(a, b)
        lose_q()
        m.init_factors()
        for a, b in zip(m.get_factors(), full):
            np.testing.assert_array_equal(a, b)
        lose_q()
        m.load_factors(path)
        for a, b in zip(m.get_factors(), full):
            np.testing.assert_array_equal(a, b)
        if have_gpu():
            m.fit(1)


@pytest.mark.skipif(have_gpu(), reason="checks the no-device error path")
def test_compute_without_device_fails_loudly(mf):
    with mf.MatrixFactorizationSGD(4, 3, 8, 0.01, 0.05, 1) as m:
        m.set_ratings([0, 1], [0, 1], [1.0, 2.0])
        m.init_factors()
        for call in (lambda: m.fit(1), lambda: m.rmse(), lambda: m.predict([0], [0])):
            with pytest.raises(mf.MfsgdError) as ei:
                call()
            assert ei.value.code == -2  # MFSGD_ERR_NO_DEVICE, never a CPU result
            assert "no CPU fallback" in str(ei.value) or "device" in str(ei.value)


def test_product_does_not_reference_the_oracle():
    """The product tree must not import, link or name anything under oracle/."""
    pkg = os.path.join(ROOT, "matrixfactorizationsgd.java_amd")
    for dp, _, files in os.walk(pkg):
        for fn in files:
            if fn.endswith((".py", ".cpp", ".hpp", ".hip", ".h", ".java", "Makefile")):
                txt = open(os.path.join(dp, fn), errors="ignore").read()
                assert "mfsgd_oracle" not in txt and "oracle_bind" not in txt and "mfo_" not in txt, fn


def test_same_ratings_are_recognised_exactly(mf):
    """mfsgd_set_ratings keeps the schedules when it is handed the same triples again -- decided on
    every byte (round 1's Python-side sampled fingerprint missed a change in the middle of the
    arrays) -- and rebuilds them for any change, wherever it is."""
    rng = np.random.default_rng(1)
    n = 300_000
    U, I = 5000, 4000
    u = rng.integers(0, U, n).astype(np.int32)
    i = rng.integers(0, I, n).astype(np.int32)
    r = rng.random(n).astype(np.float32)
    with mf.MatrixFactorizationSGD(U, I, 16, 0.01, 0.05, 1) as m:
        m.set_ratings(u, i, r)
        o0 = m.order()[0].copy()
        assert m.debug_counters()["schedule_builds"] == 1
        m.set_ratings(u.copy(), i.copy(), r.copy())  # other buffers, same triples
        assert m.debug_counters()["schedule_builds"] == 1
        for arr, pos, val in ((r, 100_000, 9.0), (u, 150_001, (int(u[150_001]) + 1) % U), (i, n - 1, (int(i[n - 1]) + 1) % I),
                              (r, 0, -1.0)):
            arr[pos] = val
            before = m.debug_counters()["schedule_builds"]
            m.set_ratings(u, i, r)
            assert m.debug_counters()["schedule_builds"] == before + 1, (pos, "a changed triple must rebuild the schedule")
        cells, rows, subs, entries = m.debug_schedule()
        # the rebuilt schedule carries the NEW rating values
        got = np.sort(entries[:, 1].view(np.float32))
        assert got[0] == -1.0 and got[-1] == 9.0
        m.set_ratings(u[:-1], i[:-1], r[:-1])  # a prefix is a different set
        assert m.schedule_info()["nnz"] == n - 1
        assert o0.size == n


def test_jni_shim_is_well_formed_cpp():
    """No JDK exists here, so jni/mfsgd_jni.cpp cannot be built or run; it is at least checked for
    syntax and types against a declaration-only stub of the JNI signatures it uses
    (tests/jni_stub/jni.h).  UNTESTED UNDER A JVM all the same."""
    import shutil
    import subprocess

    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx, "no C++ compiler"
    p = subprocess.run([cxx, "-std=c++17", "-fsyntax-only", "-Wall", "-Wextra", "-Werror",
                        "-I" + os.path.join(ROOT, "tests", "jni_stub"), "-I" + os.path.join(ROOT, "include"),
                        os.path.join(ROOT, "matrixfactorizationsgd.java_amd", "jni", "mfsgd_jni.cpp")],
                       stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0, p.stdout
    src = open(os.path.join(ROOT, "matrixfactorizationsgd.java_amd", "jni", "mfsgd_jni.cpp")).read()
    # the rule the shim states: nothing pinned around a call that can launch a kernel or wait for the device
    # (since round 3 nothing is pinned at all: every C-ABI call may wait for the device, and no JNI call -- a throw,
    # say -- may be made inside a critical region)
    code = "\n".join(line for line in src.splitlines() if not line.lstrip().startswith("//"))
    assert "GetPrimitiveArrayCritical" not in code and "Pinned<" not in code
    # every native method the Java class declares has its JNI function, and vice versa
    java = open(os.path.join(ROOT, "matrixfactorizationsgd.java_amd", "java", "MatrixFactorizationSGD.java")).read()
    declared = set(re.findall(r"private static native \S+ (native\w+)\(", java))
    defined = set(re.findall(r"Java_MatrixFactorizationSGD_(native\w+)\(", src))
    assert declared == defined and len(declared) >= 20
    # the distributed surface the header cites exists on the Java side and reaches the ring under the C-ABI
    assert "public double[] trainDistributed(" in java
    for sym in ("mfsgd_dsgd_unique_id", "mfsgd_dsgd_create", "mfsgd_dsgd_init_q", "mfsgd_dsgd_train", "mfsgd_dsgd_get_q", "mfsgd_dsgd_destroy",
                "mfsgd_dsgd_plan", "mfsgd_set_item_partition", "mfsgd_init_p_offset"):
        assert sym in code, sym


def test_dsgd_driver_fails_cleanly_without_a_gpu(mf):
    """The ring under the C-ABI needs a device (and RCCL): on a box without one every entry point returns an
    error code and a message -- no crash, no hang, nothing half-created."""
    if have_gpu():
        pytest.skip("covered on the GPU by tests/test_gpu_parity.py::test_native_dsgd_*")
    from mfsgd_amd.dsgd import NativeDSGD

    with mf.MatrixFactorizationSGD(10, 9, 8, 0.01, 0.05, 1, n_parts=2) as t:
        t.set_ratings([0, 1, 2], [0, 1, 2], [1.0, 2.0, 3.0])  # host-side: works without a GPU
        try:
            uid = NativeDSGD.unique_id()
        except mf.MfsgdError as e:
            assert e.code in (-6, -3, -2), e  # UNSUPPORTED (no librccl), HIP or NO_DEVICE
            return
        with pytest.raises(mf.MfsgdError) as ei:
            NativeDSGD(t, 0, 1, uid)
        assert ei.value.code in (-2, -3, -4), ei.value


def test_dsgd_rehearsal_transport_is_not_in_the_product_library(mf, monkeypatch, tmp_path):
    """The ring's shared-memory rehearsal transport (several ranks on one GPU) ships in lib/libmfsgd_rehearsal.so only
    (round 3: it used to sit in the product library behind the environment variable).  libmfsgd.so: MFSGD_DSGD_TRANSPORT
    = shm is refused, and the library does not even import shm_open; libmfsgd_rehearsal.so: the 128-byte id is the magic
    and a segment name (no RCCL, no GPU needed for the id), creating the ring still needs a device and fails cleanly
    here, leaving no segment behind; it exports every symbol of the header too."""
    import subprocess
    import sys

    from mfsgd_amd import _lib
    from mfsgd_amd.dsgd import NativeDSGD

    monkeypatch.setenv("MFSGD_DSGD_TRANSPORT", "shm")
    with pytest.raises(mf.MfsgdError) as ei:
        NativeDSGD.unique_id()  # this process holds the product library
    assert ei.value.code == -6 and "rehearsal" in str(ei.value)
    fake = b"MFSGDSHM/mfsgd_nowhere" + b"\0" * 106
    with mf.MatrixFactorizationSGD(10, 9, 8, 0.01, 0.05, 1, n_parts=2) as t:
        t.set_ratings([0, 1, 2], [0, 1, 2], [1.0, 2.0, 3.0])
        with pytest.raises(mf.MfsgdError) as ei:
            NativeDSGD(t, 0, 1, fake)
        assert ei.value.code == -6
    nm = subprocess.run(["nm", "-D", _lib.library_path()], stdout=subprocess.PIPE, text=True).stdout
    assert "shm_open" not in nm and "mfsgd_dsgd_create" in nm
    nm_r = subprocess.run(["nm", "-D", _lib.rehearsal_library_path()], stdout=subprocess.PIPE, text=True).stdout
    assert "shm_open" in nm_r
    for name in _lib.SIGNATURES:
        assert f" T {name}" in nm_r, name
    code = (
        "import os, sys; sys.path.insert(0, os.getcwd())\n"
        "import mfsgd_amd as mf\n"
        "from mfsgd_amd.dsgd import NativeDSGD\n"
        "a, b = NativeDSGD.unique_id(), NativeDSGD.unique_id()\n"
        "assert len(a) == 128 and a[:8] == b'MFSGDSHM' and a != b\n"
        "name = a[8:].split(b'\\0')[0].decode(); assert name.startswith('/mfsgd_')\n"
        "if sys.argv[1] == 'nogpu':\n"
        "    with mf.MatrixFactorizationSGD(10, 9, 8, 0.01, 0.05, 1, n_parts=2) as t:\n"
        "        t.set_ratings([0, 1, 2], [0, 1, 2], [1.0, 2.0, 3.0])\n"
        "        try:\n"
        "            NativeDSGD(t, 0, 1, a); raise SystemExit('created a ring without a device')\n"
        "        except mf.MfsgdError:\n"
        "            pass\n"
        "    assert not os.path.exists('/dev/shm' + name)\n"
        "print('ok')\n")
    env = dict(os.environ, MFSGD_LIBRARY=_lib.rehearsal_library_path(), MFSGD_DSGD_TRANSPORT="shm")
    p = subprocess.run([sys.executable, "-c", code, "gpu" if have_gpu() else "nogpu"], cwd=ROOT, env=env, stdout=subprocess.PIPE,
                       stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), p.stdout



def test_every_environment_variable_the_library_reads_is_documented():
    """INTEGRATION.md's table of environment variables covers every getenv("MFSGD_...") in the library's sources
    (they are A/B and test switches: none is needed in production, all must be findable)."""
    import glob
    import os
    import re

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    doc = open(os.path.join(root, "INTEGRATION.md")).read()
    read = set()
    for f in glob.glob(os.path.join(root, "matrixfactorizationsgd.java_amd", "csrc", "*")):
        if f.endswith((".cpp", ".hip", ".hpp")):
            read |= set(re.findall(r'getenv\("(MFSGD_[A-Z0-9_]+)"\)', open(f).read()))
    assert len(read) >= 10, read
    missing = sorted(v for v in read if v not in doc)
    assert not missing, missing
