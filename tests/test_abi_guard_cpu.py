"""include/mfsgd.h promises that no C++ exception crosses the boundary.  A host allocation that fails inside a serving
call comes back as MFSGD_ERR_OOM and leaves the handle usable (it used to end the process), and every `int` entry point
of the boundary units (csrc/handle.cpp, ratings.cpp, train.cpp, online_update.cpp, serve_topn.cpp, serve_rank.cpp, serve_fold.cpp, dsgd.cpp,
io.cpp) runs its body inside the guard of csrc/guard.hpp, through the wrapper of its unit."""
import os
import re
import subprocess
import sys

from tests.conftest import ROOT

CSRC = os.path.join(ROOT, "matrixfactorizationsgd.java_amd", "csrc")
RING, REHEARSAL_ONLY = "dsgd.cpp", ("shm_transport.cpp",)  # the rest goes into libmfsgd.so
UNITS = ("handle.cpp", "ratings.cpp", "train.cpp", "online_update.cpp", "serve_lists.cpp", "serve_topn.cpp", "serve_rank.cpp", "serve_fold.cpp",
         RING, "io.cpp", "rccl_transport.cpp") + REHEARSAL_ONLY
# calls that allocate nothing and throw nothing: a cap, not a target
UNGUARDED = {"mfsgd_abi_version", "mfsgd_get_dims", "mfsgd_get_parts", "mfsgd_get_hyper", "mfsgd_debug_device_bytes",
             "mfsgd_dsgd_stats", "mfsgd_ratings_file_info", "mfsgd_ratings_file_read"}

CHILD = r"""
import ctypes as C, resource, sys
import numpy as np
from mfsgd_amd import _lib

lib = _lib.load_library()
U = 2**31 - 1
cfg = _lib.Config(n_users=U, n_items=4, k=1, lr=0.01, lambda_=0.05)
h = C.c_void_p()
assert lib.mfsgd_create(C.byref(cfg), C.byref(h)) == 0, lib.mfsgd_last_error(None)
# the limit is process-wide: what is mapped now plus 2 GiB, so that a request of 8 GiB must fail
vm_kb = int(next(l for l in open("/proc/self/status") if l.startswith("VmSize:")).split()[1])
limit = vm_kb * 1024 + (2 << 30)
resource.setrlimit(resource.RLIMIT_AS, (limit, limit))

i32, f32 = C.POINTER(C.c_int32), C.POINTER(C.c_float)
one = np.zeros(1, np.int32)
items, scores = np.zeros(1, np.int32), np.zeros(1, np.float32)
row = np.zeros(1, np.float32)
p = lambda a, t: a.ctypes.data_as(t)

def oom(name, rc):
    msg = lib.mfsgd_last_error(h).decode()
    assert rc == -4 and msg.endswith("out of host memory"), (name, rc, msg)
    print(name, rc, msg)

oom("recommend_excluding", lib.mfsgd_recommend_excluding(h, p(one, i32), 1, 1, p(one, i32), p(one, i32), 1,
                                                         p(items, i32), p(scores, f32)))
oom("recommend_rows", lib.mfsgd_recommend_rows(h, p(row, f32), U, 1, None, None, 0, p(items, i32), p(scores, f32)))
oom("rank_items", lib.mfsgd_rank_items(h, p(one, i32), p(one, i32), 1, None, None, 0, p(items, i32)))
# the handle still serves
nu, ni, k = C.c_int32(), C.c_int32(), C.c_int32()
assert lib.mfsgd_get_dims(h, C.byref(nu), C.byref(ni), C.byref(k)) == 0
assert (nu.value, ni.value, k.value) == (U, 4, 1)
lib.mfsgd_destroy(h)
print("ok")
"""

CHILD_IO = r"""
import ctypes as C, os, resource, sys, tempfile
from mfsgd_amd import _lib

lib = _lib.load_library()
U = 2**31 - 1
cfg = _lib.Config(n_users=U, n_items=4, k=1, lr=0.01, lambda_=0.05)
h = C.c_void_p()
assert lib.mfsgd_create(C.byref(cfg), C.byref(h)) == 0, lib.mfsgd_last_error(None)
vm_kb = int(next(l for l in open("/proc/self/status") if l.startswith("VmSize:")).split()[1])
limit = vm_kb * 1024 + (2 << 30)
resource.setrlimit(resource.RLIMIT_AS, (limit, limit))
with tempfile.TemporaryDirectory() as tmp:
    rc = lib.mfsgd_save_factors(h, os.path.join(tmp, "factors.bin").encode())
    msg = lib.mfsgd_io_last_error().decode()
    assert rc == -4 and msg.endswith("save_factors: out of host memory"), (rc, msg)
    assert os.listdir(tmp) == []
# the handle still serves
nu, ni, k = C.c_int32(), C.c_int32(), C.c_int32()
assert lib.mfsgd_get_dims(h, C.byref(nu), C.byref(ni), C.byref(k)) == 0
assert (nu.value, ni.value, k.value) == (U, 4, 1)
lib.mfsgd_destroy(h)
print("ok")
"""


def test_a_failed_host_allocation_is_an_error_code_not_an_abort():
    p = subprocess.run([sys.executable, "-c", CHILD], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.returncode, p.stdout)
    for name in ("recommend_excluding", "recommend_rows", "rank_items"):
        assert re.search(rf"^{name} -4 .*out of host memory$", p.stdout, flags=re.M), p.stdout


def test_a_failed_host_allocation_in_save_factors_is_an_error_code_not_an_abort():
    """io.cpp under the same guard: the two 8 GiB host copies of the factors fail before any device is needed."""
    p = subprocess.run([sys.executable, "-c", CHILD_IO], cwd=ROOT, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
    assert p.returncode == 0 and p.stdout.strip().endswith("ok"), (p.returncode, p.stdout)


def _definitions():
    """name -> body of every function defined at the top level of the boundary units' extern "C" blocks."""
    out = {}
    for unit in UNITS:
        src = open(os.path.join(CSRC, unit)).read()
        for m in re.finditer(r"^int (mfsgd_[a-z0-9_]+)\(", src, flags=re.M):
            start = src.index("{", src.index(")", m.start()))
            end = src.index("\n", start)  # a definition on one line ...
            if not src[start:end].rstrip().endswith("}"):
                end = src.index("\n}\n", start)  # ... or up to its own closing brace: the first one in column 0
            body = src[start:end]
            assert m.group(1) not in out, m.group(1)
            out[m.group(1)] = body
    return out


def test_every_int_entry_point_runs_inside_the_guard():
    hdr = open(os.path.join(ROOT, "include", "mfsgd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"^int\s+(mfsgd_[a-z0-9_]+)\s*\(", hdr, flags=re.M))
    defs = _definitions()
    assert declared == set(defs), sorted(declared ^ set(defs))
    assert len(defs) >= 59 and UNGUARDED <= set(defs) and len(UNGUARDED) <= 8
    unguarded = sorted(n for n, body in defs.items() if not re.search(r"\breturn (guarded(_free)?|dsgd_guarded|io_guarded)\(", body))
    assert unguarded == sorted(UNGUARDED), unguarded
    # nothing hand-written is left beside it: apply_hyper keeps its clean-up, host_copies its message
    n_catch = sum(open(os.path.join(CSRC, u)).read().count("catch (") for u in UNITS)
    assert n_catch <= 3, n_catch


def test_the_ring_knows_its_transports_through_the_seam_only():
    """csrc/dsgd.cpp is the ring; what moves its blocks is behind csrc/transport.hpp.  One conditional tells the two
    libraries apart, and nothing of the shared-memory rehearsal transport is in a unit of the product library."""
    ring = open(os.path.join(CSRC, RING)).read()
    assert len(re.findall(r"^\s*#\s*(?:if|ifdef|ifndef|elif)\b.*MFSGD_DSGD_REHEARSAL", ring, flags=re.M)) <= 1
    for unit in UNITS:
        src = open(os.path.join(CSRC, unit)).read()
        assert (unit in REHEARSAL_ONLY) == ("shm_open" in src), unit
        assert unit in REHEARSAL_ONLY or "mmap(" not in src, unit
    mk = open(os.path.join(CSRC, "Makefile")).read()
    assert re.search(r"^OBJS\s*:=(?!.*shm_transport)", mk, flags=re.M) and "shm_transport.o" not in re.search(r"^HOST_OBJS\s*:=.*$", mk, flags=re.M).group(0)
