"""The builder of the small C restatements the tests compare with (tests/pairwise_common.py, tests/warp_common.py,
tests/fold_in_pairwise_common.py): the host compiler at -O2 -ffp-contract=off, linked to the oracle for its canonical dot."""
import atexit
import ctypes as C
import os
import shutil
import subprocess
import tempfile

from tests.conftest import ROOT

_built = {}


def build(tag, c_source, prototypes):
    """The compiled restatement `tag` (built once per process, in a directory of its own that goes when the process does).
    prototypes: {function: (restype, argtypes)}."""
    if tag not in _built:
        from tests.oracle_bind import Oracle

        Oracle()  # builds oracle/libmfsgd_oracle.so when it is not there
        cc = shutil.which("gcc") or shutil.which("cc")
        assert cc, "no C compiler"
        tmp = tempfile.mkdtemp(prefix=f"mfsgd_{tag}_")
        atexit.register(shutil.rmtree, tmp, ignore_errors=True)
        src, so = os.path.join(tmp, f"{tag}_restatement.c"), os.path.join(tmp, f"lib{tag}_restatement.so")
        with open(src, "w") as f:
            f.write(c_source)
        oracle_dir = os.path.join(ROOT, "oracle")
        p = subprocess.run([cc, "-O2", "-ffp-contract=off", "-fno-fast-math", "-fPIC", "-shared", "-Wall", "-Wextra", "-o", so, src,
                            "-L" + oracle_dir, "-Wl,-rpath," + oracle_dir, "-l:libmfsgd_oracle.so", "-lm"],
                           stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True)
        assert p.returncode == 0, p.stdout
        lib = C.CDLL(so)
        for name, (restype, argtypes) in prototypes.items():
            getattr(lib, name).restype, getattr(lib, name).argtypes = restype, argtypes
        _built[tag] = lib
    return _built[tag]
